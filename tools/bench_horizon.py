#!/usr/bin/env python3
"""mgic_horizon_expansion: the expansion kernel of libmgic_horizon.so, and one
full find_horizon.

2^20 random points (default) on one n^3 box (default 256^3), and the same
points on tools/bench_sample.py's three-level hierarchy over it (level 1 the
middle half of the base in every direction as 2 x 2 x 2 boxes, level 2 the
middle half of level 1), without and with the six LW_ij.  Each sample is `reps`
back-to-back calls between HIP events on the library's stream, so it covers
what the call puts on the stream (the upload of the points, normals,
divergences and the box table, k_horizon_expansion, the download of the
results); the wall time per call, which adds the call's one allocation and its
stream synchronisation, is given next to it.  Then one find_horizon (lmax = 8,
12 x 24 points) of a single puncture of bare mass 1 off the centre, psi = 1 on
a 24^3 box: its wall time, iterations and time per iteration.  The kernel runs
a few dozen times per solve on a few hundred points.  Stated as measured:
there is no bar.

Prints one JSON line.  usage: bench_horizon.py [--n 256] [--points 1048576]
                                                [--reps 10] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class _LW:
    def __init__(self, per_level):
        self.per_level, self.num_levels = per_level, len(per_level)

    def lw(self, level=0):
        return self.per_level[level]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import numpy as np
    import torch

    import mg_ic_code_amd as mg
    from mg_ic_code_amd.horizon import expansion_points, find_horizon
    n, length = args.n, 100.0
    comm = mg.Comm()

    def grid(l, boxes):
        dom = (0, 0, 0) + ((n << l) - 1,) * 3
        return mg.Grid(comm, dom, boxes, length / (n << l), patches=l > 0)

    def field(g, value):
        f = mg.LevelData(g)
        f.set_val_all(value)
        return f

    def middle(l, parts):
        """The middle half of level l - 1, in level l's cells, as parts^3 boxes."""
        lo, size = (n << l) // 4 if l == 1 else 3 * (n << l) // 8, (n << l) // (2 if l == 1 else 4)
        e = [lo + size * i // parts for i in range(parts + 1)]
        return [(e[i], e[j], e[k], e[i + 1] - 1, e[j + 1] - 1, e[k + 1] - 1)
                for k in range(parts) for j in range(parts) for i in range(parts)]

    grids = [grid(0, [(0, 0, 0, n - 1, n - 1, n - 1)]), grid(1, middle(1, 2)), grid(2, middle(2, 2))]
    psi = [field(g, 1.0 + 0.25 * l) for l, g in enumerate(grids)]
    lw = _LW([[field(g, 0.01 * (k + 1)) for k in range(6)] for g in grids])
    rng = np.random.default_rng(20261021)
    pts = rng.uniform(-0.5, 0.5, (args.points, 3)) * length
    nrm = rng.normal(size=(args.points, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    divn = rng.uniform(0.5, 3.0, args.points)
    table = [(0.5, 10.0, 0.0, 0.0, 0.0, 0.05, 0.0, 0.0, 0.0, 0.1),
             (0.5, -10.0, 0.0, 0.0, 0.0, -0.05, 0.0, 0.0, 0.0, 0.1)]
    stream = torch.cuda.ExternalStream(comm.stream)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        for _ in range(args.reps):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / args.reps, (time.perf_counter() - t0) * 1e3 / args.reps

    out = {"config": f"{args.points} random points, {n}^3 base, 2 punctures; {args.rounds} samples "
                     f"of {args.reps} calls each, HIP events on the library's stream",
           "data": "synthetic"}
    for name, nlev in (("one_box", 1), ("three_levels", 3)):
        for with_lw in (False, True):
            def fn(nlev=nlev, with_lw=with_lw):
                return expansion_points(psi[:nlev], pts, nrm, divn, None, punctures=table,
                                        momentum=_LW(lw.per_level[:nlev]) if with_lw else None)
            r = fn()  # warm up the code object
            comm.synchronize()
            ev, wall = zip(*[timed(fn) for _ in range(args.rounds)])
            out[f"{name}_{'lw' if with_lw else 'by'}"] = {
                "boxes": sum(len(g.boxes) for g in grids[:nlev]),
                "points_per_level": [int((r.level == l).sum()) for l in range(nlev)],
                "points_per_order": {str(o): int((r.order == o).sum()) for o in (0, 2, 4)},
                "event_ms": round(statistics.median(ev), 4),
                "event_ms_min_max": [round(min(ev), 4), round(max(ev), 4)],
                "wall_ms": round(statistics.median(wall), 4)}
    dom = (0, 0, 0, 23, 23, 23)
    small = field(mg.Grid(comm, dom, [dom], 0.25), 1.0)
    hole = [(1.0, 0.2, 0.1, -0.15, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)]
    find_horizon(small, None, (0.0, 0.0, 0.0), 1.3, punctures=hole)  # warm up
    walls = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        h = find_horizon(small, None, (0.0, 0.0, 0.0), 1.3, punctures=hole)
        walls.append((time.perf_counter() - t0) * 1e3)
    out["find_horizon"] = {"status": h.status, "iterations": h.iterations, "points": 288,
                           "irreducible_mass": h.irreducible_mass,
                           "wall_ms": round(statistics.median(walls), 3),
                           "wall_ms_per_evaluation": round(statistics.median(walls)
                                                           / (h.iterations + 1), 4)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
