#!/usr/bin/env python3
"""mgic_sample_points: the point-sampling kernel of libmgic_sample.so.

2^20 random points (default) on one n^3 box (default 256^3), and the same
points on a three-level hierarchy over it (level 1 the middle half of the base
in every direction as 2 x 2 x 2 boxes, level 2 the middle half of level 1),
requested orders 2 and 4.  Each sample is `reps` back-to-back calls between HIP
events on the library's stream, so it covers what the call puts on the stream
(the upload of the points and of the box table, k_sample_points, the download
of the three result arrays); the wall time per call, which adds the call's one
allocation and its stream synchronisation, is given next to it.  The call runs
once per solve on a handful of points.  Stated as measured: there is no bar.

Prints one JSON line.  usage: bench_sample.py [--n 256] [--points 1048576]
                                               [--reps 10] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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
    from mg_ic_code_amd.sample import sample_points
    n, length = args.n, 100.0
    comm = mg.Comm()

    def level(l, boxes):
        dom = (0, 0, 0) + ((n << l) - 1,) * 3
        grid = mg.Grid(comm, dom, boxes, length / (n << l), patches=l > 0)
        f = mg.LevelData(grid)
        f.set_val_all(1.0 + 0.25 * l)
        return f

    def middle(l, parts):
        """The middle half of level l - 1, in level l's cells, as parts^3 boxes."""
        lo, size = (n << l) // 4 if l == 1 else 3 * (n << l) // 8, (n << l) // (2 if l == 1 else 4)
        e = [lo + size * i // parts for i in range(parts + 1)]
        return [(e[i], e[j], e[k], e[i + 1] - 1, e[j + 1] - 1, e[k + 1] - 1)
                for k in range(parts) for j in range(parts) for i in range(parts)]

    base = level(0, [(0, 0, 0, n - 1, n - 1, n - 1)])
    three = [base, level(1, middle(1, 2)), level(2, middle(2, 2))]
    pts = np.random.default_rng(20261021).uniform(-0.5, 0.5, (args.points, 3)) * length
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

    out = {"config": f"{args.points} random points, {n}^3 base; {args.rounds} samples of "
                     f"{args.reps} calls each, HIP events on the library's stream",
           "data": "synthetic"}
    for name, fields in (("one_box", [base]), ("three_levels", three)):
        for order in (2, 4):
            def fn(fields=fields, order=order):
                return sample_points(fields, pts, order)
            r = fn()  # warm up the code object
            comm.synchronize()
            ev, wall = zip(*[timed(fn) for _ in range(args.rounds)])
            out[f"{name}_order_{order}"] = {
                "boxes": sum(len(f.grid.boxes) for f in fields),
                "points_per_level": [int((r.level == l).sum()) for l in range(len(fields))],
                "points_per_order": {str(o): int((r.order == o).sum()) for o in (1, 2, 4)},
                "event_ms": round(statistics.median(ev), 4),
                "event_ms_min_max": [round(min(ev), 4), round(max(ev), 4)],
                "wall_ms": round(statistics.median(wall), 4)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
