#!/usr/bin/env python3
"""mgic_adm_charges on one box: the surface-charge kernels of libmgic_adm.so.

One n^3 box (default 256^3), psi = 1, the deck's two holes as a table, the
surfaces n_R = 64, 96, 127 each in a call of its own and all three in one
call, without and with six stored LW_ij.  Each sample is `reps` back-to-back
calls between HIP events on the library's stream, so it covers what the call
puts on the stream (the box table's upload, k_adm_surface, k_adm_finish, the
download of the sums); the wall time per call, which adds the call's three
allocations and its stream synchronisation, is given next to it.  The call
runs once per solve.  Stated as measured: there is no bar.

Prints one JSON line.  usage: bench_adm.py [--n 256] [--reps 10] [--rounds 7]
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--half-widths", default="64 96 127")
    args = ap.parse_args()
    import torch

    import mg_ic_code_amd as mg
    from mg_ic_code_amd.adm import charges, parse_half_widths
    from mg_ic_code_amd.params import read_params_file
    from mg_ic_code_amd.punctures import PunctureSet
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prm = read_params_file(os.path.join(root, "tests", "golden", "params.txt"))
    n = args.n
    hws = parse_half_widths(args.half_widths)
    comm = mg.Comm()
    dom = (0, 0, 0, n - 1, n - 1, n - 1)
    grid = mg.Grid(comm, dom, [dom], prm.domainLength[0] / n)
    psi = mg.LevelData(grid)
    psi.set_val_all(1.0)
    lw = [mg.LevelData(grid) for _ in range(6)]
    for i, f in enumerate(lw):
        f.set_val_all(1e-3 * (i + 1))
    deck = PunctureSet.from_params(prm)
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

    out = {"config": f"{n}^3 box, params.txt BH as a table, psi = 1; {args.rounds} samples of "
                     f"{args.reps} calls each, HIP events on the library's stream",
           "data": "synthetic"}
    for with_lw in (False, True):
        fields = lw if with_lw else None
        for case in [[h] for h in hws] + [hws]:
            def fn(case=case, fields=fields):
                return charges(psi, case, deck, fields)
            fn()  # warm up the code object
            comm.synchronize()
            ev, wall = zip(*[timed(fn) for _ in range(args.rounds)])
            key = ("lw" if with_lw else "by") + "_n_R_" + "_".join(str(h) for h in case)
            out[key] = {"faces": sum(6 * (2 * h) ** 2 for h in case),
                        "event_ms": round(statistics.median(ev), 4),
                        "event_ms_min_max": [round(min(ev), 4), round(max(ev), 4)],
                        "wall_ms": round(statistics.median(wall), 4)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
