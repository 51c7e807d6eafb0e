#!/usr/bin/env python3
"""The puncture-table generators against today's: set_nl_coefs and the regrid
condition.

The TABLE instantiations (k_binary_bh<.., .., true>, k_regrid_condition<..,
true>) take the holes from a table passed as a kernel argument and sum the
Bowen-York terms over its pairs in a run-time loop; today's (<.., false>)
evaluate one pair with the deck's special vectors.  A one-pair table (the
deck's two holes as a table) does the deck's arithmetic; a four-pair table
(eight punctures) does it four times.  All three on the same n^3 box,
interleaved (deck, one pair, four pairs, deck, ...), each sample the device
time of `reps` back-to-back calls between HIP events on the library's stream.

Prints one JSON line.  usage: bench_punctures.py [--n 256] [--reps 20] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch

    import mg_ic_code_amd as mg
    from mg_ic_code_amd.grids import set_regrid_condition
    from mg_ic_code_amd.params import read_params_file
    from mg_ic_code_amd.punctures import (Puncture, PunctureSet, set_nl_coefs_punct,
                                          set_regrid_condition_punct)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prm = read_params_file(os.path.join(root, "tests", "golden", "params.txt"))
    bh = prm.bh(constant_K=-0.1)
    n = args.n
    comm = mg.Comm()
    dom = (0, 0, 0, n - 1, n - 1, n - 1)
    grid = mg.Grid(comm, dom, [dom], prm.domainLength[0] / n)
    psi, a, rhs = mg.LevelData(grid), mg.LevelData(grid), mg.LevelData(grid)
    psi.set_val_all(1.0)
    one = PunctureSet.from_params(prm)
    # eight punctures: the deck's pair and three more pairs off the axes, none
    # on a cell centre of an even n
    four = PunctureSet(list(one) + [
        Puncture(0.1, (3.0 * s + 0.2, 5.0 * t, -7.0 * s), (0.01 * t, -0.02, 0.01 * s),
                 (0.01, 0.02 * s, -0.01 * t))
        for s, t in ((1, 1), (-1, 1), (1, -1), (-1, -1), (2, 3), (-3, 2))])
    assert len(four) == 8
    stream = torch.cuda.ExternalStream(comm.stream)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.reps):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / args.reps

    cases = {
        "set_nl_coefs": (lambda: mg.set_nl_coefs(psi, a, rhs, bh),
                         lambda: set_nl_coefs_punct(psi, a, rhs, bh, one),
                         lambda: set_nl_coefs_punct(psi, a, rhs, bh, four)),
        "regrid_condition": (lambda: set_regrid_condition(psi, a, bh),
                             lambda: set_regrid_condition_punct(psi, a, bh, one),
                             lambda: set_regrid_condition_punct(psi, a, bh, four)),
    }
    names = ("deck", "one_pair", "four_pairs")
    out = {"config": f"{n}^3 box, params.txt BH, psi = 1; {args.rounds} interleaved samples of "
                     f"{args.reps} calls each, HIP events on the library's stream",
           "data": "synthetic"}
    for case, fns in cases.items():
        for fn in fns:  # warm up every code object
            fn()
        comm.synchronize()
        t = {k: [] for k in names}
        for _ in range(args.rounds):
            for k, fn in zip(names, fns):
                t[k].append(timed(fn))
        med = {k: statistics.median(v) for k, v in t.items()}
        out[case] = {f"{k}_ms": round(med[k], 4) for k in names}
        out[case].update({f"{k}_ms_min_max": [round(min(t[k]), 4), round(max(t[k]), 4)]
                          for k in names})
        out[case]["one_pair_over_deck"] = round(med["one_pair"] / med["deck"], 3)
        out[case]["four_pairs_over_deck"] = round(med["four_pairs"] / med["deck"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
