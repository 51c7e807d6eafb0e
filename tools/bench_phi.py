#!/usr/bin/env python3
"""Stored phi_0 against analytic phi_0: set_nl_coefs and the regrid condition.

The STORED instantiations of the generators (k_binary_bh<.., true>,
k_regrid_condition<true>) load phi_0 from a device field -- 7 reads of one
extra 8-byte stream per cell, 6 of them neighbours that the caches serve --
where the analytic ones (<.., false>) evaluate six exp per cell.  Both on the
same n^3 box, interleaved (analytic, stored, analytic, ...), each sample the
device time of `reps` back-to-back calls between HIP events on the library's
stream; the fill kernel (once per solve) is timed the same way.

Prints one JSON line.  usage: bench_phi.py [--n 256] [--reps 20] [--rounds 7]
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
    from mg_ic_code_amd.phi import PhiProfile, set_nl_coefs_phi, set_regrid_condition_phi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prm = read_params_file(os.path.join(root, "tests", "golden", "params.txt"))
    bh = prm.bh(constant_K=-0.1)
    n = args.n
    comm = mg.Comm()
    dom = (0, 0, 0, n - 1, n - 1, n - 1)
    grid = mg.Grid(comm, dom, [dom], prm.domainLength[0] / n)
    psi, a, rhs = mg.LevelData(grid), mg.LevelData(grid), mg.LevelData(grid)
    psi.set_val_all(1.0)
    phi = PhiProfile.gaussian().fill(grid, bh)
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
                         lambda: set_nl_coefs_phi(psi, phi, a, rhs, bh)),
        "regrid_condition": (lambda: set_regrid_condition(psi, a, bh),
                             lambda: set_regrid_condition_phi(psi, phi, a, bh)),
    }
    out = {"config": f"{n}^3 box, params.txt BH, psi = 1; {args.rounds} interleaved samples of "
                     f"{args.reps} calls each, HIP events on the library's stream",
           "data": "synthetic"}
    for name, (analytic, stored) in cases.items():
        for fn in (analytic, stored):  # warm up both code objects
            fn()
        comm.synchronize()
        ta, ts = [], []
        for _ in range(args.rounds):
            ta.append(timed(analytic))
            ts.append(timed(stored))
        out[name] = {"analytic_ms": round(statistics.median(ta), 4),
                     "stored_ms": round(statistics.median(ts), 4),
                     "analytic_ms_min_max": [round(min(ta), 4), round(max(ta), 4)],
                     "stored_ms_min_max": [round(min(ts), 4), round(max(ts), 4)],
                     "stored_over_analytic": round(statistics.median(ts) / statistics.median(ta), 3)}
    fill = lambda: mg._lib.call("mgic_field_fill_phi", phi.handle, 0, _bhv(bh))  # noqa: E731
    fill()
    comm.synchronize()
    tf = [timed(fill) for _ in range(args.rounds)]
    out["fill_phi_gaussian_ms"] = round(statistics.median(tf), 4)
    print(json.dumps(out), flush=True)


def _bhv(bh):
    import ctypes

    from mg_ic_code_amd.core import BH_KEYS
    return (ctypes.c_double * 13)(*[float(bh[k]) for k in BH_KEYS])


if __name__ == "__main__":
    main()
