#!/usr/bin/env python3
"""The matter generators against today's: set_nl_coefs and the regrid condition.

The MATTER instantiations (k_binary_bh<.., .., .., true>, k_regrid_condition<..,
.., true>) evaluate rho = Pi^2 / 2 + V(phi_0) where today's (<.., false>) carry
the reference's literal zero: phi_0 at the cell (one more exp on the analytic
path, one more load on the stored one), seven multiplications and two
additions for V, and, with a stored Pi_0, one 8-byte stream, its square and an
addition.  Three variants on the same n^3 box, interleaved (none, potential,
potential + Pi, none, ...), each sample the device time of `reps`
back-to-back calls between HIP events on the library's stream; once with the
analytic phi_0 and once with the stored one.

Prints one JSON line.  usage: bench_matter.py [--n 256] [--reps 20] [--rounds 7]
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
    from mg_ic_code_amd.matter import (PiProfile, ScalarPotential, set_nl_coefs_matter,
                                       set_regrid_condition_matter)
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
    pot = ScalarPotential(1e-5, 0.02, 0.01)
    pi = PiProfile.constant(0.005).fill(grid, prm)
    stored = PhiProfile.gaussian().fill(grid, prm)
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
                         lambda: set_nl_coefs_matter(psi, a, rhs, bh, pot),
                         lambda: set_nl_coefs_matter(psi, a, rhs, bh, pot, pi=pi)),
        "regrid_condition": (lambda: set_regrid_condition(psi, a, bh),
                             lambda: set_regrid_condition_matter(psi, a, bh, pot),
                             lambda: set_regrid_condition_matter(psi, a, bh, pot, pi=pi)),
        "set_nl_coefs_stored_phi": (
            lambda: set_nl_coefs_phi(psi, stored, a, rhs, bh),
            lambda: set_nl_coefs_matter(psi, a, rhs, bh, pot, phi=stored),
            lambda: set_nl_coefs_matter(psi, a, rhs, bh, pot, pi=pi, phi=stored)),
        "regrid_condition_stored_phi": (
            lambda: set_regrid_condition_phi(psi, stored, a, bh),
            lambda: set_regrid_condition_matter(psi, a, bh, pot, phi=stored),
            lambda: set_regrid_condition_matter(psi, a, bh, pot, pi=pi, phi=stored)),
    }
    names = ("none", "potential", "potential_pi")
    out = {"config": f"{n}^3 box, params.txt BH, psi = 1, V0 1e-5 mass 0.02 lambda 0.01, "
                     f"Pi 0.005; {args.rounds} interleaved samples of {args.reps} calls each, "
                     "HIP events on the library's stream",
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
        out[case]["potential_over_none"] = round(med["potential"] / med["none"], 3)
        out[case]["potential_pi_over_none"] = round(med["potential_pi"] / med["none"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
