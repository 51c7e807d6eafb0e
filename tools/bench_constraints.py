#!/usr/bin/env python3
"""The constraint kernel against the integrand kernel on one box.

k_constraints evaluates the Bowen-York terms seven times per cell (the cell
and its six neighbours, for the centred difference of Abar_ij) where
k_binary_bh<INTEGRAND> evaluates them once, and writes five fields where that
writes one; it runs once per solve.  mgic_field_constraints and
set_nl_integrand_matter on the same n^3 box with the same sources, interleaved
(integrand, constraints, integrand, ...), each sample the device time of
`reps` back-to-back calls between HIP events on the library's stream; with the
analytic phi_0 and the deck's two holes, and with the stored phi_0 and the
same holes as a table.  Stated as measured: there is no bar.

Prints one JSON line.  usage: bench_constraints.py [--n 256] [--reps 10] [--rounds 7]
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch

    import mg_ic_code_amd as mg
    from mg_ic_code_amd.constraints import ConstraintFields, set_constraints
    from mg_ic_code_amd.matter import PiProfile, ScalarPotential, set_nl_integrand_matter
    from mg_ic_code_amd.params import read_params_file
    from mg_ic_code_amd.phi import PhiProfile
    from mg_ic_code_amd.punctures import PunctureSet
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prm = read_params_file(os.path.join(root, "tests", "golden", "params.txt"))
    bh = prm.bh(constant_K=-0.1)
    n = args.n
    comm = mg.Comm()
    dom = (0, 0, 0, n - 1, n - 1, n - 1)
    grid = mg.Grid(comm, dom, [dom], prm.domainLength[0] / n)
    psi, integ = mg.LevelData(grid), mg.LevelData(grid)
    psi.set_val_all(1.0)
    out_f = ConstraintFields(grid)
    pot = ScalarPotential(1e-5, 0.02, 0.01)
    pi = PiProfile.constant(0.005).fill(grid, prm)
    stored = PhiProfile.gaussian().fill(grid, prm)
    deck = PunctureSet([[bh[f"bh{i}_bare_mass"], bh[f"bh{i}_offset"], 0.0, 0.0, 0.0,
                         bh[f"bh{i}_momentum"], 0.0, 0.0, 0.0, bh[f"bh{i}_spin"]] for i in (1, 2)])
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
        "analytic_phi_deck_holes": (
            lambda: set_nl_integrand_matter(psi, integ, bh, pot, pi=pi),
            lambda: set_constraints(psi, out_f, bh, potential=pot, pi=pi)),
        "stored_phi_table": (
            lambda: set_nl_integrand_matter(psi, integ, bh, pot, pi=pi, punctures=deck,
                                            phi=stored),
            lambda: set_constraints(psi, out_f, bh, potential=pot, pi=pi, punctures=deck,
                                    phi=stored)),
    }
    names = ("integrand", "constraints")
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
        out[case]["constraints_over_integrand"] = round(med["constraints"] / med["integrand"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
