#!/usr/bin/env python3
"""Run the reference program's solve (Main_PoissonSolver.cpp main / poissonSolve)
on device: read a params.txt, build the base level, and iterate the
nonlinear loop.  The per-iteration |dpsi| and linear iteration counts are
printed as the reference's pout() does.

With --max-level K > 0 the AMR hierarchy is generated first as the reference's
set_grids does (tagging on the regrid condition, up to K levels above the
base), and the loop runs over it.

With --phi gaussian|sine the scalar field phi_0 is stored on the device once
(mg_ic_code_amd/phi.py) and read by the stored-field generators; without the
flag phi_0 is the Gaussian evaluated in the kernels.  A deck with is_periodic
set runs on a periodic base level.

With --puncture "m x y z Px Py Pz Jx Jy Jz" (repeatable, 1 to 8 times) the
holes are that puncture table (mg_ic_code_amd/punctures.py) instead of the
deck's two holes or the deck's own table (num_punctures, puncture1 ...).

usage: python tools/run_poisson.py [params.txt] [--size N] [--boxes-per-rank x,y,z]
                                   [--max-level K] [--phi gaussian|sine]
                                   [--puncture "m x y z Px Py Pz Jx Jy Jz"]...
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("params", nargs="?", default=os.path.join(ROOT, "tests", "golden", "params.txt"))
    ap.add_argument("--size", type=int, default=0, help="override N (cells per side)")
    ap.add_argument("--boxes-per-rank", default="1,1,1")
    ap.add_argument("--max-depth", type=int, default=-1)
    ap.add_argument("--max-level", type=int, default=0,
                    help="generate up to K AMR levels above the base with set_grids (0: one level)")
    ap.add_argument("--phi", choices=("gaussian", "sine"), default=None,
                    help="store phi_0 on the device from this profile (default: analytic Gaussian)")
    ap.add_argument("--puncture", action="append", default=None, metavar="ROW",
                    help="a Bowen-York puncture, \"m x y z Px Py Pz Jx Jy Jz\"; repeatable; "
                         "overrides the deck's table")
    args = ap.parse_args()
    import mg_ic_code_amd as mg
    from mg_ic_code_amd.decomposition import decompose
    from mg_ic_code_amd.nl import poisson_solve
    from mg_ic_code_amd.params import read_params_file
    prm = read_params_file(args.params)
    n = args.size or prm.N[0]
    bpr = tuple(int(v) for v in args.boxes_per_rank.split(","))
    dom, boxes, owners = decompose((n, n, n), 1, boxes_per_rank=bpr)
    grid = mg.Grid(mg.Comm(), dom, boxes, prm.domainLength[0] / n,
                   periodic=(1, 1, 1) if prm.is_periodic else (0, 0, 0), owners=owners)
    levels = grid
    phi0 = mg.PhiProfile(args.phi) if args.phi else None
    from mg_ic_code_amd.punctures import resolve_punctures
    punct = resolve_punctures([row.split() for row in args.puncture] if args.puncture else None,
                              prm)
    if punct is not None:
        for i, p in enumerate(punct):
            print(f"puncture {i + 1}: m {p.mass!r} at {p.position} P {p.momentum} J {p.spin}")
    if args.max_level > 0:
        from mg_ic_code_amd.grids import set_grids
        levels = set_grids(grid.comm, prm, grid, max_level=args.max_level, phi0=phi0,
                           punctures=punct)
        for lev, g in enumerate(levels):
            cells = sum((b[3] - b[0] + 1) * (b[4] - b[1] + 1) * (b[5] - b[2] + 1) for b in g.boxes)
            print(f"level {lev}: {len(g.boxes)} boxes, {cells} cells")
    t0 = time.perf_counter()
    res = poisson_solve(levels, prm, max_depth=args.max_depth, phi0=phi0, punctures=punct)
    mg.device_synchronize()
    dt = time.perf_counter() - t0
    for i, (nrm, it) in enumerate(zip(res.dpsi_norms, res.linear_iterations)):
        print(f"Main Loop Iteration {i + 1}: {it} BiCGStab iterations, norm of dpsi {nrm:.6e}")
    out = {"n": n, "boxes": len(boxes), "nl_iterations": len(res.dpsi_norms),
           "converged": res.converged, "seconds": round(dt, 3)}
    if punct is not None:
        out["punctures"] = [list(p.row()) for p in punct]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
