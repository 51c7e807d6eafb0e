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

With --potential "V0 mass lambda" and/or --pi VALUE the scalar field's
potential V = V0 + mass^2 phi^2 / 2 + lambda phi^4 / 4 and a constant velocity
Pi enter the sources as rho = Pi^2 / 2 + V (mg_ic_code_amd/matter.py); either
flag overrides the deck's scalar_V0, scalar_mass, scalar_self_coupling and
pi_amplitude.

With --constraints the Hamiltonian and momentum constraints of the solved data
(mg_ic_code_amd/constraints.py) are reported after the loop: one line per
component (Ham, Mom1, Mom2, Mom3) with its max norm and its L2 norm, then
max|Ham| / max Ham_abs.

With --momentum (or the deck's solve_momentum = 1) the momentum constraint is
solved for the matter's Pi d_i phi source (mg_ic_code_amd/momentum.py): needs
a matter with a Pi, and a base that is not periodic -- unless
--momentum-zero-mode project (or the deck's momentum_zero_mode = project) is
given: on a periodic one-level base the mean of every right-hand side and
solution of the momentum solve is then removed, and the means removed from
S_i (the net momentum density the torus cannot carry) are printed per
iteration and put in the JSON summary.

With --reflux (or the deck's reflux = 1) every multi-level operator of the
solve adds the reflux term at the coarse-fine faces: the
composite operator is conservative, and a periodic hierarchy takes
--momentum-zero-mode project.  --level-boxes gives the boxes of one finer
level explicitly (repeat it per level) instead of --max-level's tagging.  The
levels take the deck's is_periodic, as the base does.

With --regrid-periodic (or the deck's regrid_periodic = 1) --max-level's
tagging and proper nesting go through the wrap of a periodic base (DESIGN.md
3m): a periodic hierarchy has to be nested through the wrap, which the
tagging does not see to without it.  It has no effect on a base that is not
periodic.

With --adm "n1 n2 ..." (or the deck's adm_half_widths) the ADM mass, momentum
and spin of the solved data (mg_ic_code_amd/adm.py) are reported
after the loop on the cubes of those half-widths (level-0 cells): one line per
surface, then the totals the puncture table asks for.  Not on a periodic deck.

With --puncture-masses (or the deck's puncture_masses = 1) psi at every
puncture and the ADM mass it gives, M_i = 2 m_i (psi(x_i) + sum m_j / d_ij)
(mg_ic_code_amd/sample.py), are reported after the loop: one line
per puncture, with the level and the stencil psi was sampled on.

With --target-masses "T1 T2 ..." (or the deck's target_masses) the bare masses
are iterated, one full solve per step on the same grids, until the punctures
have those ADM masses (sample.solve_for_masses); one line per solve.  It
implies --puncture-masses; everything reported is the last solve's.

With --lineout "x0 y0 z0 x1 y1 z1 n" the solved psi is sampled at n points
from (x0, y0, z0) to (x1, y1, z1), both included: "lineout s value level order"
per point, s the arc length.

With --horizon "cx cy cz r0" (repeatable; or the deck's num_horizons, horizon1
...) the apparent horizon about (cx, cy, cz) is looked for in the solved data
from the sphere of radius r0 (mg_ic_code_amd/horizon.py);
--horizons-at-punctures (or the deck's horizons = punctures) looks about every
puncture of the table from r0 = m_i.  Per surface: its status, and when found
its radii, area, irreducible mass and the punctures it encloses; with
--puncture-masses also M_irr next to M_i.  Not on a periodic deck.

usage: python tools/run_poisson.py [params.txt] [--size N] [--boxes-per-rank x,y,z]
                                   [--max-level K] [--phi gaussian|sine]
                                   [--puncture "m x y z Px Py Pz Jx Jy Jz"]...
                                   [--potential "V0 mass lambda"] [--pi VALUE]
                                   [--constraints] [--momentum]
                                   [--momentum-zero-mode refuse|project] [--reflux]
                                   [--level-boxes "lo0 lo1 lo2 hi0 hi1 hi2; ..."]...
                                   [--regrid-periodic] [--adm "n1 n2 ..."]
                                   [--puncture-masses] [--target-masses "T1 T2 ..."]
                                   [--lineout "x0 y0 z0 x1 y1 z1 n"]
                                   [--horizon "cx cy cz r0"]... [--horizons-at-punctures]
                                   [--cttk] [--cttk-tol TOL] [--cttk-max-iter N] [--hybrid-K]

With --cttk (or the deck's cttk = 1) a periodic one-level deck without holes is
closed by the CTTK method (mg_ic_code_amd/cttk.py) in place of poisson_solve:
psi = 1, K varies in space.  The momentum solves and max|K - K_prev| of every
pass, K's range and, with --constraints, the corrected constraint norms are
printed, and the JSON line carries them under the key "cttk".

With --hybrid-K (or the deck's hybrid_K = 1) a deck that is not periodic, holes
or none, is solved by the hybrid CTTK method (mg_ic_code_amd/khyb.py): K varies
in space so that the matter's energy drops out of the psi equation, and the
momentum solve carries its gradient.  It implies --momentum.  max|K| and, with
--constraints, the corrected constraint norms are printed, and the JSON line
carries them under the key "hybrid_K".
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run_cttk(args, prm, levels, matter, phi0, n, nboxes):
    """--cttk (or the deck's cttk = 1): cttk_solve in place of poisson_solve."""
    import mg_ic_code_amd as mg
    t0 = time.perf_counter()
    res = mg.cttk_solve(levels, prm, matter=matter, phi0=phi0, tol=args.cttk_tol,
                        max_iterations=args.cttk_max_iter, constraints=args.constraints,
                        max_depth=args.max_depth)
    mg.device_synchronize()
    dt = time.perf_counter() - t0
    for i, its in enumerate(res.momentum_iterations):
        print(f"CTTK pass {i + 1}: momentum solves V1 V2 V3 U: "
              + " ".join(str(v) for v in its) + " BiCGStab iterations; removed means of S1 S2 S3: "
              + " ".join(f"{m:.16e}" for m in res.momentum_net[i]))
    for i, s in enumerate(res.k_steps):
        print(f"CTTK pass {i + 1}: max|K - K_prev| = {s:.16e}")
    print(f"CTTK K: max|K| = {res.k_max:.16e} mean = {res.k_mean:.16e}; "
          f"{res.iterations} passes, converged {res.converged}")
    if args.constraints:
        for line in res.constraints.lines():
            print(line)
    out = {"n": n, "boxes": nboxes, "converged": res.converged, "seconds": round(dt, 3),
           "cttk": {"iterations": res.iterations, "k_steps": res.k_steps, "k_max": res.k_max,
                    "k_mean": res.k_mean},
           "momentum_iterations": res.momentum_iterations, "momentum_net": res.momentum_net,
           "momentum_net_relative": res.momentum_net_relative}
    if args.constraints:
        out["cttk"]["max_norm"] = res.constraints.max_norm
        out["cttk"]["relative_ham"] = res.constraints.relative_ham
    print(json.dumps(out))


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
    ap.add_argument("--potential", default=None, metavar="\"V0 MASS LAMBDA\"",
                    help="the scalar potential's three coefficients; overrides the deck's")
    ap.add_argument("--pi", type=float, default=None, metavar="VALUE",
                    help="a constant field velocity Pi; overrides the deck's pi_amplitude")
    ap.add_argument("--constraints", action="store_true",
                    help="report the constraint norms of the solved data")
    ap.add_argument("--momentum", action="store_true",
                    help="solve the momentum constraint for the matter's Pi d_i phi source")
    ap.add_argument("--momentum-zero-mode", choices=("refuse", "project"), default=None,
                    help="the momentum solve on a periodic base: refuse it, or project the zero "
                         "mode out (default: the deck's momentum_zero_mode)")
    ap.add_argument("--reflux", action="store_true",
                    help="add the reflux term at coarse-fine faces (default: the deck's reflux)")
    ap.add_argument("--level-boxes", action="append", default=None, metavar="BOXES",
                    help="the boxes of the next finer level, \"lo0 lo1 lo2 hi0 hi1 hi2; ...\" in "
                         "that level's index space; repeatable, coarsest first; instead of "
                         "--max-level")
    ap.add_argument("--regrid-periodic", action="store_true",
                    help="--max-level's tags and nesting go through the wrap of a periodic base "
                         "(default: the deck's regrid_periodic)")
    ap.add_argument("--adm", default=None, metavar="\"N1 N2 ...\"",
                    help="report the ADM mass, momentum and spin on the cubes of these "
                         "half-widths in level-0 cells (default: the deck's adm_half_widths)")
    ap.add_argument("--puncture-masses", action="store_true",
                    help="report psi at the punctures and their ADM masses (default: the deck's "
                         "puncture_masses)")
    ap.add_argument("--target-masses", default=None, metavar="\"T1 T2 ...\"",
                    help="iterate the bare masses until the punctures have these ADM masses "
                         "(default: the deck's target_masses); implies --puncture-masses")
    ap.add_argument("--lineout", default=None, metavar="\"X0 Y0 Z0 X1 Y1 Z1 N\"",
                    help="sample the solved psi at N points from (X0, Y0, Z0) to (X1, Y1, Z1)")
    ap.add_argument("--horizon", action="append", default=None, metavar="\"CX CY CZ R0\"",
                    help="look for the apparent horizon about (CX, CY, CZ) from the sphere of "
                         "radius R0; repeatable; overrides the deck's")
    ap.add_argument("--horizons-at-punctures", action="store_true",
                    help="look for a horizon about every puncture, from r0 = its bare mass")
    ap.add_argument("--cttk", action="store_true",
                    help="close the constraints of a periodic one-level deck by the CTTK method: "
                         "psi = 1, K varies in space (default: the deck's cttk)")
    ap.add_argument("--cttk-tol", type=float, default=None, metavar="TOL",
                    help="the CTTK loop stops at max|K - K_prev| <= TOL max|K| (default: the "
                         "deck's cttk_tolerance)")
    ap.add_argument("--cttk-max-iter", type=int, default=None, metavar="N",
                    help="the momentum passes the CTTK loop may take (default: the deck's "
                         "cttk_max_iterations)")
    ap.add_argument("--hybrid-K", dest="hybrid_K", action="store_true",
                    help="solve a deck that is not periodic by the hybrid CTTK method: K(x) from "
                         "the matter's energy (default: the deck's hybrid_K); implies --momentum")
    args = ap.parse_args()
    if args.horizon and args.horizons_at_punctures:
        ap.error("--horizon and --horizons-at-punctures exclude each other")
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
    from mg_ic_code_amd.matter import Matter, PiProfile, ScalarPotential
    matter = Matter.from_params(prm)
    if args.potential is not None or args.pi is not None:
        pot = matter.potential if matter is not None else ScalarPotential()
        pi = matter.pi if matter is not None else None
        if args.potential is not None:
            coefs = args.potential.split()
            if len(coefs) != 3:
                ap.error("--potential needs three numbers: V0 mass lambda")
            pot = ScalarPotential(*coefs)
        if args.pi is not None:
            pi = PiProfile.constant(args.pi)
        matter = Matter(pot, pi)
    if matter is not None:
        print(f"matter: {matter.potential}, Pi {matter.pi.value if matter.pi else 0.0!r}")
    if args.max_level > 0:
        from mg_ic_code_amd.grids import set_grids
        levels = set_grids(grid.comm, prm, grid, max_level=args.max_level, phi0=phi0,
                           punctures=punct, matter=matter,
                           periodic_regrid=True if args.regrid_periodic else None)
        for lev, g in enumerate(levels):
            cells = sum((b[3] - b[0] + 1) * (b[4] - b[1] + 1) * (b[5] - b[2] + 1) for b in g.boxes)
            print(f"level {lev}: {len(g.boxes)} boxes, {cells} cells")
    if args.level_boxes:
        if args.max_level > 0:
            ap.error("--level-boxes and --max-level exclude each other")
        levels, ldom, ldx = [grid], dom, grid.dx
        for spec in args.level_boxes:
            lboxes = [tuple(int(v) for v in b.split()) for b in spec.split(";") if b.strip()]
            if not lboxes or any(len(b) != 6 for b in lboxes):
                ap.error("--level-boxes needs six integers per box")
            ldom = tuple(2 * v if i < 3 else 2 * v + 1 for i, v in enumerate(ldom))
            ldx /= 2
            levels.append(mg.Grid(grid.comm, ldom, lboxes, ldx,
                                  periodic=(1, 1, 1) if prm.is_periodic else (0, 0, 0),
                                  patches=True))
    if args.cttk or prm.cttk:
        return run_cttk(args, prm, levels, matter, phi0, n, len(boxes))
    from mg_ic_code_amd import sample
    lineout_spec =sample.parse_lineout(args.lineout) if args.lineout is not None else None
    targets = args.target_masses if args.target_masses is not None else prm.target_masses
    kwargs = dict(max_depth=args.max_depth, phi0=phi0, matter=matter,
                  constraints=args.constraints, momentum=True if args.momentum else None,
                  zero_mode=args.momentum_zero_mode, reflux=True if args.reflux else None,
                  adm=args.adm,
                  horizons="punctures" if args.horizons_at_punctures else args.horizon,
                  hybrid_K=True if args.hybrid_K else None)
    t0 = time.perf_counter()
    msolve = None
    if targets is not None:
        msolve = sample.solve_for_masses(levels, prm, targets, punctures=punct, **kwargs)
        res, punct = msolve.result, msolve.punctures
    else:
        res = poisson_solve(levels, prm, punctures=punct,
                            puncture_masses=True if args.puncture_masses else None, **kwargs)
    mg.device_synchronize()
    dt = time.perf_counter() - t0
    for i, (nrm, it) in enumerate(zip(res.dpsi_norms, res.linear_iterations)):
        print(f"Main Loop Iteration {i + 1}: {it} BiCGStab iterations, norm of dpsi {nrm:.6e}")
    for i, its in enumerate(res.momentum_iterations):
        print(f"Main Loop Iteration {i + 1}: momentum solves V1 V2 V3 U: "
              + " ".join(str(v) for v in its) + " BiCGStab iterations"
              + ("; removed means of S1 S2 S3: "
                 + " ".join(f"{m:.16e}" for m in res.momentum_net[i])
                 if res.momentum_net else ""))
    if res.K is not None:
        print(f"hybrid K: max|K| = {res.k_max:.16e}")
    if args.constraints:
        for line in res.constraints.lines():
            print(line)
    if res.adm is not None:
        for line in res.adm.lines():
            print(line)
    if msolve is not None:
        for text in msolve.lines():
            print(text)
    if res.puncture_masses is not None:
        for text in res.puncture_masses.lines():
            print(text)
    if res.horizons is not None:
        from mg_ic_code_amd.horizon import horizon_lines
        for text in horizon_lines(res.horizons, res.puncture_masses):
            print(text)
    if lineout_spec is not None:
        for text in sample.lineout(res.psi, *lineout_spec).lines():
            print(text)
    out = {"n": n, "boxes": len(boxes), "nl_iterations": len(res.dpsi_norms),
           "converged": res.converged, "seconds": round(dt, 3)}
    if punct is not None:
        out["punctures"] = [list(p.row()) for p in punct]
    if res.puncture_masses is not None:
        out["puncture_masses"] = res.puncture_masses.adm_masses
    if res.horizons is not None:
        out["horizons"] = [h.summary() for h in res.horizons]
    if msolve is not None:
        out["mass_solves"] = len(msolve.history)
        out["mass_solve_converged"] = msolve.converged
    if matter is not None:
        p = matter.potential
        out["matter"] = {"V0": p.V0, "mass": p.mass, "self_coupling": p.self_coupling,
                         "pi": matter.pi.value if matter.pi else 0.0}
        out["dpsi_norms"] = res.dpsi_norms
        out["linear_iterations"] = res.linear_iterations
        out["constant_K"] = res.constant_K
    if res.momentum is not None:
        out["momentum_iterations"] = res.momentum_iterations
    if res.K is not None:
        out["hybrid_K"] = {"k_max": res.k_max}
        if args.constraints:
            out["hybrid_K"]["max_norm"] = res.constraints.max_norm
            out["hybrid_K"]["relative_ham"] = res.constraints.relative_ham
    if res.momentum_net:
        out["momentum_net"] = res.momentum_net
        out["momentum_net_relative"] = res.momentum_net_relative
    print(json.dumps(out))


if __name__ == "__main__":
    main()
