"""Worker for test_fused_residual.py: one case in a fresh interpreter, so that
MGIC_FUSED_RES, MGIC_TB2_TRIM and MGIC_TB2_KC (read once per process) take
the values the test sets.

    python tests/fused_res_worker.py CASE

A V-cycle case runs K = 4 pipelined iterations() on one hierarchy and checks,
bit for bit: K iteration() calls on a second, identically built hierarchy
(phi, resid, every norm), the oracle's iteration(0) (phi, norms), and the
launch ledger -- the k_residual_zl<true, double, ...> count rises by 1 over
the K iterations when the residuals are formed inside the next V-cycle's
first launch, by K when they are not (MGIC_FUSED_RES=0, or a case the fused
form does not apply to).  The precondition case runs the two-iteration
preconditioner.  Prints "digest <sha256 of the results>" -- the test compares
it between MGIC_FUSED_RES unset and 0 -- and "fused res worker OK".
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import mg_ic_code_amd as mg  # noqa: E402
import oracle  # noqa: E402

K = 4
# shape (nx, ny, nz), depths, alpha, beta, (bc_lo, bc_hi, bc_value), fusible
CASES = {
    # 3 x 3 tiles of 64 x 22 (interior, x-, y- and corner-face classes, ragged
    # last tiles), three 4-plane z chunks
    "ragged": ((136, 52, 12), 2, 1.0, -1.0, ((0, 0, 0), (0, 0, 0), 0.0), True),
    # the general constants (no alpha = 1, beta = -1 specialisation)
    "general": ((136, 52, 12), 2, 0.75, -1.3, ((0, 0, 0), (0, 0, 0), 0.0), True),
    # one tile column, 3 depths
    "cube": ((64, 64, 64), 3, 1.0, -1.0, ((0, 0, 0), (0, 0, 0), 0.0), True),
    # Dirichlet 0.375 / Neumann faces: the residual's ghost rules are not the
    # correction's, so the residual launches stay
    "mixed": ((72, 20, 28), 2, 1.0, -1.0, ((0, 1, 0), (1, 0, 0), 0.375), False),
    "precond": ((136, 52, 12), 2, 1.0, -1.0, ((0, 0, 0), (0, 0, 0), 0.0), True),
}
CASES["steady"] = CASES["cube"]  # run with MGIC_TB2_KC=32: chunks with steady-state steps


def residual_launches():
    return sum(v for k, v in mg.launch_ledger().items()
               if k.startswith("k_residual_zl<true, double,") and "#" not in k)


def build(comm, shape, depths, alpha, beta, bc, a, rhs):
    nx, ny, nz = shape
    dom = (0, 0, 0, nx - 1, ny - 1, nz - 1)
    dx = 100.0 / nx
    grid = mg.Grid(comm, dom, [dom], dx)
    fa, fb, frhs, fphi, fres = (mg.LevelData(grid) for _ in range(5))
    fa.upload(0, a)
    fb.set_val(1.0)
    frhs.upload(0, rhs)
    fphi.set_zero()
    prm = mg.OperatorParams(alpha=alpha, beta=beta, bc_lo=bc[0], bc_hi=bc[1], bc_value=bc[2],
                            fused_smoother=2)
    fac = mg.defineOperatorFactory(grid, fa, fb, prm)
    amg = mg.AMRMultiGrid(fac, mg.SolverParams(max_depth=depths - 1, bottom_solver=0))
    assert amg.num_depths == depths
    return dict(dom=dom, dx=dx, grid=grid, fa=fa, fb=fb, frhs=frhs, fphi=fphi, fres=fres, fac=fac,
                amg=amg)


def vcycle_case(comm, rng, name):
    shape, depths, alpha, beta, bc, fusible = CASES[name]
    nx, ny, nz = shape
    a = rng.uniform(-2.0, -0.5, (nz, ny, nx))
    rhs = rng.uniform(-1, 1, (nz, ny, nx))
    fused = fusible and os.environ.get("MGIC_FUSED_RES", "1") != "0"

    A = build(comm, shape, depths, alpha, beta, bc, a, rhs)
    A["amg"].init_residual(A["fphi"], A["frhs"], A["fres"])
    before = residual_launches()
    got = A["amg"].iterations(A["fphi"], A["frhs"], A["fres"], K, norm_type=0)
    rose = residual_launches() - before
    print(f"{name}: residual launches over {K} iterations: {rose}", flush=True)
    assert rose == (1 if fused else K), (rose, fused)
    phi, res = A["fphi"].download(0), A["fres"].download(0)

    B = build(comm, shape, depths, alpha, beta, bc, a, rhs)
    B["amg"].init_residual(B["fphi"], B["frhs"], B["fres"])
    want = [B["amg"].iteration(B["fphi"], B["frhs"], B["fres"], norm_type=0) for _ in range(K)]
    assert got == want, (got, want)
    for what, g, w in (("phi", phi, B["fphi"].download(0)), ("resid", res, B["fres"].download(0))):
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            print(what, "differs at", len(bad), "cells, e.g. (k, j, i)", bad[:8].tolist(),
                  "max |diff|", float(np.abs(g - w).max()), flush=True)
        assert np.array_equal(g, w), what

    o = oracle.OracleMG([A["dom"]], A["dom"], A["dx"], alpha=alpha, beta=beta, bc_lo=bc[0],
                        bc_hi=bc[1], bc_value=bc[2], nlevels=depths, bottom_solver=0)
    o.set(0, oracle.ACOEF, 0, a)
    o.set(0, oracle.BCOEF, 0, np.ones_like(a))
    o.set(0, oracle.RHS, 0, rhs)
    o.setup()
    o.init_residual(0)
    ref = [o.iteration(0) for _ in range(K)]
    assert got == ref, (got, ref)
    assert np.array_equal(phi, o.get(0, oracle.PHI, 0))
    return [phi, res, np.array(got)]


def precond_case(comm, rng, name):
    shape, depths, alpha, beta, bc, fusible = CASES[name]
    nx, ny, nz = shape
    a = rng.uniform(-2.0, -0.5, (nz, ny, nx))
    r = rng.uniform(-1, 1, (nz, ny, nx))
    fused = os.environ.get("MGIC_FUSED_RES", "1") != "0"
    A = build(comm, shape, depths, alpha, beta, bc, a, r)
    fe = mg.LevelData(A["grid"])
    before = residual_launches()
    mg.MultilevelLinearOp(A["amg"], 2).preCond(fe, A["frhs"])
    rose = residual_launches() - before
    print(f"{name}: residual launches in precondition(e, r, 2): {rose}", flush=True)
    assert rose == (0 if fused else 1), (rose, fused)
    return [fe.download(0)]


def main():
    name = sys.argv[1]
    comm = mg.Comm()
    rng = np.random.default_rng(20261020)
    out = (precond_case if name == "precond" else vcycle_case)(comm, rng, name)
    comm.synchronize()
    h = hashlib.sha256()
    for x in out:
        h.update(np.ascontiguousarray(x).tobytes())
    print("digest", h.hexdigest(), flush=True)
    print("fused res worker OK", flush=True)


if __name__ == "__main__":
    main()
