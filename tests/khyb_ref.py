"""Reference side of the hybrid CTTK tests (tests/test_khyb.py): the kernel of
libmgic_khyb.so restated literally in numpy (include/mgic_khyb.h gives every
expression with its order), and the hybrid coupled loop of
mg_ic_code_amd/nl.py (poisson_solve(hybrid_K=True)) on one Dirichlet box that
is the whole domain, on top of tests/momentum_ref.py (exact DST solves, the
oracle's NL loop), tests/matter_ref.py (V, rho) and tests/cttk_ref.py (the
source and constraint kernels of libmgic_cttk.so).  Test infrastructure only.

Arrays are (nz, ny, nx), i fastest; a `_g` array covers the box grown by one.
"""
import numpy as np

from tests import cttk_ref as CK
from tests import matter_ref as M
from tests import momentum_ref as R
from tests import phi_ref


def m16(phi, pi, pot, G):
    """16 pi G rho in the order of matter_ref.m_value; pi None: Pi = 0."""
    rho = M.rho(pot, 0.0 if pi is None else pi, phi)
    return 16.0 * np.pi * G * rho


def kernel_K(phi, pi, pot, G):
    """k_khyb_K: (K, bad) over the valid cells; pi None: Pi = 0."""
    v = 1.5 * m16(phi, pi, pot, G)
    ok = v >= 0.0
    with np.errstate(invalid="ignore"):
        K = np.where(ok, -np.sqrt(np.where(ok, v, 0.0)), 0.0)
    return K, int(np.count_nonzero(~ok))


def momentum_step(bh, lo, hi, dx, psi_g, phi_g, pot, pi, K_g, table=None):
    """momentum_ref.momentum_step with (2/3) psi^6 D_i K added to S_i (K_g
    None: left out): the six LW_ij with their extrapolated ghosts."""
    psi = R.valid(psi_g)
    S, _ = R.source(bh, lo, hi, dx, psi, phi_g, pot, pi, table)
    if K_g is not None:
        S = CK.kernel_source(psi, K_g, S, dx)
    V = [R.solve_dirichlet(s, dx) for s in S]
    U = R.solve_dirichlet(R.div_rhs([R.pad_dirichlet(v) for v in V], dx), dx)
    W = R.w(V, R.pad_dirichlet(U), dx)
    LW = R.lw([R.pad_extrap(x) for x in W], dx)
    return [R.pad_extrap(x) for x in LW]


def hybrid_solve(prm, n, max_depth, phi_g, pot, pi, source_term=True, table=None):
    """poisson_solve(hybrid_K=True) on one Dirichlet n^3 box: K from the
    matter once, then the oracle's NL loop with the momentum step (its source
    with the D_i K term; source_term False: without it) before every
    coefficient evaluation, the coefficients with a zero potential, no Pi and
    constant_K = 0.  Returns dict(psi_g, norms, iters, K, K_g, LW_g, ham,
    ham_abs, mom): the constraints of the final psi and tensor with K's terms
    (always with the D_i K term: the report does not leave it out)."""
    lo, hi, dx = (0, 0, 0), (n - 1,) * 3, prm.domainLength[0] / n
    bh = prm.bh(constant_K=0.0)
    K, bad = kernel_K(R.valid(phi_g), pi, pot, bh["G_Newton"])
    assert bad == 0, bad
    K_g = R.pad_extrap(K)
    state = {}

    def coefs(bh_, lo_, hi_, dx_, psi_g, phi_g_):
        if psi_g is None:
            psi_g = np.ones((n + 2,) * 3)
        state["LW_g"] = momentum_step(bh_, lo_, hi_, dx_, psi_g, phi_g_, pot, pi,
                                      K_g if source_term else None, table)
        return R.nl_coefs(bh_, lo_, hi_, dx_, psi_g, phi_g_, (0.0, 0.0, 0.0), 0.0,
                          [R.valid(a) for a in state["LW_g"]], table)

    saved = phi_ref.nl_coefs_phi
    phi_ref.nl_coefs_phi = coefs
    try:
        psi_g, norms, iters, _ = phi_ref.oracle_poisson_solve_phi(prm, n, max_depth,
                                                                  prm.max_NL_iterations, phi_g)
    finally:
        phi_ref.nl_coefs_phi = saved
    out = R.constraints(bh, lo, hi, dx, psi_g, phi_g, pot, pi, state["LW_g"], table)
    ham, mom, ham_abs = CK.kernel_constraints(K_g, out["ham"], out["mom"], out["ham_abs"], dx)
    return dict(psi_g=psi_g, norms=norms, iters=iters, K=K, K_g=K_g, LW_g=state["LW_g"], ham=ham,
                ham_abs=ham_abs, mom=mom)
