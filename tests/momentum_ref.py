"""Reference side of the momentum-solve tests (tests/test_momentum.py): the
conformal transverse-traceless step of mg_ic_code_amd/momentum.py restated in
numpy on top of tests/constraints_ref.py, tests/matter_ref.py and
tests/puncture_ref.py.  Test infrastructure only.

    D_d f   = 0.5/dx * (f(+e_d) - f(-e_d))
    div_rhs = -0.25 * (D_x V_x + D_y V_y + D_z V_z)
    W_i     = V_i + D_i U
    d[a][b] = D_a W_b,  div = d[0][0] + d[1][1] + d[2][2]
    LW_ii   = 2.0 * d[i][i] - (2.0/3.0) * div,   LW_ij = d[i][j] + d[j][i]
    ghost   = 2.0 * f(face cell) - f(next cell in)       (domain faces only)
    S_i     = -(divA^BY_i + psi_0**6.0 * (8.0*pi*G * Pi * dphi_i))

each evaluated left to right: only + - x and the one division 0.5/dx, so in
this association numpy gives the kernels' bits.  The consumers take the total
tensor Abar^BY_ij + abar_ij wherever the restatements they are built on take
the Bowen-York one.  Arrays are (nz, ny, nx), i fastest; a `_g` array covers
the box grown by one; the six components are in puncture_ref.IJ's order (11,
12, 13, 22, 23, 33).
"""
import contextlib

import numpy as np

from tests import constraints_ref as C
from tests import matter_ref as M
from tests import phi_ref
from tests import puncture_ref as P


def cdiff(f_g, d, dx):
    """D_d of an array over the box grown by one -> over the box (d = 0: x)."""
    return 0.5 / dx * (C._shift(f_g, d, +1) - C._shift(f_g, d, -1))


def valid(f_g):
    return f_g[1:-1, 1:-1, 1:-1]


def div_rhs(V_g, dx):
    """k_ctt_div_rhs"""
    return -0.25 * (cdiff(V_g[0], 0, dx) + cdiff(V_g[1], 1, dx) + cdiff(V_g[2], 2, dx))


def w(V, U_g, dx):
    """k_ctt_w: V over the box, U over the box grown by one"""
    return [V[i] + cdiff(U_g, i, dx) for i in range(3)]


def lw(W_g, dx):
    """k_ctt_lw: the six LW_ij over the box from W over the box grown by one"""
    d = [[cdiff(W_g[b], a, dx) for b in range(3)] for a in range(3)]
    div = d[0][0] + d[1][1] + d[2][2]
    third = (2.0 / 3.0) * div
    return [2.0 * d[0][0] - third, d[0][1] + d[1][0], d[0][2] + d[2][0],
            2.0 * d[1][1] - third, d[1][2] + d[2][1], 2.0 * d[2][2] - third]


def extrap(f_g, box, domain):
    """k_ctt_extrap: a copy of f_g (over `box` grown by one) with ghost layer 1
    across every face of the box that is a face of `domain` extrapolated;
    faces only, everything else as it was."""
    out = f_g.copy()
    inner = [slice(1, -1)] * 3
    for d in range(3):
        ax = 2 - d
        for side, on_domain in ((0, box[d] == domain[d]), (1, box[3 + d] == domain[3 + d])):
            if not on_domain:
                continue
            g, c, n = (0, 1, 2) if side == 0 else (-1, -2, -3)
            sg, sc, sn = list(inner), list(inner), list(inner)
            sg[ax], sc[ax], sn[ax] = g, c, n
            out[tuple(sg)] = 2.0 * f_g[tuple(sc)] - f_g[tuple(sn)]
    return out


def pad_extrap(f):
    """f over a box that is the whole domain -> over the box grown by one,
    faces extrapolated (edges and corners zero: nothing reads them)."""
    n = f.shape
    box = (0, 0, 0, n[2] - 1, n[1] - 1, n[0] - 1)
    return extrap(np.pad(f, 1), box, box)


def pad_dirichlet(u):
    """u over the whole domain -> grown by one with the homogeneous Dirichlet
    ghost of the operator (ghost = -near)."""
    g = np.pad(u, 1)
    for ax in range(3):
        lo, lo1, hi, hi1 = ([slice(None)] * 3 for _ in range(4))
        lo[ax], lo1[ax], hi[ax], hi1[ax] = 0, 1, -1, -2
        g[tuple(lo)] = -g[tuple(lo1)]
        g[tuple(hi)] = -g[tuple(hi1)]
    return g


# ---- the consumers: the total tensor in the restatements of the generators
def total_tensor(bh, table, lo, hi, dx, abar):
    """(A, psi_bh) over [lo, hi]: puncture_ref.bowen_york's dict with abar[c]
    (arrays over the same box) added to component IJ[c]."""
    A, psi_bh = P.bowen_york(C._table(bh, table), bh["domain_length"], lo, hi, dx)
    return {ij: A[ij] + abar[c] for c, ij in enumerate(P.IJ)}, psi_bh


@contextlib.contextmanager
def _total_in(abar):
    """matter_ref's and constraints_ref's A2 from the total tensor (abar over
    the valid box of the call)."""
    saved = M._holes

    def holes(bh, table, lo, hi, dx):
        A, psi_bh = total_tensor(bh, table, lo, hi, dx, abar)
        return P.contract(A), psi_bh

    M._holes = holes
    try:
        yield
    finally:
        M._holes = saved


def nl_coefs(bh, lo, hi, dx, psi_g, phi_g, pot, pi, abar, table=None):
    """matter_ref.nl_coefs with A2 of the total tensor."""
    with _total_in(abar):
        return M.nl_coefs(bh, lo, hi, dx, psi_g, phi_g, pot, pi, table)


def nl_integrand(bh, lo, hi, dx, psi_g, phi_g, pot, pi, abar, table=None):
    with _total_in(abar):
        return M.nl_integrand(bh, lo, hi, dx, psi_g, phi_g, pot, pi, table)


def momentum(bh, lo, hi, dx, psi, phi_g, pot, pi, abar_g, table=None):
    """constraints_ref.momentum (float64) with the total tensor: abar_g the six
    stored components over the box grown by one (None: the Bowen-York tensor
    alone).  Returns (Mom, scale, divA, src): three arrays each."""
    L, G = bh["domain_length"], bh["G_Newton"]
    glo, ghi = tuple(v - 1 for v in lo), tuple(v + 1 for v in hi)
    A, psi_bh = P.bowen_york(C._table(bh, table), L, glo, ghi, dx)
    if abar_g is not None:
        A = {ij: A[ij] + abar_g[c] for c, ij in enumerate(P.IJ)}
    psi_0 = psi + psi_bh[1:-1, 1:-1, 1:-1]
    wgt = psi_0 ** -6.0
    h = 0.5 / dx
    mom, scale, divs, srcs = [], [], [], []
    for i in range(3):
        div = np.zeros(psi_0.shape)
        mag = np.zeros(psi_0.shape)
        for j in range(3):
            Ap, Am = C._shift(A[C._KEY[i, j]], j, +1), C._shift(A[C._KEY[i, j]], j, -1)
            div = div + h * (Ap - Am)
            mag = mag + h * (np.abs(Ap) + np.abs(Am))
        dphi = h * (C._shift(phi_g, i, +1) - C._shift(phi_g, i, -1))
        src = 8.0 * np.pi * G * pi * dphi
        mom.append(wgt * div + src)
        scale.append(wgt * mag + np.abs(src))
        divs.append(div)
        srcs.append(src)
    return mom, scale, divs, srcs


def source(bh, lo, hi, dx, psi, phi_g, pot, pi, table=None):
    """(S, scale): S_i = -(divA_i + psi_0**6.0 * src_i) and the cell's sum of
    absolute terms psi_0^6 times that of Mom_i."""
    _, psi_bh = P.bowen_york(C._table(bh, table), bh["domain_length"], lo, hi, dx)
    p6 = (psi + psi_bh) ** 6.0
    _, scale, divs, srcs = momentum(bh, lo, hi, dx, psi, phi_g, pot, pi, None, table)
    return [-(d + p6 * s) for d, s in zip(divs, srcs)], [p6 * s for s in scale]


def constraints(bh, lo, hi, dx, psi_g, phi_g, pot, pi, abar_g, table=None):
    """constraints_ref.constraints with the total tensor."""
    with _total_in([valid(a) for a in abar_g]):
        ham, ham_abs = C.hamiltonian(bh, lo, hi, dx, psi_g, phi_g, pot, pi, table)
    mom, scale, _, _ = momentum(bh, lo, hi, dx, valid(psi_g), phi_g, pot, pi, abar_g, table)
    return dict(ham=ham, ham_abs=ham_abs, mom=mom, scale=scale)


# ---- the coupled loop on one Dirichlet box: the oracle's NL loop with the
# momentum step in front of every set_a_coef / set_rhs
def solve_dirichlet(s, dx):
    """Lap u = s on a cubic box with the operator's homogeneous Dirichlet
    ghost (ghost = -near): the 7-point Laplacian inverted exactly (DST-II)."""
    from scipy.fft import dstn, idstn
    lam = [(2.0 * np.cos(np.pi * np.arange(1, n + 1) / n) - 2.0) / dx ** 2 for n in s.shape]
    ev = lam[0][:, None, None] + lam[1][None, :, None] + lam[2][None, None, :]
    return idstn(dstn(s, type=2) / ev, type=2)


def momentum_step(bh, lo, hi, dx, psi_g, phi_g, pot, pi, table=None):
    """Steps 2-5 of an NL iteration on one box that is the whole domain:
    (V, U, W, LW_g), LW_g the six components with their extrapolated ghosts."""
    S, _ = source(bh, lo, hi, dx, valid(psi_g), phi_g, pot, pi, table)
    V = [solve_dirichlet(s, dx) for s in S]
    U = solve_dirichlet(div_rhs([pad_dirichlet(v) for v in V], dx), dx)
    W = w(V, pad_dirichlet(U), dx)
    LW = lw([pad_extrap(x) for x in W], dx)
    return V, U, W, [pad_extrap(x) for x in LW]


def coupled_solve(prm, n, max_depth, phi_g, pot, pi, momentum_on=True, table=None):
    """The oracle's NL loop (phi_ref.oracle_poisson_solve_phi) on one Dirichlet
    n^3 box with the matter, and with momentum_on the momentum step before
    every coefficient evaluation.  Returns dict(psi_g, norms, mom, ham, ham_abs,
    LW_g): the constraints of the final psi with the final total tensor."""
    lo, hi, dx = (0, 0, 0), (n - 1,) * 3, prm.domainLength[0] / n
    state = {}

    def coefs(bh, lo_, hi_, dx_, psi_g, phi_g_):
        if psi_g is None:
            psi_g = np.ones((n + 2,) * 3)
        if not momentum_on:
            return M.nl_coefs(bh, lo_, hi_, dx_, psi_g, phi_g_, pot, pi, table)
        state["LW_g"] = momentum_step(bh, lo_, hi_, dx_, psi_g, phi_g_, pot, pi, table)[3]
        return nl_coefs(bh, lo_, hi_, dx_, psi_g, phi_g_, pot, pi,
                        [valid(a) for a in state["LW_g"]], table)

    saved = phi_ref.nl_coefs_phi
    phi_ref.nl_coefs_phi = coefs
    try:
        psi_g, norms, _, _ = phi_ref.oracle_poisson_solve_phi(prm, n, max_depth,
                                                              prm.max_NL_iterations, phi_g)
    finally:
        phi_ref.nl_coefs_phi = saved
    bh = prm.bh(constant_K=0.0)
    zeros = [np.zeros((n + 2,) * 3) for _ in range(6)]
    LW_g = state.get("LW_g", zeros)
    out = constraints(bh, lo, hi, dx, psi_g, phi_g, pot, pi, LW_g, table)
    out.update(psi_g=psi_g, norms=norms, LW_g=LW_g)
    return out
