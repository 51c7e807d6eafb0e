"""Reference side of the constraint tests (tests/test_constraints.py): the
Hamiltonian and momentum constraints of mg_ic_code_amd/constraints.py restated
in numpy on top of tests/phi_ref.py, tests/puncture_ref.py and
tests/matter_ref.py.  Test infrastructure only.

    m       = (2.0/3.0)*(K*K) - 16.0*pi*G*rho
    t_A     = A2 * psi_0**-12.0
    t_grad  = 16.0*pi*G * rho_grad * psi_0**-4.0
    t_lap   = 8.0 * lap * psi_0**-5.0
    Ham     = m - t_A - t_grad - t_lap
    Ham_abs = |(2.0/3.0)*(K*K)| + |16.0*pi*G*rho| + |t_A| + |t_grad| + |t_lap|
    divA_i  = sum over j = 0, 1, 2 of 0.5/dx * (Abar_ij(iv + e_j) - Abar_ij(iv - e_j))
    dphi_i  = 0.5/dx * (phi_0(iv + e_i) - phi_0(iv - e_i))
    Mom_i   = psi_0**-6.0 * divA_i + 8.0*pi*G * Pi * dphi_i

each evaluated left to right.  Abar_ij at the neighbours is
puncture_ref.bowen_york on the box grown by one (the deck's two holes as
puncture_ref.deck_table: the same bits, pinned by tests/test_punctures.py).
`pot` None: no matter (rho = 0, the momentum source the literal zero), else
(V0, mass, lambda) with `pi` a scalar or an array over the valid cells.
`psi_g` / `phi_g` cover the box grown by one; arrays are (nz, ny, nx), i
fastest.
"""
import numpy as np

import oracle
from tests import matter_ref as M
from tests import puncture_ref as P

# A_ij of puncture_ref.bowen_york's dict for any (i, j)
_KEY = {(i, j): (min(i, j), max(i, j)) for i in range(3) for j in range(3)}


def _shift(a, axis_dir, s):
    """a over the box grown by one -> over the box, shifted by s cells along
    direction axis_dir (0: x, the last array axis)."""
    sl = [slice(1, -1)] * 3
    sl[2 - axis_dir] = slice(1 + s, a.shape[2 - axis_dir] - 1 + s)
    return a[tuple(sl)]


def _table(bh, table):
    return P.deck_table(bh) if table is None else P.as_table(table)


def bowen_york_as(dtype, table, L, lo, hi, dx):
    """puncture_ref.bowen_york with every operation in `dtype` (np.float64:
    its bits; np.longdouble: the same expressions in extended precision)."""
    ax = [(np.arange(lo[d], hi[d] + 1, dtype=np.float64).astype(dtype) + dtype(0.5)) * dtype(dx)
          - dtype(L) / dtype(2.0) for d in range(3)]
    shape = (ax[2].size, ax[1].size, ax[0].size)
    x, y, z = (np.broadcast_to(v, shape) for v in
               (ax[0].reshape(1, 1, -1), ax[1].reshape(1, -1, 1), ax[2].reshape(-1, 1, 1)))
    t = P.completed(table).astype(dtype)
    A, psi_bh = P._pair(x, y, z, t[0], t[1])
    for q in range(1, len(t) // 2):
        Aq, pq = P._pair(x, y, z, t[2 * q], t[2 * q + 1])
        A = {ij: A[ij] + Aq[ij] for ij in P.IJ}
        psi_bh = psi_bh + pq
    return A, psi_bh


def momentum(bh, lo, hi, dx, psi, phi_g, pot, pi, table=None, dtype=np.float64):
    """(Mom, scale): three arrays each over [lo, hi]; scale is the cell's sum
    of absolute terms, psi_0^-6 sum_j 0.5/dx (|A(+)| + |A(-)|) + |8 pi G Pi
    dphi_i|.  psi over the valid cells.  Everything is evaluated in `dtype`."""
    f = dtype
    L, G = bh["domain_length"], f(bh["G_Newton"])
    glo, ghi = tuple(v - 1 for v in lo), tuple(v + 1 for v in hi)
    if dtype is np.float64:
        A, psi_bh = P.bowen_york(_table(bh, table), L, glo, ghi, dx)
    else:
        A, psi_bh = bowen_york_as(dtype, _table(bh, table), L, glo, ghi, dx)
    psi_0 = np.asarray(psi, dtype=f) + psi_bh[1:-1, 1:-1, 1:-1]
    w = psi_0 ** f(-6.0)
    h = f(0.5) / f(dx)
    mom, scale = [], []
    for i in range(3):
        div = np.zeros(psi_0.shape, dtype=f)
        mag = np.zeros(psi_0.shape, dtype=f)
        for j in range(3):
            Ap, Am = _shift(A[_KEY[i, j]], j, +1), _shift(A[_KEY[i, j]], j, -1)
            div = div + h * (Ap - Am)
            mag = mag + h * (np.abs(Ap) + np.abs(Am))
        if pot is None:
            src = f(0.0)
        else:
            pg = np.asarray(phi_g, dtype=f)
            dphi = h * (_shift(pg, i, +1) - _shift(pg, i, -1))
            src = f(8.0) * f(np.pi) * G * np.asarray(pi, dtype=f) * dphi
        mom.append(w * div + src)
        scale.append(w * mag + np.abs(src))
    return mom, scale


def hamiltonian(bh, lo, hi, dx, psi_g, phi_g, pot, pi, table=None):
    """(Ham, Ham_abs) over [lo, hi] at K = bh['constant_K']."""
    G, K = bh["G_Newton"], bh["constant_K"]
    lap = oracle.getlaplacianpsif(psi_g, lo, hi, dx)
    rho_grad = oracle.getrhogradphif(phi_g, lo, hi, dx)
    A2, psi_bh = M._holes(bh, table, lo, hi, dx)
    if pot is None:
        rho = 0.5 * 0.0 * 0.0 + 0.0
    else:
        rho = M.rho(pot, pi, phi_g[1:-1, 1:-1, 1:-1])
    psi_0 = psi_g[1:-1, 1:-1, 1:-1] + psi_bh
    m_K, m_rho = (2.0 / 3.0) * (K * K), 16.0 * np.pi * G * rho
    m = m_K - m_rho
    t_A = A2 * psi_0 ** -12.0
    t_grad = 16.0 * np.pi * G * rho_grad * psi_0 ** -4.0
    t_lap = 8.0 * lap * psi_0 ** -5.0
    ham = m - t_A - t_grad - t_lap
    ham_abs = np.abs(m_K) + np.abs(m_rho) + np.abs(t_A) + np.abs(t_grad) + np.abs(t_lap)
    return ham, ham_abs + np.zeros_like(ham)


def constraints(bh, lo, hi, dx, psi_g, phi_g, pot, pi, table=None):
    """dict(ham, ham_abs, mom=[3], scale=[3]) over [lo, hi]."""
    ham, ham_abs = hamiltonian(bh, lo, hi, dx, psi_g, phi_g, pot, pi, table)
    mom, scale = momentum(bh, lo, hi, dx, psi_g[1:-1, 1:-1, 1:-1], phi_g, pot, pi, table)
    return dict(ham=ham, ham_abs=ham_abs, mom=mom, scale=scale)


def far_mask(table, L, lo, hi, dx, dist):
    """Cells of [lo, hi] at least `dist` from every puncture of the table."""
    from tests import phi_ref
    x, y, z = phi_ref.centres(lo, hi, dx, L, grow=0)
    ok = True
    for r in P.as_table(table):
        ok = ok & (np.sqrt((x - r[1]) ** 2 + (y - r[2]) ** 2 + (z - r[3]) ** 2) >= dist)
    return np.broadcast_to(ok, (z.size, y.size, x.size))


def l2(x, mask, dx):
    """sqrt(sum over the mask of x^2 dx^3)"""
    return float(np.sqrt(np.sum(x[mask] ** 2) * dx ** 3))
