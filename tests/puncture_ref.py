"""Reference side of the puncture-table tests (tests/test_punctures.py): the
pair semantics of mg_ic_code_amd/punctures.py restated in numpy on top of
get_Aij as tests/phi_ref.py writes it.  Test infrastructure only.

A table is an (n, 10) array of rows m, x, y, z, Px, Py, Pz, Jx, Jy, Jz,
positions relative to the domain centre.  It is taken in pairs (0, 1),
(2, 3), ...; one pair is get_Aij's two holes with l_a = loc - (x_a, y_a, z_a)
and psi_bh = m_a / r_a + m_b / r_b; A_ij and psi_bh are the sums over the
pairs in pair order, the first pair's value being the sum's first value.  An
odd count is completed by a row of m = P = J = 0 at the last puncture's
position.  Arrays are (nz, ny, nx), i fastest.
"""
import contextlib
import math

import numpy as np

import oracle
from tests import phi_ref, regrid_ref

IJ = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))  # A11 A12 A13 A22 A23 A33


def as_table(rows):
    t = np.asarray(rows, dtype=np.float64).reshape(-1, 10)
    assert 1 <= len(t) <= 8
    return t


def deck_table(bh):
    """The deck's two holes (the bh dict of BH_KEYS) as a table."""
    return as_table([[bh[f"bh{i}_bare_mass"], bh[f"bh{i}_offset"], 0.0, 0.0,
                      0.0, bh[f"bh{i}_momentum"], 0.0, 0.0, 0.0, bh[f"bh{i}_spin"]]
                     for i in (1, 2)])


def completed(table):
    """The table with an odd count completed."""
    t = as_table(table)
    if len(t) % 2:
        pad = np.zeros(10)
        pad[1:4] = t[-1, 1:4]
        t = np.vstack([t, pad])
    return t


def scaled(table, s):
    """The table with every position times s (masses, momenta and spins as
    they are): the same punctures moved into a box s times the size."""
    t = as_table(table).copy()
    t[:, 1:4] *= s
    return t


def conditioning(bh, table, lo, hi, dx, psi=1.0):
    """(aCoef, regrid condition): the largest sum of |terms| / |sum of terms|
    over [lo, hi] at constant psi, with the Gaussian phi_0 -- how far a
    relative error of one term is magnified in the result."""
    A2, psi_bh = a2_psi_bh(table, bh["domain_length"], lo, hi, dx)
    rho_grad = oracle.getrhogradphif(gaussian_on_box(bh, lo, hi, dx), lo, hi, dx)
    G, m = bh["G_Newton"], (2.0 / 3.0) * bh["constant_K"] ** 2
    psi_0 = psi + psi_bh
    ta = (-0.625 * m * psi_0 ** 4.0, -A2 * psi_0 ** -8.0, 2.0 * np.pi * G * rho_grad)
    tc = (1.5 * A2 * psi_0 ** -7.0, 24.0 * np.pi * G * np.abs(rho_grad) * psi_0, np.log(psi_0))
    return tuple(float(np.max(sum(np.abs(v) for v in t) / np.abs(sum(t)))) for t in (ta, tc))


def permuted(table):
    """Axes permuted cyclically: every vector (vx, vy, vz) becomes (vz, vx, vy)."""
    t = as_table(table).copy()
    for c in (1, 4, 7):
        t[:, c:c + 3] = np.roll(t[:, c:c + 3], 1, axis=1)
    return t


def _pair(x, y, z, a, b):
    l1, l2 = (x - a[1], y - a[2], z - a[3]), (x - b[1], y - b[2], z - b[3])
    r1 = np.sqrt(l1[0] * l1[0] + l1[1] * l1[1] + l1[2] * l1[2])
    r2 = np.sqrt(l2[0] * l2[0] + l2[1] * l2[1] + l2[2] * l2[2])
    n1, n2 = [v / r1 for v in l1], [v / r2 for v in l2]
    P1, P2, J1, J2 = tuple(a[4:7]), tuple(b[4:7]), tuple(a[7:10]), tuple(b[7:10])
    A = {ij: phi_ref._get_Aij(ij[0], ij[1], r1, r2, n1, n2, J1, J2, P1, P2) for ij in IJ}
    return A, a[0] / r1 + b[0] / r2


def bowen_york(table, L, lo, hi, dx):
    """(A, psi_bh) over [lo, hi]: A a dict of the six components keyed by IJ."""
    x, y, z = phi_ref.centres(lo, hi, dx, L, grow=0)
    shape = (z.size, y.size, x.size)
    x, y, z = (np.broadcast_to(v, shape) for v in (x, y, z))
    t = completed(table)
    A, psi_bh = _pair(x, y, z, t[0], t[1])
    for q in range(1, len(t) // 2):
        Aq, pq = _pair(x, y, z, t[2 * q], t[2 * q + 1])
        A = {ij: A[ij] + Aq[ij] for ij in IJ}
        psi_bh = psi_bh + pq
    return A, psi_bh


def contract(A):
    """A2 = A_ij A^ij as SetLevelData.cpp:312-317 writes it."""
    return (A[0, 0] ** 2.0 + A[1, 1] ** 2.0 + A[2, 2] ** 2.0 + 2 * A[0, 1] ** 2.0
            + 2 * A[0, 2] ** 2.0 + 2 * A[1, 2] ** 2.0)


def a2_psi_bh(table, L, lo, hi, dx):
    """What phi_ref.bowen_york returns, from the table."""
    A, psi_bh = bowen_york(table, L, lo, hi, dx)
    return contract(A), psi_bh


def min_distance(table, L, lo, hi, dx):
    """The smallest distance of a cell centre of [lo, hi] to a puncture."""
    x, y, z = phi_ref.centres(lo, hi, dx, L, grow=0)
    return min(np.sqrt((x - r[1]) ** 2 + (y - r[2]) ** 2 + (z - r[3]) ** 2).min()
               for r in as_table(table))


@contextlib.contextmanager
def _holes_from(table):
    """phi_ref's set_a_coef / set_rhs / integrand / NL loop with the Bowen-York
    terms of the table instead of the deck's two holes."""
    saved = phi_ref.bowen_york
    phi_ref.bowen_york = lambda bh, lo, hi, dx: a2_psi_bh(table, bh["domain_length"], lo, hi, dx)
    try:
        yield
    finally:
        phi_ref.bowen_york = saved


def gaussian_on_box(bh, lo, hi, dx):
    return phi_ref.phi_on_box(phi_ref.gaussian, bh, lo, hi, dx)


def nl_coefs(bh, table, lo, hi, dx, psi_g, phi_g):
    with _holes_from(table):
        return phi_ref.nl_coefs_phi(bh, lo, hi, dx, psi_g, phi_g)


def nl_integrand(bh, table, lo, hi, dx, psi_g, phi_g):
    with _holes_from(table):
        return phi_ref.nl_integrand_phi(bh, lo, hi, dx, psi_g, phi_g)


def regrid_condition(bh, table, lo, hi, dx, psi=None, phi_g=None):
    """set_regrid_condition (SetLevelData.cpp:190-240) in the expression order
    of regrid_ref.regrid_condition; phi_g None: the analytic Gaussian, else
    the stored phi_0 over the box grown by one; psi: None or over the box."""
    L, G = bh["domain_length"], bh["G_Newton"]
    if phi_g is None:
        phi_g = gaussian_on_box(bh, lo, hi, dx)
    rho_grad = oracle.getrhogradphif(phi_g, lo, hi, dx)
    A2, psi_bh = a2_psi_bh(table, L, lo, hi, dx)
    rho = 0.0
    m = (2.0 / 3.0) * (0.0 * 0.0) - 16.0 * math.pi * G * rho
    psi_0 = (1.0 if psi is None else psi) + psi_bh
    return (1.5 * abs(m) + 1.5 * A2 * np.power(psi_0, -7.0) +
            24.0 * math.pi * G * np.abs(rho_grad) * np.power(psi_0, 1.0) + np.log(psi_0))


def chi(table, L, lo, hi, dx, psi):
    """set_output_data's chi (SetLevelData.cpp:381-383); psi over the box."""
    _, psi_bh = bowen_york(table, L, lo, hi, dx)
    return np.power(psi + psi_bh, -4.0)


def oracle_poisson_solve(prm, table, n, max_depth, n_nl, perturb=None):
    """phi_ref.oracle_poisson_solve_phi with the table's coefficients and the
    Gaussian as the stored phi_0."""
    phi_g = gaussian_on_box(prm.bh(), (0, 0, 0), (n - 1,) * 3, prm.domainLength[0] / n)
    with _holes_from(table):
        return phi_ref.oracle_poisson_solve_phi(prm, n, max_depth, n_nl, phi_g, perturb=perturb)


def reference_hierarchy(prm, table, n0, max_level):
    """The restatement's set_grids (the loop of tests/test_regrid.py's
    _reference_hierarchy) with the table's regrid condition: (levels, margins),
    margins[l] the smallest | |cond| / tagVal - 1 | of level l's last pass."""
    bh = prm.bh()
    c, _ = regrid_ref.lattice_params(prm.block_factor, prm.max_grid_size)
    dom0 = (0, 0, 0, n0 - 1, n0 - 1, n0 - 1)
    levels = [[dom0]]
    top, margins = 0, {}
    more = max_level > 0
    while more:
        more = False
        old_top = top
        tags = []
        dom, dx = dom0, prm.L / n0
        for l, boxes in enumerate(levels):
            conds = [regrid_condition(bh, table, b[:3], b[3:], dx) for b in boxes]
            tag_val = max(np.abs(a).max() for a in conds) * prm.refine_threshold
            margins[l] = min(np.abs(np.abs(a) / tag_val - 1.0).min() for a in conds)
            tags.append(regrid_ref.tag_lattice(conds, boxes, dom, tag_val, 2, c))
            dom = tuple(2 * v for v in dom[:3]) + tuple(2 * v + 1 for v in dom[3:])
            dx /= 2
        new, fin = regrid_ref.regrid(dom0, tags, prm.block_factor, prm.max_grid_size,
                                     prm.fill_ratio)
        if fin > top:
            top += 1
        levels = [[dom0]] + new[:top]
        if top < max_level and top > old_top:
            more = True
    return levels, margins
