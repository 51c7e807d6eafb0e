"""Reference side of the matter tests (tests/test_matter.py): the scalar
field's kinetic and potential energy in set_m_value's slot
(SetLevelData.cpp:266-278), restated in numpy on top of tests/phi_ref.py,
tests/puncture_ref.py and tests/regrid_ref.py.  Test infrastructure only.

    V(phi) = V0 + 0.5 * mass * mass * phi * phi + 0.25 * lambda * phi * phi * phi * phi
    rho    = 0.5 * Pi * Pi + V(phi_0)
    m      = (2.0 / 3.0) * (K * K) - 16.0 * pi * G * rho

each evaluated left to right; rho and m use only + - x, so in this
association numpy gives the device's bits for them.  `pot` is (V0, mass,
lambda); `pi` a scalar or an array over the valid cells; `phi_g` the stored
phi_0 over the box grown by one (phi_0 itself is its interior); `table` None
(the deck's two holes of bh) or a puncture table.  Arrays are (nz, ny, nx),
i fastest.
"""
import contextlib
import math

import numpy as np

import oracle
from tests import phi_ref, regrid_ref
from tests import puncture_ref as P


def potential(pot, phi):
    V0, mass, lam = (float(v) for v in pot)
    return V0 + 0.5 * mass * mass * phi * phi + 0.25 * lam * phi * phi * phi * phi


def rho(pot, pi, phi):
    return 0.5 * pi * pi + potential(pot, phi)


def m_value(bh, K, rho_):
    """set_m_value (SetLevelData.cpp:266-278)."""
    return (2.0 / 3.0) * (K * K) - 16.0 * np.pi * bh["G_Newton"] * rho_


def _holes(bh, table, lo, hi, dx):
    if table is None:
        return phi_ref.bowen_york(bh, lo, hi, dx)
    return P.a2_psi_bh(table, bh["domain_length"], lo, hi, dx)


def _common(bh, lo, hi, dx, psi_g, phi_g, K, pot, pi, table):
    """phi_ref._common with rho from the matter."""
    shape = tuple(hi[d] - lo[d] + 1 for d in (2, 1, 0))
    if psi_g is None:
        psi_g = np.ones(tuple(s + 2 for s in shape))
    assert psi_g.shape == phi_g.shape == tuple(s + 2 for s in shape)
    lap = oracle.getlaplacianpsif(psi_g, lo, hi, dx)
    rho_grad = oracle.getrhogradphif(phi_g, lo, hi, dx)
    A2, psi_bh = _holes(bh, table, lo, hi, dx)
    m = m_value(bh, K, rho(pot, pi, phi_g[1:-1, 1:-1, 1:-1]))
    psi_0 = psi_g[1:-1, 1:-1, 1:-1] + psi_bh
    return lap, rho_grad, A2, m, psi_0


def nl_coefs(bh, lo, hi, dx, psi_g, phi_g, pot, pi, table=None):
    """(aCoef, rhs) as phi_ref.nl_coefs_phi writes them, m with the matter."""
    lap, rho_grad, A2, m, psi_0 = _common(bh, lo, hi, dx, psi_g, phi_g, bh["constant_K"], pot, pi,
                                          table)
    G = bh["G_Newton"]
    a = -0.625 * m * psi_0 ** 4.0 - A2 * psi_0 ** -8.0 + 2.0 * np.pi * G * rho_grad
    r = (0.125 * m * psi_0 ** 5.0 - 0.125 * A2 * psi_0 ** -7.0
         - 2.0 * np.pi * G * rho_grad * psi_0 - lap)
    return a, r


def nl_integrand(bh, lo, hi, dx, psi_g, phi_g, pot, pi, table=None):
    """set_constant_K_integrand as phi_ref.nl_integrand_phi writes it (m at K = 0)."""
    lap, rho_grad, A2, m, psi_0 = _common(bh, lo, hi, dx, psi_g, phi_g, 0.0, pot, pi, table)
    return (-1.5 * m + 1.5 * A2 * psi_0 ** -12.0
            + 24.0 * np.pi * bh["G_Newton"] * rho_grad * psi_0 ** -4.0
            + 12.0 * lap * psi_0 ** -5.0)


def regrid_condition(bh, lo, hi, dx, pot, pi, psi=None, phi_g=None, table=None):
    """set_regrid_condition in the expression order of
    puncture_ref.regrid_condition, 1.5 |m| with the matter (K = 0).  phi_g
    None: the analytic Gaussian."""
    G = bh["G_Newton"]
    if phi_g is None:
        phi_g = P.gaussian_on_box(bh, lo, hi, dx)
    rho_grad = oracle.getrhogradphif(phi_g, lo, hi, dx)
    A2, psi_bh = _holes(bh, table, lo, hi, dx)
    rho_ = rho(pot, pi, phi_g[1:-1, 1:-1, 1:-1])
    m = (2.0 / 3.0) * (0.0 * 0.0) - 16.0 * math.pi * G * rho_
    psi_0 = (1.0 if psi is None else psi) + psi_bh
    return (1.5 * np.abs(m) + 1.5 * A2 * np.power(psi_0, -7.0) +
            24.0 * math.pi * G * np.abs(rho_grad) * np.power(psi_0, 1.0) + np.log(psi_0))


def conditioning(bh, lo, hi, dx, pot, pi, phi_g, psi=1.0, table=None):
    """(aCoef, regrid condition): the largest sum of |terms| / |sum of terms|
    over [lo, hi] at constant psi, as puncture_ref.conditioning, with the
    matter in m."""
    A2, psi_bh = _holes(bh, table, lo, hi, dx)
    rho_grad = oracle.getrhogradphif(phi_g, lo, hi, dx)
    G = bh["G_Newton"]
    rho_ = rho(pot, pi, phi_g[1:-1, 1:-1, 1:-1])
    psi_0 = psi + psi_bh
    ta = (-0.625 * m_value(bh, bh["constant_K"], rho_) * psi_0 ** 4.0, -A2 * psi_0 ** -8.0,
          2.0 * np.pi * G * rho_grad)
    tc = (1.5 * np.abs(m_value(bh, 0.0, rho_)), 1.5 * A2 * psi_0 ** -7.0,
          24.0 * np.pi * G * np.abs(rho_grad) * psi_0, np.log(psi_0))
    return tuple(float(np.max(sum(np.abs(v) for v in t) / np.abs(sum(t)))) for t in (ta, tc))


@contextlib.contextmanager
def _matter_in(pot, pi, table=None):
    """phi_ref's NL loop with the coefficients above."""
    saved = phi_ref.nl_coefs_phi, phi_ref.nl_integrand_phi
    phi_ref.nl_coefs_phi = lambda bh, lo, hi, dx, psi_g, phi_g: nl_coefs(
        bh, lo, hi, dx, psi_g, phi_g, pot, pi, table)
    phi_ref.nl_integrand_phi = lambda bh, lo, hi, dx, psi_g, phi_g: nl_integrand(
        bh, lo, hi, dx, psi_g, phi_g, pot, pi, table)
    try:
        yield
    finally:
        phi_ref.nl_coefs_phi, phi_ref.nl_integrand_phi = saved


def oracle_poisson_solve(prm, n, max_depth, n_nl, phi_g, pot, pi, perturb=None):
    """phi_ref.oracle_poisson_solve_phi on one n^3 box with the matter; pi a
    scalar or an (n, n, n) array."""
    with _matter_in(pot, pi):
        return phi_ref.oracle_poisson_solve_phi(prm, n, max_depth, n_nl, phi_g, perturb=perturb)


def pi_on_box(f, L, lo, hi, dx):
    """f(x, y, z) over the valid cells of [lo, hi], as a full array."""
    x, y, z = phi_ref.centres(lo, hi, dx, L, grow=0)
    return np.ascontiguousarray(np.broadcast_to(f(x, y, z), (z.size, y.size, x.size)))


def reference_hierarchy(prm, n0, max_level, pot, pi, table=None):
    """puncture_ref.reference_hierarchy with the matter's regrid condition (pi
    a constant): (levels, margins), margins[l] the smallest
    | |cond| / tagVal - 1 | of level l over every pass."""
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
            conds = [regrid_condition(bh, b[:3], b[3:], dx, pot, pi, table=table) for b in boxes]
            tag_val = max(np.abs(a).max() for a in conds) * prm.refine_threshold
            margins[l] = min([margins.get(l, np.inf)] +
                             [np.abs(np.abs(a) / tag_val - 1.0).min() for a in conds])
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
