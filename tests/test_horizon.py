"""Apparent horizons (mg_ic_code_amd/horizon.py, libmgic_horizon.so, DESIGN.md
3p) against the numpy restatement tests/horizon_ref.py.

CPU: the restatement itself (polynomial reproduction of the value and the
gradient, the derivative weights), the surface basis (orthonormality, the
derivative matrices, the flat geometry of a displaced sphere), the finder with
an analytic evaluator on the prototype cases of the issue, the deck keys and
every refusal that needs no device.  GPU: the point outputs against the
restatement (the interpolated parts bit for bit) on one box, three layouts, two
and three levels and an L-shaped level; real puncture tables with and without
LW; the finder on the device; refusals and ledger coverage; the solve end to
end; the command-line tool.
"""
import ctypes
import dataclasses
import json
import math
import os
import subprocess
import sys
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

from tests import adm_ref
from tests import horizon_ref as H
from tests import test_sample as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "horizon_worker.py")
WORKER_TIMEOUT = 300
U = 2.0 ** -53
# m = P = J = 0 far outside every domain: the analytic parts are +-0
ZERO = [(0.0, 1000.0, 2000.0, 3000.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)]
TOL = 1e-10


def Z(m, x, P=(0.0, 0.0, 0.0), J=(0.0, 0.0, 0.0)):
    return (float(m),) + tuple(x) + tuple(P) + tuple(J)


SCHW = [Z(1.0, (0.2, 0.1, -0.15))]
BL_CLOSE = [Z(0.5, (0.4, 0.0, 0.0)), Z(0.5, (-0.4, 0.0, 0.0))]
BL_FAR = [Z(0.5, (1.2, 0.0, 0.0)), Z(0.5, (-1.2, 0.0, 0.0))]
BOWEN_YORK = [Z(1.0, (0.0, 0.0, 0.0), (0.0, 0.3, 0.0), (0.0, 0.0, 0.5))]


# ------------------------------------------------------------------ CPU: the restatement
def _poly_exact(coef, p, d=None):
    """The polynomial of TS._poly_field at p in exact arithmetic; d: its
    derivative in direction d."""
    x = [Fraction(float(v)) for v in p]
    total = Fraction(0)
    for a in range(coef.shape[0]):
        for b in range(coef.shape[1]):
            for c in range(coef.shape[2]):
                e = [a, b, c]
                k = Fraction(int(coef[a, b, c]))
                if d is not None:
                    if e[d] == 0:
                        continue
                    k *= e[d]
                    e[d] -= 1
                total += k * x[0] ** e[0] * x[1] ** e[1] * x[2] ** e[2]
    return total


def test_restatement_reproduces_polynomials_and_their_derivatives(rng):
    # Exact data (integer coefficients, dx = 1/2) at points that are multiples
    # of 2^-20, so x + half, q, s and t are exact and the interpolant of exact
    # arithmetic IS the polynomial, its derivative the polynomial's.  What is
    # left is the restatement's own rounding, relative to each term
    # |wz wy wx u|.  The value is 3o's count: a weight rounds 3 times, each nest
    # level once for the product and at most 3 times for the additions,
    # 3 * (3 + 1 + 3) = 21, the bar 24 U of the sum of absolute contributions.
    # The gradient has the same nest; in one direction dw takes w's place.  t is
    # a multiple of 2^-19 here, so the products a .. f are multiples of 2^-38
    # below 8 and they and their sums are exact: dw rounds once (the division
    # by 6), fewer than w's 3, and the division by dx = 1/2 is exact: 24 U
    # again.  Order 2: exact weights (1 - t, -1, 1), one product and one
    # addition per level: 6, the bar 8 U.
    n, dx = 12, 0.5
    for order, deg, bar in ((4, 4, 24 * U), (2, 2, 8 * U)):
        worst_v = worst_g = 0.0
        for _ in range(3):
            coef = rng.integers(-3, 4, (deg, deg, deg))
            full = TS._poly_field(coef, n, dx)
            if order == 2:
                # the 4-stencil must not be available: the level is the box of cells
                # 4, 5 alone, the points between their centres (-0.75 .. -0.25)
                h = H.Hierarchy((n,) * 3, dx, [[((4, 4, 4), (5, 5, 5), full[4:6, 4:6, 4:6])]])
                pts = rng.integers(-3 * 2 ** 18, -2 ** 18, (40, 3)) / 2.0 ** 20
            else:
                h = H.single_box(full, dx)
                pts = rng.integers(-2 * 2 ** 20, 2 * 2 ** 20, (40, 3)) / 2.0 ** 20
            for p in pts:
                r = H.expansion_one(h, ZERO, p, (0.0, 0.0, 1.0), 0.0)
                assert (r.level, r.order) == (0, order), (p, r.level, r.order)
                err = abs(Fraction(r.v) - _poly_exact(coef, p))
                worst_v = max(worst_v, float(err) / r.scale[1])
                assert err <= Fraction(bar) * Fraction(r.scale[1]), (order, p, float(err))
                assert r.out[1] == r.v and r.out[2:5] == r.g   # the zero table adds +-0
                for d in range(3):
                    err = abs(Fraction(r.g[d]) - _poly_exact(coef, p, d))
                    if r.scale[2 + d] > 0.0:
                        worst_g = max(worst_g, float(err) / r.scale[2 + d])
                    assert err <= Fraction(bar) * Fraction(r.scale[2 + d]), (order, d, p, float(err))
        print(f"order {order}: worst error / sum of |contributions|: value {worst_v / U:.2f} U, "
              f"gradient {worst_g / U:.2f} U")


def test_derivative_weights(rng):
    from mg_ic_code_amd.horizon import (cubic_derivative_weights, cubic_weights,
                                        linear_derivative_weights, linear_weights)
    # sum dw = 0 in exact arithmetic.  Each dw_k is a sum of three products (one
    # rounding each), two additions and a division: its error is at most 4 U of
    # S_k = (|p1| + |p2| + |p3|) / den; the three additions of the check itself
    # add 3 U of sum |dw|.  The bar is that bound, (4 sum S_k + 3 sum |dw|) U.
    worst = 0.0
    for t in rng.uniform(0.0, 1.0, 1000):
        t = float(t)
        dw = H.dweights4(t)
        # the package states the same expressions: bit for bit
        assert dw == cubic_derivative_weights(t) and H.weights4(t) == cubic_weights(t)
        assert H.weights2(t) == linear_weights(t) and H.dweights2(t) == linear_derivative_weights(t)
        tm1, tm2, tp1 = t - 1.0, t - 2.0, t + 1.0
        a, b, c, d, e, f = (abs(v) for v in (tm1 * tm2, t * tm2, t * tm1, tp1 * tm2, tp1 * tm1, tp1 * t))
        S = (a + b + c) / 6.0 + (a + d + e) / 2.0 + (b + d + f) / 2.0 + (c + e + f) / 6.0
        total = abs(((dw[0] + dw[1]) + dw[2]) + dw[3])
        mag = sum(abs(v) for v in dw)
        worst = max(worst, total / mag)
        assert total <= (4.0 * S + 3.0 * mag) * U, (t, total)
    print("worst |sum dw| / sum |dw| =", worst / 2.0 ** -52, "ulp")
    assert worst <= 4 * 2.0 ** -52   # "a few ulp of sum |dw|"
    assert H.dweights4(0.0) == [-1.0 / 3.0, -0.5, 1.0, -1.0 / 6.0]
    assert H.dweights2(0.3) == [-1.0, 1.0]


def test_binding_covers_the_header():
    import re
    from mg_ic_code_amd import _lib
    with open(os.path.join(ROOT, "include", "mgic_horizon.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"MGIC_HORIZON_API\s+[^;()]*?\b(mgic_horizon_\w+)\s*\(", text))
    assert declared == set(_lib.HORIZON_SIGNATURES) and len(declared) == 4
    assert "#define MGIC_HORIZON_MAX_LEVELS 8" in text
    assert "#define MGIC_HORIZON_MAX_POINTS (1 << 20)" in text
    assert "#define MGIC_HORIZON_TERMS 6" in text


# ------------------------------------------------------------------ CPU: the basis
_BASIS = {}


def basis(lmax=8):
    from mg_ic_code_amd.horizon import SurfaceBasis
    if lmax not in _BASIS:
        _BASIS[lmax] = SurfaceBasis(lmax)
    return _BASIS[lmax]


def test_basis_is_orthonormal():
    B = basis()
    assert (B.ntheta, B.nphi, B.npts, B.ncoef) == (12, 24, 288, 81)
    assert abs(float(np.sum(B.W)) - 4.0 * math.pi) <= 1e-13
    err = float(np.max(np.abs(B.Y.T @ (B.W[:, None] * B.Y) - np.eye(B.ncoef))))
    print("max |Y^T W Y - I| =", err)
    assert err <= 1e-13
    assert list(B.l[:4]) == [0, 1, 1, 1] and list(B.m[:4]) == [0, -1, 0, 1]


def test_basis_derivatives_against_central_differences():
    from mg_ic_code_amd.horizon import real_harmonics
    # A harmonic of degree l restricted to a great circle, or to a circle of
    # latitude, is a trigonometric polynomial of degree <= l, so each derivative
    # along theta or phi is bounded by l times the maximum (Bernstein).  A
    # central difference with step e is off by e^2 / 6 max|f'''| plus the
    # rounding of the difference, 2 U max|f| / e (4 U for slack).
    B = basis()
    L, e = B.lmax, 1e-5
    theta = np.arccos(B.cos_theta)
    ymax = float(np.max(np.abs(B.Y)))

    def at(th, ph):
        return real_harmonics(L, np.cos(th), ph)

    up, dn = at(theta + e, B.phi), at(theta - e, B.phi)
    east, west = at(theta, B.phi + e), at(theta, B.phi - e)
    worst = {}
    for name, have, hi, lo, power in (
            ("Y_theta", B.Y_theta, up[0], dn[0], 0), ("Y_phi", B.Y_phi, east[0], west[0], 0),
            ("Y_theta_theta", B.Y_theta_theta, up[1], dn[1], 1),
            ("Y_theta_phi", B.Y_theta_phi, east[1], west[1], 1),
            ("Y_phi_phi", B.Y_phi_phi, east[2], west[2], 1)):
        fmax = ymax * L ** power        # the differenced function's own bound
        bar = e * e / 6.0 * fmax * L ** 3 + 4.0 * U * fmax / e
        err = float(np.max(np.abs((hi - lo) / (2.0 * e) - have)))
        worst[name] = (err, bar)
        assert err <= bar, (name, err, bar)
    print("central differences, (error, bar):", worst)


def test_flat_geometry_of_a_displaced_sphere():
    # A sphere of radius R about x_p = 0.27 R away from the centre: the exact
    # h(theta, phi) = d cos(gamma) + sqrt(R^2 - d^2 sin^2(gamma)) projected onto
    # the basis.  What the truncation at lmax leaves, dh = max |h - Y a| on the
    # grid, is dominated by degree lmax + 2 (odd degrees above 1 vanish), whose
    # first and second derivatives are up to (lmax + 2) and (lmax + 2)(lmax + 3)
    # times larger; n is built from h_theta / h, div n from Lap_S h / h^2.  The
    # bars are those, times 10.
    B = basis()
    L, R = B.lmax, 1.3
    d = 0.27 * R
    dhat = np.array([0.6, -0.5, 0.62])
    dhat /= np.linalg.norm(dhat)
    cg = B.rhat @ dhat
    h = d * cg + np.sqrt(R * R - d * d * (1.0 - cg * cg))
    a = B.project(h)
    dh = float(np.max(np.abs(B.Y @ a - h)))
    geo = B.geometry(a, (0.0, 0.0, 0.0))
    err_div = float(np.max(np.abs(geo.divn - 2.0 / R)))
    err_n = float(np.max(np.abs(np.sum(geo.normal * (geo.points - d * dhat), axis=1) / R - 1.0)))
    bar_div = 10.0 * (L + 2) * (L + 3) * dh / (R * R)
    bar_n = 10.0 * (L + 2) * dh / R
    print(f"dh = {dh:.3e}: |div n - 2/R| = {err_div:.3e} (bar {bar_div:.3e}), "
          f"|n.(x - x_p)/R - 1| = {err_n:.3e} (bar {bar_n:.3e})")
    assert 0.0 < dh < 1e-8 and err_div <= bar_div and err_n <= bar_n
    assert np.max(np.abs(np.sum(geo.normal ** 2, axis=1) - 1.0)) <= 8 * U * 2
    # a centred sphere is exact: h = R, n = rhat, div n = 2 / R, g = 1
    a0 = np.zeros(B.ncoef)
    a0[0] = R * math.sqrt(4.0 * math.pi)
    g0 = B.geometry(a0, (1.0, 2.0, 3.0))
    assert np.max(np.abs(g0.divn - 2.0 / R)) <= 1e-13 and np.max(np.abs(g0.g - 1.0)) <= 1e-14
    assert np.max(np.abs(g0.points - (np.array([1.0, 2.0, 3.0]) + R * B.rhat))) <= 1e-14


# ------------------------------------------------------------------ CPU: the finder
_FOUND = {}


def found(name, table, centre, r0, **kw):
    """find_horizon with the analytic evaluator (psi_reg = 1, no grid), once."""
    from mg_ic_code_amd.horizon import find_horizon
    key = (name, tuple(centre), r0, tuple(sorted(kw.items())))
    if key not in _FOUND:
        _FOUND[key] = find_horizon(None, None, centre, r0, punctures=table,
                                   evaluator=H.analytic_evaluator(), basis=basis(), **kw)
    return _FOUND[key]


def test_off_centre_schwarzschild():
    # measured: 45, 38 and 42 iterations, area - 64 pi = 0 to the last bit,
    # r = 0.7311 .. 1.2686, contraction 0.5407 per step
    runs = [found("schw", SCHW, (0.0, 0.0, 0.0), r0) for r0 in (0.6, 1.3, 2.0)]
    want = 64.0 * math.pi
    for r in runs:
        print(r.status, r.iterations, repr(r.area), (r.area - want) / want, r.r_min, r.r_max,
              "theta max", r.theta_max, "contraction", r.steps[-1] / r.steps[-2])
        assert r.status == "converged" and r.found and r.iterations <= 60
        assert abs(r.area - want) / want <= 1e-12
        assert abs(r.irreducible_mass - 2.0) <= 2e-12
        assert r.enclosed == [0] and r.spin == 0.0 and r.christodoulou_mass == r.irreducible_mass
        assert r.degraded_points == 0 and r.theta_max < 1e-6
        assert 0.73 < r.r_min < 0.732 and 1.268 < r.r_max < 1.27
        assert np.max(np.abs(r.coeffs - runs[0].coeffs)) <= 10 * TOL
        assert len(r.lines()) == 4 and r.lines()[0].endswith(f"converged after {r.iterations} iterations")


def test_brill_lindquist_common_horizon():
    r = found("bl04", BL_CLOSE, (0.0, 0.0, 0.0), 1.5)   # measured: 36 iterations, 1.99856888
    print(r.status, r.iterations, repr(r.irreducible_mass))
    assert r.found and 1.9985 <= r.irreducible_mass <= 1.9987
    assert r.enclosed == [0, 1] and r.christodoulou_mass is None and r.spin is None


def test_brill_lindquist_separate_horizons():
    r = found("bl12", BL_FAR, (0.0, 0.0, 0.0), 1.5)
    assert r.status == "collapsed" and not r.found and r.r_min <= 0.05 * 1.5
    assert math.isnan(r.area) or r.area > 0.0
    want = 2.0 * 0.5 * (1.0 + 0.5 / 2.4)                # 3o's formula, psi_reg = 1
    for k, c in enumerate(((1.2, 0.0, 0.0), (-1.2, 0.0, 0.0))):
        for r0 in (0.5, 0.8):
            r = found("bl12", BL_FAR, c, r0)            # measured: 31 / 35 iterations, -6.28e-7
            print(c, r0, r.status, r.iterations, repr(r.irreducible_mass), r.irreducible_mass - want)
            assert r.found and r.enclosed == [k]
            assert abs(r.irreducible_mass - want) <= 5e-6


def test_boosted_spinning_bowen_york_hole():
    r = found("by", BOWEN_YORK, (0.0, 0.0, 0.0), 1.0)   # measured: 23 iterations
    print(r.status, r.iterations, "M_irr", repr(r.irreducible_mass), "M_chr",
          repr(r.christodoulou_mass))
    assert r.found and r.enclosed == [0] and r.spin == 0.5
    assert r.christodoulou_mass >= r.irreducible_mass > 2.0
    m = r.irreducible_mass
    assert r.christodoulou_mass == math.sqrt(m * m + 0.25 / (4.0 * m * m))
    assert abs(m - 2.000175) < 1e-5 and "M_chr" in r.lines()[-1]


def test_max_iter_runs_out():
    r = found("schw", SCHW, (0.0, 0.0, 0.0), 0.6, max_iter=3)
    assert r.status == "max_iter" and not r.found and r.iterations == 3
    assert r.enclosed == [] and r.christodoulou_mass is None and len(r.lines()) == 1


def test_step_limiter_is_part_of_the_flow():
    # from r0 = 2.0 the first steps are cut to 0.1 min h
    r = found("schw", SCHW, (0.0, 0.0, 0.0), 2.0)
    assert r.steps[0] == pytest.approx(0.2, rel=1e-12) and r.steps[0] > 10 * r.steps[12]


# ------------------------------------------------------------------ CPU: no device needed
def test_deck_keys():
    from mg_ic_code_amd.params import read_params
    txt = TS._deck_text()
    assert read_params(txt).horizons is None
    assert read_params(txt + "\nhorizons = punctures\n").horizons == "punctures"
    p = read_params(txt + "\nnum_horizons = 2\nhorizon1 = 0 0 0 1.5\nhorizon2 = 10 0.5 -1 0.6\n")
    assert p.horizons == [[0.0, 0.0, 0.0, 1.5], [10.0, 0.5, -1.0, 0.6]]
    for bad in ("horizons = all", "horizons = punctures\nnum_horizons = 1\nhorizon1 = 0 0 0 1",
                "num_horizons = 0", "num_horizons = 1\nhorizon1 = 0 0 0", "num_horizons = 1\nhorizon1 = 0 0 0 0",
                "num_horizons = 1\nhorizon1 = 0 0 0 -1", "num_horizons = 1\nhorizon1 = 0 x 0 1",
                "num_horizons = 1\nhorizon1 = 0 nan 0 1", "num_horizons = 1\nhorizon1 = 0 0 0 inf",
                "num_horizons = 1\nhorizon1 = 0 0 0 1 2"):
        with pytest.raises(ValueError):
            read_params(txt + "\n" + bad + "\n")
    with pytest.raises(KeyError):
        read_params(txt + "\nnum_horizons = 2\nhorizon1 = 0 0 0 1\n")
    with pytest.raises(ValueError, match="periodic"):
        read_params(txt + "\nhorizons = punctures\n", {"is_periodic": "1"})


def test_requests_and_refusals_need_no_device():
    from mg_ic_code_amd import _lib
    from mg_ic_code_amd.horizon import (HorizonArgumentError, expansion_points, find_horizon,
                                        horizons_of, resolve_horizons)
    from mg_ic_code_amd.nl import poisson_solve
    from mg_ic_code_amd.punctures import PunctureSet
    prm = TS._deck()
    table = PunctureSet.from_params(prm)
    assert resolve_horizons("punctures", table) == [((10.0, 0.0, 0.0), 0.5), ((-10.0, 0.0, 0.0), 0.5)]
    assert resolve_horizons([(1, 2, 3, 0.5), "0 0 0 2"], table) == [((1.0, 2.0, 3.0), 0.5),
                                                                   ((0.0, 0.0, 0.0), 2.0)]
    for bad in ("holes", [], [(0, 0, 0)], [(0, 0, 0, 0.0)], [(0, 0, 0, -1.0)], 3,
                [(0, float("nan"), 0, 1.0)], [(0, 0, 0, True)], [(0, 0, 0, float("inf"))]):
        with pytest.raises(ValueError) as e:
            resolve_horizons(bad, table)
        assert isinstance(e.value, HorizonArgumentError) and e.value.code == -1
    with pytest.raises(ValueError, match="bare mass"):
        resolve_horizons("punctures", PunctureSet([Z(0.0, (1.0, 0.0, 0.0)), Z(0.5, (0.0, 0.0, 0.0))]))
    periodic = dataclasses.replace(prm, is_periodic=1)
    ev = H.analytic_evaluator()
    for call in (lambda: find_horizon(None, periodic, (0, 0, 0), 1.0, evaluator=ev),
                 lambda: horizons_of(None, periodic, "punctures", evaluator=ev),
                 lambda: expansion_points(None, [[0, 0, 0]], [[0, 0, 1]], [0.0], periodic),
                 lambda: poisson_solve(None, periodic, horizons="punctures"),
                 lambda: poisson_solve(None, dataclasses.replace(periodic, horizons="punctures")),
                 lambda: poisson_solve(None, prm, horizons=[(0, 0, 0, -1.0)]),
                 lambda: poisson_solve(None, prm, horizons="everywhere")):
        with pytest.raises(ValueError):
            call()
    for kw in (dict(centre=(0, 0)), dict(centre=(0, 0, float("inf"))), dict(r0=0.0), dict(r0=-1.0),
               dict(r0=float("nan")), dict(r0="x"), dict(lmax=-1), dict(lmax=2.5), dict(lmax=33),
               dict(tol=0.0), dict(tol=-1e-3), dict(max_iter=0), dict(max_iter=2.5)):
        args = dict(centre=(0.0, 0.0, 0.0), r0=1.0)
        args.update(kw)
        with pytest.raises(ValueError) as e:
            find_horizon(None, prm, evaluator=ev, punctures=SCHW, **args)
        assert isinstance(e.value, HorizonArgumentError), kw
    # refused on the host by expansion_points: nothing is loaded
    one, up, zero = [[0.0, 0.0, 0.0]], [[0.0, 0.0, 1.0]], [0.0]
    for psi, pts, nrm, dv in (([], one, up, zero), ([None] * 9, one, up, zero),
                              ([None], [[0.0, 0.0]], up, zero), ([None], one, up * 2, zero),
                              ([None], one, up, [0.0, 1.0]), ([None], np.zeros((0, 3)), up, zero),
                              ([None], "abc", up, zero)):
        with pytest.raises(ValueError):
            expansion_points(psi, pts, nrm, dv, prm)
    assert not _lib.horizon_loaded()


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def comm():
    import mg_ic_code_amd as mg
    return mg.Comm()


class LW:
    """What expansion_points needs of a MomentumFields: the six fields per level."""

    def __init__(self, per_level):
        self.per_level = per_level
        self.num_levels = len(per_level)

    def lw(self, level=0):
        return self.per_level[level]


LW_SEED = 100


def _device(comm, n0, dx0, level_boxes, seed, with_lw):
    """psi per level (TS._device: random data, 1e300 in every ghost) and, with
    LW, six more fields per level on the same grids."""
    psi = TS._device(comm, n0, dx0, level_boxes, seed=seed)
    if not with_lw:
        return psi, None
    per_level = []
    for l, f in enumerate(psi):
        per_level.append([TS._field(f.grid, TS._full(n0, len(level_boxes), seed + LW_SEED + k)[l] - 1.0)
                          for k in range(6)])
    return psi, LW(per_level)


def _reference(n0, dx0, level_boxes, seed, with_lw):
    def hier(s, shift):
        full = TS._full(n0, len(level_boxes), s)
        return H.Hierarchy(n0, dx0, [[(b[:3], b[3:], full[l][b[2]:b[5] + 1, b[1]:b[4] + 1, b[0]:b[3] + 1] - shift)
                                      for b in boxes] for l, boxes in enumerate(level_boxes)])
    return hier(seed, 0.0), ([hier(seed + LW_SEED + k, 1.0) for k in range(6)] if with_lw else None)


def _normals(npts, seed=41):
    rng = np.random.default_rng(seed)
    n = rng.normal(size=(npts, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    return np.ascontiguousarray(n), rng.uniform(0.5, 3.0, npts)


_REF = {}


def _ref(key, h, lw, table, pts, nrm, dv):
    """The restatement's answer, computed once per case."""
    if key not in _REF:
        _REF[key] = H.expansion(h, table, pts, nrm, dv, lw)
    return _REF[key]


def _bits(got, want, with_lw, what):
    """level, order and the interpolated parts bit for bit (a zero table: psi
    is v, dpsi is g); A_nn and theta at 1e-13 of their absolute contributions."""
    for name, g, w in (("level", got.level, want.level), ("order", got.order, want.order),
                       ("psi", got.psi, want.v), ("dpsi", got.dpsi, want.g)):
        if not H.same_bits(g, w):
            g2, w2 = np.asarray(g, np.float64), np.asarray(w, np.float64)
            bad = np.argwhere(~((g2 == w2) | (np.isnan(g2) & np.isnan(w2))))
            raise AssertionError(f"{what}: {name} differ at {len(bad)} places, first {bad[:4].tolist()}")
    none = got.order == 0
    assert np.all(np.isnan(got.theta[none])) and np.all(np.isnan(got.a_nn[none]))
    ok = ~none
    assert np.all(np.isfinite(got.theta[ok])) and np.all(np.abs(got.psi[ok]) < 2.0)
    if not with_lw:
        assert np.all(got.a_nn[ok] == 0.0)
    _close(got, want, what)


def _close(got, want, what):
    """Every output within 1e-13 of its sum of absolute contributions (the bar
    of 3j and 3n: a sqrt and divisions are involved); returns the worst ratios."""
    ok = got.order > 0
    have = np.column_stack([got.theta, got.psi, got.dpsi, got.a_nn])[ok]
    err = np.abs(have - want.out[ok])
    scale = want.scale[ok]
    ratio = np.max(np.where(scale > 0.0, err / np.where(scale > 0.0, scale, 1.0), err), axis=0)
    assert np.all(err <= 1e-13 * scale), (what, ratio)
    return ratio


ONE = TS.ONE
ONE_BOXES = [[(0, 0, 0, 11, 7, 15)]]


def _one_box(comm, with_lw):
    from mg_ic_code_amd.horizon import expansion_points
    pts = TS._points(ONE["n0"], ONE["dx0"])
    nrm, dv = _normals(len(pts))
    psi, lw = _device(comm, ONE["n0"], ONE["dx0"], ONE_BOXES, 1, with_lw)
    h, hl = _reference(ONE["n0"], ONE["dx0"], ONE_BOXES, 1, with_lw)
    want = _ref(("one", with_lw), h, hl, ZERO, pts, nrm, dv)
    got = expansion_points(psi[0], pts, nrm, dv, None, punctures=ZERO, momentum=lw)
    _bits(got, want, with_lw, f"12x8x16, lw {with_lw}")
    again = expansion_points(psi, pts, nrm, dv, None, punctures=ZERO, momentum=lw)
    for name in ("theta", "psi", "dpsi", "a_nn", "level", "order"):   # two calls: the same bits
        assert H.same_bits(getattr(got, name), getattr(again, name)), name
    return got, want, pts, nrm, dv


@pytest.mark.gpu
@pytest.mark.parametrize("with_lw", [False, True])
def test_one_box_against_the_restatement(comm, with_lw):
    got, want, pts, _, _ = _one_box(comm, with_lw)
    assert set(np.unique(got.order)) == {0, 2, 4} and set(np.unique(got.level)) == {-1, 0}
    outside = got.level < 0
    assert np.all(got.order[outside] == 0) and 8 <= outside.sum() < 0.2 * len(pts)
    # inside and yet no stencil: within half a cell of a domain face
    assert np.any((got.level == 0) & (got.order == 0))


@pytest.mark.gpu
def test_three_box_layouts_agree(comm):
    from mg_ic_code_amd.horizon import expansion_points
    n0, dx0 = (16, 16, 16), 0.75
    pts = TS._points(n0, dx0)
    nrm, dv = _normals(len(pts))
    h, hl = _reference(n0, dx0, [[(0, 0, 0, 15, 15, 15)]], 4, True)
    want = _ref("sixteen", h, hl, ZERO, pts, nrm, dv)
    for parts in ((1, 1, 1), (2, 2, 1), (2, 2, 2)):
        boxes = TS._split(n0, parts)
        psi, lw = _device(comm, n0, dx0, [boxes], 4, True)
        assert psi[0].grid.num_local == len(boxes) == parts[0] * parts[1] * parts[2]
        got = expansion_points(psi, pts, nrm, dv, None, punctures=ZERO, momentum=lw)
        _bits(got, want, True, f"16^3 as {parts}")


def _two_levels(comm, name, level1, with_lw=True):
    from mg_ic_code_amd.horizon import expansion_points
    n0, dx0 = (16, 16, 16), 0.625
    boxes = [[(0, 0, 0, 15, 15, 15)], level1]
    rng = np.random.default_rng(17)
    f = dx0 / 2  # a fine cell
    pts = [TS._points(n0, dx0, nrand=300, seed=5), rng.uniform(-3.0, 3.0, (60, 3)) * dx0,
           rng.uniform(-4.0, 4.0, (120, 3)) * dx0]
    for d in range(3):
        for side in (-1, 1):
            for off in (-2.2, -1.4, -0.6, -0.3, -1e-9, 0.0, 0.3, 0.8, 1.3, 1.7, 2.6, 3.4):
                # off fine cells outside (> 0) or inside (< 0) the faces at +-4 coarse cells
                p = rng.uniform(-2.5, 2.5, 3) * dx0
                p[d] = side * (4 * dx0 + off * f)
                pts.append(p[None, :])
    pts = np.ascontiguousarray(np.concatenate(pts))
    nrm, dv = _normals(len(pts), seed=43)
    psi, lw = _device(comm, n0, dx0, boxes, 2, with_lw)
    h, hl = _reference(n0, dx0, boxes, 2, with_lw)
    want = _ref((name, with_lw), h, hl, ZERO, pts, nrm, dv)
    got = expansion_points(psi, pts, nrm, dv, None, punctures=ZERO, momentum=lw)
    _bits(got, want, with_lw, name)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name,level1", [("patch", TS.PATCH), ("lshape", TS.LSHAPE)])
def test_two_levels_against_the_restatement(comm, name, level1):
    got = _two_levels(comm, name, level1)
    for lev in (0, 1):
        assert {0, 2, 4} <= set(np.unique(got.order[got.level == lev])), lev


@pytest.mark.gpu
def test_three_levels_with_two_boxes_each(comm):
    from mg_ic_code_amd.horizon import expansion_points
    n0, dx0 = (16, 16, 16), 0.625
    boxes = [TS._split(n0, (2, 1, 1)),
             [(8, 8, 8, 23, 15, 23), (8, 16, 8, 23, 23, 23)],
             [(24, 24, 24, 39, 39, 31), (24, 24, 32, 39, 39, 39)]]
    rng = np.random.default_rng(23)
    pts = np.concatenate([TS._points(n0, dx0, nrand=200, seed=8), rng.uniform(-4.5, 4.5, (150, 3)) * dx0,
                          rng.uniform(-2.3, 2.3, (150, 3)) * dx0])
    nrm, dv = _normals(len(pts), seed=44)
    psi, lw = _device(comm, n0, dx0, boxes, 9, True)
    h, hl = _reference(n0, dx0, boxes, 9, True)
    got = expansion_points(psi, pts, nrm, dv, None, punctures=ZERO, momentum=lw)
    _bits(got, _ref("three", h, hl, ZERO, pts, nrm, dv), True, "three levels")
    assert set(np.unique(got.level)) == {-1, 0, 1, 2}
    # one level fewer: level 1 is then the finest and nothing of it is covered
    h2, hl2 = _reference(n0, dx0, boxes[:2], 9, True)
    got = expansion_points(psi[:2], pts, nrm, dv, None, punctures=ZERO, momentum=LW(lw.per_level[:2]))
    _bits(got, H.expansion(h2, ZERO, pts, nrm, dv, hl2), True, "the first two levels")


@pytest.mark.gpu
@pytest.mark.parametrize("npts", [1, 257, 70000])
def test_point_counts(comm, npts):
    from mg_ic_code_amd.horizon import expansion_points
    base = TS._points(ONE["n0"], ONE["dx0"])
    nrm, dv = _normals(len(base))
    psi, lw = _device(comm, ONE["n0"], ONE["dx0"], ONE_BOXES, 1, True)
    h, hl = _reference(ONE["n0"], ONE["dx0"], ONE_BOXES, 1, True)
    want = _ref(("one", True), h, hl, ZERO, base, nrm, dv)
    # point p of the call is base point (7 p + 11) mod len(base): every thread
    # is independent, so the expected answer is the restatement's, re-indexed
    idx = (7 * np.arange(npts) + 11) % len(base)
    got = expansion_points(psi, base[idx], nrm[idx], dv[idx], None, punctures=ZERO, momentum=lw)
    sub = SimpleNamespace(**{k: (v[idx] if v is not None else None) for k, v in vars(want).items()})
    _bits(got, sub, True, f"npts = {npts}")


@pytest.mark.gpu
@pytest.mark.parametrize("table_name", ["two", "three"])
@pytest.mark.parametrize("with_lw", [False, True])
def test_real_tables_against_the_restatement(comm, table_name, with_lw):
    from mg_ic_code_amd.horizon import expansion_points
    table = dict(two=adm_ref.TWO_HOLES, three=adm_ref.THREE_HOLES)[table_name]
    pts = TS._points(ONE["n0"], ONE["dx0"])
    # and points on and next to the punctures
    near = np.array([list(r[1:4]) for r in table])
    pts = np.concatenate([pts, near, near + 1e-3, near - np.array([0.0, 0.2, 0.0])])
    nrm, dv = _normals(len(pts), seed=47)
    psi, lw = _device(comm, ONE["n0"], ONE["dx0"], ONE_BOXES, 1, with_lw)
    h, hl = _reference(ONE["n0"], ONE["dx0"], ONE_BOXES, 1, with_lw)
    want = _ref(("real", table_name, with_lw), h, hl, table, pts, nrm, dv)
    got = expansion_points(psi, pts, nrm, dv, None, punctures=table, momentum=lw)
    assert H.same_bits(got.level, want.level) and H.same_bits(got.order, want.order)
    on = np.zeros(len(pts), bool)
    on[len(pts) - 3 * len(near):len(pts) - 2 * len(near)] = True
    # a point on a puncture: not refused, nothing finite
    assert np.all(got.order[on] == 4) and not np.any(np.isfinite(got.theta[on]))
    keep = ~on
    sub = lambda r: SimpleNamespace(out=r.out[keep], scale=r.scale[keep])  # noqa: E731
    g = SimpleNamespace(theta=got.theta[keep], psi=got.psi[keep], dpsi=got.dpsi[keep],
                        a_nn=got.a_nn[keep], order=got.order[keep])
    ratio = _close(g, sub(want), f"{table_name}, lw {with_lw}")
    print(f"{table_name} holes, lw {with_lw}: worst error / sum of |contributions| "
          f"(theta, psi, dpsi_x, dpsi_y, dpsi_z, A_nn) =", ratio)
    assert np.any(got.a_nn[keep & (got.order > 0)] != 0.0)


# ---------------------------------------------------------------- the finder on the device
FINDER = dict(n=24, dx=0.25)


def _unit_psi(comm, level1=None):
    import mg_ic_code_amd as mg
    n, dx = FINDER["n"], FINDER["dx"]
    dom = (0, 0, 0, n - 1, n - 1, n - 1)
    grids = [mg.Grid(comm, dom, [dom], dx)]
    if level1:
        grids.append(mg.Grid(comm, (0, 0, 0, 2 * n - 1, 2 * n - 1, 2 * n - 1), level1, dx / 2,
                             patches=True))
    out = []
    for g in grids:
        f = mg.LevelData(g)
        f.set_val_all(TS.POISON)
        f.set_val(1.0)
        out.append(f)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,table,r0", [("schw", SCHW, 1.3), ("bl04", BL_CLOSE, 1.5)])
def test_finder_on_the_device_follows_the_numpy_evaluator(comm, name, table, r0):
    from mg_ic_code_amd.horizon import find_horizon
    want = found(name, table, (0.0, 0.0, 0.0), r0)
    got = find_horizon(_unit_psi(comm), None, (0.0, 0.0, 0.0), r0, punctures=table)
    rate = [b / a for a, b in zip(got.steps[-6:], got.steps[-5:])]
    print(name, got.status, got.iterations, repr(got.irreducible_mass), "contraction", rate)
    assert (got.status, got.iterations) == (want.status, want.iterations) and got.found
    a00 = r0 * math.sqrt(4.0 * math.pi)
    assert np.max(np.abs(got.coeffs - want.coeffs)) <= 10 * TOL * a00
    assert got.steps[-1] <= TOL * got.r_mean and want.steps[-1] <= TOL * want.r_mean
    assert all(0.4 <= r <= 0.65 for r in rate), rate      # about 0.5 per step (measured 0.5407)
    assert got.degraded_points == 0 and got.enclosed == want.enclosed
    assert abs(got.irreducible_mass - want.irreducible_mass) <= 1e-9


@pytest.mark.gpu
def test_finder_on_the_device_collapse_and_left_grid(comm):
    from mg_ic_code_amd.horizon import find_horizon
    psi = _unit_psi(comm)
    r = find_horizon(psi, None, (0.0, 0.0, 0.0), 1.5, punctures=BL_FAR)
    assert r.status == "collapsed" and not r.found
    assert r.iterations == found("bl12", BL_FAR, (0.0, 0.0, 0.0), 1.5).iterations
    # the domain is +-3: a start radius of 3.2 reaches outside
    r = find_horizon(psi, None, (0.0, 0.0, 0.0), 3.2, punctures=SCHW)
    assert r.status == "left_grid" and not r.found and r.iterations == 0
    assert math.isnan(r.area) and len(r.lines()) == 1


# level 1 over coarse cells (14..16, 14..16, 11..12) of 24: x, y in [0.5, 1.25),
# z in [-0.25, 0.25).  Its faces x = 0.5, y = 0.5 and z = +-0.25 cut through the
# horizon of the off-centre hole (the corner (0.5, 0.5, -0.25) is 0.51 from the
# puncture, the corner (1.25, 1.25, 0.25) is 1.57).
CUT_PATCH = [(28, 28, 22, 33, 33, 25)]


@pytest.mark.gpu
def test_finder_with_a_patch_face_through_the_horizon(comm):
    """The off-centre Schwarzschild case with a level-1 patch whose faces cut
    through the horizon: the same result, some points at order 2.

    The rule has no candidate below order 2, so a point within half a fine cell
    inside a patch face, or within half a coarse cell outside it, has no
    stencil (order 0) and would end the flow as "left_grid".  The patch is
    placed where the flow from r0 = 1.3 moves the surface least (the hole is
    displaced towards it), and of all boxes of 1 to 6 coarse cells a side that
    cut the horizon it is one of the 31 that keep every point of every
    iteration out of those slabs; the nearest any point comes to a slab's edge
    is 4.8e-3 (the numpy flow with tests/horizon_ref.py on the same hierarchy),
    against 1e-10 between the device's flow and that one.  Measured there: 38
    iterations, 6 of the 288 final points on level 1, 25 below order 4."""
    from mg_ic_code_amd.horizon import find_horizon
    want = found("schw", SCHW, (0.0, 0.0, 0.0), 1.3)
    got = find_horizon(_unit_psi(comm, CUT_PATCH), None, (0.0, 0.0, 0.0), 1.3, punctures=SCHW)
    print(got.status, got.iterations, got.degraded_points, repr(got.area))
    assert got.found and got.status == "converged" and got.iterations == want.iterations
    assert np.max(np.abs(got.coeffs - want.coeffs)) <= 10 * TOL * 1.3 * math.sqrt(4.0 * math.pi)
    assert abs(got.area - 64.0 * math.pi) / (64.0 * math.pi) <= 1e-12
    assert got.degraded_points > 0


# ---------------------------------------------------------------- refusals, ledger, end to end
def _raw(comm, psi, lw, table, pts, npts=None, nlev=None, npunct=None):
    """The arguments of mgic_horizon_expansion and its output arrays."""
    xyz = np.ascontiguousarray(pts, dtype=np.float64)
    n = len(xyz) if npts is None else npts
    nrm = np.ascontiguousarray(np.tile([0.0, 0.0, 1.0], (max(len(xyz), 1), 1)))
    dv = np.ones(max(len(xyz), 1))
    out = (np.zeros((max(len(xyz), 1), 6)), np.zeros(max(len(xyz), 1), np.int32),
           np.zeros(max(len(xyz), 1), np.int32))
    PD, PI = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    handles = (ctypes.c_void_p * max(len(psi), 1))(*[f.handle.value if f is not None else None
                                                     for f in psi])
    lwh = None if lw is None else (ctypes.c_void_p * len(lw))(
        *[f.handle.value if f is not None else None for f in lw])
    t = np.ascontiguousarray(np.array(table, dtype=np.float64).ravel())
    keep = (xyz, nrm, dv, t, handles, lwh)
    return [comm.handle, len(psi) if nlev is None else nlev, handles, lwh,
            len(t) // 10 if npunct is None else npunct, t.ctypes.data_as(PD), n,
            xyz.ctypes.data_as(PD), nrm.ctypes.data_as(PD), dv.ctypes.data_as(PD),
            out[0].ctypes.data_as(PD), out[1].ctypes.data_as(PI), out[2].ctypes.data_as(PI)], out, keep


@pytest.mark.gpu
def test_refusals_leave_the_ledger_untouched(comm, tmp_path):
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import _lib
    from mg_ic_code_amd.core import read_launch_ledger
    from mg_ic_code_amd.horizon import expansion_points

    def ledger():
        p = tmp_path / "horizon.ledger"
        _lib.horizon_call("mgic_horizon_launch_ledger_dump", str(p).encode())
        return read_launch_ledger(p)

    def field(grid):
        f = mg.LevelData(grid)
        f.set_val_all(1.0)
        return f

    dom = (0, 0, 0, 15, 15, 15)
    g0 = mg.Grid(comm, dom, [dom], 1.0)
    g1 = mg.Grid(comm, (0, 0, 0, 31, 31, 31), TS.PATCH, 0.5, patches=True)
    base, fine = field(g0), field(g1)
    lw0, lw1 = [field(g0) for _ in range(6)], [field(g1) for _ in range(6)]
    pts = np.array([[0.1, 0.2, 0.3], [1.0, 2.0, 3.0]])
    T = adm_ref.TWO_HOLES
    args, out, _k = _raw(comm, [base, fine], lw0 + lw1, T, pts)
    start = ledger()
    _lib.horizon_call("mgic_horizon_expansion", *args)  # the accepted call the refusals are held against
    assert np.all(out[1] == 1) and np.all(out[2] == 4) and np.all(np.isfinite(out[0]))
    before = ledger()
    assert sorted(before) == ["k_horizon_expansion<false>", "k_horizon_expansion<true>"]
    # one launch per call, whatever the number of levels, boxes and points
    assert before["k_horizon_expansion<true>"] == start["k_horizon_expansion<true>"] + 1
    assert before["k_horizon_expansion<false>"] == start["k_horizon_expansion<false>"]
    shifted = field(mg.Grid(comm, (1, 0, 0, 16, 15, 15), [(1, 0, 0, 16, 15, 15)], 1.0))
    periodic = field(mg.Grid(comm, dom, [dom], 1.0, periodic=(1, 1, 1)))
    periodic_x = field(mg.Grid(comm, dom, [dom], 1.0, periodic=(1, 0, 0)))
    periodic_fine = field(mg.Grid(comm, (0, 0, 0, 31, 31, 31), TS.PATCH, 0.5, periodic=(1, 1, 1),
                                  patches=True))
    same_size = field(mg.Grid(comm, dom, [(4, 4, 4, 11, 11, 11)], 0.5, patches=True))
    by_four = field(mg.Grid(comm, (0, 0, 0, 63, 63, 63), [(16, 16, 16, 47, 47, 47)], 0.25, patches=True))
    lw_split = [field(mg.Grid(comm, dom, TS._split((16, 16, 16), (2, 1, 1)), 1.0)) for _ in range(6)]
    lw_dx = [field(mg.Grid(comm, dom, [dom], 0.5)) for _ in range(6)]
    nan_table = [list(T[0]), list(T[1])]
    nan_table[1][5] = float("nan")
    inf_table = [list(T[0]), list(T[1])]
    inf_table[0][0] = float("inf")
    cases = {
        "nlev 0": _raw(comm, [base], None, T, pts, nlev=0),
        "nlev 9": _raw(comm, [base] * 9, None, T, pts),
        "npts 0": _raw(comm, [base], None, T, pts, npts=0),
        "npts 2^20 + 1": _raw(comm, [base], None, T, pts, npts=(1 << 20) + 1),
        "low corner not 0": _raw(comm, [shifted], None, T, pts),
        "level 1 not refined": _raw(comm, [base, same_size], None, T, pts),
        "level 1 refined by 4": _raw(comm, [base, by_four], None, T, pts),
        "levels in the wrong order": _raw(comm, [fine, base], None, T, pts),
        "a null field": _raw(comm, [base, None], None, T, pts),
        "periodic": _raw(comm, [periodic], None, T, pts),
        "periodic in x": _raw(comm, [periodic_x], None, T, pts),
        "a periodic level 1": _raw(comm, [base, periodic_fine], None, T, pts),
        "no punctures": _raw(comm, [base], None, T, pts, npunct=0),
        "nine punctures": _raw(comm, [base], None, [T[0]] * 9, pts),
        "a NaN in the table": _raw(comm, [base], None, nan_table, pts),
        "an inf in the table": _raw(comm, [base], None, inf_table, pts),
        "lw on other boxes": _raw(comm, [base], lw_split, T, pts),
        "lw with another spacing": _raw(comm, [base], lw_dx, T, pts),
        "lw of the other level": _raw(comm, [base, fine], lw0 + lw0, T, pts),
        "a null among lw": _raw(comm, [base, fine], lw0 + lw1[:5] + [None], T, pts),
        "a null first lw": _raw(comm, [base], [None] + lw0[1:], T, pts),
    }
    for name, at in (("comm", 0), ("psi", 2), ("table", 5), ("xyz", 7), ("normal", 8), ("divn", 9),
                     ("out", 10), ("level_used", 11), ("order_used", 12)):
        a = _raw(comm, [base, fine], lw0 + lw1, T, pts)
        a[0][at] = None
        cases["null " + name] = a
    for name, (a, _o, _k) in cases.items():
        with pytest.raises(mg.MgicError) as e:
            _lib.horizon_call("mgic_horizon_expansion", *a)
        assert e.value.code == -1, (name, str(e.value))
    # the same through the package: a ValueError
    up, one = np.tile([0.0, 0.0, 1.0], (2, 1)), np.ones(2)
    for psi, lw, table in (([base, same_size], None, T), ([shifted], None, T), ([periodic], None, T),
                           ([fine, base], None, T), ([base], LW([lw_split]), T),
                           ([base, fine], LW([lw0]), T), ([base], None, [T[0]] * 9)):
        with pytest.raises(ValueError):
            expansion_points(psi, pts, up, one, None, punctures=table, momentum=lw)
    assert ledger() == before


def _worker(*args):
    env = dict(os.environ)
    env.pop("MGIC_LAUNCH_LEDGER", None)
    r = subprocess.run([sys.executable, WORKER] + [str(a) for a in args], capture_output=True,
                       text=True, env=env, timeout=WORKER_TIMEOUT)
    assert r.returncode == 0, f"{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return r.stdout


def run_kernel_cases(comm):
    """What tests/horizon_worker.py runs before it dumps the ledger: both
    instantiations of k_horizon_expansion against the restatement."""
    _one_box(comm, False)
    _one_box(comm, True)


@pytest.mark.gpu
def test_every_kernel_of_the_horizon_library_is_launched_against_its_reference(tmp_path):
    from mg_ic_code_amd.core import read_launch_ledger
    out = tmp_path / "horizon.ledger"
    _worker("kernel", out)
    ledger = read_launch_ledger(out)
    assert sorted(ledger) == ["k_horizon_expansion<false>", "k_horizon_expansion<true>"], ledger
    missing = sorted(n for n, c in ledger.items() if c == 0)
    assert not missing, f"{len(missing)} of {len(ledger)} kernels never launched:\n" + "\n".join(missing)


def _check_solve(out, level):
    assert out["loaded_after_plain_solve"] is False and out["loaded_after_flag_solve"] is True
    assert out["same_solve"] and out["same_report"] and out["deck_key_same"]
    assert out["found"] == [True, True] and out["enclosed"] == [[0], [1]]
    assert out["levels"] == [level]
    print("M_irr:", out["M_irr"], "M_chr:", out["M_chr"], "M_i (3o):", out["M_i"])
    print("iterations:", out["iterations"], "degraded:", out["degraded"])
    print("oracle M_irr:", out["M_irr_oracle"], "dM_irr/du:", out["sensitivity"])
    # the bar at which the suite compares the two psi (1e-10 of the norm, psi of
    # order 1) times the measured sensitivity of M_irr to a uniform shift of u
    for got, want, s in zip(out["M_irr"], out["M_irr_oracle"], out["sensitivity"]):
        assert abs(got - want) <= 1e-10 * abs(s) * out["psi_scale"], (got, want, s)
    assert all(e <= 1e-10 for e in out["psi_rel_l2"])
    for m, c in zip(out["M_irr"], out["M_chr"]):
        assert c >= m > 0.0


@pytest.mark.gpu
def test_solve_with_horizons_is_the_same_solve_and_off_loads_nothing():
    # a fresh process (tests/horizon_worker.py solve): without the switch
    # libmgic_horizon.so stays unloaded; with horizons="punctures" (the keyword,
    # and the deck's key) psi, the norms, the iteration counts and libmgic's
    # ledger are the plain solve's, NLResult.horizons is find_horizon(res.psi,
    # ...) bit for bit, both horizons are found, and M_irr is that of the numpy
    # evaluator fed the restatement on the CPU oracle's psi
    _check_solve(json.loads(_worker("solve").strip().splitlines()[-1]), 0)


@pytest.mark.gpu
def test_solve_with_horizons_on_two_levels():
    _check_solve(json.loads(_worker("solve2").strip().splitlines()[-1]), 1)


@pytest.mark.gpu
def test_a_box_that_is_not_local_is_refused(tmp_path):
    # two ranks on the one device, as tests/test_sample.py runs them: each holds
    # one box of the level and not the other
    import socket
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", PYTHONUNBUFFERED="1")
    env.pop("MGIC_LAUNCH_LEDGER", None)
    logs = [open(tmp_path / f"w{r}.log", "w") for r in range(2)]
    procs = [subprocess.Popen([sys.executable, WORKER, "nonlocal", str(r), str(port), str(tmp_path)],
                              stdout=logs[r], stderr=subprocess.STDOUT, env=env) for r in range(2)]
    try:
        rcs = [p.wait(timeout=WORKER_TIMEOUT) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
        for log in logs:
            log.close()
    texts = [(tmp_path / f"w{r}.log").read_text() for r in range(2)]
    assert rcs == [0, 0], "\n".join(t[-3000:] for t in texts)
    for r in range(2):
        out = json.loads((tmp_path / f"rank{r}.json").read_text())
        assert out["code"] == -1 and "must be local" in out["message"], out
        assert out["value_error"] is True
        assert sorted(out["ledger"]) == ["k_horizon_expansion<false>", "k_horizon_expansion<true>"]
        assert not any(out["ledger"].values()), out["ledger"]


@pytest.mark.gpu
def test_run_poisson_cli_lines(tmp_path):
    # the tool against the same solve through the library, both in fresh
    # processes (tests/horizon_worker.py cli): the horizon lines, M_irr next to
    # M_i with --puncture-masses, and the JSON keys
    out = json.loads(_worker("cli", tmp_path).strip().splitlines()[-1])
    assert out["punctures_lines_same"] and out["punctures_json_same"], out
    assert out["explicit_lines_same"] and out["explicit_json_same"], out
    assert out["n_lines"] >= 8 and out["mirr_next_to_mi"] == 2
