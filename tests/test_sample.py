"""A field of the hierarchy at points (mg_ic_code_amd/sample.py,
libmgic_sample.so) against the numpy restatement
tests/sample_ref.py.

CPU: the restatement itself (polynomial reproduction, the weights, the degrade
order), the puncture-mass arithmetic, the deck keys, the refusals, and the
target-mass fixed point on the CPU oracle.  GPU: values, levels and orders bit
for bit against the restatement on one box, three box layouts, a periodic box,
two and three levels; refusals and ledger coverage; the solve end to end; the
target-mass solve; the command-line tool.
"""
import ctypes
import dataclasses
import json
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from tests import sample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "sample_worker.py")
WORKER_TIMEOUT = 300
U = 2.0 ** -53
START = (0.5, 0.35)     # the issue's bare masses and targets
TARGETS = (1.0, 0.7)


# ------------------------------------------------------------------ CPU
def _poly_field(coef, n, dx):
    """coef[a][b][c] x^a y^b z^c at the cell centres of an n^3 box about the
    origin; with small integer coefficients and dx a power of two every value
    is exact."""
    x = (np.arange(n) + 0.5) * dx - n * dx / 2.0
    full = np.zeros((n, n, n))
    for a in range(coef.shape[0]):
        for b in range(coef.shape[1]):
            for c in range(coef.shape[2]):
                full += coef[a, b, c] * (x[None, None, :] ** a) * (x[None, :, None] ** b) \
                    * (x[:, None, None] ** c)
    return full


def _poly_exact(coef, p):
    x, y, z = (Fraction(float(v)) for v in p)
    return sum(int(coef[a, b, c]) * x ** a * y ** b * z ** c for a in range(coef.shape[0])
               for b in range(coef.shape[1]) for c in range(coef.shape[2]))


def test_restatement_reproduces_polynomials(rng):
    # Exact data (integer coefficients, dx = 1/2) at points that are multiples
    # of 2^-20, so x + half, q, s and t are exact and the interpolant of exact
    # arithmetic IS the polynomial.  What is left is the restatement's own
    # rounding, relative to each term |wz wy wx u|: order 4 rounds a weight 3
    # times (two products, one division), each nest level once for the product
    # and at most 3 times for the additions: 3 * (3 + 1 + 3) = 21 roundings;
    # order 2 has exact weights (1 - t is exact), one product and one addition
    # per level: 6.  The bars are 24 U and 8 U of the sum of absolute
    # contributions (3 and 2 roundings of slack for that sum's own rounding).
    n, dx = 12, 0.5
    for order, deg, bar in ((4, 4, 24 * U), (2, 2, 8 * U)):
        worst = 0.0
        for _ in range(3):
            coef = rng.integers(-3, 4, (deg, deg, deg))
            h = R.single_box(_poly_field(coef, n, dx), dx)
            pts = rng.integers(-2 * 2 ** 20, 2 * 2 ** 20, (40, 3)) / 2.0 ** 20
            vals, lev, used = R.sample(h, pts, order)
            assert np.all(used == order) and np.all(lev == 0)
            for p, v in zip(pts, vals):
                scale = R.abs_sum(h, p, order)
                err = abs(Fraction(float(v)) - _poly_exact(coef, p))
                worst = max(worst, float(err) / scale)
                assert err <= Fraction(bar) * Fraction(scale), (order, p, float(err), scale)
        print(f"order {order}: worst error / sum of |contributions| = {worst / U:.2f} U")


def test_cubic_weights_sum_to_one(rng):
    worst = 0.0
    from mg_ic_code_amd.sample import cubic_weights, linear_weights
    for t in rng.uniform(0.0, 1.0, 1000):
        w = R.weights4(float(t))
        # the package states the same expressions: bit for bit
        assert w == cubic_weights(float(t)) and R.weights2(float(t)) == linear_weights(float(t))
        worst = max(worst, abs(((w[0] + w[1]) + w[2]) + w[3] - 1.0))
    print("worst |sum w - 1| =", worst / 2.0 ** -52, "ulp")
    assert worst <= 4 * 2.0 ** -52
    assert R.weights4(0.0) == [0.0, 1.0, 0.0, 0.0] and R.weights4(1.0) == [0.0, 0.0, 1.0, 0.0]
    assert R.weights2(0.25) == [0.75, 0.25]


def _two_level_ref(level1_boxes, seed=7, n0=16, dx0=1.0):
    rng = np.random.default_rng(seed)
    full = [rng.uniform(0.5, 1.5, (n0 << l,) * 3) for l in range(2)]
    levels = [[((0, 0, 0), (n0 - 1,) * 3, full[0])],
              [(b[:3], b[3:], full[1][b[2]:b[5] + 1, b[1]:b[4] + 1, b[0]:b[3] + 1])
               for b in level1_boxes]]
    return R.Hierarchy((n0,) * 3, dx0, levels), full


PATCH = [(8, 8, 8, 23, 23, 23)]                                 # coarse cells 4..11
LSHAPE = [(8, 8, 8, 23, 15, 23), (8, 16, 8, 15, 23, 23)]        # an L in the x-y plane


def test_degrade_order_next_to_a_domain_face(rng):
    h = R.single_box(rng.uniform(0.5, 1.5, (16, 16, 16)), 1.0)
    # x measured in cells from the low face: the 4-stencil needs cells i-1..i+2
    for off, want in ((0.2, 1), (0.49, 1), (0.5, 2), (1.2, 2), (1.49, 2), (1.5, 4), (3.3, 4),
                      (14.49, 4), (14.5, 2), (15.49, 2), (15.5, 1), (15.99, 1)):
        for d in range(3):
            p = [0.3, -0.4, 0.2]
            p[d] = off - 8.0
            v, lev, used = R.sample_one(h, p, 4)
            assert (lev, used) == (0, want), (off, d, used)
            assert R.sample_one(h, p, 2)[2] == min(want, 2)
            assert R.sample_one(h, p, 1)[2] == 1
    assert R.sample_one(h, (8.0, 0.0, 0.0))[1:] == (-1, 0)      # the high face is outside
    assert R.sample_one(h, (-8.0, 0.0, 0.0))[1:] == (0, 1)      # the low face is inside
    assert R.sample_one(h, (float("nan"), 0.0, 0.0))[1:] == (-1, 0)
    assert math.isnan(R.sample_one(h, (0.0, float("inf"), 0.0))[0])


def test_degrade_order_at_a_coarse_fine_boundary():
    h, full = _two_level_ref(PATCH)
    # the patch is fine cells 8..23 = coarse cells 4..11 = x in [-4, 4)
    inside = lambda x: R.sample_one(h, (x, 0.1, -0.2))[1:]      # noqa: E731
    assert inside(0.1) == (1, 4)
    assert inside(3.9) == (1, 1)       # fine cell 23: s = 23.3, cells 22..25
    assert inside(3.7) == (1, 2)       # s = 22.9: cells 22, 23
    assert inside(3.2) == (1, 4)       # s = 21.9: cells 20..23
    assert inside(3.26) == (1, 2)      # s = 22.02: cells 21..24
    # from the coarse side: coarse cells 4..11 are covered and never read
    assert inside(4.1) == (0, 1)       # coarse cell 12, s = 11.6: cells 11, 12
    assert inside(4.6) == (0, 2)       # s = 12.1: cells 12, 13 (y, z: 7, 8 -- not covered at x >= 12)
    assert inside(5.4) == (0, 2)       # s = 12.9: the 4-stencil starts at 11
    assert inside(5.6) == (0, 4)       # s = 13.1: cells 12..15
    assert inside(-4.1) == (0, 1) and inside(-5.7) == (0, 4)
    # the value just outside is the coarse cell's own, never the covered neighbour's
    assert R.sample_one(h, (4.1, 0.1, -0.2))[0] == full[0][7, 8, 12]
    # a covered level-0 cell is not level 0's: deep in the patch nothing of level 0 is used
    for x in (-3.0, 0.0, 2.0):
        assert R.sample_one(h, (x, x, x))[1] == 1


def test_degrade_order_at_a_concave_corner():
    h, _ = _two_level_ref(LSHAPE)
    # level 1: x fine 8..23 for y fine 8..15, x fine 8..15 for y fine 16..23.
    # The concave corner is at x = 0, y = 0 (fine cell 16, 16 is missing).
    at = lambda x, y: R.sample_one(h, (x, y, 0.1))[1:]          # noqa: E731
    assert at(-1.5, -1.5) == (1, 4)     # cells 11..14 in x and y: all in the L
    assert at(-0.6, -0.6) == (1, 2)     # s = 14.3: 4-stencil 13..16 holds (16, 16); 2-stencil 14, 15
    assert at(-0.1, -0.1) == (1, 1)     # s = 15.3: cells 15, 16 hold (16, 16)
    assert at(-0.1, -1.5) == (1, 4)     # along the long arm x runs on to 23
    assert at(-1.5, -0.1) == (1, 4)
    assert at(0.2, 0.2) == (0, 1)       # coarse cell (8, 8): its neighbours 7 are covered
    assert at(1.7, 1.7) == (0, 4)       # s = 9.2: coarse cells 8..11, none covered
    assert at(0.7, 0.7) == (0, 2)       # s = 8.2: the 4-stencil reaches the covered 7


# a spacing and a point just inside the high face (found by search) at which
# r < len and yet r / dx rounds to N: the cell is the last one, not outside
EDGE_N, EDGE_DX, EDGE_X = 12, 1.0658299143456331, 6.394979486073797


def test_point_just_inside_the_high_face_takes_the_last_cell(rng):
    full = rng.uniform(0.5, 1.5, (EDGE_N,) * 3)
    half, length = EDGE_N * EDGE_DX / 2.0, EDGE_N * EDGE_DX
    r = EDGE_X + half
    assert r < length and math.floor(r / EDGE_DX) == EDGE_N
    for d in range(3):
        p = [0.3, -0.4, 0.2]
        p[d] = EDGE_X
        want = [6, 5, 6]
        want[d] = EDGE_N - 1
        v, lev, used = R.sample_one(R.single_box(full, EDGE_DX), p)
        assert (lev, used) == (0, 1) and v == full[want[2], want[1], want[0]]
        v, lev, used = R.sample_one(R.single_box(full, EDGE_DX, (1, 1, 1)), p)
        assert (lev, used) == (0, 4) and np.isfinite(v)


def test_restatement_does_not_depend_on_the_box_layout(rng):
    full = rng.uniform(0.5, 1.5, (16, 16, 16))
    one = R.single_box(full, 1.0)
    boxes = [((i, j, k), (i + 7, j + 7, k + 7), full[k:k + 8, j:j + 8, i:i + 8])
             for k in (0, 8) for j in (0, 8) for i in (0, 8)]
    eight = R.Hierarchy((16,) * 3, 1.0, [boxes])
    pts = rng.uniform(-8.5, 8.5, (60, 3))
    pts[:8] = rng.uniform(-1.0, 1.0, (8, 3))
    a, b = R.sample(one, pts), R.sample(eight, pts)
    assert all(R.same_bits(x, y) for x, y in zip(a, b))


def test_puncture_mass_arithmetic_on_a_stub():
    from mg_ic_code_amd import _lib
    from mg_ic_code_amd.punctures import PunctureSet
    from mg_ic_code_amd.sample import (adm_masses, check_distinct, mass_report, puncture_masses)
    table = PunctureSet([(0.5, 3.0, 0.0, 0.0, 0, 0.05, 0, 0, 0, 0.1),
                         (0.35, 0.0, 4.0, 0.0, 0, 0, 0, 0, 0, 0),
                         (0.2, 0.0, 0.0, -12.0, 0, 0, 0, 0, 0, 0)])  # an odd count
    u = [1.25, 1.5, 1.125]
    M = adm_masses(table, u)
    want = [2 * 0.5 * (1.25 + 0.35 / 5.0 + 0.2 / math.sqrt(153.0)),
            2 * 0.35 * (1.5 + 0.5 / 5.0 + 0.2 / math.sqrt(160.0)),
            2 * 0.2 * (1.125 + 0.5 / math.sqrt(153.0) + 0.35 / math.sqrt(160.0))]
    np.testing.assert_allclose(M, want, rtol=4 * 2.0 ** -52)
    rep = mass_report(table, u, [2, 1, 0], [4, 2, 1])
    assert len(rep.punctures) == 3 and rep.adm_masses == M    # the odd table's dummy gets no row
    assert [p.level for p in rep.punctures] == [2, 1, 0]
    assert rep.punctures[1].position == (0.0, 4.0, 0.0) and rep.punctures[1].u == 1.5
    lines = rep.lines()
    assert len(lines) == 3 and lines[0].startswith("puncture mass 1: ")
    assert float(lines[2].split("M = ")[1]) == M[2] and "(level 0, order 1)" in lines[2]
    # one puncture: M = 2 m u
    assert adm_masses(PunctureSet([(0.7, 1, 2, 3, 0, 0, 0, 0, 0, 0)]), [1.5]) == [2 * 0.7 * 1.5]
    # two punctures at one position: refused before anything is loaded
    twice = [(0.5, 1.0, 2.0, 3.0, 0, 0, 0, 0, 0, 0), (0.3, 1.0, 2.0, 3.0, 0, 0, 0, 0, 0, 0)]
    with pytest.raises(ValueError, match="same position"):
        check_distinct(PunctureSet(twice))
    with pytest.raises(ValueError, match="same position"):
        puncture_masses(None, _deck(), punctures=twice)
    assert not _lib.sample_loaded()


def test_binding_covers_the_header():
    import re
    from mg_ic_code_amd import _lib
    with open(os.path.join(ROOT, "include", "mgic_sample.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"MGIC_SAMPLE_API\s+[^;()]*?\b(mgic_sample_\w+)\s*\(", text))
    assert declared == set(_lib.SAMPLE_SIGNATURES) and len(declared) == 4
    assert "#define MGIC_SAMPLE_MAX_LEVELS 8" in text
    assert "#define MGIC_SAMPLE_MAX_POINTS (1 << 20)" in text


def _deck_text():
    with open(os.path.join(ROOT, "tests", "golden", "params.txt")) as f:
        return f.read()


def _deck(n=16, **kw):
    """params.txt (Dirichlet, its two holes at x = +-10) at n cells a side."""
    from mg_ic_code_amd.params import read_params
    prm = read_params(_deck_text())
    assert prm.is_periodic == 0 and prm.puncture_masses == 0 and prm.target_masses is None
    return dataclasses.replace(prm, N=[n] * 3, coarsestDx=prm.L / n, max_level=0, **kw)


def test_deck_keys():
    from mg_ic_code_amd.params import read_params
    txt = _deck_text()
    assert read_params(txt + "\npuncture_masses = 1\n").puncture_masses == 1
    assert read_params(txt, {"puncture_masses": "0"}).puncture_masses == 0
    for bad in ("2", "-1", "yes", "0.5"):
        with pytest.raises(ValueError):
            read_params(txt + f"\npuncture_masses = {bad}\n")
    assert read_params(txt + "\ntarget_masses = 1.0 0.7\n").target_masses == [1.0, 0.7]
    table = "\nnum_punctures = 3\n" + "".join(
        f"puncture{i} = 0.{i} {i} 0 0 0 0 0 0 0 0\n" for i in (1, 2, 3))
    assert read_params(txt + table + "target_masses = 1 2 3\n").target_masses == [1.0, 2.0, 3.0]
    for bad in ("1.0", "1.0 0.7 0.2", "1.0 x", "1.0 0", "1.0 -0.7", "nan 1", "inf 1"):
        with pytest.raises(ValueError):
            read_params(txt + f"\ntarget_masses = {bad}\n")
    with pytest.raises(ValueError):
        read_params(txt + table + "target_masses = 1 2\n")


def test_solve_for_masses_refusals():
    from mg_ic_code_amd import _lib
    from mg_ic_code_amd.sample import SampleArgumentError, solve_for_masses
    prm = _deck()
    for targets in ([1.0], [1.0, 0.7, 0.2], [1.0, 0.0], [1.0, -0.7], [1.0, float("nan")],
                    ["x", 1.0], [], [True, 1.0]):
        with pytest.raises(ValueError) as e:
            solve_for_masses(None, prm, targets)
        assert isinstance(e.value, SampleArgumentError) and e.value.code == -1
    with pytest.raises(ValueError, match="bare mass 0"):
        solve_for_masses(None, dataclasses.replace(prm, bh2_bare_mass=0.0), [1.0, 0.7])
    with pytest.raises(ValueError, match="same position"):
        solve_for_masses(None, dataclasses.replace(prm, bh2_offset=prm.bh1_offset), [1.0, 0.7])
    with pytest.raises(ValueError, match="3 punctures"):
        solve_for_masses(None, prm, [1.0, 0.7],
                         punctures=[(0.1 * i, i, 0, 0, 0, 0, 0, 0, 0, 0) for i in (1, 2, 3)])
    with pytest.raises(ValueError, match="max_solves"):
        solve_for_masses(None, prm, [1.0, 0.7], max_solves=0)
    assert not _lib.sample_loaded()


def test_lineout_points_and_host_refusals():
    from mg_ic_code_amd import _lib
    from mg_ic_code_amd.sample import lineout_points, parse_lineout, sample_points
    s, pts = lineout_points((0, 0, 0), (3, 4, 0), 6)
    assert np.array_equal(s, np.arange(6.0)) and np.array_equal(pts[-1], (3.0, 4.0, 0.0))
    assert np.array_equal(pts[0], (0.0, 0.0, 0.0)) and pts.shape == (6, 3)
    s, pts = lineout_points((1, 2, 3), (4, 5, 6), 1)
    assert np.array_equal(s, [0.0]) and np.array_equal(pts, [[1.0, 2.0, 3.0]])
    assert parse_lineout("0 0 0 1 2 3 5") == ((0.0, 0.0, 0.0), (1.0, 2.0, 3.0), 5)
    for bad in ("0 0 0 1 2 3", "0 0 0 1 2 3 2.5", "a 0 0 1 2 3 4"):
        with pytest.raises(ValueError):
            parse_lineout(bad)
    for a, b, n in (((0, 0), (1, 1, 1), 3), ((0, 0, 0), (1, 1, 1), 0), ((0, 0, 0), (1, 1, 1), 2.5)):
        with pytest.raises(ValueError):
            lineout_points(a, b, n)
    # refused on the host: nothing is loaded
    for fields, pts, order in (([], [[0, 0, 0]], 4), ([None] * 9, [[0, 0, 0]], 4),
                               ([None], [[0, 0, 0]], 3), ([None], [[0, 0]], 4),
                               ([None], np.zeros((0, 3)), 4), ([None], [[0, 0, 0]], True)):
        with pytest.raises(ValueError):
            sample_points(fields, pts, order)
    assert not _lib.sample_loaded()


_FIXED = {}


def oracle_fixed_point(n=16, solves=8):
    """The issue's feasibility run: m_i <- m_i T_i / M_i on the CPU oracle
    (tests/nl_ref.oracle_poisson_solve, the Dirichlet deck, depth 2, its 6 NL
    iterations), psi at the punctures by the order-4 restatement.  Computed
    once: [(bare masses, ADM masses, error, u)] per solve."""
    if n not in _FIXED:
        from mg_ic_code_amd.punctures import PunctureSet
        from mg_ic_code_amd.sample import adm_masses
        from tests.nl_ref import oracle_poisson_solve
        masses, hist = list(START), []
        for _ in range(solves):
            prm = _deck(n, bh1_bare_mass=masses[0], bh2_bare_mass=masses[1])
            psi = oracle_poisson_solve(prm, n, max_depth=2, n_nl=prm.max_NL_iterations)[0]
            table = PunctureSet.from_params(prm)
            h = R.single_box(psi[1:-1, 1:-1, 1:-1], prm.domainLength[0] / n)
            u, lev, used = R.sample(h, [p.position for p in table], 4)
            assert np.all(lev == 0) and np.all(used == 4)
            M = adm_masses(table, u)
            hist.append((list(masses), M, max(abs(m - t) for m, t in zip(M, TARGETS)), list(u)))
            masses = [m * t / big for m, t, big in zip(masses, TARGETS, M)]
        _FIXED[n] = hist
    return _FIXED[n]


def test_target_mass_fixed_point_on_the_oracle():
    hist = oracle_fixed_point()
    errs = [h[2] for h in hist]
    print("max|M - T| per solve:", errs)
    print("bare masses:", hist[-1][0])
    for a, b in zip(errs, errs[1:]):
        if a > 1e-10:
            assert b <= 0.1 * a, errs
    within = next(k + 1 for k, e in enumerate(errs) if e <= 1e-8 * max(TARGETS))
    assert within <= 6, errs
    np.testing.assert_allclose(hist[-1][0], (0.491558005, 0.341568662), rtol=0, atol=2e-9)


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def comm():
    import mg_ic_code_amd as mg
    return mg.Comm()


POISON = 1e300  # in every ghost cell: a ghost read cannot go unnoticed


def _split(n, parts):
    edges = [np.linspace(0, n[d], parts[d] + 1).astype(int) for d in range(3)]
    return [(int(edges[0][i]), int(edges[1][j]), int(edges[2][k]),
             int(edges[0][i + 1]) - 1, int(edges[1][j + 1]) - 1, int(edges[2][k + 1]) - 1)
            for k in range(parts[2]) for j in range(parts[1]) for i in range(parts[0])]


def _field(grid, full):
    """A LevelData holding the level's (nz, ny, nx) array in its boxes."""
    import mg_ic_code_amd as mg
    f = mg.LevelData(grid)
    f.set_val_all(POISON)
    for n in range(grid.num_local):
        b = grid.local_box(n)
        f.upload(n, full[b[2]:b[5] + 1, b[1]:b[4] + 1, b[0]:b[3] + 1])
    return f


_FULL = {}


def _full(n0, nlev, seed):
    """The random arrays of a hierarchy, one per level over its whole domain."""
    key = (tuple(n0), nlev, seed)
    if key not in _FULL:
        rng = np.random.default_rng(seed)
        _FULL[key] = [rng.uniform(0.5, 1.5, (n0[2] << l, n0[1] << l, n0[0] << l))
                      for l in range(nlev)]
    return _FULL[key]


def _device(comm, n0, dx0, level_boxes, periodic=(0, 0, 0), seed=1):
    """One LevelData per level with the arrays of _full in the given boxes."""
    import mg_ic_code_amd as mg
    full = _full(n0, len(level_boxes), seed)
    out = []
    for l, boxes in enumerate(level_boxes):
        dom = (0, 0, 0) + tuple((n << l) - 1 for n in n0)
        grid = mg.Grid(comm, dom, boxes, dx0 / 2 ** l, periodic=periodic, patches=l > 0)
        out.append(_field(grid, full[l]))
    return out


def _reference(n0, dx0, level_boxes, periodic=(0, 0, 0), seed=1):
    full = _full(n0, len(level_boxes), seed)
    return R.Hierarchy(n0, dx0, [[(b[:3], b[3:], full[l][b[2]:b[5] + 1, b[1]:b[4] + 1, b[0]:b[3] + 1])
                                  for b in boxes] for l, boxes in enumerate(level_boxes)], periodic)


def _points(n0, dx0, nrand=500, seed=3):
    """Random points (a few outside), cell centres, points exactly on cell
    faces, the box corners, points within 1.5 cells of each domain face, around
    the centre (where 2 x 2 x 2 boxes meet), outside, NaN and inf."""
    rng = np.random.default_rng(seed)
    half = np.array(n0) * dx0 / 2.0
    pts = [rng.uniform(-1.04, 1.04, (nrand, 3)) * half]
    cells = rng.integers(0, n0, (30, 3))
    pts.append((cells + 0.5) * dx0 - half)                       # cell centres
    faces = rng.integers(0, np.array(n0) + 1, (30, 3))
    pts.append(faces * dx0 - half)                               # on faces in all three directions
    mixed = (cells + 0.5) * dx0 - half
    mixed[:, 0] = faces[:, 0] * dx0 - half[0]                    # on an x face only
    pts.append(mixed)
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * half
    pts += [corners, corners * (1 - 1e-9), corners * 0.97]
    for d in range(3):
        for side in (-1, 1):
            for off in (0.0, 1e-7, 0.25, 0.49, 0.51, 0.75, 1.25, 1.49, 1.51, 2.2):
                p = rng.uniform(-0.6, 0.6, 3) * half
                p[d] = side * (half[d] - off * dx0)
                pts.append(p[None, :])
    pts.append(rng.uniform(-2.0, 2.0, (40, 3)) * dx0)            # around the centre
    centre = rng.uniform(-2.0, 2.0, (20, 3)) * dx0
    centre[:10, 1] = 0.0                                         # on the faces through the centre
    centre[5:15, 2] = 0.0
    pts.append(centre)
    pts.append(np.array([[half[0] + 0.1 * dx0, 0.0, 0.0], [0.0, -half[1] - 3.3 * dx0, 0.0],
                         [1e6, 0.0, 0.0], [0.0, 0.0, -1e6], [3.7 * half[0], -5.2 * half[1], 2.4 * half[2]],
                         [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -np.inf]]))
    return np.ascontiguousarray(np.concatenate(pts))


_REF = {}


def _ref(key, h, pts, order):
    """The restatement's answer, computed once per (case, order)."""
    if (key, order) not in _REF:
        _REF[(key, order)] = R.sample(h, pts, order)
    return _REF[(key, order)]


def _same(got, want, what=""):
    for name, w in zip(("values", "level", "order"), want):
        g = getattr(got, name)
        if not R.same_bits(g, w):
            bad = np.flatnonzero(~((g == w) | (np.isnan(g) & np.isnan(w)))
                                 if g.dtype.kind == "f" else g != w)
            raise AssertionError(f"{what}: {name} differ at {len(bad)} of {len(w)} points, first "
                                 f"{bad[:5]}: {g[bad[:5]]} != {w[bad[:5]]}")


ONE = dict(n0=(12, 8, 16), dx0=0.75)


def _one_box(comm, order):
    from mg_ic_code_amd.sample import sample_points
    boxes = [[(0, 0, 0, 11, 7, 15)]]
    fields = _device(comm, ONE["n0"], ONE["dx0"], boxes)
    pts = _points(ONE["n0"], ONE["dx0"])
    want = _ref("one", _reference(ONE["n0"], ONE["dx0"], boxes), pts, order)
    got = sample_points(fields[0], pts, order)
    _same(got, want, f"12x8x16, order {order}")
    _same(sample_points(fields, pts, order), want, "a second call")
    return got, pts


@pytest.mark.gpu
@pytest.mark.parametrize("order", [1, 2, 4])
def test_one_box_against_the_restatement(comm, order):
    got, pts = _one_box(comm, order)
    assert set(np.unique(got.order)) == {0} | {o for o in (1, 2, 4) if o <= order}
    assert set(np.unique(got.level)) == {-1, 0}
    outside = got.level < 0
    assert np.all(np.isnan(got.values[outside])) and np.all(got.order[outside] == 0)
    assert np.all(np.isfinite(got.values[~outside])) and np.all(got.values[~outside] < 2.0)
    assert 8 <= outside.sum() < 0.2 * len(pts)


def _two_levels(comm, name, level1):
    from mg_ic_code_amd.sample import sample_points
    n0, dx0 = (16, 16, 16), 0.625
    boxes = [[(0, 0, 0, 15, 15, 15)], level1]
    rng = np.random.default_rng(17)
    f = dx0 / 2  # a fine cell
    pts = [_points(n0, dx0, nrand=300, seed=5),
           rng.uniform(-3.0, 3.0, (60, 3)) * dx0,                  # deep in the patch
           rng.uniform(-4.0, 4.0, (120, 3)) * dx0]                 # all over it
    for d in range(3):
        for side in (-1, 1):
            for off in (-2.2, -1.4, -0.6, -1e-9, 0.0, 0.3, 0.8, 1.3, 1.7, 2.6, 3.4):
                # off fine cells outside (> 0) or inside (< 0) the faces at +-4 coarse cells
                p = rng.uniform(-2.5, 2.5, 3) * dx0
                p[d] = side * (4 * dx0 + off * f)
                pts.append(p[None, :])
    pts = np.ascontiguousarray(np.concatenate(pts))
    fields = _device(comm, n0, dx0, boxes, seed=2)
    out = {}
    for order in (4, 2):
        want = _ref(name, _reference(n0, dx0, boxes, seed=2), pts, order)
        got = sample_points(fields, pts, order)
        _same(got, want, f"{name}, order {order}")
        out[order] = got
    return out[4]


@pytest.mark.gpu
def test_two_levels_against_the_restatement(comm):
    got = _two_levels(comm, "patch", PATCH)
    for lev in (0, 1):
        assert {1, 2, 4} <= set(np.unique(got.order[got.level == lev])), lev


@pytest.mark.gpu
def test_l_shaped_level_against_the_restatement(comm):
    got = _two_levels(comm, "lshape", LSHAPE)
    for lev in (0, 1):
        assert {1, 2, 4} <= set(np.unique(got.order[got.level == lev])), lev


def run_kernel_cases(comm):
    """What tests/sample_worker.py runs before it dumps the ledger: every
    instantiation of k_sample_points against the restatement."""
    for order in (1, 2, 4):
        _one_box(comm, order)
    _two_levels(comm, "patch", PATCH)


@pytest.mark.gpu
def test_three_box_layouts_agree(comm):
    from mg_ic_code_amd.sample import sample_points
    n0, dx0 = (16, 16, 16), 0.75
    pts = _points(n0, dx0)
    want = _ref("sixteen", _reference(n0, dx0, [[(0, 0, 0, 15, 15, 15)]], seed=4), pts, 4)
    for parts in ((1, 1, 1), (2, 2, 1), (2, 2, 2)):
        boxes = _split(n0, parts)
        fields = _device(comm, n0, dx0, [boxes], seed=4)
        assert fields[0].grid.num_local == len(boxes) == parts[0] * parts[1] * parts[2]
        _same(sample_points(fields, pts, 4), want, f"16^3 as {parts}")


@pytest.mark.gpu
def test_periodic_box_wraps(comm):
    from mg_ic_code_amd.sample import sample_points
    n0, dx0 = (12, 12, 12), 0.75
    boxes = [_split(n0, (2, 1, 1))]
    pts = _points(n0, dx0)
    h = _reference(n0, dx0, boxes, periodic=(1, 1, 1), seed=6)
    fields = _device(comm, n0, dx0, boxes, periodic=(1, 1, 1), seed=6)
    for order in (4, 2):
        want = _ref("periodic", h, pts, order)
        got = sample_points(fields, pts, order)
        _same(got, want, f"periodic 12^3, order {order}")
        finite = np.all(np.isfinite(pts), axis=1)
        # nothing degrades at the faces and the points outside are wrapped in
        assert np.all(got.order[finite] == order) and np.all(got.level[finite] == 0)
        assert np.all(got.level[~finite] == -1) and (~finite).sum() == 3
    # a point and its images one and three periods away: the same cell, and a
    # value equal up to the rounding of the wrap
    p = np.array([[0.3, -1.1, 2.2]])
    L = 12 * dx0
    a = sample_points(fields, p, 4).values
    for shift in ((L, 0, 0), (0, -L, 0), (3 * L, -2 * L, L)):
        b = sample_points(fields, p + np.array(shift), 4).values
        assert abs(b[0] - a[0]) <= 1e-12, (shift, a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("periodic", [(0, 0, 0), (1, 1, 1)])
def test_point_just_inside_the_high_face_on_the_device(comm, periodic):
    from mg_ic_code_amd.sample import sample_points
    n0 = (EDGE_N,) * 3
    boxes = [[(0, 0, 0) + (EDGE_N - 1,) * 3]]
    pts = np.array([[EDGE_X, -0.4, 0.2], [0.3, EDGE_X, 0.2], [0.3, -0.4, EDGE_X], [EDGE_X] * 3])
    h = _reference(n0, EDGE_DX, boxes, periodic=periodic, seed=12)
    got = sample_points(_device(comm, n0, EDGE_DX, boxes, periodic=periodic, seed=12), pts, 4)
    _same(got, R.sample(h, pts, 4), f"the rounding edge, periodic {periodic}")
    assert np.all(got.level == 0) and np.all(got.order == (4 if periodic[0] else 1))


@pytest.mark.gpu
def test_three_levels_check_the_prefix_tables(comm):
    from mg_ic_code_amd.sample import sample_points
    n0, dx0 = (16, 16, 16), 0.625
    boxes = [_split(n0, (2, 1, 1)),
             [(8, 8, 8, 23, 15, 23), (8, 16, 8, 23, 23, 23)],   # coarse cells 4..11, two boxes
             [(24, 24, 24, 39, 39, 31), (24, 24, 32, 39, 39, 39)]]  # level-1 cells 12..19
    rng = np.random.default_rng(23)
    pts = np.concatenate([_points(n0, dx0, nrand=200, seed=8), rng.uniform(-4.5, 4.5, (150, 3)) * dx0,
                          rng.uniform(-2.3, 2.3, (150, 3)) * dx0])
    h = _reference(n0, dx0, boxes, seed=9)
    fields = _device(comm, n0, dx0, boxes, seed=9)
    for order in (4, 1):
        got = sample_points(fields, pts, order)
        _same(got, _ref("three", h, pts, order), f"three levels, order {order}")
    assert set(np.unique(got.level)) == {-1, 0, 1, 2}
    # one level fewer: level 1 is then the finest and nothing of it is covered
    got = sample_points(fields[:2], pts, 4)
    _same(got, R.sample(_reference(n0, dx0, boxes[:2], seed=9), pts[:], 4), "the first two levels")


@pytest.mark.gpu
@pytest.mark.parametrize("npts", [1, 257, 70000])
def test_point_counts(comm, npts):
    from mg_ic_code_amd.sample import sample_points
    boxes = [[(0, 0, 0, 11, 7, 15)]]
    fields = _device(comm, ONE["n0"], ONE["dx0"], boxes)
    base = _points(ONE["n0"], ONE["dx0"])
    want = _ref("one", _reference(ONE["n0"], ONE["dx0"], boxes), base, 4)
    # point p of the call is base point (7 p + 11) mod len(base): every thread
    # is independent, so the expected answer is the restatement's, re-indexed
    idx = (7 * np.arange(npts) + 11) % len(base)
    got = sample_points(fields, base[idx], 4)
    _same(got, tuple(w[idx] for w in want), f"npts = {npts}")


@pytest.mark.gpu
def test_unit_psi_gives_the_algebraic_masses(comm):
    import mg_ic_code_amd as mg
    from mg_ic_code_amd.sample import puncture_masses
    dom = (0, 0, 0, 15, 15, 15)
    psi = mg.LevelData(mg.Grid(comm, dom, [dom], 100.0 / 16))
    psi.set_val_all(1.0)
    table = [(0.5, 10.0, 0.0, 0.0, 0, 0.05, 0, 0, 0, 0.1), (0.35, -10.0, 3.0, 0.0, 0, 0, 0, 0, 0, 0),
             (0.2, 1.0, -7.0, 22.0, 0, 0, 0, 0, 0, 0)]
    rep = puncture_masses(psi, _deck(), punctures=table)
    assert len(rep.punctures) == 3
    for i, p in enumerate(rep.punctures):
        others = sum(table[j][0] / math.dist(table[i][1:4], table[j][1:4])
                     for j in range(3) if j != i)
        want = 2.0 * table[i][0] * (1.0 + others)
        assert (p.level, p.order) == (0, 4)
        # the weights sum to 1 within 4 ulp (test_cubic_weights_sum_to_one), three times over
        assert abs(p.u - 1.0) <= 12 * 2.0 ** -52, p.u
        print(f"puncture {i + 1}: u - 1 = {p.u - 1.0:.3e}, M - want = "
              f"{(p.adm_mass - want) / math.ulp(want):.2f} ulp")
        assert abs(p.adm_mass - want) <= 4 * math.ulp(want), (i, p.adm_mass, want)
    # with u = 1 exactly the formula itself is within 4 ulp
    from mg_ic_code_amd.sample import adm_masses
    from mg_ic_code_amd.punctures import PunctureSet
    for i, m in enumerate(adm_masses(PunctureSet(table), [1.0] * 3)):
        others = sum(table[j][0] / math.dist(table[i][1:4], table[j][1:4])
                     for j in range(3) if j != i)
        assert abs(m - 2.0 * table[i][0] * (1.0 + others)) <= 4 * math.ulp(m)


def _raw(comm, fields, pts, order, npts=None, nlev=None):
    """The arguments of mgic_sample_points and the three output arrays."""
    xyz = np.ascontiguousarray(pts, dtype=np.float64)
    n = len(xyz) if npts is None else npts
    out = (np.zeros(max(len(xyz), 1)), np.zeros(max(len(xyz), 1), np.int32),
           np.zeros(max(len(xyz), 1), np.int32))
    PD, PI = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    handles = (ctypes.c_void_p * max(len(fields), 1))(
        *[f.handle.value if f is not None else None for f in fields])
    return [comm.handle, len(fields) if nlev is None else nlev, handles, n, xyz.ctypes.data_as(PD),
            order, out[0].ctypes.data_as(PD), out[1].ctypes.data_as(PI), out[2].ctypes.data_as(PI)], out


@pytest.mark.gpu
def test_refusals_leave_the_ledger_untouched(comm, tmp_path):
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import _lib
    from mg_ic_code_amd.core import read_launch_ledger
    from mg_ic_code_amd.sample import lineout, sample_points

    def ledger():
        p = tmp_path / "sample.ledger"
        _lib.sample_call("mgic_sample_launch_ledger_dump", str(p).encode())
        return read_launch_ledger(p)

    dom = (0, 0, 0, 15, 15, 15)
    base = mg.LevelData(mg.Grid(comm, dom, [dom], 1.0))
    base.set_val_all(1.0)
    fine = mg.LevelData(mg.Grid(comm, (0, 0, 0, 31, 31, 31), PATCH, 0.5, patches=True))
    fine.set_val_all(1.0)
    pts = np.array([[0.1, 0.2, 0.3], [1.0, 2.0, 3.0]])
    args, out = _raw(comm, [base, fine], pts, 4)
    _lib.sample_call("mgic_sample_points", *args)   # the accepted call the refusals are held against
    assert np.all(out[1] == 1) and np.all(out[2] == 4)
    before = ledger()
    assert sum(before.values()) > 0
    shifted = mg.LevelData(mg.Grid(comm, (1, 0, 0, 16, 15, 15), [(1, 0, 0, 16, 15, 15)], 1.0))
    periodic_fine = mg.LevelData(mg.Grid(comm, (0, 0, 0, 31, 31, 31), PATCH, 0.5,
                                         periodic=(1, 1, 1), patches=True))
    same_size = mg.LevelData(mg.Grid(comm, dom, [(4, 4, 4, 11, 11, 11)], 0.5, patches=True))
    by_four = mg.LevelData(mg.Grid(comm, (0, 0, 0, 63, 63, 63), [(16, 16, 16, 47, 47, 47)], 0.25,
                                   patches=True))
    cases = {
        "nlev 0": _raw(comm, [base], pts, 4, nlev=0)[0],
        "nlev 9": _raw(comm, [base] * 9, pts, 4)[0],
        "npts 0": _raw(comm, [base], pts, 4, npts=0)[0],
        "npts 2^20 + 1": _raw(comm, [base], pts, 4, npts=(1 << 20) + 1)[0],
        "order 0": _raw(comm, [base], pts, 0)[0],
        "order 3": _raw(comm, [base], pts, 3)[0],
        "order 8": _raw(comm, [base], pts, 8)[0],
        "low corner not 0": _raw(comm, [shifted], pts, 4)[0],
        "level 1 not refined": _raw(comm, [base, same_size], pts, 4)[0],
        "level 1 refined by 4": _raw(comm, [base, by_four], pts, 4)[0],
        "level 1 of another periodicity": _raw(comm, [base, periodic_fine], pts, 4)[0],
        "levels in the wrong order": _raw(comm, [fine, base], pts, 4)[0],
        "a null field": _raw(comm, [base, None], pts, 4)[0],
    }
    for name, at in (("comm", 0), ("fields", 2), ("xyz", 4), ("values", 6), ("level_used", 7),
                     ("order_used", 8)):
        a = _raw(comm, [base, fine], pts, 4)[0]
        a[at] = None
        cases["null " + name] = a
    for name, a in cases.items():
        with pytest.raises(mg.MgicError) as e:
            _lib.sample_call("mgic_sample_points", *a)
        assert e.value.code == -1, (name, str(e.value))
    # the same through the package: a ValueError
    for fields, p, order in (([base, same_size], pts, 4), ([shifted], pts, 4), ([base], pts, 3),
                             ([base] * 9, pts, 4), ([fine, base], pts, 2),
                             ([base], np.zeros(((1 << 20) + 1, 3)), 4)):
        with pytest.raises(ValueError):
            sample_points(fields, p, order)
    with pytest.raises(ValueError):
        lineout([base, by_four], (0, 0, 0), (1, 1, 1), 5)
    assert ledger() == before
    # and a line-out that is accepted
    line = lineout([base, fine], (-7.5, 0.1, 0.2), (7.5, 0.1, 0.2), 16)
    np.testing.assert_allclose(line.s, np.arange(16.0), rtol=1e-15)
    assert np.all(np.abs(line.values - 1.0) < 1e-14)
    assert list(line.level) == [0] * 4 + [1] * 8 + [0] * 4
    assert len(line.lines()) == 16 and line.lines()[0].startswith("lineout 0.0000000000000000e+00 ")


def _worker(*args):
    env = dict(os.environ)
    env.pop("MGIC_LAUNCH_LEDGER", None)
    r = subprocess.run([sys.executable, WORKER] + [str(a) for a in args], capture_output=True,
                       text=True, env=env, timeout=WORKER_TIMEOUT)
    assert r.returncode == 0, f"{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return r.stdout


@pytest.mark.gpu
def test_every_kernel_of_the_sample_library_is_launched_against_its_reference(tmp_path):
    from mg_ic_code_amd.core import read_launch_ledger
    out = tmp_path / "sample.ledger"
    _worker("kernel", out)
    ledger = read_launch_ledger(out)
    assert sorted(ledger) == ["k_sample_points<1>", "k_sample_points<2>", "k_sample_points<4>"], ledger
    missing = sorted(n for n, c in ledger.items() if c == 0)
    assert not missing, f"{len(missing)} of {len(ledger)} kernels never launched:\n" + "\n".join(missing)


@pytest.mark.gpu
def test_a_box_that_is_not_local_is_refused(tmp_path):
    # two ranks on the one device (tests/sample_worker.py nonlocal, the peer-mapped
    # transport as tests/test_multiprocess.py runs it): each holds one box of the
    # level and not the other
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
        assert sorted(out["ledger"]) == ["k_sample_points<1>", "k_sample_points<2>",
                                         "k_sample_points<4>"]
        assert not any(out["ledger"].values()), out["ledger"]


def _check_solve(out, level):
    assert out["loaded_after_plain_solve"] is False and out["loaded_after_flag_solve"] is True
    assert out["same_solve"] and out["same_report"] and out["deck_key_same"]
    assert out["levels"] == [level, level] and out["orders"] == [4, 4]
    print("u at the punctures:", out["u"], "oracle:", out["u_oracle"], "M:", out["masses"])
    print("psi GPU vs oracle, rel-L2 per level:", out["psi_rel_l2"])
    # the bar at which the suite compares the two psi (tests/test_gpu_parity.py,
    # tests/test_amr.py: 1e-10 of the norm), here of each sampled value
    for u, w in zip(out["u"], out["u_oracle"]):
        assert abs(u - w) <= 1e-10 * abs(w), (u, w)
    assert all(e <= 1e-10 for e in out["psi_rel_l2"])


@pytest.mark.gpu
def test_solve_with_the_flag_is_the_same_solve_and_off_loads_nothing():
    # a fresh process (tests/sample_worker.py solve): without the flag
    # libmgic_sample.so stays unloaded; with it (the keyword, and the deck's key)
    # psi, the norms, the iteration counts and libmgic's ledger are the plain
    # solve's, NLResult.puncture_masses is puncture_masses(res.psi, ...) bit for
    # bit, and psi at the punctures is the oracle's
    _check_solve(json.loads(_worker("solve").strip().splitlines()[-1]), 0)


@pytest.mark.gpu
def test_solve_on_two_levels_reports_the_level():
    # the same on the two-level hierarchy of tests/test_adm.py: both punctures
    # lie in the patch and are sampled on level 1
    _check_solve(json.loads(_worker("solve2").strip().splitlines()[-1]), 1)


@pytest.mark.gpu
def test_solve_for_masses_converges_to_the_oracle_fixed_point(comm):
    import mg_ic_code_amd as mg
    from mg_ic_code_amd.sample import solve_for_masses
    prm = _deck(16, bh1_bare_mass=START[0], bh2_bare_mass=START[1])
    dom = (0, 0, 0, 15, 15, 15)
    grid = mg.Grid(comm, dom, [dom], prm.domainLength[0] / 16)
    r = solve_for_masses(grid, prm, TARGETS, max_depth=2)
    errs = [h.error for h in r.history]
    print("max|M - T| per solve:", errs, "bare masses:", [p.mass for p in r.punctures])
    assert r.converged and len(r.history) <= 6
    assert r.history[0].bare_masses == list(START)
    for a, b in zip(errs, errs[1:]):
        if a > 1e-10:
            assert b <= 0.1 * a, errs
    assert errs[-1] <= 1e-8 * max(TARGETS)
    assert r.result.puncture_masses.adm_masses == r.history[-1].adm_masses
    assert [p.mass for p in r.punctures] == r.history[-1].bare_masses
    want = oracle_fixed_point()[len(r.history) - 1][0]
    np.testing.assert_allclose([p.mass for p in r.punctures], want, rtol=0, atol=1e-8)
    # max_solves runs out: not converged, nothing raised
    short = solve_for_masses(grid, prm, TARGETS, max_solves=2, max_depth=2)
    assert not short.converged and len(short.history) == 2
    assert [h.error for h in short.history] == errs[:2]


@pytest.mark.gpu
def test_run_poisson_cli_lines(comm, tmp_path):
    import mg_ic_code_amd as mg
    from mg_ic_code_amd.nl import poisson_solve
    from mg_ic_code_amd.params import read_params_file
    from mg_ic_code_amd.sample import lineout
    deck = tmp_path / "deck.txt"
    deck.write_text(_deck_text().replace("max_NL_iterations = 6", "max_NL_iterations = 2"))
    tool = os.path.join(ROOT, "tools", "run_poisson.py")
    r = subprocess.run([sys.executable, tool, str(deck), "--size", "16", "--max-depth", "2",
                        "--puncture-masses", "--lineout=-20 0.5 0.5 20 0.5 0.5 9"],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    prm = read_params_file(str(deck))
    dom = (0, 0, 0, 15, 15, 15)
    res = poisson_solve(mg.Grid(comm, dom, [dom], prm.domainLength[0] / 16), prm, max_depth=2,
                        puncture_masses=True)
    got = [ln for ln in r.stdout.splitlines() if ln.startswith("puncture mass ")]
    assert got == res.puncture_masses.lines() and len(got) == 2
    got = [ln for ln in r.stdout.splitlines() if ln.startswith("lineout ")]
    assert got == lineout(res.psi, (-20, 0.5, 0.5), (20, 0.5, 0.5), 9).lines() and len(got) == 9
    assert json.loads(r.stdout.strip().splitlines()[-1])["puncture_masses"] == \
        res.puncture_masses.adm_masses


@pytest.mark.gpu
def test_run_poisson_cli_target_masses(comm, tmp_path):
    import mg_ic_code_amd as mg
    from mg_ic_code_amd.params import read_params_file
    from mg_ic_code_amd.sample import solve_for_masses
    deck = tmp_path / "deck.txt"
    deck.write_text(_deck_text().replace("max_NL_iterations = 6", "max_NL_iterations = 3")
                    .replace("bh2_bare_mass = 0.5", "bh2_bare_mass = 0.35"))
    tool = os.path.join(ROOT, "tools", "run_poisson.py")
    r = subprocess.run([sys.executable, tool, str(deck), "--size", "16", "--max-depth", "2",
                        "--target-masses", "1.0 0.7"],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    prm = read_params_file(str(deck))
    assert (prm.bh1_bare_mass, prm.bh2_bare_mass) == START
    dom = (0, 0, 0, 15, 15, 15)
    want = solve_for_masses(mg.Grid(comm, dom, [dom], prm.domainLength[0] / 16), prm, "1.0 0.7",
                            max_depth=2)
    got = [ln for ln in r.stdout.splitlines() if ln.startswith("mass solve")]
    assert got == want.lines() and len(got) == len(want.history) + 1 and want.converged
    got = [ln for ln in r.stdout.splitlines() if ln.startswith("puncture mass ")]
    assert got == want.result.puncture_masses.lines()
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert summary["mass_solves"] == len(want.history) and summary["mass_solve_converged"] is True
    assert summary["puncture_masses"] == want.result.puncture_masses.adm_masses
    assert [row[0] for row in summary["punctures"]] == [p.mass for p in want.punctures]
    # the deck's key asks for the same
    deck.write_text(deck.read_text() + "\ntarget_masses = 1.0 0.7\n")
    r2 = subprocess.run([sys.executable, tool, str(deck), "--size", "16", "--max-depth", "2"],
                        capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-2000:]
    assert [ln for ln in r2.stdout.splitlines() if ln.startswith("mass solve")] == want.lines()
