"""The level's LinearOp vector interface (csrc/kernels.hip: k_reduce_partial,
k_reduce_final, k_reduce_final_wide, k_blas, k_axpy2_reduce, k_dot2,
k_bicg_p; op.cpp: reduce, finish_reduce, resetLambda) against plain
references.

The sums are held to tests/reduce_ref.py, a numpy restatement of the
reduction's order, bit for bit, and to the exact sum within the bound that
order's own addition tree gives (tests/test_reduce_ref.py shows on the CPU
that the shapes used here tell a dropped row tail or a dropped last row from
the right order).  The maxima are exact.  The BLAS-1 passes and the fused
BiCGStab updates are compared with the numpy expressions as 64-bit patterns,
ghost cells included.  The two detectors behind resetLambda (constant bCoef,
lambda range) are tried with one outlier at the places a reduction loses
first: a row's tail, the last row, the last box.
"""
import math

import numpy as np
import pytest

import oracle
from tests import reduce_ref as rr

pytestmark = pytest.mark.gpu

mg = pytest.importorskip("mg_ic_code_amd")

DX = 0.7
SENTINEL = 123.0


@pytest.fixture(scope="module")
def comm():
    return mg.Comm()


class Level:
    """One level of the shape table: grid, operator (aCoef random, bCoef 1),
    the local boxes' numpy shapes."""

    def __init__(self, comm, case):
        shape, lo, split = case
        self.dom = rr.domain_of(shape, lo)
        self.grid = mg.Grid(comm, self.dom, rr.split_boxes(shape, lo, split), DX)
        self.boxes = [self.grid.local_box(n) for n in range(self.grid.num_local)]
        assert len(self.boxes) == split[0] * split[1] * split[2]
        self.shapes = [(b[5] - b[2] + 1, b[4] - b[1] + 1, b[3] - b[0] + 1) for b in self.boxes]
        rng = np.random.default_rng(7)
        self.fa = self.field([rng.uniform(-2.0, -0.5, s) for s in self.shapes], 0.0)
        self.fb = self.field([np.ones(s) for s in self.shapes], 0.0)
        self.op = mg.defineOperatorFactory(
            self.grid, self.fa, self.fb, mg.OperatorParams(alpha=1.0, beta=-1.0)).AMRnewOp()

    def field(self, arrays=None, ghost=math.nan):
        """A field whose every cell, ghosts included, holds `ghost`, then the
        valid cells of each local box from `arrays`."""
        f = mg.LevelData(self.grid)
        f.set_val_all(ghost)
        if arrays is not None:
            for n, a in enumerate(arrays):
                f.upload(n, a)
        return f

    def random(self, rng, lo=-1.0, hi=1.0):
        return [rng.uniform(lo, hi, s) for s in self.shapes]

    def valid(self, f):
        return [f.download(n) for n in range(len(self.boxes))]

    def full(self, f):
        return [f.download(n, with_ghosts=True) for n in range(len(self.boxes))]

    def assemble(self, arrays):
        """The per-box arrays as one array over the domain."""
        d = self.dom
        out = np.zeros((d[5] - d[2] + 1, d[4] - d[1] + 1, d[3] - d[0] + 1))
        for b, a in zip(self.boxes, arrays):
            out[b[2] - d[2]:b[5] - d[2] + 1, b[1] - d[1]:b[4] - d[1] + 1,
                b[0] - d[0]:b[3] - d[0] + 1] = a
        return out


@pytest.fixture(scope="module")
def levels(comm):
    made = {}

    def get(case):
        if case not in made:
            made[case] = Level(comm, case)
        return made[case]

    return get


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same_bits(got, want):
    """Lists of arrays, equal as 64-bit patterns (-0.0 and subnormals count)."""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape
        assert np.array_equal(bits(g), bits(w))


def with_ghosts(valid, ghost):
    """What a field holds after `valid` went into an allocation full of `ghost`."""
    out = []
    for v in valid:
        a = np.full(tuple(n + 2 for n in v.shape), ghost)
        a[1:-1, 1:-1, 1:-1] = v
        out.append(a)
    return out


def assert_ghosts_nan(full):
    for a in full:
        inner = np.zeros(a.shape, dtype=bool)
        inner[1:-1, 1:-1, 1:-1] = True
        assert np.all(np.isnan(a[~inner]))


# ------------------------------------------------------------------ reductions
@pytest.mark.parametrize("case", rr.SHAPES, ids=rr.shape_id)
def test_reductions_equal_the_stated_order(levels, rng, case):
    # ghosts are NaN: one cell read outside the valid region turns every sum
    # into NaN and fails the bit comparison
    L = levels(case)
    xs, ys = L.random(rng), L.random(rng)
    fx, fy = L.field(xs), L.field(ys)
    ratios = rr.assert_level_reductions(L.op, fx, fy, xs, ys)
    print(rr.shape_id(case), {k: f"{v:.3g}" for k, v in ratios.items()})
    if len(L.boxes) > 1:
        # the oracle sums cell after cell (chains of n terms: worst case
        # n u = 3e-11 of sum |terms|, a random walk of roundings gives
        # ~sqrt(n) u = 6e-14); 1e-12 as test_operator_methods_bitwise has it
        o = oracle.OracleMG([L.dom], L.dom, DX, nlevels=1)
        o.set(0, oracle.PHI, 0, L.assemble(xs))
        o.set(0, oracle.RHS, 0, L.assemble(ys))
        d_o = o.dot(0, oracle.PHI, oracle.RHS)
        assert abs(L.op.dotProduct(fx, fy) - d_o) <= 1e-12 * abs(d_o)
        for ord in (1, 2):
            n_o = o.norm(0, oracle.PHI, ord)
            assert abs(L.op.norm(fx, ord) - n_o) <= 1e-12 * n_o
        assert L.op.norm(fx, 0) == o.norm(0, oracle.PHI, 0)


SIGN_CASES = [c for c in rr.SHAPES if c[0] in ((1, 1, 1), (257, 2, 3), (5, 96, 90), (130, 46, 44))]


@pytest.mark.parametrize("case", SIGN_CASES, ids=rr.shape_id)
def test_reductions_signs_and_magnitudes(levels, rng, case):
    L = levels(case)
    op = L.op
    ones = [np.ones(s) for s in L.shapes]
    f1 = L.field(ones)
    # all negative
    xs = L.random(rng, -1.0, -0.1)
    fx = L.field(xs)
    rr.assert_level_reductions(op, fx, f1, xs, ones)
    assert op.dotProduct(fx, f1) == -op.norm(fx, 1)  # the same terms, negated
    # -0.0: alone (every sum is +0.0: the accumulators start there), and mixed in
    zs = [np.full(s, -0.0) for s in L.shapes]
    fz = L.field(zs)
    for got in (op.dotProduct(fz, f1), op.norm(fz, 0), op.norm(fz, 1), op.norm(fz, 2)):
        assert rr.same_bits(got, 0.0)
    xs = L.random(rng)
    for x in xs:
        x.flat[::3] = -0.0
    rr.assert_level_reductions(op, L.field(xs), f1, xs, ones)
    # subnormals: their sums are exact, their squares underflow to 0
    xs = [rng.integers(1, 1000, s).astype(np.float64) * 5e-324 * rng.choice([-1.0, 1.0], s)
          for s in L.shapes]
    fx = L.field(xs)
    rr.assert_level_reductions(op, fx, f1, xs, ones, bounds=False)
    assert op.norm(fx, 1) == math.fsum(float(v) for x in xs for v in np.abs(x).flat) > 0.0
    assert op.dotProduct(fx, f1) == math.fsum(float(v) for x in xs for v in x.flat)
    assert op.norm(fx, 2) == 0.0
    # a sum that cancels: x, then -x mirrored, per box; a dropped cell leaves
    # its |x| ~ 0.5 against a bound of ~1e-13
    xs = L.random(rng)
    for x in xs:
        h = x.size // 2
        x.flat[x.size - h:] = -x.flat[:h][::-1]
        if x.size % 2:
            x.flat[h] = 0.0
    fx = L.field(xs)
    rr.assert_level_reductions(op, fx, f1, xs, ones)
    _, d = rr.reduce_model(0, xs, ones)
    assert abs(op.dotProduct(fx, f1)) <= rr.gamma(d) * sum(float(np.sum(np.abs(x))) for x in xs)
    # one huge cell, the last of the last box
    xs = L.random(rng)
    xs[-1].flat[-1] = -1.0e300
    assert op.norm(L.field(xs), 0) == 1.0e300


NAN_SHAPE = ((130, 3, 2), (0, 0, 0), (1, 1, 1))
NAN_AT = {"same_lane_later": (0, 0, 64), "lane_last_term": (0, 0, 129),
          "last_row_first": (1, 2, 0), "last_cell": (1, 2, 129)}


def test_max_norm_keeps_the_maximum_past_a_nan(levels, rng):
    # 5.0 at i = 0 of row 0, everything else at most 1, one NaN: the oracle's
    # max keeps its running value when the term is NaN (orc_mg_norm), so
    # norm(x, 0) is 5.0 wherever the NaN sits; the sums are NaN
    L = levels(NAN_SHAPE)
    base = L.random(rng)[0]
    base[0, 0, 0] = 5.0
    zero = L.field([np.zeros(L.shapes[0])])
    got = {}
    for name, at in NAN_AT.items():
        x = base.copy()
        x[at] = math.nan
        fx = L.field([x])
        o = oracle.OracleMG([L.dom], L.dom, DX, nlevels=1)
        o.set(0, oracle.PHI, 0, x)
        assert o.norm(0, oracle.PHI, 0) == 5.0
        got[name] = L.op.norm(fx, 0)
        # the fused norm shares the rule: s = x + 0 * 0 (e, pt untouched)
        fs = L.field()
        fused = L.op.axpy2Norm(fs, fx, zero, 0.0, L.field([x]), zero, 0.0, 0)
        assert rr.same_bits(fused, got[name])
        for v in (L.op.norm(fx, 1), L.op.norm(fx, 2), L.op.dotProduct(fx, fx)):
            assert math.isnan(v)
    assert got == {name: 5.0 for name in NAN_AT}


# ------------------------------------------- the detectors behind resetLambda
DETECTOR_CASES = [((257, 6, 5), (0, 0, 0), (1, 1, 1)), ((6, 288, 96), (0, 0, 0), (1, 3, 1))]
# (box, cell): the places a reduction loses first
PLACES = {"row0_tail": (0, lambda s: (0, 0, s[2] - 1)),
          "last_row_tail": (0, lambda s: (s[0] - 1, s[1] - 1, s[2] - 1)),
          "first_cell": (0, lambda s: (0, 0, 0)),
          "last_box_last_cell": (-1, lambda s: (s[0] - 1, s[1] - 1, s[2] - 1))}


def relax_pair(levels, case, place, *, a_out=None, b_out=None):
    """relax(fu, fr, 2) with fused_smoother = 2, alpha = 1, beta = -1 and the
    oracle's, with one outlier cell in aCoef or bCoef.  The constant-b flag
    selects the kernel body on every path (single sweep, pair, passes)."""
    L = levels(case)
    rng = np.random.default_rng(11)
    a, b = L.random(rng, -2.0, -0.5), [np.ones(s) for s in L.shapes]
    box, cell = PLACES[place]
    for arrs, v in ((a, a_out), (b, b_out)):
        if v is not None:
            arrs[box][cell(L.shapes[box])] = v
    rhs, u0 = L.random(rng), L.random(rng)
    fa, fb, fr, fu = (L.field(x, 0.0) for x in (a, b, rhs, u0))
    op = mg.defineOperatorFactory(L.grid, fa, fb, mg.OperatorParams(
        alpha=1.0, beta=-1.0, fused_smoother=2)).AMRnewOp()
    op.relax(fu, fr, 2)
    o = oracle.OracleMG([L.dom], L.dom, DX, alpha=1.0, beta=-1.0, nlevels=1)
    for f, x in ((oracle.ACOEF, a), (oracle.BCOEF, b), (oracle.RHS, rhs), (oracle.PHI, u0)):
        o.set(0, f, 0, L.assemble(x))
    o.setup()
    o.relax(0, oracle.PHI, oracle.RHS, 2)
    return L.assemble(L.valid(fu)), o.get(0, oracle.PHI, 0)


# The lambda-range flag (rcp_fast) is read in one place, the two-sweep launch
# (smoother_tb.hip: launch_tb2), which relax() takes only on a level of boxes
# with domain faces alone and every extent >= 8 (gsrb_sweep_tb2_applies).
# Neither detector layout gets there (ny = 6, nz = 5; nx = 6 and three boxes):
# on them these cases hold the single-sweep kernel, which reads the stored
# lambda, to the oracle at extreme coefficients, and nothing more.  257 x 9 x 8
# in one box takes the pair launch and still has a row tail and a last row.
GUARD_CASES = DETECTOR_CASES + [((257, 9, 8), (0, 0, 0), (1, 1, 1))]


@pytest.mark.parametrize("place", list(PLACES))
@pytest.mark.parametrize("case", GUARD_CASES, ids=rr.shape_id)
def test_bcoef_detector_sees_one_outlier(levels, case, place):
    # bCoef 1.0 but for one cell at 1.5: a missed outlier sends the level to
    # the constant-b kernel, and the result differs at that cell and around it
    got, want = relax_pair(levels, case, place, b_out=1.5)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("place", list(PLACES))
@pytest.mark.parametrize("case", GUARD_CASES, ids=rr.shape_id)
def test_lambda_range_guard_sees_one_outlier(levels, case, place):
    # one aCoef cell at -1e308: lambda is subnormal there, outside the range
    # the host admits for the short reciprocal (rcp_div1).  That the code
    # differs there cannot be read from it, and on an MI355X it does not:
    # rcp_div1 returns the division's bits at +-1e308
    # (tools/rcp_div1_probe.hip, profiles/r07_rcp_div1_probe.txt).  So this
    # case holds the result to the oracle but could not show a missed
    # outlier at any placement; the zero denominator below can.
    got, want = relax_pair(levels, case, place, a_out=-1.0e308)
    assert np.array_equal(got, want, equal_nan=True)


# alpha a + 6 beta / dx^2 == 0 exactly at alpha = 1, beta = -1 (coefs(): lamshift)
ZERO_DENOMINATOR = -(2.0 * 3 * -1.0 / (DX * DX))


@pytest.mark.parametrize("place", list(PLACES))
@pytest.mark.parametrize("case", GUARD_CASES, ids=rr.shape_id)
def test_lambda_range_guard_sees_a_zero_denominator(levels, case, place):
    # lambda = 1 / 0 = inf at one cell: not finite, so the guard must turn the
    # short reciprocal off.  rcp_div1(0) is NaN where the division gives inf
    # (same probe), and every inf of the oracle's result descends from that
    # lambda.  On 257 x 9 x 8 a guard that misses the cell, at any of the four
    # placements, therefore leaves NaN where the oracle has inf; the other two
    # layouts never reach the two-sweep kernel (above).
    got, want = relax_pair(levels, case, place, a_out=ZERO_DENOMINATOR)
    assert np.isinf(want).any()
    assert np.array_equal(got, want, equal_nan=True)


@pytest.mark.parametrize("place", ["first_cell", "last_box_last_cell"])
@pytest.mark.parametrize("case", GUARD_CASES, ids=rr.shape_id)
def test_nan_in_bcoef_never_selects_the_constant_b_kernel(levels, case, place):
    got, want = relax_pair(levels, case, place, b_out=math.nan)
    assert np.array_equal(got, want, equal_nan=True)
    assert np.isnan(want).any()  # the oracle shows the NaN; so must the level


# ---------------------------------------------------------------------- BLAS-1
SPECIAL = [math.inf, -math.inf, -0.0, 5e-324, -2.2e-308, 1.0e308, -1.0e308, 0.0]


def blas_operands(L, rng):
    """x, y, z: random, with +-inf, -0.0, subnormals and +-1e308 (doubled: an
    overflow) in each, at cells where the other two operands are ordinary, so
    that no inf - inf or 0 * inf arises: the comparison is of bit patterns,
    without equal_nan."""
    x, y, z = L.random(rng), L.random(rng), L.random(rng)
    if x[0].size >= 3 * len(SPECIAL):
        for n in range(len(x)):
            at = rng.choice(x[n].size, 3 * len(SPECIAL), replace=False).reshape(3, -1)
            for a, cells in zip((x[n], y[n], z[n]), at):
                a.flat[cells] = SPECIAL
    else:  # a single cell: one special operand
        y[0].flat[0] = -0.0
    return x, y, z


@pytest.mark.parametrize("case", rr.SHAPES, ids=rr.shape_id)
def test_blas1_matches_numpy_and_keeps_ghosts(levels, rng, case):
    L = levels(case)
    op = L.op
    x, y, z = blas_operands(L, rng)
    s, t = 2.0, -0.75
    fy, fz = L.field(y, SENTINEL), L.field(z, SENTINEL)

    def check(f, want):
        assert_same_bits(L.full(f), with_ghosts(want, SENTINEL))

    with np.errstate(over="ignore"):
        fx = L.field(x, SENTINEL)
        op.incr(fx, fy, s)  # x + s * y
        check(fx, [a + s * b for a, b in zip(x, y)])
        fx = L.field(x, SENTINEL)
        op.scale(fx, s)  # x * s
        check(fx, [a * s for a in x])
        fx = L.field(x, SENTINEL)
        op.axby(fx, fy, fz, s, t)  # s * y + t * z, two roundings and a third
        check(fx, [s * b + t * c for b, c in zip(y, z)])
        fx = L.field(x, SENTINEL)
        op.assignLocal(fx, fy)
        check(fx, y)
        check(fy, y)  # the sources are read only
        check(fz, z)
        # aliased arguments, as Krylov callers may pass them
        fx = L.field(x, SENTINEL)
        op.incr(fx, fx, s)
        check(fx, [a + s * a for a in x])
        fx = L.field(x, SENTINEL)
        op.axby(fx, fx, fy, s, t)
        check(fx, [s * a + t * b for a, b in zip(x, y)])
        fx = L.field(x, SENTINEL)
        op.axby(fx, fy, fx, s, t)
        check(fx, [s * b + t * a for a, b in zip(x, y)])
    # s = 2 makes s * y exact, so a contracted x + s * y (one rounding) has the
    # bits of the separate product and sum; 1/3 and -0.7 on ordinary operands
    # tell them apart
    s, t = 1.0 / 3.0, -0.7
    x, y, z = L.random(rng), L.random(rng), L.random(rng)
    fy, fz = L.field(y, SENTINEL), L.field(z, SENTINEL)
    fx = L.field(x, SENTINEL)
    op.incr(fx, fy, s)
    check(fx, [a + s * b for a, b in zip(x, y)])
    fx = L.field(x, SENTINEL)
    op.scale(fx, s)
    check(fx, [a * s for a in x])
    fx = L.field(x, SENTINEL)
    op.axby(fx, fy, fz, s, t)
    check(fx, [s * b + t * c for b, c in zip(y, z)])
    fx = L.field(x, SENTINEL)
    op.axby(fx, fx, fy, s, t)
    check(fx, [s * a + t * b for a, b in zip(x, y)])
    # setToZero clears the whole allocation (set_zero_all), ghosts included
    fx = L.field(x, SENTINEL)
    op.setToZero(fx)
    assert_same_bits(L.full(fx), [np.zeros(tuple(n + 2 for n in a.shape)) for a in x])


def test_blas1_nan_operands(levels, rng):
    # NaN put in on purpose: inf - inf, 0 * inf and a NaN operand stay NaN at
    # their cell and touch no other
    L = levels(((65, 3, 2), (0, 0, 0), (1, 1, 1)))
    x, y = L.random(rng), L.random(rng)
    x[0].flat[:3] = [math.inf, 0.0, math.nan]
    y[0].flat[:3] = [-math.inf, math.inf, 1.0]
    fx, fy = L.field(x, SENTINEL), L.field(y, SENTINEL)
    L.op.incr(fx, fy, 1.0)
    got = L.full(fx)[0]
    with np.errstate(invalid="ignore"):
        want = with_ghosts([x[0] + 1.0 * y[0]], SENTINEL)[0]
    assert np.isnan(want[1, 1, 1:4]).tolist() == [True, False, True]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    keep = ~np.isnan(want)
    assert np.array_equal(bits(got)[keep], bits(want)[keep])
    fx = L.field(x, SENTINEL)
    L.op.axby(fx, fx, fy, 0.0, 0.0)  # 0 * inf at cells 0 and 1, 0 * nan at 2
    got = L.full(fx)[0]
    assert np.isnan(got[1, 1, 1:4]).all() and np.isnan(got).sum() == 3


# ------------------------------------------------------- fused BiCGStab updates
@pytest.mark.parametrize("case", rr.SHAPES, ids=rr.shape_id)
def test_fused_bicgstab_updates(levels, rng, case):
    L = levels(case)
    op = L.op
    r, v, e, pt = (L.random(rng) for _ in range(4))
    fr, fv, fe, fpt = (L.field(a) for a in (r, v, e, pt))
    ca, cb = -0.8125 + 2.0 ** -30, 0.3
    s = [a + ca * b for a, b in zip(r, v)]
    for ord in (0, 1, 2):
        fs = L.field()  # NaN everywhere: every valid cell must be written
        got = op.axpy2Norm(fs, fr, fv, ca, fe, fpt, cb, ord)
        e = [a + cb * b for a, b in zip(e, pt)]  # E += cb PT, once per call
        assert_same_bits(L.valid(fs), s)
        assert_same_bits(L.valid(fe), e)
        assert_ghosts_nan(L.full(fs) + L.full(fe))
        assert rr.same_bits(got, op.norm(fs, ord))  # the separate pass
        want = max(float(np.max(np.abs(a))) for a in s) if ord == 0 else rr.norm_model(s, ord)[0]
        assert rr.same_bits(got, want)
    assert_same_bits(L.valid(fr) + L.valid(fv) + L.valid(fpt), r + v + pt)
    # dot2(t, s) = (dot(t, s), dot(t, t))
    t = L.random(rng)
    ft = L.field(t)
    ts, tt = op.dot2(ft, fs)
    assert rr.same_bits(ts, op.dotProduct(ft, fs)) and rr.same_bits(tt, op.dotProduct(ft, ft))
    assert rr.same_bits(ts, rr.reduce_model(0, t, s)[0])
    assert rr.same_bits(tt, rr.reduce_model(0, t, t)[0])
    # bicgP: p = ((p * beta) + c * v) + 1.0 * r
    p = L.random(rng)
    fp = L.field(p)
    beta, c = 1.0 / 3.0, -0.7
    op.bicgP(fp, fv, fr, beta, c)
    assert_same_bits(L.valid(fp), [((a * beta) + c * b) + 1.0 * d for a, b, d in zip(p, v, r)])
    assert_ghosts_nan(L.full(fp))
