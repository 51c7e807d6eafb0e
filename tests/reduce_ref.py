"""The order of the level reductions (csrc/kernels.hip), restated in numpy.

Test infrastructure only.  `reduce(kind, x, y)` of the operator sums its
terms in a fully defined order, so the sums can be held to the bit:

  * per box, `reduce_blocks` blocks of 256 threads (4 waves): one block per
    4 rows, at most 2048 (kMaxPartsPerBox);
  * rows r = k * ny + j dealt round-robin to the 4 * blocks waves of the box;
  * per lane, four accumulators a0..a3 fed at i, i + 64, i + 128, i + 192
    while i + 192 < nx (i += 256), then a0 alone in steps of 64;
  * (a0 + a1) + (a2 + a3), then the 256-entry LDS tree (w = 128 .. 1:
    sm[t] += sm[t + w] for t < w);
  * the boxes' partials concatenated in local box order;
  * k_reduce_final: thread t sums partials t, t + 256, ... in order, then
    the same tree.

k_axpy2_reduce and k_dot2 use the same deal and accumulators, so the model
serves the fused kernels too.  Kinds: 0 dot(x, y), 1 sum |x|, 2 sum x^2.
The max kinds need no model: any order gives the same maximum.

Besides the value the model returns D, the longest chain of additions any
term passes through (additions to an accumulator that has met no term yet
are exact and are not counted), so that
    |model - exact| <= gamma_D * sum |terms|,  gamma_D = D u / (1 - D u),
u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, 4.2: any
summation order, with D the depth of the addition tree).
"""
import math

import numpy as np

RB = 256           # threads per reduction block
WAVES = RB // 64   # rows a block takes per round
MAX_BLOCKS = 2048  # kern::kMaxPartsPerBox
U = 2.0 ** -53

# the shapes of the level-algebra tests: (nx, ny, nz), lo corner, split.
# Each is the smallest that reaches its branch.
SHAPES = [
    ((1, 1, 1), (0, 0, 0), (1, 1, 1)),       # one cell, 255 idle threads at the identity
    ((63, 3, 2), (0, 0, 0), (1, 1, 1)),      # rows shorter than a wave; a second block
    ((64, 1, 5), (0, 0, 0), (1, 1, 1)),      # five rows: a second block with one live wave
    ((65, 3, 2), (0, 0, 0), (1, 1, 1)),      # first lane wrap
    ((193, 2, 3), (0, 0, 0), (1, 1, 1)),     # only lane 0 enters the four-accumulator round
    ((256, 2, 3), (0, 0, 0), (1, 1, 1)),     # every lane, no tail
    ((257, 2, 3), (0, 0, 0), (1, 1, 1)),     # tail after a full round
    ((520, 3, 3), (0, 0, 0), (1, 1, 1)),     # two rounds plus tail
    ((5, 96, 90), (0, 0, 0), (1, 1, 1)),     # 8640 rows > 4 * 2048: the cap, 1 and 2 rows a wave
    ((130, 47, 45), (-64, 1, 1), (1, 1, 1)),  # ragged everything, odd offset
    ((6, 288, 96), (0, 0, 0), (1, 3, 1)),    # 6144 partials: the finals' loops wrap
    ((130, 46, 44), (3, -5, 7), (2, 2, 2)),  # multi-box, boxes of 65 and 23
]


def shape_id(case):
    shape, _, split = case
    return "x".join(map(str, shape)) + ("" if split == (1, 1, 1) else "-" + "".join(map(str, split)))


def domain_of(shape, lo):
    return tuple(lo) + tuple(lo[d] + shape[d] - 1 for d in range(3))


def gamma(d):
    return d * U / (1.0 - d * U)


def reduce_blocks(ny, nz):
    return min((ny * nz + WAVES - 1) // WAVES, MAX_BLOCKS)


def _add(a, da, b, db):
    """a + b with the chain lengths: -1 marks an operand that has met no term
    (it holds +0.0, and adding it is exact)."""
    s = a + b
    d = np.where(da < 0, db, np.where(db < 0, da, np.maximum(da, db) + 1))
    return s, d


def _tree(sm, dm):
    """The LDS tree over the last axis (length RB); returns entry 0."""
    w = RB // 2
    while w > 0:
        s, d = _add(sm[..., :w], dm[..., :w], sm[..., w:2 * w], dm[..., w:2 * w])
        sm = np.concatenate([s, sm[..., w:]], axis=-1)
        dm = np.concatenate([d, dm[..., w:]], axis=-1)
        w >>= 1
    return sm[..., 0], dm[..., 0]


def box_partials(t, *, drop_tail=False, skip_last_row=False):
    """k_reduce_partial's partials of one box; t: the terms, shape (nz, ny, nx).
    drop_tail / skip_last_row: deliberately wrong variants (the a0 tail loop
    left out; the last row of the box never visited) for the tests that show
    the shapes can tell."""
    nz, ny, nx = t.shape
    nrows = ny * nz
    nb = reduce_blocks(ny, nz)
    nwaves = nb * WAVES
    rows = t.reshape(nrows, nx)
    if skip_last_row:
        nrows -= 1
    lane = np.arange(64)
    # rounds of four a lane makes: the t with lane + 256 t + 192 < nx
    full = np.maximum(0, -(-(nx - 192 - lane) // 256))
    acc = np.zeros((4, nwaves, 64))
    dep = np.full((4, nwaves, 64), -1, dtype=np.int64)
    nchunk = (nx + 63) // 64
    for first in range(0, nrows, nwaves):
        blk = rows[first:min(first + nwaves, nrows)]
        c = blk.shape[0]  # waves 0 .. c-1 have a row in this round
        for q in range(nchunk):
            col = q * 64 + lane
            live = col < nx
            in_round = (q // 4) < full
            for a in range(4):
                m = live & (in_round if a == q % 4 else False)
                if a == 0:
                    m = m | (live & ~in_round & (not drop_tail))
                if not np.any(m):
                    continue
                ls = lane[m]
                av, dv = acc[a], dep[a]  # views, (nwaves, 64)
                av[:c, ls] = av[:c, ls] + blk[:, col[m]]
                d = dv[:c, ls]
                dv[:c, ls] = np.where(d < 0, 0, d + 1)
    s01, d01 = _add(acc[0], dep[0], acc[1], dep[1])
    s23, d23 = _add(acc[2], dep[2], acc[3], dep[3])
    sm, dm = _add(s01, d01, s23, d23)
    return _tree(sm.reshape(nb, RB), dm.reshape(nb, RB))


def final(parts, deps):
    """k_reduce_final<0..2> over the concatenated partials."""
    n = parts.size
    rounds = (n + RB - 1) // RB
    p = np.zeros(rounds * RB)
    d = np.full(rounds * RB, -1, dtype=np.int64)
    p[:n] = parts
    d[:n] = deps
    p = p.reshape(rounds, RB)
    d = d.reshape(rounds, RB)
    acc = np.zeros(RB)
    da = np.full(RB, -1, dtype=np.int64)
    for r in range(rounds):
        live = d[r] >= 0
        s, dd = _add(acc, da, p[r], d[r])
        acc = np.where(live, s, acc)
        da = np.where(live, dd, da)
    v, dv = _tree(acc, da)
    return float(v), int(max(dv, 0))


def terms_of(kind, x, y=None):
    if kind == 0:
        return x * y
    return np.abs(x) if kind == 1 else x * x


def reduce_model(kind, xs, ys=None, **wrong):
    """(value, D) of reduce(kind, x, y); xs / ys: the per-box arrays of the
    level, shape (nz, ny, nx) each, in local box order."""
    ps, ds = [], []
    for n, x in enumerate(xs):
        p, d = box_partials(terms_of(kind, x, ys[n] if ys is not None else None), **wrong)
        ps.append(p)
        ds.append(d)
    return final(np.concatenate(ps), np.concatenate(ds))


def norm_model(xs, ord):
    """(value, D) of norm(x, ord), ord 1 or 2."""
    v, d = reduce_model(1 if ord == 1 else 2, xs)
    return (math.sqrt(v) if ord == 2 else v), d


def _split(a):
    c = 134217729.0 * a  # Veltkamp: 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def exact_sums(kind, xs, ys=None):
    """(fsum(terms), fsum(|terms|)) with the products of kinds 0 and 2 taken
    exactly: x * y = p + e (Dekker's two-product, exact for the magnitudes the
    tests use it with: no overflow or underflow in the split), so the sums are
    those of the unrounded terms."""
    vals, mags = [], []
    for n, x in enumerate(xs):
        x = np.ravel(x)
        if kind == 1:
            vals.append(np.abs(x))
            mags.append(np.abs(x))
            continue
        y = np.ravel(ys[n]) if kind == 0 else x
        p = x * y
        xh, xl = _split(x)
        yh, yl = _split(y)
        e = ((xh * yh - p) + xh * yl + xl * yh) + xl * yl
        sgn = np.where(p < 0, -1.0, 1.0)
        vals += [p, e]
        mags += [sgn * p, sgn * e]
    return math.fsum(np.concatenate(vals)), math.fsum(np.concatenate(mags))


def sum_bound(kind, d, mag):
    """gamma_D * sum |terms|; one more rounding for the products of kinds 0, 2."""
    return gamma(d + (0 if kind == 1 else 1)) * mag


def split_boxes(shape, lo, split):
    """The (nx, ny, nz) domain cut into split[d] near-equal parts along d, as
    (lo..., hi...) boxes, x fastest (decomposition.split_domain's order is not
    relied on: the tests read the layout back from the grid)."""
    cuts = []
    for d in range(3):
        n, p = shape[d], split[d]
        edges = [lo[d] + (n * i) // p for i in range(p + 1)]
        cuts.append([(edges[i], edges[i + 1] - 1) for i in range(p)])
    return [(x[0], y[0], z[0], x[1], y[1], z[1]) for z in cuts[2] for y in cuts[1] for x in cuts[0]]


def same_bits(a, b):
    """Two doubles with the same 64 bits (so -0.0 != 0.0, and a NaN equals
    only the same NaN)."""
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def assert_level_reductions(op, fx, fy, xs, ys, bounds=True):
    """dotProduct(fx, fy), norm(fx, 1), norm(fx, 2) of the operator equal the
    model bit for bit and sit within the derived bound of the exact sums;
    norm(fx, 0) is max |x| exactly.  xs / ys: what the fields hold, per local
    box.  bounds=False: fields whose products overflow or underflow (the
    exact-product split does not apply); the bit comparison stays.
    Returns the measured errors as fractions of their bounds."""
    ratios = {}
    cases = (("dot", 0, lambda: op.dotProduct(fx, fy), False),
             ("norm1", 1, lambda: op.norm(fx, 1), False),
             ("norm2", 2, lambda: op.norm(fx, 2), True))
    for name, kind, run, root in cases:
        got = run()
        want, d = reduce_model(kind, xs, ys)
        if root:
            want = math.sqrt(want)
        assert same_bits(got, want), (name, got, want)
        if not bounds:
            continue
        exact, mag = exact_sums(kind, xs, ys)
        if root:  # the same relative bound on the square root
            exact, bound = math.sqrt(exact), gamma(d + 1) * math.sqrt(exact)
        else:
            bound = sum_bound(kind, d, mag)
        err = abs(got - exact)
        print(f"{name}: D = {d}, |err| = {err:.3e}, bound = {bound:.3e}")
        assert err <= bound, (name, err, bound)
        ratios[name] = err / bound if bound else 0.0
    got = op.norm(fx, 0)
    want = max(float(np.max(np.abs(x))) for x in xs)
    assert same_bits(got, want), ("norm0", got, want)
    return ratios
