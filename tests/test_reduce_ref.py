"""The numpy model of the level reductions (tests/reduce_ref.py) on the CPU:
it sums what it should, to the accuracy its own addition tree allows, and
the shapes of the level-algebra tests can tell a subtly wrong order from the
right one.  (The GPU side, tests/test_level_algebra.py, holds the kernels to
this model bit for bit.)
"""
import math

import numpy as np
import pytest

from tests import reduce_ref as rr


def level_arrays(rng, case, lo=-1.0, hi=1.0):
    shape, corner, split = case
    out = []
    for b in rr.split_boxes(shape, corner, split):
        out.append(rng.uniform(lo, hi, (b[5] - b[2] + 1, b[4] - b[1] + 1, b[3] - b[0] + 1)))
    return out


def test_split_boxes_tile_the_domain():
    for shape, lo, split in rr.SHAPES:
        boxes = rr.split_boxes(shape, lo, split)
        assert len(boxes) == split[0] * split[1] * split[2]
        cells = sum((b[3] - b[0] + 1) * (b[4] - b[1] + 1) * (b[5] - b[2] + 1) for b in boxes)
        assert cells == shape[0] * shape[1] * shape[2]
        dom = rr.domain_of(shape, lo)
        assert min(b[0] for b in boxes) == dom[0] and max(b[5] for b in boxes) == dom[5]
    # the layouts the table names
    assert {b[3] - b[0] + 1 for b in rr.split_boxes(*rr.SHAPES[-1])} == {65}
    assert {b[4] - b[1] + 1 for b in rr.split_boxes(*rr.SHAPES[-1])} == {23}
    six = rr.split_boxes(*rr.SHAPES[-2])
    assert sum(rr.reduce_blocks(b[4] - b[1] + 1, b[5] - b[2] + 1) for b in six) == 6144


@pytest.mark.parametrize("case", rr.SHAPES, ids=rr.shape_id)
def test_model_within_its_own_error_bound(rng, case):
    # |model - exact| <= gamma_D * sum |terms|: derived from the model's own
    # addition tree (D; one more rounding for the products), not tuned.
    xs, ys = level_arrays(rng, case), level_arrays(rng, case)
    for kind in (0, 1, 2):
        got, d = rr.reduce_model(kind, xs, ys)
        exact, mag = rr.exact_sums(kind, xs, ys)
        err, bound = abs(got - exact), rr.sum_bound(kind, d, mag)
        print(f"{rr.shape_id(case)} kind {kind}: D = {d}, |err| = {err:.3e}, "
              f"bound = {bound:.3e}, ratio = {err / bound if bound else 0.0:.3g}")
        assert d <= 44
        assert err <= bound
    # norm(x, 2): the same relative bound g = gamma_(D+1) on the square root.
    # sqrt halves the sum's relative error and rounds once (g/2 + u); the
    # reference rounds its sum and its root (1.5 u): g/2 + 2.5 u <= g from
    # D + 1 = 5 on.  A single cell has no addition: both sides are
    # sqrt(fl(x^2)).
    got, d = rr.norm_model(xs, 2)
    exact, _ = rr.exact_sums(2, xs)
    ncell = sum(x.size for x in xs)
    assert d + 1 >= 5 or ncell == 1
    assert abs(got - math.sqrt(exact)) <= rr.gamma(d + 1) * math.sqrt(exact)
    got1, d1 = rr.norm_model(xs, 1)
    assert (got1, d1) == rr.reduce_model(1, xs)


def test_single_cell_and_identity():
    x = [np.array([[[-0.375]]])]
    assert rr.reduce_model(1, x) == (0.375, 0)
    assert rr.reduce_model(2, x) == (0.375 * 0.375, 0)
    assert rr.reduce_model(0, x, [np.array([[[2.0]]])]) == (-0.75, 0)
    z = [np.full((2, 3, 5), -0.0)]
    v, _ = rr.reduce_model(0, z, [np.ones((2, 3, 5))])
    assert v == 0.0 and not np.signbit(v)  # accumulators start at +0.0


def test_model_order_is_the_stated_one():
    # powers of two far enough apart that the order of the additions shows:
    # nx = 193, one row.  Lane 0 holds cells 0, 64, 128, 192 in a0..a3 and adds
    # (a0 + a1) + (a2 + a3); lane 1 holds 1, 65, 129 in a0 alone, in order.
    x = np.zeros((1, 1, 193))
    x[0, 0, [0, 64, 128, 192]] = [1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -53]
    # ((1 + 2^-53) = 1 (ties to even)) + (2^-53 + 2^-53 = 2^-52) = 1 + 2^-52
    v, _ = rr.reduce_model(1, [x])
    assert v == 1.0 + 2.0 ** -52
    x = np.zeros((1, 1, 193))
    x[0, 0, [1, 65, 129]] = [1.0, 2.0 ** -53, 2.0 ** -53]
    # sequential in a0: (1 + 2^-53) + 2^-53 = 1
    v, _ = rr.reduce_model(1, [x])
    assert v == 1.0
    # LDS tree: thread 0 meets thread 128 first (w = 128), then thread 64
    x = np.zeros((1, 3, 1))  # rows 0, 1, 2 -> waves 0, 1, 2 -> threads 0, 64, 128
    x[0, :, 0] = [1.0, 2.0 ** -53, 2.0 ** -53]
    v, _ = rr.reduce_model(1, [x])
    assert v == 1.0  # (1 + 2^-53) + 2^-53; wave-major order would give 1 + 2^-52
    x[0, :, 0] = [2.0 ** -53, 1.0, 2.0 ** -53]
    v, _ = rr.reduce_model(1, [x])
    assert v == 1.0 + 2.0 ** -52  # (2^-53 + 2^-53) + 1
    # two boxes: the partials are concatenated, the final adds them pairwise
    v, _ = rr.reduce_model(1, [np.full((1, 1, 1), 1.0), np.full((1, 1, 1), 2.0 ** -53)])
    assert v == 1.0


# nx = 256: every lane ends with its round of four, the a0 tail loop never runs
NO_TAIL = [c for c in rr.SHAPES if c[0] == (256, 2, 3)]


@pytest.mark.parametrize("case", rr.SHAPES, ids=rr.shape_id)
def test_wrong_models_violate_the_bound(rng, case):
    # the evidence that the shapes can tell a subtly wrong kernel from a right
    # one: a model without the a0 tail loop, and one that never visits a box's
    # last row, miss the derived bound on every shape meant to reach that code
    xs, ys = level_arrays(rng, case), level_arrays(rng, case)
    for kind in (0, 1, 2):
        right, d = rr.reduce_model(kind, xs, ys)
        exact, mag = rr.exact_sums(kind, xs, ys)
        bound = rr.sum_bound(kind, d, mag)
        tail, _ = rr.reduce_model(kind, xs, ys, drop_tail=True)
        if case in NO_TAIL:
            assert tail == right  # nx = 256: no tail, the variant changes nothing
        else:
            assert abs(tail - exact) > bound, (kind, abs(tail - exact) / bound)
        row, _ = rr.reduce_model(kind, xs, ys, skip_last_row=True)
        assert abs(row - exact) > bound, (kind, abs(row - exact) / bound)
