"""set_grids (SetGrids.cpp:31-149): the AMR hierarchy from
tagging.

CPU: the host clustering / nesting / owners of csrc/regrid.cpp, driven through
the C ABI with numpy masks, against the Python restatement tests/regrid_ref.py
(box lists equal exactly) and the invariants of a valid hierarchy.
GPU: the condition kernel against the numpy formula, the tag kernel against a
numpy restatement (exactly), set_grids end to end against the restatement,
the NL solve on the generated hierarchy against the oracle loop, two ranks
against one, and tools/run_poisson.py --max-level as a user starts it.
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests import regrid_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = os.path.join(ROOT, "tests", "golden", "params.txt")


def _grids():
    from mg_ic_code_amd import grids
    return grids


# ------------------------------------------------------------------ masks
def _mask(shape_xyz, cells=(), boxes=()):
    nx, ny, nz = shape_xyz
    m = np.zeros((nz, ny, nx), dtype=np.uint8)
    for i, j, k in cells:
        m[k, j, i] = 1
    for b in boxes:
        m[b[2]:b[5] + 1, b[1]:b[4] + 1, b[0]:b[3] + 1] = 1
    return m


def _l_shape():
    return _mask((8, 8, 2), boxes=[(0, 0, 0, 7, 1, 1), (0, 2, 0, 1, 7, 1)])


def _plus_shape():
    return _mask((9, 9, 1), boxes=[(3, 0, 0, 5, 8, 0), (0, 3, 0, 8, 5, 0)])


def _diagonal():
    return _mask((8, 8, 8), cells=[(i, i, i) for i in range(8)])


def _slab():
    return _mask((12, 5, 3), boxes=[(0, 0, 0, 11, 4, 2)])


NAMED = {
    "empty": _mask((4, 4, 4)),
    "one_cell": _mask((5, 4, 3), cells=[(3, 1, 2)]),
    "full": _mask((5, 4, 3), boxes=[(0, 0, 0, 4, 3, 2)]),
    "two_blobs": _mask((10, 6, 4), boxes=[(0, 0, 0, 2, 2, 1), (6, 3, 2, 9, 5, 3)]),
    "l_shape": _l_shape(),
    "plus_shape": _plus_shape(),
    "diagonal": _diagonal(),
    "slab": _slab(),
}
FILLS = (0.3, 0.5, 0.75, 1.0)
MAXLENS = (1, 2, 5)


def _random_masks():
    rng = np.random.default_rng(20261019)
    return [(rng.random((6, 7, 9)) < 0.15).astype(np.uint8) for _ in range(20)]


def _check_invariants(mask, boxes, pre, fill_ratio, maxlen):
    assert R.disjoint(boxes)
    cover = R.paint(boxes, mask.shape)
    assert cover.max(initial=0) <= 1
    assert np.all(cover[mask != 0] == 1)  # every set cell is covered
    for b in boxes:
        assert all(0 <= b[d] <= b[3 + d] < mask.shape[2 - d] for d in range(3))
        assert all(b[3 + d] - b[d] + 1 <= maxlen for d in range(3))
    assert sum(R.box_cells(b) for b in boxes) == sum(R.box_cells(q) for q in pre)
    for q in pre:  # accepted boxes: full enough, or one lattice cell
        n = int(np.count_nonzero(mask[q[2]:q[5] + 1, q[1]:q[4] + 1, q[0]:q[3] + 1]))
        assert n >= fill_ratio * R.box_cells(q) or R.box_cells(q) == 1
    assert boxes == sorted(boxes, key=lambda b: (b[2], b[1], b[0]))


@pytest.mark.parametrize("name", sorted(NAMED))
@pytest.mark.parametrize("fill_ratio", FILLS)
def test_cluster_named_masks_match_restatement(name, fill_ratio):
    G = _grids()
    mask = NAMED[name]
    for maxlen in MAXLENS + (64,):
        ref, pre = R.cluster(mask, fill_ratio, maxlen)
        assert G.regrid_cluster(mask, fill_ratio, maxlen) == ref
        _check_invariants(mask, ref, pre, fill_ratio, maxlen)


def test_cluster_random_masks_match_restatement():
    G = _grids()
    for mask in _random_masks():
        for fill_ratio in FILLS:
            for maxlen in MAXLENS:
                ref, pre = R.cluster(mask, fill_ratio, maxlen)
                assert G.regrid_cluster(mask, fill_ratio, maxlen) == ref
                _check_invariants(mask, ref, pre, fill_ratio, maxlen)


def test_cluster_cut_kinds_and_simple_results():
    G = _grids()
    assert G.regrid_cluster(NAMED["empty"], 0.5, 4) == []
    assert G.regrid_cluster(NAMED["one_cell"], 0.5, 4) == [(3, 1, 2, 3, 1, 2)]
    assert G.regrid_cluster(NAMED["full"], 1.0, 8) == [(0, 0, 0, 4, 3, 2)]
    # the cuts the restatement takes (the C side returns the same boxes)
    tr = []
    ref, _ = R.cluster(NAMED["two_blobs"], 0.75, 64, tr)
    assert tr == ["hole"] and ref == [(0, 0, 0, 2, 2, 1), (6, 3, 2, 9, 5, 3)]
    assert G.regrid_cluster(NAMED["two_blobs"], 0.75, 64) == ref
    for name in ("l_shape", "plus_shape"):
        tr = []
        R.cluster(NAMED[name], 0.75, 64, tr)
        assert tr and tr[0] == "inflection", (name, tr)
    tr = []
    ref, _ = R.cluster(NAMED["diagonal"], 0.5, 64, tr)
    assert tr and set(tr) == {"bisect"}
    assert ref == [(i, i, i, i, i, i) for i in range(8)]  # down to single cells
    assert G.regrid_cluster(NAMED["diagonal"], 0.5, 64) == ref


def test_split_max_sizes_on_the_slab():
    G = _grids()
    slab = NAMED["slab"]
    for maxlen, nbox in ((1, 180), (2, 6 * 3 * 2), (5, 3 * 1 * 1)):
        boxes = G.regrid_cluster(slab, 0.5, maxlen)
        assert len(boxes) == nbox
        assert boxes == R.cluster(slab, 0.5, maxlen)[0]
        for d in range(3):
            sizes = sorted({b[3 + d] - b[d] + 1 for b in boxes})
            assert sizes[-1] <= maxlen and sizes[-1] - sizes[0] <= 1
    # 12 cells at maxlen 5: pieces of 4 (ceil(12 / 5) = 3 equal pieces)
    assert [b[3] - b[0] + 1 for b in G.regrid_cluster(slab, 0.5, 5)] == [4, 4, 4]
    # 5 cells at maxlen 2: 2, 2, 1 -- the larger pieces first
    col = _mask((1, 5, 1), boxes=[(0, 0, 0, 0, 4, 0)])
    assert [b[4] - b[1] + 1 for b in G.regrid_cluster(col, 0.5, 2)] == [2, 2, 1]


# ------------------------------------------------------------------ regrid over levels
BF, MGS, FR = 8, 16, 0.5


def _three_level_tags():
    """Synthetic tag lattices of levels 0..2 of a 32^3 base (c = 4): level-2
    tags at the +x edge of the old level-2 box, so the new level-3 boxes reach
    beyond what level 1's own tags produce and nesting tags must be added."""
    c = 4
    # level 0 (lattice 8^3): tags around the centre
    m0 = np.zeros((8, 8, 8), np.uint8)
    m0[3:5, 3:5, 3:5] = 1
    # level 1 (domain 64^3): the old box [24, 39]^3 grown by 2 -> lattice [5, 10]
    lo1 = (5, 5, 5)
    m1 = np.zeros((6, 6, 6), np.uint8)
    m1[2:4, 2:4, 2:4] = 1  # lattice [7, 8]: cells [28, 35]
    # level 2 (domain 128^3): the old box [56, 71]^3 grown by 2 -> lattice [13, 18]
    lo2 = (13, 13, 13)
    m2 = np.zeros((6, 6, 6), np.uint8)
    m2[2:4, 2:4, 4:6] = 1  # x lattice [17, 18]: cells [68, 75], the +x edge
    return c, [((0, 0, 0), m0), (lo1, m1), (lo2, m2)]


def _nested(fine, coarse, dom_fine, radius, periodic=False):
    """coarsen(fine, 2) grown by radius (clipped to the coarse domain; periodic:
    wrapped round it) lies in the union of `coarse` boxes, for every fine box."""
    dom_c = tuple(v // 2 for v in dom_fine)
    n = dom_c[3] - dom_c[0] + 1
    cover = R.paint([tuple(v - dom_c[i % 3] for i, v in enumerate(b)) for b in coarse], (n, n, n))
    for f in fine if periodic else ():
        ix = [[(v - dom_c[d]) % n for v in range(f[d] // 2 - radius, f[3 + d] // 2 + radius + 1)]
              for d in range(3)]
        if not np.all(cover[np.ix_(ix[2], ix[1], ix[0])] == 1):
            return False
    for f in fine:
        lo = [max(f[d] // 2 - radius, dom_c[d]) - dom_c[d] for d in range(3)]
        hi = [min(f[3 + d] // 2 + radius, dom_c[3 + d]) - dom_c[d] for d in range(3)]
        if not np.all(cover[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] == 1):
            return False
    return True


def test_regrid_levels_nesting_alignment_and_restatement():
    G = _grids()
    c, tags = _three_level_tags()
    dom0 = (0, 0, 0, 31, 31, 31)
    boxes, fin = G.regrid_levels(dom0, tags, BF, MGS, FR)
    ref, rfin = R.regrid(dom0, tags, BF, MGS, FR)
    assert boxes == ref and fin == rfin == 3
    # without the nesting tags level 2 would not hold level 3
    lone, _ = R.regrid(dom0, tags[:2], BF, MGS, FR)
    dom3 = (0, 0, 0, 255, 255, 255)
    assert not _nested(boxes[2], lone[1], dom3, 2)
    doms = [dom0]
    for _ in range(3):
        doms.append(tuple(2 * v for v in doms[-1][:3]) + tuple(2 * v + 1 for v in doms[-1][3:]))
    for l in (1, 2, 3):
        bl = boxes[l - 1]
        assert bl and R.disjoint(bl)
        for b in bl:
            assert all(doms[l][d] <= b[d] <= b[3 + d] <= doms[l][3 + d] for d in range(3))
            assert all(b[d] % BF == 0 and (b[3 + d] + 1) % BF == 0 for d in range(3))
            assert all(b[3 + d] - b[d] + 1 <= MGS for d in range(3))
    # the nesting inequality, on the integer boxes: coarsen(level l + 1) grown
    # by 2 level-l cells inside the union of level l
    assert _nested(boxes[1], boxes[0], doms[2], 2)
    assert _nested(boxes[2], boxes[1], doms[3], 2)
    # every tagged lattice cell is covered by the next level
    for l, (lo, m) in enumerate(tags):
        n = doms[l + 1][3] + 1
        cover = R.paint(boxes[l], (n, n, n))
        for k, j, i in zip(*np.nonzero(m)):
            x, y, z = ((i + lo[0]) * c * 2, (j + lo[1]) * c * 2, (k + lo[2]) * c * 2)
            assert np.all(cover[z:z + 2 * c, y:y + 2 * c, x:x + 2 * c] == 1)


def test_regrid_levels_no_tags_and_single_level():
    G = _grids()
    dom0 = (0, 0, 0, 31, 31, 31)
    boxes, fin = G.regrid_levels(dom0, [((0, 0, 0), np.zeros((8, 8, 8), np.uint8))], BF, MGS, FR)
    assert boxes == [[]] and fin == 0
    m = np.zeros((8, 8, 8), np.uint8)
    m[0, 0, 0] = m[7, 7, 7] = 1
    boxes, fin = G.regrid_levels(dom0, [((0, 0, 0), m)], BF, MGS, FR)
    assert fin == 1 and boxes == R.regrid(dom0, [((0, 0, 0), m)], BF, MGS, FR)[0]
    assert boxes[0] == [(0, 0, 0, 7, 7, 7), (56, 56, 56, 63, 63, 63)]


def test_regrid_error_returns():
    G = _grids()
    from mg_ic_code_amd import MgicError
    m = np.ones((2, 2, 2), np.uint8)
    with pytest.raises(MgicError) as e:  # block_factor not a power of two
        G.regrid_levels((0, 0, 0, 31, 31, 31), [((0, 0, 0), m)], 6, 16, 0.5)
    assert e.value.code == -1
    with pytest.raises(MgicError) as e:
        G.regrid_lattice(12, 16)
    assert e.value.code == -1
    with pytest.raises(MgicError) as e:  # 30 is not a multiple of c = 4
        G.regrid_levels((0, 0, 0, 29, 29, 29), [((0, 0, 0), m)], 8, 16, 0.5)
    assert e.value.code == -1
    with pytest.raises(ValueError):
        R.regrid((0, 0, 0, 29, 29, 29), [((0, 0, 0), m)], 8, 16, 0.5)
    assert G.regrid_lattice(8, 16) == (4, 2) == R.lattice_params(8, 16)
    assert G.regrid_lattice(1, 16) == (1, 16) == R.lattice_params(1, 16)


def test_owners_contiguous_balanced_and_match_restatement():
    G = _grids()
    rng = np.random.default_rng(7)
    lists = [R.cluster(m, 0.5, 2)[0] for m in _random_masks()[:6]]
    lists.append([(16 * i, 16 * j, 16 * k, 16 * i + 15, 16 * j + 15, 16 * k + 15)
                  for k in range(3) for j in range(3) for i in range(3)])
    lists.append([(0, 0, 0, int(rng.integers(1, 9)), 3, 3)])
    for boxes in lists:
        for size in (1, 2, 3, 8):
            own = G.regrid_owners(boxes, size)
            assert own == R.owners(boxes, size)
            assert all(0 <= r < size for r in own)
            assert own == sorted(own)  # contiguous runs of the sorted list
            cells = [R.box_cells(b) for b in boxes]
            mean = sum(cells) / size
            for r in range(size):
                load = sum(n for n, o in zip(cells, own) if o == r)
                assert abs(load - mean) <= max(cells)
    assert G.regrid_owners([], 4) == []


def test_params_reads_regrid_keys():
    from mg_ic_code_amd.params import read_params_file
    p = read_params_file(PARAMS)
    assert (p.refine_threshold, p.fill_ratio, p.buffer_size) == (0.1, 0.5, 3)


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def comm():
    import mg_ic_code_amd as mg
    return mg.Comm()


TWO_HOLES = "two holes"  # params.txt's own configuration (both punctures)


def _centred_params(bh1_offset="0.0", **more):
    from mg_ic_code_amd.params import read_params_file
    if bh1_offset == TWO_HOLES:
        return read_params_file(PARAMS, overrides=dict(
            block_factor="8", max_grid_size="16", fill_ratio="0.5", **more))
    return read_params_file(PARAMS, overrides=dict(
        bh1_offset=bh1_offset, bh2_bare_mass="0.0", bh2_spin="0.0", bh2_momentum="0.0",
        block_factor="8", max_grid_size="16", fill_ratio="0.5"))


PATCH_DOM = (0, 0, 0, 63, 63, 63)  # level 1 of a 32^3 base
PATCH_BOXES = [(8, 8, 8, 23, 23, 23), (24, 8, 8, 39, 23, 23)]  # lows (8,8,8), (24,8,8)


@pytest.mark.gpu
def test_regrid_condition_single_box(comm):
    import mg_ic_code_amd as mg
    from mg_ic_code_amd.params import read_params_file
    G = _grids()
    p = read_params_file(PARAMS)
    n = 16
    dom = (0, 0, 0, n - 1, n - 1, n - 1)
    dx = p.L / n
    grid = mg.Grid(comm, dom, [dom], dx)
    out = mg.LevelData(grid)
    G.set_regrid_condition(None, out, p.bh())
    ref = R.regrid_condition(p.bh(), dom[:3], dom[3:], dx)
    got = out.download(0)
    print("condition 16^3: max rel err", np.max(np.abs(got - ref) / np.abs(ref)))
    np.testing.assert_allclose(got, ref, rtol=1e-13, atol=1e-300)


@pytest.mark.gpu
@pytest.mark.parametrize("with_psi", [False, True], ids=["psi_null", "psi_field"])
def test_regrid_condition_patch_level(comm, with_psi):
    import mg_ic_code_amd as mg
    from mg_ic_code_amd.params import read_params_file
    G = _grids()
    p = read_params_file(PARAMS)
    dx = p.L / 32 / 2
    grid = mg.Grid(comm, PATCH_DOM, PATCH_BOXES, dx, patches=True)
    out = mg.LevelData(grid)
    psi, psis = None, {}
    if with_psi:
        rng = np.random.default_rng(20261019)
        psi = mg.LevelData(grid)
        for k in range(grid.num_local):
            psis[k] = rng.uniform(0.9, 1.1, tuple(s + 2 for s in _shape(grid.local_box(k))))
            psi.upload(k, psis[k], with_ghosts=True)
    G.set_regrid_condition(psi, out, p.bh())
    assert grid.num_local == 2
    for k in range(grid.num_local):
        b = grid.local_box(k)
        ref = R.regrid_condition(p.bh(), b[:3], b[3:], dx,
                                 psis[k][1:-1, 1:-1, 1:-1] if with_psi else None)
        got = out.download(k)
        print("condition patch", k, "max rel err", np.max(np.abs(got - ref) / np.abs(ref)))
        np.testing.assert_allclose(got, ref, rtol=1e-13, atol=1e-300)


def _tag_case(comm, dom, boxes, patches, conds, tag_val, grow, c):
    import mg_ic_code_amd as mg
    G = _grids()
    grid = mg.Grid(comm, dom, boxes, 1.0, patches=patches)
    f = mg.LevelData(grid)
    local = []
    for k in range(grid.num_local):
        b = grid.local_box(k)
        local.append(b)
        f.upload(k, conds[boxes.index(b)])
    lo, mask = G.tag_lattice(f, tag_val, grow, c)
    rlo, rmask = R.tag_lattice([conds[boxes.index(b)] for b in local], local, dom, tag_val, grow, c,
                               all_boxes=boxes)
    assert tuple(lo) == tuple(rlo)
    assert mask.shape == rmask.shape
    assert np.array_equal(mask, rmask), (np.argwhere(mask != rmask)[:8], lo)
    return lo, mask


def _shape(b):
    return (b[5] - b[2] + 1, b[4] - b[1] + 1, b[3] - b[0] + 1)


TAG_VAL = 0.75


def _single_box_cond():
    """24 x 16 x 8: tags on the domain corners, an interior pair, one value
    exactly tag_val, a negative one above it in magnitude; everything else
    below (one just below tag_val)."""
    a = np.full((8, 16, 24), 0.25)
    for k, j, i in ((0, 0, 0), (7, 15, 23), (0, 15, 0), (7, 0, 23)):
        a[k, j, i] = 2.0
    a[3, 7, 11] = TAG_VAL             # exactly the threshold: tagged (>=)
    a[4, 9, 17] = -3.0                # negative, above in magnitude
    a[2, 3, 5] = np.nextafter(TAG_VAL, 0.0)  # just below: not tagged
    a[5, 12, 20] = -np.nextafter(TAG_VAL, 0.0)
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("c,grow", [(4, 2), (1, 2), (8, 0)])
def test_tag_lattice_single_box(comm, c, grow):
    dom = (0, 0, 0, 23, 15, 7)
    a = _single_box_cond()
    lo, mask = _tag_case(comm, dom, [dom], False, [a], TAG_VAL, grow, c)
    assert tuple(lo) == (0, 0, 0) and mask.shape == (-(-8 // c), -(-16 // c), -(-24 // c))
    assert 0 < mask.sum() < mask.size
    # tagVal = 0 tags every cell (the reference's >=)
    lo, mask = _tag_case(comm, dom, [dom], False, [np.zeros_like(a)], 0.0, grow, c)
    assert mask.all()


@pytest.mark.gpu
@pytest.mark.parametrize("c,grow", [(1, 2), (4, 2), (2, 1)])
def test_tag_lattice_across_wave_boundaries(comm, c, grow):
    # a row of 160 cells is three waves of the kernel (64 lanes along x): runs
    # of tagged cells across the wave boundaries (lane 63 -> lane 0 of the next
    # wave, which has no lane before it to leave a lattice column to), a whole
    # tagged wave, and single tags either side of a boundary
    dom = (0, 0, 0, 159, 5, 3)
    a = np.full((4, 6, 160), 0.25)
    a[1, 2, 63:66] = 1.0        # i = 63, 64, 65
    a[2, 4, 60:132] = -1.0      # a run over two boundaries, lanes 0..63 of wave 1 all tagged
    a[0, 0, 127] = 2.0          # the last lane of a wave alone
    a[3, 5, 128] = 2.0          # the first lane of a wave alone
    a[3, 1, 0] = a[3, 1, 159] = TAG_VAL
    lo, mask = _tag_case(comm, dom, [dom], False, [a], TAG_VAL, grow, c)
    assert 0 < mask.sum() < mask.size
    _tag_case(comm, dom, [dom], False, [np.ones_like(a)], TAG_VAL, grow, c)


THREE_DOM = (0, 0, 0, 31, 31, 31)
# two boxes sharing an x face, one isolated box in the far domain corner
THREE_BOXES = [(8, 8, 8, 15, 15, 15), (16, 8, 8, 23, 15, 15), (24, 24, 24, 31, 31, 31)]


def _three_box_conds():
    conds = [np.full(_shape(b), 0.25) for b in THREE_BOXES]
    conds[0][0, 0, 0] = 1.0        # a box corner: grows into cells of no box
    conds[0][3, 4, 7] = -1.0       # on the face shared with box 1: grows into it
    conds[1][7, 7, 0] = TAG_VAL    # the other side of the shared face, exactly tag_val
    conds[1][2, 2, 7] = 5.0        # +x face of box 1: grows out of every box
    conds[2][7, 7, 7] = -2.0       # the domain corner: growth clipped at the domain
    conds[2][0, 7, 3] = 1.5
    return conds


@pytest.mark.gpu
@pytest.mark.parametrize("c,grow", [(4, 2), (1, 2), (8, 0), (2, 3)])
def test_tag_lattice_three_boxes(comm, c, grow):
    conds = _three_box_conds()
    lo, mask = _tag_case(comm, THREE_DOM, THREE_BOXES, True, conds, TAG_VAL, grow, c)
    # the bounding box of the level grown by `grow`, not the domain
    assert tuple(lo) == ((8 - grow) // c,) * 3
    assert mask.shape == ((31 // c) - (8 - grow) // c + 1,) * 3
    if grow:
        # the corner tag of box 0 reaches below the box (cells of no box)
        assert mask[0, 0, 0] == 1
    lo, mask = _tag_case(comm, THREE_DOM, THREE_BOXES, True,
                         [np.zeros_like(a) for a in conds], 0.0, grow, c)
    full = R.paint([tuple(max(b[d] - grow, 0) // c - lo[d] for d in range(3)) +
                    tuple(min(b[3 + d] + grow, 31) // c - lo[d] for d in range(3))
                    for b in THREE_BOXES], mask.shape)
    assert np.array_equal(mask != 0, full != 0)


# ---- set_grids end to end: params.txt with one centred black hole, 32^3
# base, max_level 2, block_factor 8, max_grid_size 16, fill_ratio 0.5
N0 = 32
_REF = {}


def _reference_hierarchy(bh1_offset="0.0", n0=N0, **more):
    """The restatement's set_grids for the one-hole configuration (the
    centred one by default) or TWO_HOLES, computed once each: per pass the
    level conditions, tagVal margins, lattice fills and boxes."""
    key = (bh1_offset, n0) + tuple(sorted(more.items()))
    if key in _REF:
        return _REF[key]
    prm = _centred_params(bh1_offset, **more)
    bh = prm.bh()
    c, _ = R.lattice_params(prm.block_factor, prm.max_grid_size)
    dom0 = (0, 0, 0, n0 - 1, n0 - 1, n0 - 1)
    levels = [[dom0]]
    top, margins, fills = 0, {}, {}
    more = True
    while more:
        more = False
        old_top = top
        tags = []
        dom, dx = dom0, prm.L / n0
        for l, boxes in enumerate(levels):
            conds = [R.regrid_condition(bh, b[:3], b[3:], dx) for b in boxes]
            mx = max(np.abs(a).max() for a in conds)
            tag_val = mx * prm.refine_threshold
            margins[l] = min(np.abs(np.abs(a) / tag_val - 1.0).min() for a in conds)
            lo, mask = R.tag_lattice(conds, boxes, dom, tag_val, 2, c)
            tags.append((lo, mask))
            zz, yy, xx = np.nonzero(mask)
            fills[l] = mask.sum() / ((np.ptp(zz) + 1) * (np.ptp(yy) + 1) * (np.ptp(xx) + 1))
            dom = tuple(2 * v for v in dom[:3]) + tuple(2 * v + 1 for v in dom[3:])
            dx /= 2
        new, fin = R.regrid(dom0, tags, prm.block_factor, prm.max_grid_size, prm.fill_ratio)
        if fin > top:
            top += 1
        levels = [[dom0]] + new[:top]
        if top < 2 and top > old_top:
            more = True
    _REF[key] = dict(prm=prm, levels=levels, margins=margins, fills=fills)
    return _REF[key]


def _union_box(boxes):
    u = tuple(min(b[d] for b in boxes) for d in range(3)) + \
        tuple(max(b[3 + d] for b in boxes) for d in range(3))
    assert R.disjoint(boxes) and sum(R.box_cells(b) for b in boxes) == R.box_cells(u)
    return u


def test_reference_hierarchy_of_the_centred_configuration():
    # the restatement alone (no GPU): no cell sits on the tagging threshold,
    # and the hierarchy is the one DESIGN.md 3f quotes
    ref = _reference_hierarchy()
    print("margins", ref["margins"], "fills", ref["fills"])
    assert all(m > 1e-9 for m in ref["margins"].values())
    lv = ref["levels"]
    assert len(lv) == 3
    assert _union_box(lv[1]) == (8, 8, 8, 55, 55, 55)
    assert _union_box(lv[2]) == (40, 40, 40, 87, 87, 87)
    for l in (1, 2):
        assert len(lv[l]) == 27
        assert all(b[3 + d] - b[d] + 1 == 16 for b in lv[l] for d in range(3))
    assert abs(ref["fills"][0] - 0.85) < 0.01 and abs(ref["fills"][1] - 0.96) < 0.01


def _device_hierarchy(comm, bh1_offset="0.0", n0=N0, **more):
    import mg_ic_code_amd as mg
    G = _grids()
    prm = _centred_params(bh1_offset, **more)
    dom0 = (0, 0, 0, n0 - 1, n0 - 1, n0 - 1)
    base = mg.Grid(comm, dom0, [dom0], prm.L / n0)
    return prm, G.set_grids(comm, prm, base, max_level=2)


@pytest.mark.gpu
def test_set_grids_matches_restatement(comm):
    import mg_ic_code_amd as mg
    ref = _reference_hierarchy()
    assert all(m > 1e-9 for m in ref["margins"].values()), ref["margins"]
    prm, grids = _device_hierarchy(comm)
    assert [g.boxes for g in grids] == ref["levels"]
    assert len(grids) == 3
    for l in (1, 2):
        g = grids[l]
        n = N0 << l
        assert g.domain == (0, 0, 0, n - 1, n - 1, n - 1) and g.dx == prm.L / n
        assert R.disjoint(g.boxes)
        for b in g.boxes:
            assert all(b[d] % 8 == 0 and (b[3 + d] + 1) % 8 == 0 for d in range(3))
            assert all(b[3 + d] - b[d] + 1 <= 16 for d in range(3))
        assert g.owners == [0] * len(g.boxes)
    assert _nested(grids[2].boxes, grids[1].boxes, grids[2].domain, 2)
    # AMRSolver's CFLevel checks the proper nesting of every level
    fields = [(g, mg.LevelData(g), mg.LevelData(g)) for g in grids]
    for _, a, b in fields:
        a.set_val(-1.0)
        b.set_val(1.0)
    amr = mg.AMRSolver(fields, mg.OperatorParams(alpha=1.0, beta=-1.0),
                       mg.SolverParams(max_depth=2, bottom_solver=0))
    assert amr.num_levels == 3


@pytest.mark.gpu
def test_nl_solve_on_generated_hierarchy_matches_oracle(comm):
    # poisson_solve on the generated multi-box grids (32^3 + 27 x 16^3 + 27 x
    # 16^3) against the oracle loop on each level's union box (48^3 each), with
    # the comparisons of test_amr_nl_loop_matches_oracle
    from mg_ic_code_amd.nl import poisson_solve
    from tests.nl_ref import oracle_poisson_solve_amr
    prm, grids = _device_hierarchy(comm)
    unions = [_union_box(g.boxes) for g in grids]  # asserts each union is a box
    res = poisson_solve(grids, prm, max_depth=3, max_NL_iterations=2)
    psi_o, norms_o, iters_o = oracle_poisson_solve_amr(prm, unions, N0, max_depth=3, n_nl=2)
    print("linear iterations", res.linear_iterations, iters_o, "norms", res.dpsi_norms, norms_o)
    assert res.linear_iterations[:2] == iters_o[:2]
    np.testing.assert_allclose(res.dpsi_norms[:2], norms_o[:2], rtol=1e-6)
    for l, (g, u) in enumerate(zip(grids, unions)):
        got = np.zeros(_shape(u))
        for k in range(g.num_local):
            b = g.local_box(k)
            got[b[2] - u[2]:b[5] - u[2] + 1, b[1] - u[1]:b[4] - u[1] + 1,
                b[0] - u[0]:b[3] - u[0] + 1] = res.psi[l].download(k)
        c = psi_o[l][1:-1, 1:-1, 1:-1]
        err = np.linalg.norm(got - c) / np.linalg.norm(c)
        print("level", l, "relative L2 difference", err)
        assert np.linalg.norm(got - c) <= 1e-10 * np.linalg.norm(c), l


# ---- a generated hierarchy whose union is not a box.  The off-centre hole
# and params.txt's two equal holes give cubes of 16^3 boxes on every level
# (at a 16^3 and a 32^3 base, for thresholds 0.1 ... 0.7), so: two unequal
# holes, the light one further out, on a 16^3 base.  Level 1 is the whole
# 32^3 index space as 8 boxes; level 2 is a 16 x 32 x 32 slab of four boxes
# around the heavy hole with a bar of two boxes (16 and 8 cells long) towards
# the light one on its x-lo face: a T, with faces that are part fine-fine and
# part coarse-fine and concave corners.
NONBOX = dict(refine_threshold="0.3", bh2_bare_mass="0.1", bh2_offset="-20.0")
NONBOX_N0 = 16


def _is_box(boxes):
    u = tuple(min(b[d] for b in boxes) for d in range(3)) + \
        tuple(max(b[3 + d] for b in boxes) for d in range(3))
    return sum(R.box_cells(b) for b in boxes) == R.box_cells(u)


def test_reference_hierarchy_whose_union_is_not_a_box():
    for bh1_offset, kw in ((OFF_CENTRE, {}), (TWO_HOLES, {})):  # (why neither is used)
        assert all(_is_box(bs) for bs in _reference_hierarchy(bh1_offset, NONBOX_N0, **kw)["levels"])
    ref = _reference_hierarchy(TWO_HOLES, NONBOX_N0, **NONBOX)
    print("margins", ref["margins"], "fills", ref["fills"])
    assert all(m > 1e-9 for m in ref["margins"].values())  # no cell on the tagging threshold
    lv = ref["levels"]
    assert [len(bs) for bs in lv] == [1, 8, 6]
    assert all(R.disjoint(bs) for bs in lv)
    assert _is_box(lv[1]) and not _is_box(lv[2])
    assert _nested(lv[2], lv[1], (0, 0, 0, 63, 63, 63), 2)


def test_regrid_is_not_periodic_aware():
    # DESIGN.md 3f, the limitation that stands: tags and nesting are clipped to
    # the domain, so a hole near a face gives a level 2 on that face with no
    # level 1 at the opposite one -- properly nested on a bounded domain, not
    # on a periodic one, where AMRSolver rejects it (test_amr_multibox.py)
    lv = _reference_hierarchy("30.0")["levels"]
    assert max(b[3] for b in lv[2]) == 4 * N0 - 1 and min(b[0] for b in lv[1]) > 0
    assert _nested(lv[2], lv[1], (0, 0, 0, 4 * N0 - 1, 4 * N0 - 1, 4 * N0 - 1), 1)
    assert not _nested(lv[2], lv[1], (0, 0, 0, 4 * N0 - 1, 4 * N0 - 1, 4 * N0 - 1), 1, periodic=True)


@pytest.mark.gpu
def test_nl_solve_on_generated_non_box_hierarchy_matches_oracle(comm):
    # poisson_solve on set_grids' output (16^3 + 8 x 16^3 + 6 boxes in a T)
    # against the oracle loop on the same box lists, every box with its own
    # ghosts; the comparisons of test_nl_solve_on_generated_hierarchy_matches_oracle
    from mg_ic_code_amd.nl import poisson_solve
    from tests.nl_ref import oracle_poisson_solve_amr
    ref = _reference_hierarchy(TWO_HOLES, NONBOX_N0, **NONBOX)
    assert all(m > 1e-9 for m in ref["margins"].values()), ref["margins"]
    prm, grids = _device_hierarchy(comm, TWO_HOLES, NONBOX_N0, **NONBOX)
    assert [g.boxes for g in grids] == ref["levels"]
    assert not _is_box(grids[2].boxes)
    res = poisson_solve(grids, prm, max_depth=2, max_NL_iterations=2)
    psi_o, norms_o, iters_o = oracle_poisson_solve_amr(
        prm, [grids[0].boxes[0]] + [g.boxes for g in grids[1:]], NONBOX_N0, max_depth=2, n_nl=2)
    print("linear iterations", res.linear_iterations, iters_o, "norms", res.dpsi_norms, norms_o)
    assert res.linear_iterations[:2] == iters_o[:2]
    np.testing.assert_allclose(res.dpsi_norms[:2], norms_o[:2], rtol=1e-6)
    for l, g in enumerate(grids):
        got = [None] * len(g.boxes)
        for k in range(g.num_local):
            got[g.boxes.index(g.local_box(k))] = res.psi[l].download(k)
        want = [p[1:-1, 1:-1, 1:-1] for p in psi_o[l]]
        num = np.sqrt(sum(np.sum((a - b) ** 2) for a, b in zip(got, want)))
        den = np.sqrt(sum(np.sum(b ** 2) for b in want))
        print("level", l, "relative L2 difference", num / den)
        assert num <= 1e-10 * den, l


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_workers(tmp_path, script, args, world, timeout):
    """Fresh interpreters, one per rank, each with its own time limit; the
    first non-zero exit ends the run."""
    port = _free_port()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", PYTHONUNBUFFERED="1")
    procs, logs = [], []
    for r in range(world):
        log = open(tmp_path / f"w{r}.log", "w")
        logs.append(log)
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(ROOT, "tests", script), "--rank", str(r),
             "--world", str(world), "--port", str(port), "--out", str(tmp_path)] + args,
            stdout=log, stderr=subprocess.STDOUT, env=env))
    rcs = []
    try:
        for p in procs:
            rcs.append(p.wait(timeout=timeout))
            if rcs[-1] != 0:
                break
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
        for log in logs:
            log.close()
    texts = [(tmp_path / f"w{r}.log").read_text() for r in range(world)]
    if any(rcs) or len(rcs) != world:
        pytest.fail(f"workers exited {rcs}:\n" + "\n".join(x[-3000:] for x in texts))
    return [json.load(open(tmp_path / f"rank{r}.json")) for r in range(world)]


OFF_CENTRE = "10.0"  # params.txt's own bh1_offset


def test_two_rank_case_needs_the_global_max_norm():
    # the two-rank case below: one hole at x = +10, the base level split in x.
    # The low-x rank's own maximum of the condition is far below the level's,
    # so a tagVal from a rank-local norm would tag other cells there
    prm = _centred_params(OFF_CENTRE)
    cond = R.regrid_condition(prm.bh(), (0, 0, 0), (N0 - 1,) * 3, prm.L / N0)
    lo_half = np.abs(cond[:, :, :N0 // 2])
    tv_global = np.abs(cond).max() * prm.refine_threshold
    tv_local = lo_half.max() * prm.refine_threshold
    assert tv_local < 0.5 * tv_global
    assert np.count_nonzero(lo_half >= tv_local) > np.count_nonzero(lo_half >= tv_global)


@pytest.mark.gpu
def test_set_grids_two_ranks_match_single_process(comm, tmp_path):
    # the base level as two x slabs, one per rank (both on device 0, peer-mapped
    # transport), the hole inside rank 1's slab: every rank returns the
    # single-process hierarchy and owners (tagVal from the all-rank max norm,
    # the masks OR-ed over the ranks)
    out = _run_workers(tmp_path, "regrid_worker.py",
                       ["--bh1-offset", OFF_CENTRE, "--split-dir", "0"], 2, 180)
    G = _grids()
    _, grids = _device_hierarchy(comm, OFF_CENTRE)
    assert len(grids) == 3
    want = [[list(b) for b in g.boxes] for g in grids[1:]]
    own = [G.regrid_owners(g.boxes, 2) for g in grids[1:]]
    for o in out:
        assert o["boxes"] == want
        assert o["owners"] == own
    assert out[0]["local"] != out[1]["local"]  # each rank holds its own share
    for l in range(2):
        assert sorted(out[0]["local"][l] + out[1]["local"][l]) == sorted(want[l])


def _run_tool(args, timeout):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_poisson.py")] + args,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = r.stdout.splitlines()
    levels = [x for x in lines if x.startswith("level ")]
    iters = [x for x in lines if x.startswith("Main Loop Iteration ")]
    tail = json.loads([x for x in lines if x.startswith("{")][-1])
    return levels, iters, tail


@pytest.mark.gpu
@pytest.mark.slow
def test_run_poisson_tool_max_level():
    # the user's entry: params.txt as it is (two black holes, max_depth -1) at
    # a 32^3 base, the hierarchy from set_grids, the NL loop to its end (six NL
    # iterations over 1 + 64 + 125 boxes: about 9 s of the test's 13 s)
    import re
    from mg_ic_code_amd.params import read_params_file
    prm = read_params_file(PARAMS)
    levels, iters, tail = _run_tool(["--size", "32", "--max-level", "2"], 120)
    assert len(levels) == 3, levels
    got = [re.fullmatch(r"level (\d+): (\d+) boxes, (\d+) cells", x) for x in levels]
    assert all(got), levels
    assert [int(m.group(1)) for m in got] == [0, 1, 2]
    assert (int(got[0].group(2)), int(got[0].group(3))) == (1, 32 ** 3)
    for m in got[1:]:
        nb, nc = int(m.group(2)), int(m.group(3))
        assert nb >= 1 and nc % 8 ** 3 == 0 and nc <= nb * 16 ** 3  # block_factor 8, max_grid_size 16
    assert 1 <= len(iters) <= prm.max_NL_iterations
    assert tail["nl_iterations"] == len(iters)
    norms = [float(x.rsplit(" ", 1)[1]) for x in iters]
    assert all(np.isfinite(norms)) and norms[-1] < 1e-3 * norms[0], iters
    # the default invocation: one level, no level lines, the same line format
    levels0, iters0, tail0 = _run_tool(["--size", "32"], 120)
    assert levels0 == [] and 1 <= len(iters0) <= prm.max_NL_iterations
    assert tail0["boxes"] == 1 and tail0["nl_iterations"] == len(iters0)
