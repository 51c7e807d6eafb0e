"""Periodic-aware set_grids: tags and proper nesting through
the wrap of a periodic base.

CPU: the restatement tests/regrid_periodic_ref.py on the one-hole deck of
tests/test_regrid.py (the box counts DESIGN.md 3m quotes, the invariants of a
hierarchy nested through the wrap), csrc/regrid.cpp's periodic nesting through
the C ABI against it on synthetic tag lattices, the deck key, and the library
without a device.
GPU: libmgic_ptag.so's kernel against the restatement bit for bit, its launch
ledger, set_grids against the restatement, the hierarchy AMRSolver rejects
without the switch and builds with it, the reflux operator and the singular
periodic solve on the generated hierarchy, and tools/run_poisson.py
--regrid-periodic.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import regrid_periodic_ref as P
from tests import regrid_ref as R
from tests.test_regrid import (BF, FR, MGS, PARAMS, _centred_params, _nested,
                               _reference_hierarchy, _shape, _three_level_tags)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(np.float64).eps)
TORUS = (1, 1, 1)
FACE = "30.0"  # bh1_offset: the hole 20 from the x-hi face of the L = 100 box
_WRAP = {}


def _grids():
    from mg_ic_code_amd import grids
    return grids


def _wrapped(bh1_offset, n0, periodic=TORUS):
    """The restatement's wrapped hierarchy of the one-hole deck, computed once
    per case, shared, left unchanged."""
    key = (bh1_offset, n0, tuple(periodic))
    if key not in _WRAP:
        _WRAP[key] = P.set_grids_wrap(_centred_params(bh1_offset), n0, periodic)
    return _WRAP[key]


def _doms(n0, nlev):
    return [(0, 0, 0) + ((n0 << l) - 1,) * 3 for l in range(nlev)]


# ------------------------------------------------------------------ CPU
# (base, bh1_offset) -> boxes per level: clipped (today's), wrapped
TABLE = {(32, FACE): ([1, 18, 27], [1, 22, 27]),
         (16, FACE): ([1, 8, 18], [1, 8, 22]),
         (16, "28.0"): ([1, 8, 27], [1, 8, 36]),
         (16, "26.0"): ([1, 8, 27], [1, 8, 36]),
         (16, "0.0"): ([1, 8, 27], [1, 8, 27]),
         (32, "0.0"): ([1, 27, 27], [1, 27, 27])}
X_LO_BOXES = [(0, 16, 16, 7, 31, 31), (0, 32, 16, 7, 47, 31), (0, 16, 32, 7, 31, 47),
              (0, 32, 32, 7, 47, 47)]


@pytest.mark.parametrize("n0,off", sorted(TABLE))
def test_restatement_reproduces_the_table(n0, off):
    clip_counts, wrap_counts = TABLE[n0, off]
    clip = _reference_hierarchy(off, n0)["levels"]
    ref = _wrapped(off, n0)
    lv = ref["levels"]
    print(n0, off, "clipped", [len(b) for b in clip], "wrapped", [len(b) for b in lv],
          "margins", ref["margins"])
    assert [len(b) for b in clip] == clip_counts
    assert [len(b) for b in lv] == wrap_counts
    assert all(m > 1e-9 for m in ref["margins"].values())  # no cell on the tagging threshold
    assert _wrapped(off, n0, (1, 0, 0))["levels"] == lv  # the hole sits on an x face only
    if off == "0.0":
        assert lv == clip
    doms = _doms(n0, 3)
    for l in (1, 2):
        assert R.disjoint(lv[l])
        for b in lv[l]:
            assert all(doms[l][d] <= b[d] <= b[3 + d] <= doms[l][3 + d] for d in range(3))
            assert all(b[d] % BF == 0 and (b[3 + d] + 1) % BF == 0 for d in range(3))
            assert all(b[3 + d] - b[d] + 1 <= MGS for d in range(3))
    assert _nested(lv[2], lv[1], doms[2], radius=2, periodic=True)


def test_the_face_cases_of_the_restatement():
    # 32^3: today's hierarchy is not nested through the wrap even at radius 1,
    # the wrapped one is at the full radius
    dom2 = _doms(32, 3)[2]
    clip = _reference_hierarchy(FACE, 32)["levels"]
    assert not _nested(clip[2], clip[1], dom2, radius=1, periodic=True)
    lv = _wrapped(FACE, 32)["levels"]
    assert min(b[0] for b in lv[1]) == 0 and max(b[3] for b in lv[2]) == 127
    # 16^3: the four new level-2 boxes lie on the x-lo face, fine-fine
    # neighbours of x-hi boxes through the wrap
    clip = _reference_hierarchy(FACE, 16)["levels"]
    lv = _wrapped(FACE, 16)["levels"]
    assert sorted(set(lv[2]) - set(clip[2])) == sorted(X_LO_BOXES)
    assert set(clip[2]) <= set(lv[2])
    for b in X_LO_BOXES:
        assert any(f[3] == 63 and f[1] <= b[4] and b[1] <= f[4] and f[2] <= b[5] and b[2] <= f[5]
                   for f in lv[2])


def _face_tags():
    """_three_level_tags moved to the x-hi face of the 32^3 base (c = 4): the
    level-2 tags sit on the face, level 1's own tags do not reach x-lo, so only
    nesting through the wrap puts level-1 and level-2 boxes on the x-lo face."""
    c, tags = _three_level_tags()
    m0 = np.zeros((8, 8, 8), np.uint8)
    m0[3:5, 3:5, 6:8] = 1                  # x lattice [6, 7]: cells [24, 31]
    (_, m1), (_, m2) = tags[1], tags[2]
    lo1, lo2 = (10, 5, 5), (26, 13, 13)    # x lattice [14, 15] of 16, [30, 31] of 32
    assert m1[2:4, 2:4, 2:4].all() and m2[2:4, 2:4, 4:6].all()
    m1 = np.roll(m1, 2, axis=2)            # [2, 3] -> [4, 5]: lattice [14, 15]
    return c, [((0, 0, 0), m0), (lo1, m1), (lo2, m2)]


def test_regrid_levels_periodic_matches_restatement_on_the_nesting_wrap():
    G = _grids()
    c, tags = _face_tags()
    dom0 = (0, 0, 0, 31, 31, 31)
    doms = _doms(32, 4)
    for per in (TORUS, (1, 0, 0)):
        boxes, fin = G.regrid_levels(dom0, tags, BF, MGS, FR, periodic=per)
        ref, rfin = P.regrid_wrap(dom0, per, tags, BF, MGS, FR)
        assert boxes == ref and fin == rfin == 3
        assert max(b[3] for b in boxes[2]) == 255       # level 3 on the x-hi face
        assert min(b[0] for b in boxes[1]) == 0 and min(b[0] for b in boxes[0]) == 0
        for l in (1, 2, 3):
            bl = boxes[l - 1]
            assert bl and R.disjoint(bl)
            for b in bl:
                assert all(doms[l][d] <= b[d] <= b[3 + d] <= doms[l][3 + d] for d in range(3))
                assert all(b[d] % BF == 0 and (b[3 + d] + 1) % BF == 0 for d in range(3))
                assert all(b[3 + d] - b[d] + 1 <= MGS for d in range(3))
        assert _nested(boxes[1], boxes[0], doms[2], 2, periodic=True)
        assert _nested(boxes[2], boxes[1], doms[3], 2, periodic=True)
    # without the wrap the same tags are nested on the bounded domain only
    clip, _ = G.regrid_levels(dom0, tags, BF, MGS, FR)
    assert clip == R.regrid(dom0, tags, BF, MGS, FR)[0]
    assert _nested(clip[2], clip[1], doms[3], 2) and _nested(clip[1], clip[0], doms[2], 2)
    assert not _nested(clip[2], clip[1], doms[3], 2, periodic=True)
    assert not _nested(clip[1], clip[0], doms[2], 2, periodic=True)
    # a direction that is not flagged stays clipped
    y_only, _ = G.regrid_levels(dom0, tags, BF, MGS, FR, periodic=(0, 1, 0))
    assert y_only == clip


def test_regrid_levels_periodic_without_flags_is_regrid_levels():
    G = _grids()
    dom0 = (0, 0, 0, 31, 31, 31)
    m = np.zeros((8, 8, 8), np.uint8)
    m[0, 0, 0] = m[7, 7, 7] = 1
    cases = [_three_level_tags()[1], _face_tags()[1], [((0, 0, 0), m)],
             [((0, 0, 0), np.zeros((8, 8, 8), np.uint8))]]
    for tags in cases:
        want = G.regrid_levels(dom0, tags, BF, MGS, FR)
        assert G.regrid_levels(dom0, tags, BF, MGS, FR, periodic=(0, 0, 0)) == want
        assert P.regrid_wrap(dom0, (0, 0, 0), tags, BF, MGS, FR) == R.regrid(dom0, tags, BF, MGS, FR)
    # a nesting radius as wide as the domain fills the direction once
    tags = _face_tags()[1]
    wide = G.regrid_levels(dom0, tags, BF, MGS, FR, nesting_radius=40, periodic=TORUS)
    assert wide == P.regrid_wrap(dom0, TORUS, tags, BF, MGS, FR, nesting_radius=40)
    from mg_ic_code_amd import MgicError
    with pytest.raises(MgicError) as e:  # 30 is not a multiple of c = 4
        G.regrid_levels((0, 0, 0, 29, 29, 29), [((0, 0, 0), np.ones((2, 2, 2), np.uint8))], 8, 16,
                        0.5, periodic=TORUS)
    assert e.value.code == -1
    with pytest.raises(ValueError):
        G.regrid_levels(dom0, tags, BF, MGS, FR, periodic=(1, 1))


def test_tag_restatement_without_flags_is_regrid_refs():
    rng = np.random.default_rng(5)
    dom = (-8, -8, -8, 7, 7, 7)
    a = rng.uniform(0.0, 1.0, (16, 16, 16))
    for c, grow in ((1, 2), (4, 3), (4, 0)):
        lo, m = P.tag_lattice_wrap([a], [dom], dom, (0, 0, 0), 0.9, grow, c)
        rlo, rm = R.tag_lattice([a], [dom], dom, 0.9, grow, c)
        assert lo == rlo and np.array_equal(m, rm)


def test_deck_key_regrid_periodic():
    from mg_ic_code_amd.params import read_params
    G = _grids()
    with open(PARAMS) as f:
        txt = f.read()
    assert "regrid_periodic" not in txt
    assert read_params(txt).regrid_periodic == 0
    for v in (0, 1):
        assert read_params(txt + f"\nregrid_periodic = {v}\n").regrid_periodic == v
        assert read_params(txt, {"regrid_periodic": str(v)}).regrid_periodic == v
        assert G.resolve_periodic_regrid(None, read_params(txt, {"regrid_periodic": str(v)})) == bool(v)
    for bad in ("2", "-1"):
        with pytest.raises(ValueError, match="regrid_periodic must be 0 or 1"):
            read_params(txt + f"\nregrid_periodic = {bad}\n")
    prm = read_params(txt)
    assert G.resolve_periodic_regrid(True, prm) and not G.resolve_periodic_regrid(0, prm)
    for bad in ("yes", 2, 1.0):
        with pytest.raises(ValueError, match="regrid_periodic must be 0 or 1"):
            G.resolve_periodic_regrid(bad, prm)
        with pytest.raises(ValueError, match="regrid_periodic must be 0 or 1"):
            G.set_grids(None, prm, None, periodic_regrid=bad)


def test_ptag_library_loads_without_a_device_and_only_on_demand(tmp_path):
    out = tmp_path / "ptag.ledger"
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import mg_ic_code_amd as mg\n"
            "from mg_ic_code_amd import _lib, grids\n"
            "assert not _lib.ptag_loaded()\n"
            "d = grids.ptag_launch_ledger()\n"
            "assert _lib.ptag_loaded() and not _lib.zm_loaded() and not _lib.reflux_loaded()\n"
            "assert _lib.ptag_call('mgic_ptag_launch_ledger_dump', %r) == 0\n"
            "assert d == {'k_ptag_lattice': 0}, d\n"
            "assert not any('ptag' in n for n in mg.launch_ledger())\n"
            % (ROOT, str(out).encode()))
    env = dict(os.environ, MGIC_NO_TORCH_PRELOAD="1")
    env.pop("MGIC_LAUNCH_LEDGER", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(out) as f:
        assert f.read() == "k_ptag_lattice\t0\n"


def test_binding_covers_the_ptag_header():
    from mg_ic_code_amd import _lib
    with open(os.path.join(ROOT, "include", "mgic_ptag.h")) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    names = set(re.findall(r"MGIC_PTAG_API\s+[\w\s\*]+?\b(mgic_ptag_\w+)\s*\(", txt))
    assert len(names) == 4 and names == set(_lib.PTAG_SIGNATURES)


def test_no_kernel_of_the_ptag_library_is_launched_around_its_ledger():
    for name in ("ptag.hip", "ptag_capi.cpp", "ptag.hpp"):
        with open(os.path.join(ROOT, "mg_ic_code_amd", "csrc", name)) as f:
            txt = f.read()
        assert "<<<" not in txt and "asm" not in txt and "atomic" not in txt.lower(), name
    with open(os.path.join(ROOT, "mg_ic_code_amd", "csrc", "ptag.hip")) as f:
        assert f.read().count("ledger::launch<k_ptag_lattice>") == 1


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def comm():
    import mg_ic_code_amd as mg
    return mg.Comm()


TAG_VAL = 0.75
FLAGS = {"xyz": (1, 1, 1), "x": (1, 0, 0), "yz": (0, 1, 1)}


def _geometries():
    """name -> (domain, boxes, conds, grows): the shapes of the kernel cases.
    Every cond holds 0.25 where it is not tagged, one NaN and one -0.0."""
    out = {}
    # a 16^3 domain with a negative low corner (floor division), one box, a
    # single tagged cell in the domain's low corner: eight images on a torus;
    # grow 8 = n / 2 fills a periodic direction
    dom = (-8, -8, -8, 7, 7, 7)
    a = np.full((16, 16, 16), 0.25)
    a[0, 0, 0] = 2.0
    a[5, 6, 7], a[9, 3, 2] = np.nan, -0.0
    out["corner"] = (dom, [dom], [a], (0, 2, 3, 8))
    # tags on both faces of every direction at once, an interior one, values
    # on the threshold and just below it
    b = np.full((16, 16, 16), 0.25)
    for k, j, i in ((0, 3, 15), (15, 12, 0), (4, 0, 9), (11, 15, 6), (15, 15, 15), (0, 0, 15)):
        b[k, j, i] = -2.0
    b[8, 8, 8] = TAG_VAL
    b[2, 9, 4] = np.nextafter(TAG_VAL, 0.0)
    b[5, 6, 7], b[9, 3, 2] = np.nan, -0.0
    out["faces"] = (dom, [dom], [b], (0, 2, 3, 8))
    # exactly one lattice cell in x at c = 4 (n_x = 4); at c = 1 four
    thin = (0, 0, 0, 3, 15, 7)
    t = np.full((8, 16, 4), 0.25)
    t[0, 0, 0] = t[7, 15, 3] = t[3, 8, 1] = 1.0
    t[1, 1, 1], t[2, 2, 2] = np.nan, -0.0
    out["thin"] = (thin, [thin], [t], (0, 2, 3, 8))
    # a box 70 cells long in x in a 72-cell domain: two waves per row, tagged
    # runs across the wave boundary (lane 63 -> lane 0 of the next wave, which
    # has no lane before it), a whole tagged wave, both ends of the box
    long_dom = (0, 0, 0, 71, 7, 3)
    long_box = (0, 0, 0, 69, 7, 3)
    w = np.full((4, 8, 70), 0.25)
    w[1, 2, 60:68] = 1.0
    w[2, 5, 0:64] = -1.0
    w[0, 0, 63] = w[3, 7, 64] = 2.0
    w[3, 1, 0] = w[3, 1, 69] = TAG_VAL
    w[0, 4, 30], w[0, 4, 31] = np.nan, -0.0
    out["long"] = (long_dom, [long_box], [w], (0, 2, 3, 36))
    # three boxes of a 32^3 level: one on the x-lo face, one on the x-hi, y-hi
    # and z-hi faces, one that touches no face
    dom3 = (0, 0, 0, 31, 31, 31)
    boxes = [(0, 8, 8, 7, 15, 15), (24, 24, 24, 31, 31, 31), (12, 12, 12, 19, 19, 19)]
    conds = [np.full(_shape(q), 0.25) for q in boxes]
    conds[0][3, 4, 0] = 1.0          # on the x-lo face
    conds[0][0, 0, 7] = -1.0         # a box corner: grows into cells of no box
    conds[1][7, 7, 7] = -2.0         # the domain's high corner
    conds[1][0, 2, 7] = TAG_VAL      # on the x-hi face
    conds[2][4, 4, 4] = 5.0          # the interior box
    conds[2][1, 1, 1], conds[2][6, 6, 6] = np.nan, -0.0
    out["three"] = (dom3, boxes, conds, (0, 2, 3, 16))
    return out


def _ptag_case(comm, dom, boxes, periodic, conds, tag_val, grow, c, grid=None, field=None):
    import mg_ic_code_amd as mg
    G = _grids()
    if grid is None:
        grid = mg.Grid(comm, dom, boxes, 1.0, periodic=periodic, patches=boxes != [dom])
        field = mg.LevelData(grid)
        for k in range(grid.num_local):
            field.upload(k, conds[boxes.index(grid.local_box(k))])
    local = [grid.local_box(k) for k in range(grid.num_local)]
    before = G.ptag_launch_ledger()
    lo, mask = G.tag_lattice_periodic(field, tag_val, grow, c)
    after = G.ptag_launch_ledger()
    # the size query launches nothing; the call launches once, whatever the boxes
    assert after["k_ptag_lattice"] - before["k_ptag_lattice"] == 1, (before, after)
    rlo, rmask = P.tag_lattice_wrap([conds[boxes.index(q)] for q in local], local, dom, periodic,
                                    tag_val, grow, c, all_boxes=boxes)
    assert tuple(lo) == tuple(rlo)
    assert mask.shape == rmask.shape
    assert np.array_equal(mask, rmask), (periodic, grow, c, np.argwhere(mask != rmask)[:8], lo)
    for d in range(3):
        if periodic[d]:
            assert lo[d] * c == dom[d] and mask.shape[2 - d] * c == dom[3 + d] - dom[d] + 1
    return grid, field, lo, mask


def run_kernel_cases(comm, names=None, flags=None):
    """Every geometry x periodic flags x c in {1, 4} x its grows against the
    restatement, bit for bit; then every cell tagged (tag_val 0: -0.0 is, NaN
    is not).  Shared with tests/ptag_worker.py.  Returns the masks by case."""
    got = {}
    geo = _geometries()
    for name in names or sorted(geo):
        dom, boxes, conds, grows = geo[name]
        for fl in flags or sorted(FLAGS):
            per = FLAGS[fl]
            grid = field = None
            for c in (1, 4):
                for grow in grows:
                    grid, field, lo, mask = _ptag_case(comm, dom, boxes, per, conds, TAG_VAL, grow,
                                                       c, grid, field)
                    got[name, fl, c, grow] = (lo, mask)
                _, _, lo, mask = _ptag_case(comm, dom, boxes, per, conds, 0.0, 2, c, grid, field)
                got[name, fl, c, "all"] = (lo, mask)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("fl", sorted(FLAGS))
@pytest.mark.parametrize("name", sorted(_geometries()))
def test_ptag_kernel_bitwise(comm, name, fl):
    got = run_kernel_cases(comm, [name], [fl])
    per = FLAGS[fl]
    dom, boxes, conds, grows = _geometries()[name]
    for c in (1, 4):
        # grow = n / 2 fills every periodic direction: the mask does not vary along it
        lo, mask = got[name, fl, c, grows[-1]]
        assert mask.any()
        for d in range(3):
            if per[d]:
                assert np.array_equal(mask, np.broadcast_to(mask.max(axis=2 - d, keepdims=True),
                                                            mask.shape)), (c, d)
        lo0, mask0 = got[name, fl, c, 0]
        assert 0 < mask0.sum() <= mask.sum()
    if name == "corner":
        # the corner cell grown by 2: images at both ends of a periodic
        # direction, the low end alone of a clipped one
        for c, wrapped, clipped in ((4, (0, 3), (0,)), (1, (0, 1, 2, 14, 15), (0, 1, 2))):
            lo, mask = got[name, fl, c, 2]
            want = np.zeros_like(mask)
            ix = [wrapped if per[d] else clipped for d in range(3)]
            want[np.ix_(ix[2], ix[1], ix[0])] = 1
            assert np.array_equal(mask, want)
            if per == TORUS and c == 4:
                assert mask.sum() == 8  # eight images
        assert got[name, fl, 4, 8][1].all() == (per == TORUS)
    if name == "thin" and per[0]:
        assert got[name, fl, 4, 2][1].shape[2] == 1  # one lattice cell in x
    if name == "three":
        lo, mask = got[name, fl, 4, 2]
        # the x-lo tag (cell (0, 12, 11): lattice y, z in [2, 3]) reaches the
        # lattice's x-hi end (x = 7) through the wrap only
        far = mask[2 - lo[2]:4 - lo[2], 2 - lo[1]:4 - lo[1], 7 - lo[0]]
        assert far.size == 4 and bool(far.any()) == bool(per[0])


@pytest.mark.gpu
def test_ptag_ledger_in_a_fresh_process(tmp_path):
    # one worker runs the three-box and the one-box case (one launch per call
    # is asserted in it, as in every case above) and dumps the library's
    # ledger: exactly its instantiations, all launched
    out = tmp_path / "ptag.ledger"
    env = dict(os.environ)
    env.pop("MGIC_LAUNCH_LEDGER", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ptag_worker.py"), "kernel",
                        str(out)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    from mg_ic_code_amd.core import read_launch_ledger
    led = read_launch_ledger(str(out))
    assert set(led) == {"k_ptag_lattice"}
    calls = json.loads(r.stdout.strip().splitlines()[-1])["calls"]
    assert calls > 0 and led["k_ptag_lattice"] == calls


@pytest.mark.gpu
def test_switch_off_or_a_bounded_base_launches_and_loads_what_it_did(tmp_path):
    # in a fresh process: the switch off on a periodic base, and the switch on
    # on a base with no periodic direction, give set_grids' hierarchy without
    # it, with one k_tag_lattice launch per box and pass as before, and
    # libmgic_ptag.so is never loaded
    env = dict(os.environ)
    env.pop("MGIC_LAUNCH_LEDGER", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ptag_worker.py"), "off"],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    clip = [[list(b) for b in bs] for bs in _reference_hierarchy(FACE, 16)["levels"]]
    assert [len(b) for b in clip] == [1, 8, 18]
    for key in ("plain", "off_periodic", "on_bounded"):
        assert out[key]["boxes"] == clip, key
        # pass 1 tags the base; pass 2 the base and the level 1 of pass 1
        assert out[key]["k_tag_lattice"] == 1 + 1 + out["level1_after_pass1"], (key, out)
    assert out["level1_after_pass1"] >= 1
    assert out["ptag_loaded"] is False


def _device_hierarchy(comm, bh1_offset, n0, periodic, **kw):
    import mg_ic_code_amd as mg
    prm = _centred_params(bh1_offset)
    dom0 = (0, 0, 0, n0 - 1, n0 - 1, n0 - 1)
    base = mg.Grid(comm, dom0, [dom0], prm.L / n0, periodic=periodic)
    return prm, _grids().set_grids(comm, prm, base, max_level=2, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("n0", [16, 32])
def test_set_grids_periodic_matches_restatement(comm, n0):
    import dataclasses
    ref = _wrapped(FACE, n0)
    assert all(m > 1e-9 for m in ref["margins"].values()), ref["margins"]
    prm, grids = _device_hierarchy(comm, FACE, n0, TORUS, periodic_regrid=True)
    assert [g.boxes for g in grids] == ref["levels"]
    assert [len(g.boxes) for g in grids] == TABLE[n0, FACE][1]
    for l, g in enumerate(grids):
        n = n0 << l
        assert g.domain == (0, 0, 0, n - 1, n - 1, n - 1) and g.dx == prm.L / n
        assert tuple(g.periodic) == TORUS
    assert _nested(grids[2].boxes, grids[1].boxes, grids[2].domain, 2, periodic=True)
    if n0 == 16:
        # the deck's key is the keyword's default
        base = grids[0]
        on = dataclasses.replace(prm, regrid_periodic=1)
        assert [g.boxes for g in _grids().set_grids(comm, on, base, max_level=2)] == ref["levels"]
        off = _grids().set_grids(comm, on, base, max_level=2, periodic_regrid=False)
        assert [g.boxes for g in off] == _reference_hierarchy(FACE, 16)["levels"]


@pytest.mark.gpu
def test_set_grids_periodic_centred_is_set_grids(comm):
    _, want = _device_hierarchy(comm, "0.0", 16, TORUS)
    _, got = _device_hierarchy(comm, "0.0", 16, TORUS, periodic_regrid=True)
    assert [g.boxes for g in got] == [g.boxes for g in want] == _wrapped("0.0", 16)["levels"]
    _, x_only = _device_hierarchy(comm, FACE, 16, (1, 0, 0), periodic_regrid=True)
    assert [g.boxes for g in x_only] == _wrapped(FACE, 16, (1, 0, 0))["levels"]


def _amr_solver(grids):
    import mg_ic_code_amd as mg
    fields = [(g, mg.LevelData(g), mg.LevelData(g)) for g in grids]
    for _, a, b in fields:
        a.set_val(-1.0)
        b.set_val(1.0)
    return mg.AMRSolver(fields, mg.OperatorParams(alpha=1.0, beta=-1.0),
                        mg.SolverParams(max_depth=2, bottom_solver=0))


@pytest.mark.gpu
def test_periodic_base_with_a_hole_on_the_face_builds_only_with_the_switch(comm):
    # the hierarchy set_grids generates on the periodic 32^3 base without the
    # switch is the one CFLevel rejects; with it AMRSolver builds
    import mg_ic_code_amd as mg
    _, clipped = _device_hierarchy(comm, FACE, 32, TORUS)
    assert [len(g.boxes) for g in clipped] == TABLE[32, FACE][0]
    with pytest.raises(mg.MgicError, match="not properly nested"):
        _amr_solver(clipped)
    _, grids = _device_hierarchy(comm, FACE, 32, TORUS, periodic_regrid=True)
    assert _amr_solver(grids).num_levels == 3


@pytest.fixture(scope="module")
def generated(comm):
    """set_grids' hierarchy on the periodic 16^3 base with the hole on the
    x-hi face, as plain box lists"""
    _, grids = _device_hierarchy(comm, FACE, 16, TORUS, periodic_regrid=True)
    return [list(g.boxes) for g in grids]


@pytest.mark.gpu
def test_generated_hierarchy_with_reflux_operator_and_conservation(comm, generated):
    from tests import test_reflux as TR
    assert [len(b) for b in generated] == [1, 8, 22]
    lo = [b for b in generated[2] if b[0] == 0]
    hi = [b for b in generated[2] if b[3] == 63]
    assert lo and hi and all(any(f[1] <= b[4] and b[1] <= f[4] and f[2] <= b[5] and b[2] <= f[5]
                                 for f in hi) for b in lo)  # neighbours through the wrap
    rng = np.random.default_rng(20261021)
    lv = TR._data(rng, generated)
    dev, o = TR.Dev(comm, lv, TORUS, TR.TORUS_DX0), TR._oracle(lv, TORUS, TR.TORUS_DX0)
    xs = TR._random_ml(rng, o)
    fx, fl = dev.field(xs), dev.field()
    dev.amr.applyOp(fl, fx, True)
    want = o.apply_op([x.copy() for x in xs], True)
    for i, got in enumerate(dev.down_all(fl)):
        assert TR._same_bits(got, want[i][1:-1, 1:-1, 1:-1]), ("applyOp", i)
    # conservation needs the pure divergence form: a = 0
    lv0 = TR._data(rng, generated, bvar=False, azero=True)
    dev0, o0 = TR.Dev(comm, lv0, TORUS, TR.TORUS_DX0), TR._oracle(lv0, TORUS, TR.TORUS_DX0)
    fx, fl = dev0.field(xs), dev0.field()
    dev0.amr.applyOp(fl, fx, True)
    total = abs(dev0.amr.computeSum(fl))
    bound = o0.num_uncovered() * EPS * dev0.amr.norm(fl, 1)  # N eps sum_l dx_l^3 sum |L phi|
    print("generated hierarchy: |composite sum| %.3e, bound %.3e" % (total, bound))
    assert total <= bound


@pytest.mark.gpu
def test_generated_hierarchy_singular_periodic_solve(comm, generated):
    # tests/test_reflux.py's singular solve (a = 0, b = 1, the composite mean
    # of the right-hand side removed) on the generated hierarchy
    import mg_ic_code_amd as mg
    from tests import test_reflux as TR
    rng = np.random.default_rng(3)
    lv = TR._data(rng, generated, bvar=False, azero=True)
    o = TR._oracle(lv, TORUS, TR.TORUS_DX0)
    f = TR._zero_mean_rhs(o, TR._random_ml(rng, o))
    phis = o.zeros_ml()
    it_o, nrm_o = o.solve(phis, [x.copy() for x in f], num_mg_iterations=1, imax=30, eps=1e-9)
    dev = TR.Dev(comm, lv, TORUS, TR.TORUS_DX0)
    frhs = dev.field(f)
    solver = mg.BiCGStabSolver(mg.MultilevelLinearOp(dev.amr, 1), tolerance=1e-9,
                               max_iterations=30, norm_type=0)
    it = solver.solve(dev.phi, frhs)
    got = dev.down_all(dev.phi)
    num = np.sqrt(sum(np.sum((g - w[1:-1, 1:-1, 1:-1]) ** 2) for g, w in zip(got, phis)))
    den = np.sqrt(sum(np.sum(w[1:-1, 1:-1, 1:-1] ** 2) for w in phis))
    r0 = max(np.abs(x).max() for x in f)
    print("singular solve on the generated hierarchy: iterations", it, "restatement", it_o,
          "norm", solver.final_norm, nrm_o, "of", r0, "rel-L2", num / den)
    assert it == it_o
    assert num <= 1e-10 * den
    assert solver.final_norm <= 1e-9 * r0 and nrm_o <= 1e-9 * r0


@pytest.mark.gpu
def test_run_poisson_cli_regrid_periodic(comm, tmp_path):
    with open(PARAMS) as f:
        txt = f.read()
    for old, new in (("max_NL_iterations = 6", "max_NL_iterations = 1"),
                     ("is_periodic = 0", "is_periodic = 1"),
                     ("bh1_offset = 10.0", "bh1_offset = 30.0"),
                     ("bh2_bare_mass = 0.5", "bh2_bare_mass = 0.0"),
                     ("bh2_spin = 0.1", "bh2_spin = 0.0"),
                     ("bh2_momentum = -0.05", "bh2_momentum = 0.0")):
        assert txt.count(old) == 1, old
        txt = txt.replace(old, new)
    deck = tmp_path / "periodic.txt"
    deck.write_text(txt)
    _, grids = _device_hierarchy(comm, FACE, 16, TORUS, periodic_regrid=True)
    want = ["level %d: %d boxes, %d cells" % (l, len(g.boxes), sum(R.box_cells(b) for b in g.boxes))
            for l, g in enumerate(grids)]
    tool = os.path.join(ROOT, "tools", "run_poisson.py")
    args = [sys.executable, tool, str(deck), "--size", "16", "--max-level", "2", "--max-depth", "2"]
    r = subprocess.run(args + ["--regrid-periodic"], capture_output=True, text=True, timeout=300,
                       cwd=str(tmp_path))
    # the hierarchy is what is checked: the NL loop on a periodic deck with a
    # puncture on the face is not claimed to converge, and the
    # tool ends with NLDivergenceError when the one iteration it gets does not
    assert r.returncode == 0 or "NLDivergenceError" in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    assert [x for x in r.stdout.splitlines() if x.startswith("level ")] == want
    assert [x.split(",")[0] for x in want] == ["level 0: 1 boxes", "level 1: 8 boxes",
                                               "level 2: 22 boxes"]
