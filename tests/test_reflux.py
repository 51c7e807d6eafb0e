"""Reflux at coarse-fine faces: the numpy restatement
tests/reflux_ref.py on the CPU (conservation, independence of covered cells,
the singular periodic solve), and the device against it bit for bit -- the
primitive mgic_amr_reflux, the multilevel paths of AMRSolver(reflux=True),
conservation from computeSum, the multilevel BiCGStab, libmgic_reflux.so's
launch ledger, and the switch left off.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle.amr import MultiBoxAMROracle
from tests.reflux_ref import RefluxOracle
from tests.test_amr_multibox import (BASE, BC, DOM0, DX0, HIER, HIER_DIAG, HIER_PER, PERIODIC, _Dev,
                                     _flat, _nested, _shape)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(np.float64).eps)

# the fully periodic hierarchy: level 1 nested through the wrap in x, y and z,
# level 2 on the periodic x-lo face
TORUS = (1, 1, 1)
HIER_TORUS = [[DOM0],
              [(0, 8, 8, 15, 23, 15), (0, 8, 16, 7, 23, 23), (24, 8, 8, 31, 23, 23),
               (8, 0, 24, 15, 7, 31), (8, 24, 24, 15, 31, 31)],
              [(0, 18, 18, 21, 45, 29), (0, 18, 30, 13, 33, 45)]]
TORUS_DX0 = 1.0 / 16
# two fine boxes one coarse cell apart in x: the cells of the gap take terms
# from both sides
HIER_GAP = [[DOM0], [(4, 4, 8, 13, 13, 23), (16, 4, 8, 27, 13, 23)]]
# one box per level, as many levels as HIER
HIER_ONE = [[DOM0], [(8, 8, 8, 23, 23, 23)], [(20, 20, 20, 43, 43, 43)]]

CASES = {"lshape": (HIER, (0, 0, 0), DX0), "diagonal": (HIER_DIAG, (0, 0, 0), DX0),
         "periodic": (HIER_PER, PERIODIC, DX0), "torus": (HIER_TORUS, TORUS, TORUS_DX0),
         "gap": (HIER_GAP, (0, 0, 0), DX0)}


def _data(rng, hier, bvar=True, azero=False):
    out = []
    for boxes in hier:
        ss = [_shape(b) for b in boxes]
        out.append(dict(boxes=list(boxes),
                        a=[np.zeros(s) if azero else rng.uniform(-2.0, -0.5, s) for s in ss],
                        b=[rng.uniform(0.5, 2.0, s) if bvar else np.ones(s) for s in ss],
                        rhs=[rng.uniform(-1, 1, s) for s in ss]))
    return out


def _oracle(lv, periodic, dx0, reflux=True, **kw):
    return RefluxOracle(lv, dx0, DOM0, alpha=1.0, beta=-1.0, **BC, base=BASE, periodic=periodic,
                        reflux=reflux, **kw)


def _random_ml(rng, o):
    return [b.full(rng.uniform(-1, 1, b.shape)) for bs in o.B for b in bs]


def _same_bits(a, b):
    """bit for bit (-0.0 is not 0.0), NaN where NaN"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape:
        return False
    same = a.view(np.uint64) == b.view(np.uint64)
    return bool(np.all(same | (np.isnan(a) & np.isnan(b))))


def _torus(reflux, cycle=True, seed=1):
    rng = np.random.default_rng(seed)
    lv = _data(rng, HIER_TORUS, bvar=False, azero=True)
    o = _oracle(lv, TORUS, TORUS_DX0, reflux=reflux, reflux_cycle=cycle)
    return rng, lv, o


def _zero_mean_rhs(o, f):
    """f with its composite mean removed on the valid cells of every level,
    covered cells zeroed (the right-hand side of the singular solve)"""
    ones = [b.full(np.ones(b.shape)) for bs in o.B for b in bs]
    m = o.composite_sum(f) / o.composite_sum(ones)
    out = [x.copy() for x in f]
    for x in out:
        x[1:-1, 1:-1, 1:-1] = x[1:-1, 1:-1, 1:-1] - m
    o.zero_covered(out)
    return out


# ------------------------------------------------------------------ CPU
def test_hierarchies_are_properly_nested():
    for name, (hier, per, _) in CASES.items():
        for l in range(1, len(hier)):
            assert _nested(hier[l], hier[l - 1], 16 << (l - 1), per), (name, l)
    for l in (1, 2):
        assert _nested(HIER_ONE[l], HIER_ONE[l - 1], 16 << (l - 1))
    # the gap: one coarse cell between the two boxes
    assert HIER_GAP[1][1][0] - HIER_GAP[1][0][3] - 1 == 2


def test_interface_cells_of_the_restatement():
    """cells with 1, 2 and more interface faces exist where the issue says:
    the gap's cells see both boxes, the L shape has concave corners"""
    rng = np.random.default_rng(2)
    o = _oracle(_data(rng, HIER_GAP), (0, 0, 0), DX0)
    m = o.interface_mask(0)
    both = m[0] & m[1]  # x-lo and x-hi neighbour covered: the gap
    assert both.sum() == 5 * 8 and set(np.nonzero(both)[2]) == {7}
    o = _oracle(_data(rng, HIER), (0, 0, 0), DX0)
    for l in (0, 1):
        faces = sum(x.astype(int) for x in o.interface_mask(l))
        assert faces.max() >= 2 and (faces == 1).any()
    # never across a non-periodic domain face, through the wrap where periodic
    o = _oracle(_data(rng, HIER_PER), PERIODIC, DX0)
    m = o.interface_mask(1)
    assert not m[2][:, 0, :].any() and not m[3][:, -1, :].any()
    o = _oracle(_data(rng, HIER_TORUS, azero=True), TORUS, TORUS_DX0)
    m = o.interface_mask(0)
    assert m[4][0].any() or m[5][-1].any() or m[2][:, 0].any() or m[3][:, -1].any()


def test_conservation_of_the_restatement():
    """the composite sum of apply_op(x) vanishes to the summation bound with
    the term, and is far from it without (the issue: 4.6e-15 against 1.2)"""
    rng, _, o = _torus(True)
    xs = _random_ml(rng, o)
    got = {}
    for on in (False, True):
        o = _torus(on)[2]
        out = o.apply_op([x.copy() for x in xs])
        bound = o.num_uncovered() * EPS * o.composite_sum(out, absolute=True)
        got[on] = (abs(o.composite_sum(out)), bound)
    print("conservation: |sum| with the term %.3e (bound %.3e), without %.3e"
          % (got[True][0], got[True][1], got[False][0]))
    assert got[True][0] <= got[True][1]
    assert got[False][0] > 1e6 * got[False][1]


def _overwrite_covered(o, rng, xs, levels, amp):
    ys = [x.copy() for x in xs]
    for l in levels:  # the cells of level l - 1 that level l covers
        o.put_covered(l, [y[1:-1, 1:-1, 1:-1] for y in o.lv(ys, l - 1)],
                      [rng.uniform(-amp, amp, _shape(c)) for c in o.cov(l)])
    assert any(not np.array_equal(x, y) for x, y in zip(xs, ys))
    return ys


def test_covered_cells_do_not_matter():
    """x's covered cells overwritten with random values on every level: the
    result's uncovered cells keep their bits.  With the switch on the operator
    first writes the finer level's average into the covered cells of its
    input, so it reads uncovered data alone.  (The additive term by itself
    would not give this: a covered value cancels between the stencil and G_c
    only up to rounding, 8 eps max|x| / dx^2 measured, and QuadCFInterp's
    second fine cell behind a face may be one the next level covers.)
    Without the switch the covered values show at full size."""
    rng, _, o = _torus(True)
    xs = _random_ml(rng, o)
    want = o.masked(o.apply_op([x.copy() for x in xs]))
    for amp in (1.0, 50.0):
        got = o.masked(o.apply_op(_overwrite_covered(o, rng, xs, (1, 2), amp)))
        for i, (w, g) in enumerate(zip(want, got)):
            assert _same_bits(w[1:-1, 1:-1, 1:-1], g[1:-1, 1:-1, 1:-1]), (amp, i)
    off = _torus(False)[2]
    a = off.masked(off.apply_op([x.copy() for x in xs]))[0]
    b = off.masked(off.apply_op(_overwrite_covered(off, rng, xs, (1, 2), 1.0)))[0]
    assert float(np.abs(a - b).max()) > 1.0  # about max|x| / dx^2 = 256


@pytest.fixture(scope="module")
def singular_ref():
    """the singular periodic solve of the restatement with the term (in the
    operator, the residuals and the downsweep): (lv, rhs, phi, iterations, norm)"""
    rng, lv, o = _torus(True, seed=3)
    f = _zero_mean_rhs(o, _random_ml(rng, o))
    phis = o.zeros_ml()
    it, nrm = o.solve(phis, [x.copy() for x in f], num_mg_iterations=1, imax=30, eps=1e-9)
    return lv, f, phis, it, nrm


def test_singular_solve_of_the_restatement(singular_ref):
    _, f, _, it, nrm = singular_ref
    r0 = max(np.abs(x).max() for x in f)
    print("singular solve with the term: iterations", it, "norm", nrm, "of", r0)
    assert it <= 10 and nrm <= 1e-9 * r0  # r0: the loop's initial norm, max|f| (phi = 0)
    o = _torus(False, seed=3)[2]
    it0, nrm0 = o.solve(o.zeros_ml(), [x.copy() for x in f], num_mg_iterations=1, imax=30, eps=1e-9)
    print("without: iterations", it0, "norm", nrm0)
    assert it0 == 30 and nrm0 > 1e-9 * r0


def test_switch_off_is_the_unchanged_restatement():
    rng = np.random.default_rng(4)
    lv = _data(rng, HIER)
    off = _oracle(lv, (0, 0, 0), DX0, reflux=False)
    base = MultiBoxAMROracle(lv, DX0, DOM0, alpha=1.0, beta=-1.0, **BC, base=BASE)
    xs = _random_ml(rng, off)
    for a, b in zip(off.apply_op([x.copy() for x in xs]), base.apply_op([x.copy() for x in xs])):
        assert _same_bits(a, b)
    r = off.residual_ml(off.zeros_ml(), off.full_ml(_flat(lv, "rhs")))
    for a, b in zip(off.precondition(r, 2), base.precondition(r, 2)):
        assert _same_bits(a, b)


def test_reflux_library_loads_without_a_device_and_only_on_demand(tmp_path):
    out = tmp_path / "reflux.ledger"
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import mg_ic_code_amd as mg\n"
            "from mg_ic_code_amd import _lib\n"
            "assert not _lib.reflux_loaded()\n"
            "assert _lib.reflux_call('mgic_reflux_launch_ledger_dump', %r) == 0\n"
            "assert _lib.reflux_loaded() and not _lib.zm_loaded() and not _lib.ctt_loaded()\n"
            "assert not any('reflux' in n for n in mg.launch_ledger())\n"
            % (ROOT, str(out).encode()))
    env = dict(os.environ, MGIC_NO_TORCH_PRELOAD="1")
    env.pop("MGIC_LAUNCH_LEDGER", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(out) as f:
        assert f.read() == "k_reflux<false>\t0\nk_reflux<true>\t0\n"


def test_binding_covers_the_reflux_header():
    from mg_ic_code_amd import _lib
    with open(os.path.join(ROOT, "include", "mgic_reflux.h")) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    names = set(re.findall(r"MGIC_REFLUX_API\s+[\w\s\*]+?\b(mgic_reflux_\w+)\s*\(", txt))
    assert len(names) == 4 and names == set(_lib.REFLUX_SIGNATURES)


def test_no_kernel_of_the_reflux_library_is_launched_around_its_ledger():
    for name in ("reflux.hip", "reflux_capi.cpp", "reflux.hpp"):
        with open(os.path.join(ROOT, "mg_ic_code_amd", "csrc", name)) as f:
            assert "<<<" not in f.read(), name
    with open(os.path.join(ROOT, "mg_ic_code_amd", "csrc", "reflux.hip")) as f:
        assert f.read().count("ledger::launch<k_reflux<") == 2


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def comm():
    import mg_ic_code_amd as mg
    return mg.Comm()


class Dev(_Dev):
    """tests/test_amr_multibox.py's device hierarchy with the level spacing
    and the reflux switch as arguments"""

    def __init__(self, comm, lv, periodic=(0, 0, 0), dx0=DX0, reflux=True):
        import mg_ic_code_amd as mg
        self.mg = mg
        self.grids, self.order = [], []
        dom, dx = DOM0, dx0
        for l, x in enumerate(lv):
            grid = mg.Grid(comm, dom, x["boxes"], dx, periodic=periodic, patches=l > 0)
            self.order.append([x["boxes"].index(grid.local_box(k))
                               for k in range(grid.num_local)])
            self.grids.append(grid)
            dom = tuple(2 * v if i < 3 else 2 * v + 1 for i, v in enumerate(dom))
            dx /= 2
        self.a = self.field(_flat(lv, "a"))
        self.b = self.field(_flat(lv, "b"))
        self.rhs = self.field(_flat(lv, "rhs"))
        self.phi = self.field()
        op = mg.OperatorParams(alpha=1.0, beta=-1.0, coefficient_average_type=1, prolong_type=1,
                               **BC)
        kw = {} if reflux is None else dict(reflux=reflux)
        self.amr = mg.AMRSolver(list(zip(self.grids, self.a, self.b)), op,
                                mg.SolverParams(max_depth=2, bottom_solver=0), **kw)

    def up_full(self, f, l, arrs):
        for k, i in enumerate(self.order[l]):
            f.upload(k, arrs[i], with_ghosts=True)


def reflux_ledger():
    from mg_ic_code_amd import _lib
    from mg_ic_code_amd.core import read_launch_ledger
    import tempfile
    fd, path = tempfile.mkstemp(prefix="mgic_reflux_ledger_")
    os.close(fd)
    try:
        _lib.reflux_call("mgic_reflux_launch_ledger_dump", path.encode())
        return read_launch_ledger(path)
    finally:
        os.unlink(path)


def run_primitive_case(comm, case, bvar):
    """mgic_amr_reflux on every level with a finer one: an operator's sign
    with the coarse field, a residual's with it and with none, on a target
    that holds -0.0 and a NaN; every cell and every ghost of the target
    against the restatement.  Returns the number of cells the term changed."""
    hier, per, dx0 = CASES[case]
    rng = np.random.default_rng(41)
    lv = _data(rng, hier, bvar)
    dev, o = Dev(comm, lv, per, dx0), _oracle(lv, per, dx0)
    us = _random_ml(rng, o)
    fu, scratch = dev.field(us), dev.field()
    changed = 0
    for l in range(len(hier) - 1):
        # the ghosts the term reads: AMROperator's on both levels
        for m in (l, l + 1):
            dev.amr.AMROperator(m, scratch[m], fu[m], fu[m - 1] if m else None, False)
            o.fill(m, o.lv(us, m), o.lv(us, m - 1) if m else None, False)
        masks = o.interface_mask(l)
        for with_c, sign in ((True, 1), (True, -1), (False, -1)):
            tg = [rng.uniform(-1, 1, tuple(s + 2 for s in b.shape)) for b in o.B[l]]
            for t in tg:
                t[1:3, 1:-1, 1:-1] = -0.0
                t[3, 2, 2] = np.nan
            ft = dev.mg.LevelData(dev.grids[l])
            dev.up_full(ft, l, tg)
            dev.amr.reflux(l, ft, fu[l] if with_c else None, fu[l + 1], sign)
            want = [t.copy() for t in tg]
            o.reflux(l, [w[1:-1, 1:-1, 1:-1] for w in want], o.lv(us, l) if with_c else None,
                     o.lv(us, l + 1), sign)
            got = dev.down(ft, l, True)
            for i, (bx, g, w, t) in enumerate(zip(o.B[l], got, want, tg)):
                assert _same_bits(g, w), (case, bvar, l, with_c, sign, i)
                here = tuple(slice(bx.box[d] - o.dom[l][d], bx.box[3 + d] - o.dom[l][d] + 1)
                             for d in (2, 1, 0))
                face = np.zeros(bx.shape, bool)
                for m in masks:
                    face |= m[here]
                diff = g.view(np.uint64) != t.view(np.uint64)
                assert not diff[1:-1, 1:-1, 1:-1][~face].any()  # no interface face: its bits
                inner = np.zeros(diff.shape, bool)
                inner[1:-1, 1:-1, 1:-1] = True
                assert not diff[~inner].any()  # every ghost: its bits
                changed += int(diff.sum())
    return changed


@pytest.mark.gpu
@pytest.mark.parametrize("bvar", [False, True], ids=["bconst", "bvar"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_primitive_bitwise(comm, case, bvar):
    before = reflux_ledger()
    assert run_primitive_case(comm, case, bvar) > 100
    after = reflux_ledger()
    levels = len(CASES[case][0]) - 1
    assert after["k_reflux<true>"] - before["k_reflux<true>"] == 2 * levels
    assert after["k_reflux<false>"] - before["k_reflux<false>"] == levels


MULTI = {"lshape": (HIER, (0, 0, 0), DX0), "torus": (HIER_TORUS, TORUS, TORUS_DX0)}


def _run_multilevel(dev, o, lv, rng):
    """applyOp, initResidual + three iterations, precondition(2): the device
    against the restatement, bit for bit"""
    amr = dev.amr
    xs = _random_ml(rng, o)
    fx, fl = dev.field(xs), dev.field()
    amr.applyOp(fl, fx, True)
    want = o.apply_op([x.copy() for x in xs], True)
    for i, got in enumerate(dev.down_all(fl)):
        assert _same_bits(got, want[i][1:-1, 1:-1, 1:-1]), ("applyOp", i)
    # the solve's own residual, both BCs, on a phi whose covered cells are random
    frhs = dev.field(o.full_ml(_flat(lv, "rhs")))
    for hom in (False, True):
        fx2, fr2 = dev.field(xs), dev.field()
        amr.residual(fr2, fx2, frhs, hom)
        want = o.residual_ml([x.copy() for x in xs], o.full_ml(_flat(lv, "rhs")), hom)
        for i, got in enumerate(dev.down_all(fr2)):
            assert _same_bits(got, want[i][1:-1, 1:-1, 1:-1]), ("residual", hom, i)
    res = o.init_residual(o.zeros_ml(), _flat(lv, "rhs"))
    g = dev.amr.init_residual(dev.phi, dev.rhs, 0)
    assert g == max(np.abs(r).max() for r in res)
    for l in range(len(o.B)):
        for i, (got, w) in enumerate(zip(dev.down(amr.residual_field(l), l), o.lv(res, l))):
            assert _same_bits(got, w), ("initResidual", l, i)
    for _ in range(3):
        g = dev.amr.iteration(dev.phi, dev.rhs, 0)
        assert g == max(np.abs(r).max() for r in o.iteration())
    for l in range(len(o.B)):
        for i, (got, w) in enumerate(zip(dev.down(dev.phi[l], l), o.lv(o.phis, l))):
            assert _same_bits(got, w[1:-1, 1:-1, 1:-1]), ("iteration", l, i)
    r = o.residual_ml(o.zeros_ml(), o.full_ml(_flat(lv, "rhs")))
    fr, fe = dev.field(r), dev.field()
    amr.precondition(fe, fr, 2)
    e = o.precondition(r, 2)
    for i, got in enumerate(dev.down_all(fe)):
        assert _same_bits(got, e[i][1:-1, 1:-1, 1:-1]), ("precondition", i)
    return fl, want


@pytest.mark.gpu
@pytest.mark.parametrize("bvar", [False, True], ids=["bconst", "bvar"])
@pytest.mark.parametrize("case", sorted(MULTI))
def test_multilevel_paths_bitwise(comm, case, bvar):
    hier, per, dx0 = MULTI[case]
    rng = np.random.default_rng(42)
    lv = _data(rng, hier, bvar)
    dev, o = Dev(comm, lv, per, dx0), _oracle(lv, per, dx0)
    before = reflux_ledger()
    _run_multilevel(dev, o, lv, rng)
    after = reflux_ledger()
    assert after["k_reflux<true>"] > before["k_reflux<true>"]
    assert after["k_reflux<false>"] > before["k_reflux<false>"]  # the downsweep's


@pytest.mark.gpu
def test_conservation_on_the_device(comm):
    rng, lv, o = _torus(True)
    dev = Dev(comm, lv, TORUS, TORUS_DX0)
    off = Dev(comm, lv, TORUS, TORUS_DX0, reflux=False)
    xs = _random_ml(rng, o)
    got = {}
    for name, d in (("on", dev), ("off", off)):
        fx, fl = d.field(xs), d.field()
        d.amr.applyOp(fl, fx, True)
        bound = o.num_uncovered() * EPS * d.amr.norm(fl, 1)  # sum_l dx_l^3 sum |L phi|
        got[name] = (abs(d.amr.computeSum(fl)), bound)
    print("device conservation: |sum| with the term %.3e (bound %.3e), without %.3e"
          % (got["on"][0], got["on"][1], got["off"][0]))
    assert got["on"][0] <= got["on"][1]
    assert got["off"][0] > 1e6 * got["off"][1]


@pytest.mark.gpu
def test_covered_cells_do_not_matter_on_the_device(comm):
    rng, lv, o = _torus(True)
    dev = Dev(comm, lv, TORUS, TORUS_DX0)
    xs = _random_ml(rng, o)
    ys = _overwrite_covered(o, rng, xs, (1, 2), 50.0)
    out = []
    for v in (xs, ys):
        fx, fl = dev.field(v), dev.field()
        dev.amr.applyOp(fl, fx, True)
        out.append(dev.down_all(fl))
        # the input's covered cells now hold the finer level's average
        w = [x.copy() for x in v]
        o.average_covered(w)
        for got, want in zip(dev.down_all(fx), w):
            assert _same_bits(got, want[1:-1, 1:-1, 1:-1])
    assert all(_same_bits(a, b) for a, b in zip(*out))


@pytest.mark.gpu
def test_multilevel_bicgstab_on_the_singular_periodic_case(comm, singular_ref):
    import mg_ic_code_amd as mg
    lv, f, phis, it_o, nrm_o = singular_ref
    dev = Dev(comm, lv, TORUS, TORUS_DX0)
    frhs = dev.field(f)
    solver = mg.BiCGStabSolver(mg.MultilevelLinearOp(dev.amr, 1), tolerance=1e-9,
                               max_iterations=30, norm_type=0)
    it = solver.solve(dev.phi, frhs)
    got = dev.down_all(dev.phi)
    num = np.sqrt(sum(np.sum((g - w[1:-1, 1:-1, 1:-1]) ** 2) for g, w in zip(got, phis)))
    den = np.sqrt(sum(np.sum(w[1:-1, 1:-1, 1:-1] ** 2) for w in phis))
    print("singular solve: iterations", it, "restatement", it_o, "norm", solver.final_norm, nrm_o,
          "rel-L2", num / den)
    assert it == it_o
    assert num <= 1e-10 * den
    r0 = max(np.abs(x).max() for x in f)
    assert solver.final_norm <= 1e-9 * r0 and nrm_o <= 1e-9 * r0


@pytest.mark.gpu
def test_launch_counts_do_not_depend_on_the_number_of_boxes(comm):
    counts = {}
    for name, hier in (("three", HIER), ("one", HIER_ONE)):
        rng = np.random.default_rng(43)
        lv = _data(rng, hier)
        dev, o = Dev(comm, lv), _oracle(lv, (0, 0, 0), DX0)
        assert [len(x["boxes"]) for x in lv] == ([1, 3, 3] if name == "three" else [1, 1, 1])
        before = reflux_ledger()
        xs = _random_ml(rng, o)
        fx, fl = dev.field(xs), dev.field()
        dev.amr.applyOp(fl, fx, True)
        dev.amr.init_residual(dev.phi, dev.rhs, 0)
        dev.amr.iteration(dev.phi, dev.rhs, 0)
        dev.amr.precondition(fl, dev.rhs, 2)
        after = reflux_ledger()
        counts[name] = {k: after[k] - before[k] for k in after}
    print("reflux launches:", counts)
    assert counts["three"] == counts["one"]
    # applyOp 2, initResidual 2 (twice), precondition's second residual 2; one
    # downsweep per finer level in each of the three V-cycles
    assert counts["one"] == {"k_reflux<true>": 8, "k_reflux<false>": 6}


def run_kernel_cases(comm):
    run_primitive_case(comm, "gap", True)
    return reflux_ledger()


@pytest.mark.gpu
def test_every_kernel_of_the_reflux_library_is_launched_against_its_reference(tmp_path):
    from mg_ic_code_amd.core import read_launch_ledger
    out = tmp_path / "reflux.ledger"
    env = dict(os.environ)
    env.pop("MGIC_LAUNCH_LEDGER", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "reflux_worker.py"), str(out)],
                       capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, f"{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    ledger = read_launch_ledger(out)
    assert sorted(ledger) == ["k_reflux<false>", "k_reflux<true>"], ledger
    missing = sorted(n for n, c in ledger.items() if c == 0)
    assert not missing, missing


OFF_LEDGER = os.path.join(ROOT, "tests", "golden", "reflux_off_ledger.json")


def off_solve(comm, how, levels=HIER):
    """The switch-off case: tests/test_amr_multibox.py's multilevel BiCGStab on
    HIER (its seed, its tolerance) after an initResidual and one AMR iteration,
    libmgic.so's ledger reset in front.  how: None -- the keyword left out,
    False -- reflux=False.  Returns (lv, dev, norms, iterations, final norm,
    phi per box, ledger)."""
    import mg_ic_code_amd as mg
    rng = np.random.default_rng(23)
    lv = _data(rng, levels, bvar=False)
    dev = Dev(comm, lv, reflux=how)
    mg.launch_ledger_reset()
    g = [dev.amr.init_residual(dev.phi, dev.rhs, 0), dev.amr.iteration(dev.phi, dev.rhs, 0)]
    cycle_phi = dev.down_all(dev.phi)
    solver = mg.BiCGStabSolver(mg.MultilevelLinearOp(dev.amr, 2), tolerance=1e-10,
                               max_iterations=20, norm_type=0)
    it = solver.solve(dev.phi, dev.rhs)
    return lv, dev, g, cycle_phi, it, solver.final_norm, dev.down_all(dev.phi), mg.launch_ledger()


def off_reference(lv):
    """the same on the unchanged oracle/amr.py::MultiBoxAMROracle"""
    o = MultiBoxAMROracle(lv, DX0, DOM0, alpha=1.0, beta=-1.0, **BC, base=BASE)
    g = [max(np.abs(r).max() for r in o.init_residual(o.zeros_ml(), _flat(lv, "rhs")))]
    g.append(max(np.abs(r).max() for r in o.iteration()))
    cycle_phi = [p.copy() for p in o.phis]
    phis = o.phis
    it, nrm = o.solve(phis, o.full_ml(_flat(lv, "rhs")), num_mg_iterations=2, imax=20, eps=1e-10)
    return g, cycle_phi, it, nrm, phis


@pytest.mark.gpu
def test_switch_off_changes_nothing_and_loads_nothing(comm, tmp_path):
    # in a fresh process, with the keyword left out and with reflux=False: the
    # V-cycle is the unchanged MultiBoxAMROracle's bit for bit, the multilevel
    # BiCGStab takes its iteration count and gives its phi (rel-L2 1e-10, as
    # tests/test_amr_multibox.py takes it), libmgic.so's ledger counts are the
    # ones recorded for this sequence on the tree before the switch existed
    # (tests/golden/reflux_off_ledger.json), libmgic_reflux.so is never loaded;
    # one level with reflux=True loads nothing either
    code = """
import json, sys
sys.path.insert(0, %r)
import numpy as np
import mg_ic_code_amd as mg
from mg_ic_code_amd import _lib
from tests import test_reflux as T
comm = mg.Comm()
with open(T.OFF_LEDGER) as f:
    recorded = json.load(f)
for how in (None, False):
    lv, dev, g, cycle_phi, it, nrm, phi, ledger = T.off_solve(comm, how)
    g_o, cycle_o, it_o, nrm_o, phi_o = T.off_reference(lv)
    assert g == g_o, (g, g_o)
    for got, want in zip(cycle_phi, cycle_o):
        assert T._same_bits(got, want[1:-1, 1:-1, 1:-1])
    assert it == it_o and it >= 1, (it, it_o)
    assert abs(nrm - nrm_o) <= 1e-6 * nrm_o + 1e-14, (nrm, nrm_o)
    num = np.sqrt(sum(np.sum((a - w[1:-1, 1:-1, 1:-1]) ** 2) for a, w in zip(phi, phi_o)))
    den = np.sqrt(sum(np.sum(w[1:-1, 1:-1, 1:-1] ** 2) for w in phi_o))
    assert num <= 1e-10 * den, num / den
    diff = {k: (ledger.get(k), recorded.get(k)) for k in set(ledger) | set(recorded)
            if ledger.get(k) != recorded.get(k)}
    assert not diff, diff
    assert sum(ledger.values()) > 0
    assert not _lib.reflux_loaded(), how
rng = np.random.default_rng(1)
one = T.Dev(comm, T._data(rng, [T.HIER[0]]), reflux=True)
assert not one.amr.reflux_on and not _lib.reflux_loaded()
print("ok", it)
""" % ROOT
    env = dict(os.environ)
    env.pop("MGIC_LAUNCH_LEDGER", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env,
                       timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().startswith("ok")


# ------------------------------------------- the solve's interfaces (CPU)
def test_deck_key_reflux():
    from mg_ic_code_amd.params import read_params
    from tests.test_phi_field import PARAMS
    with open(PARAMS) as f:
        txt = f.read()
    assert "reflux" not in txt
    assert read_params(txt).reflux == 0
    for v in (0, 1):
        assert read_params(txt + f"\nreflux = {v}\n").reflux == v
        assert read_params(txt, {"reflux": str(v)}).reflux == v
    for bad in ("2", "-1"):
        with pytest.raises(ValueError, match="reflux must be 0 or 1"):
            read_params(txt + f"\nreflux = {bad}\n")


def test_keyword_and_refusals_load_and_launch_nothing():
    import dataclasses

    import mg_ic_code_amd as mg
    from mg_ic_code_amd import Matter, PiProfile, _lib
    from mg_ic_code_amd.matter import ScalarPotential
    from mg_ic_code_amd.nl import poisson_solve
    from tests import test_momentum_periodic as TP
    prm = TP._prm(16)
    matter = Matter(ScalarPotential(), PiProfile.from_function(TP.PI_BAL))
    loaded = (_lib.ctt_loaded(), _lib.zm_loaded(), _lib.reflux_loaded())
    ledger = mg.launch_ledger()
    for bad in ("yes", 2, 1.0):
        with pytest.raises(ValueError, match="reflux must be 0 or 1"):
            poisson_solve(None, prm, matter=matter, reflux=bad)
    with pytest.raises(ValueError, match="reflux must be 0 or 1"):
        poisson_solve(None, dataclasses.replace(prm, reflux=3), matter=matter)
    # without reflux (the keyword, the deck's key, or neither) the periodic
    # hierarchy is refused with the message it had
    for kw, p in (({}, prm), ({"reflux": False}, prm), ({"reflux": 0}, prm),
                  ({}, dataclasses.replace(prm, reflux=0)),
                  ({"reflux": False}, dataclasses.replace(prm, reflux=1))):
        with pytest.raises(ValueError, match="periodic hierarchy.*no refluxing.*sum to zero"):
            poisson_solve([None, None], p, matter=matter, momentum=True, zero_mode="project", **kw)
    # with it the request passes that check (and fails on the grids it was not given)
    for kw, p in (({"reflux": True}, prm), ({}, dataclasses.replace(prm, reflux=1))):
        with pytest.raises(Exception) as e:
            poisson_solve([None, None], p, matter=matter, momentum=True, zero_mode="project", **kw)
        assert "no refluxing" not in str(e.value)
    # a periodic base without the projection is refused as before, reflux or not
    with pytest.raises(ValueError, match="periodic.*sum S_i = 0"):
        poisson_solve([None, None], prm, matter=matter, momentum=True, reflux=True)
    assert (_lib.ctt_loaded(), _lib.zm_loaded(), _lib.reflux_loaded()) == loaded
    assert mg.launch_ledger() == ledger


# ------------------------------------- the momentum step on a periodic hierarchy
E2E_BOXES = HIER_TORUS[:2]
_E2E = {}


def _e2e_cpu(on):
    """the restatement's coupled loop on the two-level periodic hierarchy,
    computed once, shared, left unchanged"""
    from tests import phi_ref
    from tests import reflux_ref
    from tests import test_momentum_periodic as TP
    if ("cpu", on) not in _E2E:
        _E2E["cpu", on] = reflux_ref.coupled_solve_amr(TP._prm(16), E2E_BOXES, 16, 2, phi_ref.sine,
                                                       TP.POT, TP.PI_BAL, momentum_on=on)
    return _E2E["cpu", on]


def _e2e_grids(comm, prm):
    import mg_ic_code_amd as mg
    g0 = mg.Grid(comm, DOM0, [DOM0], prm.domainLength[0] / 16, periodic=TORUS)
    dom1 = tuple(2 * v if i < 3 else 2 * v + 1 for i, v in enumerate(DOM0))
    g1 = mg.Grid(comm, dom1, E2E_BOXES[1], prm.domainLength[0] / 32, periodic=TORUS, patches=True)
    return [g0, g1]


def _e2e_gpu(comm, on, **kw):
    from mg_ic_code_amd import Matter, PiProfile
    from mg_ic_code_amd.matter import ScalarPotential
    from mg_ic_code_amd.nl import poisson_solve
    from mg_ic_code_amd.phi import PhiProfile
    from tests import test_momentum_periodic as TP
    prm = TP._prm(16)
    mkw = dict(momentum=True, zero_mode="project") if on else {}
    mkw.update(kw)
    return poisson_solve(_e2e_grids(comm, prm), prm, max_depth=2, phi0=PhiProfile.sine(),
                         matter=Matter(ScalarPotential(), PiProfile.from_function(TP.PI_BAL)),
                         constraints=True, **mkw)


@pytest.mark.gpu
def test_momentum_step_on_a_periodic_hierarchy_end_to_end(comm):
    from tests import test_momentum_periodic as TP
    prm = TP._prm(16)
    with pytest.raises(ValueError, match="periodic hierarchy.*no refluxing.*sum to zero"):
        _e2e_gpu(comm, True)
    off = _e2e_gpu(comm, False, reflux=True)
    on = _e2e_gpu(comm, True, reflux=True)
    cpu_off, cpu_on = _e2e_cpu(False), _e2e_cpu(True)
    mom_off = TP._mom(off.constraints)
    mom_on = TP._mom(on.constraints, "max_norm_net")
    print("device: |dpsi|", on.dpsi_norms, "momentum iterations", on.momentum_iterations)
    print("momentum_net device", on.momentum_net, "restatement", cpu_on["nets"])
    print("max|Mom_i| without the step: device", mom_off, "restatement", cpu_off["mom"])
    print("max|Mom_i + m psi^-6| with it: device", mom_on, "restatement", cpu_on["mom_net"])
    print("max|Mom_i| with it: device", TP._mom(on.constraints), "restatement", cpu_on["mom"])
    TP._assert_converged(on.dpsi_norms)
    TP._assert_converged(off.dpsi_norms)
    assert all(len(its) == 4 and max(its) < prm.max_iterations for its in on.momentum_iterations)
    # every momentum solve reached the tolerance: its final residual against
    # tolerance * max|rhs| (the loop's own bar from a zero guess, and no weaker
    # from a warm one, whose first residual is smaller), or BiCGStab's absolute
    # floor reps = 1e-12 where the warm guess was already there
    print("momentum solves (final norm, max|rhs|):", on.momentum_residuals)
    assert len(on.momentum_residuals) == len(on.momentum_iterations)
    for per_it in on.momentum_residuals:
        assert len(per_it) == 4
        for final, rhs_max in per_it:
            assert rhs_max > 0.0 and final <= max(prm.tolerance * rhs_max, 1e-12), (final, rhs_max)
    assert len(on.momentum_net) == len(on.dpsi_norms) == len(cpu_on["nets"])
    smax = max(mom_off)  # the size of S_i at psi = 1, where the sums are taken
    floor = TP.mean_order_bound(RefluxOracle.num_uncovered(
        _oracle(_data(np.random.default_rng(0), E2E_BOXES), TORUS, TORUS_DX0))) * smax
    for got, want in zip(on.momentum_net, cpu_on["nets"]):
        for g, w in zip(got, want):
            assert abs(g - w) <= 1e-6 * abs(w) + floor, (got, want)
    assert on.constraints.momentum_net == on.momentum_net[-1]
    factor_dev = [a / b for a, b in zip(mom_off, mom_on)]
    factor_cpu = [a / b for a, b in zip(cpu_off["mom"], cpu_on["mom_net"])]
    print("the factor max|Mom_i| falls by: device", factor_dev, "restatement", factor_cpu)
    assert all(b < a for a, b in zip(mom_off, mom_on))
    np.testing.assert_allclose(factor_dev, factor_cpu, rtol=1e-6)


@pytest.mark.gpu
def test_run_poisson_cli_reflux(comm, tmp_path):
    import json

    from mg_ic_code_amd import Matter, PiProfile
    from mg_ic_code_amd.matter import ScalarPotential
    from mg_ic_code_amd.nl import poisson_solve
    from mg_ic_code_amd.params import read_params
    from mg_ic_code_amd.phi import PhiProfile
    from tests import test_momentum_periodic as TP
    from tests.test_phi_field import PARAMS
    with open(PARAMS) as f:
        txt = f.read()
    for old, new in (("max_NL_iterations = 6", "max_NL_iterations = 2"),
                     ("is_periodic = 0", "is_periodic = 1"),
                     ("bh1_bare_mass = 0.5", "bh1_bare_mass = 0.0"),
                     ("bh2_bare_mass = 0.5", "bh2_bare_mass = 0.0"),
                     ("bh1_spin = 0.1", "bh1_spin = 0.0"), ("bh2_spin = 0.1", "bh2_spin = 0.0"),
                     ("bh1_momentum = 0.05", "bh1_momentum = 0.0"),
                     ("bh2_momentum = -0.05", "bh2_momentum = 0.0")):
        assert txt.count(old) == 1, old
        txt = txt.replace(old, new)
    deck = tmp_path / "periodic.txt"
    deck.write_text(txt)
    prm = read_params(txt)
    want = poisson_solve(_e2e_grids(comm, prm), prm, max_depth=2, phi0=PhiProfile.sine(),
                         constraints=True, matter=Matter(ScalarPotential(), PiProfile.constant(TP.B_PI)),
                         momentum=True, zero_mode="project", reflux=True)
    assert len(want.momentum_net) == 2
    tool = os.path.join(ROOT, "tools", "run_poisson.py")
    boxes = "; ".join(" ".join(str(v) for v in b) for b in E2E_BOXES[1])
    r = subprocess.run([sys.executable, tool, str(deck), "--momentum", "--momentum-zero-mode",
                        "project", "--reflux", "--level-boxes", boxes, "--size", "16",
                        "--max-depth", "2", "--phi", "sine", "--pi", repr(TP.B_PI), "--constraints"],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["momentum_net"] == want.momentum_net
    assert out["momentum_iterations"] == want.momentum_iterations
    assert out["dpsi_norms"] == want.dpsi_norms and out["constant_K"] == want.constant_K
    assert r.stdout.count("+ m psi_0^-6") == 3
    # and without --reflux the old refusal
    r = subprocess.run([sys.executable, tool, str(deck), "--momentum", "--momentum-zero-mode",
                        "project", "--level-boxes", boxes, "--size", "16", "--phi", "sine", "--pi",
                        repr(TP.B_PI)], capture_output=True, text=True, timeout=300,
                       cwd=str(tmp_path))
    assert r.returncode != 0 and "no refluxing" in r.stderr
