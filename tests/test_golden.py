"""Committed fixtures (tests/golden/, written by make_golden.py).

CPU: the oracle still reproduces every fixture bit for bit (regression of
the checker itself).  GPU: the HIP path reproduces the same fixtures through
the C ABI -- the ChF drop-ins on the 12^3 kernel vectors, the operator-level
V-cycle on the 16^3 hierarchy -- bit for bit, without consulting the oracle.
Parity status of these fixtures: regression vectors of the restatement.  Its
ChF kernels are pinned to the compiled reference by
tests/test_reference_parity.py (whose own fixture, reference_kernels.npz, the
compiled reference wrote); lambda, the averages and the V-cycle are still
"parity unpinned" (DESIGN.md §4).
"""
import ctypes
import json
import os

import numpy as np
import pytest

import oracle
from oracle import Fab

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DX = 100.0 / 64
ALPHA, BETA = 1.0, -1.0


@pytest.fixture(scope="module")
def k12():
    with np.load(os.path.join(HERE, "kernels12.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def v16():
    with np.load(os.path.join(HERE, "vcycle16.npz")) as z:
        return {k: z[k] for k in z.files}


def test_oracle_reproduces_kernel_fixtures(k12):
    u, rhs, a, b, lam = (k12[k] for k in ("u", "rhs", "a", "b", "lam"))
    g, lo, hi = (-1, -1, -1), (0, 0, 0), (11, 11, 11)
    lam2 = np.zeros_like(lam)
    oracle.lam(Fab(lam2, g), Fab(a, g), lo, hi, ALPHA, BETA, DX)
    assert np.array_equal(lam2, lam)
    s = u.copy()
    oracle.gsrb(Fab(s, g), Fab(rhs, g), lo, hi, DX, ALPHA, Fab(a, g), BETA, Fab(b, g), Fab(lam, g), 0)
    assert np.array_equal(s, k12["gsrb_pass0"])
    oracle.gsrb(Fab(s, g), Fab(rhs, g), lo, hi, DX, ALPHA, Fab(a, g), BETA, Fab(b, g), Fab(lam, g), 1)
    assert np.array_equal(s, k12["gsrb_sweep"])
    out = np.zeros_like(u)
    oracle.apply_op(Fab(out, g), Fab(u, g), ALPHA, Fab(a, g), BETA, Fab(b, g), lo, hi, DX)
    assert np.array_equal(out, k12["op"])
    oracle.residual(Fab(out, g), Fab(u, g), Fab(rhs, g), ALPHA, Fab(a, g), BETA, Fab(b, g), lo, hi, DX)
    assert np.array_equal(out, k12["res"])
    rc = np.zeros((6, 6, 6))
    oracle.restrict_residual(Fab(rc, lo), Fab(u, g), Fab(rhs, g), ALPHA, Fab(a, g), BETA, Fab(b, g),
                             lo, hi, DX)
    assert np.array_equal(rc, k12["restrict"])
    inner = np.ascontiguousarray(b[1:-1, 1:-1, 1:-1])
    for name, harm in (("avg_arith", 0), ("avg_harm", 1)):
        c = np.zeros((6, 6, 6))
        oracle.average(Fab(c, lo), Fab(inner, lo), lo, (5, 5, 5), 2, harm)
        assert np.array_equal(c, k12[name])


def test_fixture_known_answers(k12):
    # sanity of the fixture itself: pass 0 changed exactly the red cells,
    # lambda has the closed form 1 / (alpha a + 6 beta / dx^2)
    u, p0 = k12["u"][1:-1, 1:-1, 1:-1], k12["gsrb_pass0"][1:-1, 1:-1, 1:-1]
    k, j, i = np.indices(u.shape)
    red = (i + j + k) % 2 == 0
    assert np.all(p0[~red] == u[~red]) and np.all(p0[red] != u[red])
    a = k12["a"][1:-1, 1:-1, 1:-1]
    np.testing.assert_allclose(k12["lam"][1:-1, 1:-1, 1:-1], 1.0 / (ALPHA * a + 6 * BETA / DX**2),
                               rtol=1e-15)


def test_oracle_reproduces_vcycle_fixture(v16):
    n = 16
    dom = (0, 0, 0, n - 1, n - 1, n - 1)
    o = oracle.OracleMG([dom], dom, 1.0 / n, alpha=ALPHA, beta=BETA, nlevels=3, avg_type=1,
                        prolong_type=1, bottom_solver=0, n_pre=4, n_post=4, n_bottom=4)
    o.set(0, oracle.ACOEF, 0, v16["a"])
    o.set(0, oracle.BCOEF, 0, np.ones_like(v16["a"]))
    o.set(0, oracle.RHS, 0, v16["rhs"])
    o.setup()
    hist = [o.init_residual(0)] + [o.iteration(0) for _ in range(4)]
    assert hist == list(v16["residual_max_norm"])
    assert np.array_equal(o.get(0, oracle.PHI, 0), v16["phi"])
    assert all(hist[i + 1] < hist[i] for i in range(4))


def test_oracle_reproduces_binary_bh_samples():
    from mg_ic_code_amd.params import read_params_file
    d = json.load(open(os.path.join(HERE, "binary_bh64.json")))
    p = read_params_file(os.path.join(HERE, "params.txt"))
    n = d["n"]
    a, r = oracle.binary_bh(p.bh(), (0, 0, 0), (n - 1,) * 3, p.coarsestDx)
    for (i, j, k), ah, rh in zip(d["cells_ijk"], d["aCoef"], d["rhs"]):
        assert a[k, j, i] == float.fromhex(ah) and r[k, j, i] == float.fromhex(rh)


# ------------------------------------------------------------------ GPU side
def _dbl(p):
    return p.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _ints(*v):
    return [ctypes.byref(ctypes.c_int(int(x))) for x in v]


def _fab(arr, lo):
    nz, ny, nx = arr.shape
    return [_dbl(arr)] + _ints(*lo) + _ints(lo[0] + nx - 1, lo[1] + ny - 1, lo[2] + nz - 1) + _ints(1)


@pytest.mark.gpu
def test_gpu_dropins_reproduce_kernel_fixtures(k12):
    mg = pytest.importorskip("mg_ic_code_amd")
    u, rhs, a, b, lam = (np.ascontiguousarray(k12[k]) for k in ("u", "rhs", "a", "b", "lam"))
    g, lo, hi = (-1, -1, -1), (0, 0, 0), (11, 11, 11)
    cd = ctypes.c_double
    s = u.copy()
    for rb, key in ((0, "gsrb_pass0"), (1, "gsrb_sweep")):
        mg.lib.gsrbhelmholtzvc3d_(*_fab(s, g), *_fab(rhs, g), *_ints(*lo), *_ints(*hi),
                                  ctypes.byref(cd(DX)), ctypes.byref(cd(ALPHA)), *_fab(a, g),
                                  ctypes.byref(cd(BETA)), *_fab(b, g), *_fab(lam, g),
                                  ctypes.byref(ctypes.c_int(rb)))
        assert np.array_equal(s, k12[key])
    out = np.zeros_like(u)
    mg.lib.vccomputeop3d_(*_fab(out, g), *_fab(u, g), ctypes.byref(cd(ALPHA)), *_fab(a, g),
                          ctypes.byref(cd(BETA)), *_fab(b, g), *_ints(*lo), *_ints(*hi),
                          ctypes.byref(cd(DX)))
    assert np.array_equal(out[1:-1, 1:-1, 1:-1], k12["op"][1:-1, 1:-1, 1:-1])
    mg.lib.vccomputeres3d_(*_fab(out, g), *_fab(u, g), *_fab(rhs, g), ctypes.byref(cd(ALPHA)),
                           *_fab(a, g), ctypes.byref(cd(BETA)), *_fab(b, g), *_ints(*lo), *_ints(*hi),
                           ctypes.byref(cd(DX)))
    assert np.array_equal(out[1:-1, 1:-1, 1:-1], k12["res"][1:-1, 1:-1, 1:-1])
    rc = np.zeros((6, 6, 6))
    mg.lib.restrictresvc3d_(*_fab(rc, lo), *_fab(u, g), *_fab(rhs, g), ctypes.byref(cd(ALPHA)),
                            *_fab(a, g), ctypes.byref(cd(BETA)), *_fab(b, g), *_ints(*lo),
                            *_ints(*hi), ctypes.byref(cd(DX)))
    assert np.array_equal(rc, k12["restrict"])


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [1, 0])
def test_gpu_vcycle_reproduces_fixture(v16, fused):
    mg = pytest.importorskip("mg_ic_code_amd")
    n = 16
    dom = (0, 0, 0, n - 1, n - 1, n - 1)
    comm = mg.Comm()
    grid = mg.Grid(comm, dom, [dom], 1.0 / n)
    fa, fb, frhs, fphi, fres = (mg.LevelData(grid) for _ in range(5))
    fa.upload(0, np.ascontiguousarray(v16["a"]))
    fb.set_val(1.0)
    frhs.upload(0, np.ascontiguousarray(v16["rhs"]))
    fphi.set_zero()
    prm = mg.OperatorParams(alpha=ALPHA, beta=BETA, coefficient_average_type=1, prolong_type=1,
                            relax_mode=1, fused_smoother=fused)
    fac = mg.defineOperatorFactory(grid, fa, fb, prm)
    amg = mg.AMRMultiGrid(fac, mg.SolverParams(max_depth=2, n_pre=4, n_post=4, n_bottom=4,
                                                bottom_solver=0))
    hist = [amg.init_residual(fphi, frhs, fres, norm_type=0)]
    hist += [amg.iteration(fphi, frhs, fres, norm_type=0) for _ in range(4)]
    assert hist == list(v16["residual_max_norm"])
    assert np.array_equal(fphi.download(0), v16["phi"])


@pytest.mark.gpu
def test_gpu_binary_bh_matches_samples():
    mg = pytest.importorskip("mg_ic_code_amd")
    from mg_ic_code_amd.params import read_params_file
    d = json.load(open(os.path.join(HERE, "binary_bh64.json")))
    p = read_params_file(os.path.join(HERE, "params.txt"))
    n = d["n"]
    dom = (0, 0, 0, n - 1, n - 1, n - 1)
    grid = mg.Grid(mg.Comm(), dom, [dom], p.coarsestDx)
    fa, fr = mg.LevelData(grid), mg.LevelData(grid)
    mg.set_binary_bh_coefs(fa, fr, p.bh())
    a, r = fa.download(0), fr.download(0)
    for (i, j, k), ah, rh in zip(d["cells_ijk"], d["aCoef"], d["rhs"]):
        np.testing.assert_allclose(a[k, j, i], float.fromhex(ah), rtol=1e-13)
        np.testing.assert_allclose(r[k, j, i], float.fromhex(rh), rtol=1e-13)
