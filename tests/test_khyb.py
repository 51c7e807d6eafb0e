"""Hybrid CTTK (mg_ic_code_amd/khyb.py): K(x) from the matter's
energy on decks that are not periodic, poisson_solve(hybrid_K=True).

CPU: the deck key; the refusals (raised before anything is stored, loaded or
launched, in a fresh process); libmgic_khyb.so's ledger without a device and
the binding against the header; the numpy restatement (tests/khyb_ref.py): the
cancellation bound of (2/3) K^2 against 16 pi G rho, the special values, and
the coupled loop on the cases of DESIGN.md 3r against the caps the GPU solve
is held to.  GPU: the kernel bit for bit against the restatement; the entry
point's refusals; the solve end to end on one level, with holes and on a
hierarchy; hybrid_K off is the solve it was; the command line.

The cancellation bound, per cell, with u = eps / 2: v = 1.5 * m16 carries one
rounding, K = -sqrt(v) one, which the square doubles, K * K one, the rounded
constant 2/3 one and its product one: six roundings of u, 3 eps m16.
"""
import dataclasses
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import h5read
from tests import khyb_ref as H
from tests import momentum_ref as R
from tests import phi_ref
from tests import puncture_ref as P
from tests.test_momentum import (KBOXES, KDOM, KDX, L, PARAMS, PI_0, PI_DECK, RELATIVE_HAM_BOUND,
                                 _prm, _random_field)
from tests.test_phi_field import _boxes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(float).eps)
WORKER = os.path.join(ROOT, "tests", "khyb_worker.py")

# the two cases of DESIGN.md 3r on the box of tests/test_momentum.py (no holes,
# L = 16, phi_0 = 0.1 exp(-r^2/8), Pi_0 = PI_0, G = 1): (V0, mass, lambda) and
# the NL iterations the loop may take
CASES = {"V0": ((0.01, 0.0, 0.0), 6), "mass": ((0.0, 1.0, 0.0), 20)}
# the deck itself (two holes, L = 100) with the stretched profiles
POT_DECK = (4e-4, 0.0, 0.0)
PATCH = (8, 8, 8, 23, 23, 23)  # tests/test_momentum.py's fine patch


def _case_prm(n, case):
    return dataclasses.replace(_prm(n), max_NL_iterations=CASES[case][1])


def _cpu_inputs(n):
    prm = _prm(n)
    lo, hi, dx = (0, 0, 0), (n - 1,) * 3, L / n
    phi_g = phi_ref.phi_on_box(phi_ref.gaussian, prm.bh(), lo, hi, dx)
    x, y, z = phi_ref.centres(lo, hi, dx, L, grow=0)
    pi = np.ascontiguousarray(np.broadcast_to(PI_0(x, y, z), (n, n, n)))
    return phi_g, pi


_CPU = {}


def _cpu_case(n, case, source_term=True):
    """The restatement's hybrid loop (computed once, shared, left unchanged):
    dict(norms, mom (max|Mom_i|), ham (max|Ham| / max Ham_abs), K)."""
    key = (n, case, source_term)
    if key not in _CPU:
        phi_g, pi = _cpu_inputs(n)
        r = H.hybrid_solve(_case_prm(n, case), n, 2, phi_g, CASES[case][0], pi,
                           source_term=source_term)
        _CPU[key] = dict(norms=[float(v) for v in r["norms"]],
                         mom=[float(np.abs(m).max()) for m in r["mom"]],
                         ham=float(np.abs(r["ham"]).max() / r["ham_abs"].max()), K=r["K"])
    return _CPU[key]


def _assert_v0_caps(at16, at32):
    """dict(norms, mom, ham) at 16^3 and 32^3 of the V0 case."""
    for r in (at16, at32):
        assert len(r["norms"]) <= 6 and r["norms"][-1] < 1e-10, r["norms"]
        assert r["ham"] < RELATIVE_HAM_BOUND, r["ham"]
    for i in range(3):
        assert at16["mom"][i] >= 3.0 * at32["mom"][i], (i, at16["mom"], at32["mom"])


def _assert_mass_caps(r, n):
    """dict(norms, mom, ham) of the mass case at n^3: converged, a contraction
    of 0.3 at the worst, and the D_i K term of S_i buys its factor."""
    norms = r["norms"]
    assert len(norms) <= 20 and norms[-1] < 1e-10, norms
    for a, b in zip(norms, norms[1:]):
        assert b <= 0.3 * a, norms
    without = _cpu_case(n, "mass", source_term=False)
    factor = {16: 6.0, 32: 24.0}[n]
    for i in range(3):
        assert r["mom"][i] * factor <= without["mom"][i], (n, i, r["mom"], without["mom"])


# ------------------------------------------------------------------ CPU
def test_deck_key_hybrid_K():
    from mg_ic_code_amd.params import read_params
    with open(PARAMS) as f:
        txt = f.read()
    assert "hybrid_K" not in txt
    assert read_params(txt).hybrid_K == 0
    assert read_params(txt + "\nhybrid_K = 1\n").hybrid_K == 1
    assert read_params(txt + "\nhybrid_K = 0\n").hybrid_K == 0
    assert read_params(txt, {"hybrid_K": "1"}).hybrid_K == 1
    for bad in ("2", "-1"):
        with pytest.raises(ValueError, match="hybrid_K"):
            read_params(txt + f"\nhybrid_K = {bad}\n")
    with pytest.raises(ValueError):
        read_params(txt + "\nhybrid_K = yes\n")


def _run_worker(*args, timeout=300, env_extra=None):
    env = dict(os.environ, **(env_extra or {}))
    env.pop("MGIC_LAUNCH_LEDGER", None)
    r = subprocess.run([sys.executable, WORKER] + [str(a) for a in args], capture_output=True,
                       text=True, env=env, timeout=timeout)
    assert r.returncode == 0, f"{r.stdout[-3000:]}\n{r.stderr[-4000:]}"
    return r.stdout


def run_refusals():
    """Every refusal of poisson_solve(hybrid_K=True): raised without a grid,
    with nothing loaded and nothing launched.  Run by tests/khyb_worker.py in
    a fresh process."""
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import Matter, PiProfile, ScalarPotential, _lib
    from mg_ic_code_amd.matter import MatterArgumentError
    from mg_ic_code_amd.nl import poisson_solve
    prm = _prm(16)
    matter = Matter(ScalarPotential(0.01), PiProfile.from_function(PI_0))
    ledger = mg.launch_ledger()
    for grid in (None, [None, None]):  # one level and a hierarchy
        with pytest.raises(ValueError, match="periodic deck.*cttk_solve"):
            poisson_solve(grid, dataclasses.replace(prm, is_periodic=1), matter=matter,
                          hybrid_K=True)
        with pytest.raises(ValueError, match="periodic deck"):  # the projected path too
            poisson_solve(grid, dataclasses.replace(prm, is_periodic=1), matter=matter,
                          hybrid_K=True, zero_mode="project")
        with pytest.raises(MatterArgumentError, match="needs matter"):
            poisson_solve(grid, prm, hybrid_K=True)
        with pytest.raises(MatterArgumentError, match="Pi_0"):
            poisson_solve(grid, prm, matter=Matter(ScalarPotential(0.01)), hybrid_K=True)
        with pytest.raises(MatterArgumentError, match="Pi_0"):
            poisson_solve(grid, prm, matter=ScalarPotential(0.01), hybrid_K=True)
        with pytest.raises(ValueError, match="momentum=False"):
            poisson_solve(grid, prm, matter=matter, hybrid_K=True, momentum=False)
        with pytest.raises(ValueError, match="adm.*K = 0"):
            poisson_solve(grid, prm, matter=matter, hybrid_K=True, adm=[4])
        with pytest.raises(ValueError, match="adm.*K = 0"):
            poisson_solve(grid, dataclasses.replace(prm, adm_half_widths=[4]), matter=matter,
                          hybrid_K=True)
        with pytest.raises(ValueError, match="horizons.*K = 0"):
            poisson_solve(grid, prm, matter=matter, hybrid_K=True, horizons="punctures")
        with pytest.raises(ValueError, match="horizons.*K = 0"):
            poisson_solve(grid, prm, matter=matter, hybrid_K=True, horizons=[(0.0, 0.0, 0.0, 1.0)])
        # the deck's switch asks for the same
        with pytest.raises(MatterArgumentError, match="needs matter"):
            poisson_solve(grid, dataclasses.replace(prm, hybrid_K=1))
        for bad in (2, "yes", 1.0):
            with pytest.raises(ValueError, match="hybrid_K must be"):
                poisson_solve(grid, prm, matter=matter, hybrid_K=bad)
    assert not _lib.khyb_loaded() and not _lib.cttk_loaded() and not _lib.ctt_loaded()
    assert mg.launch_ledger() == ledger and set(ledger.values()) == {0}


def test_refusals_are_raised_before_anything_is_stored_loaded_or_launched():
    out = _run_worker("refusals", env_extra={"MGIC_NO_TORCH_PRELOAD": "1"})
    assert out.strip().splitlines()[-1] == "ok refusals"


def test_khyb_library_loads_without_a_device_and_lists_its_one_kernel(tmp_path):
    out = tmp_path / "khyb.ledger"
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import mg_ic_code_amd as mg\n"
            "from mg_ic_code_amd import _lib, khyb, cttk\n"
            "assert not _lib.khyb_loaded() and not _lib.cttk_loaded() and not _lib.ctt_loaded()\n"
            "d = khyb.khyb_launch_ledger()\n"
            "assert _lib.khyb_loaded() and not _lib.cttk_loaded() and not _lib.ctt_loaded()\n"
            "assert _lib.khyb_call('mgic_khyb_launch_ledger_dump', %r) == 0\n"
            "assert d == {'k_khyb_K': 0}, d\n"
            "assert not any(n.startswith('k_khyb') for n in mg.launch_ledger())\n"
            "assert sorted(cttk.cttk_launch_ledger()) == ['k_cttk_K', 'k_cttk_constraints', "
            "'k_cttk_source']\n"
            % (ROOT, str(out).encode()))
    env = dict(os.environ, MGIC_NO_TORCH_PRELOAD="1")
    env.pop("MGIC_LAUNCH_LEDGER", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(out) as f:
        assert f.read() == "k_khyb_K\t0\n"


def test_binding_covers_the_khyb_header():
    from mg_ic_code_amd import _lib
    with open(os.path.join(ROOT, "include", "mgic_khyb.h")) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    names = set(re.findall(r"MGIC_KHYB_API\s+[\w\s\*]+?\b(mgic_khyb_\w+)\s*\(", txt))
    assert len(names) == 4 and names == set(_lib.KHYB_SIGNATURES)
    assert len(_lib.KHYB_SIGNATURES["mgic_khyb_K"]) == 7


def test_the_one_kernel_of_the_khyb_library_is_launched_through_its_ledger():
    for name in ("khyb.hip", "khyb_capi.cpp", "khyb.hpp"):
        with open(os.path.join(ROOT, "mg_ic_code_amd", "csrc", name)) as f:
            assert "<<<" not in f.read(), name
    with open(os.path.join(ROOT, "mg_ic_code_amd", "csrc", "khyb.hip")) as f:
        txt = f.read()
    assert txt.count("__global__") == txt.count("ledger::launch<k_khyb_") == 1
    assert "__shared__" not in txt


def test_restated_kernel_cancels_the_matter_term_to_six_roundings():
    rng = np.random.default_rng(20271201)
    worst = 0.0
    for _ in range(20):
        pot = (rng.uniform(0.0, 1.0), rng.uniform(-2.0, 2.0), rng.uniform(0.0, 3.0))
        G = rng.uniform(0.1, 4.0)
        phi = rng.uniform(-1.5, 1.5, (6, 7, 9))
        for pi in (None, rng.uniform(-1.0, 1.0, phi.shape)):
            K, bad = H.kernel_K(phi, pi, pot, G)
            m = H.m16(phi, pi, pot, G)
            assert bad == 0 and np.all(m > 0.0) and np.all(K < 0.0)
            err = np.abs((2.0 / 3.0) * (K * K) - m) / m
            worst = max(worst, float(err.max()))
            assert np.all(err <= 3.0 * EPS), float(err.max()) / EPS
    print("worst |(2/3) K^2 - m16| / m16, in eps:", worst / EPS)


def test_restated_kernel_on_its_special_values():
    # rho = 0.5 q^2 with a zero potential: zero (either sign of q), NaN, Inf
    q = np.array([[[0.0, -0.0, np.nan, np.inf, -np.inf, 1.0, -1.0]]])
    phi = np.zeros_like(q)
    with np.errstate(invalid="ignore"):
        K, bad = H.kernel_K(phi, q, (0.0, 0.0, 0.0), 1.0)
    k12 = -np.sqrt(1.5 * (16.0 * np.pi * 1.0 * 0.5))
    assert bad == 1
    assert np.array_equal(K[0, 0], [-0.0, -0.0, 0.0, -np.inf, -np.inf, k12, k12])
    assert np.signbit(K[0, 0, 0]) and np.signbit(K[0, 0, 1]) and not np.signbit(K[0, 0, 2])
    # a negative potential: rho < 0 where Pi^2/2 does not outweigh it; NaN and
    # Inf in phi
    q = np.array([[[0.0, 0.1, 2.0, 0.0, 0.0]]])
    phi = np.array([[[0.3, 0.3, 0.3, np.nan, np.inf]]])
    with np.errstate(invalid="ignore"):
        K, bad = H.kernel_K(phi, q, (-1.0, 0.0, 0.0), 1.0)
    assert bad == 4 and np.array_equal(K[0, 0, [0, 1, 3]], [0.0, 0.0, 0.0])
    assert not np.signbit(K[0, 0, [0, 1, 3]]).any()
    assert K[0, 0, 2] == -np.sqrt(1.5 * (16.0 * np.pi * 1.0 * (0.5 * 2.0 * 2.0 + -1.0)))
    # Inf * 0 in the mass term is NaN, as on the device: counted, K = 0
    assert K[0, 0, 4] == 0.0 and not np.signbit(K[0, 0, 4])
    with np.errstate(invalid="ignore"):
        K, bad = H.kernel_K(np.array([[[np.inf]]]), None, (0.0, 1.0, 1.0), 1.0)
    assert bad == 0 and K[0, 0, 0] == -np.inf
    # without a Pi: rho = V
    K, bad = H.kernel_K(np.array([[[0.5]]]), None, (0.25, 0.0, 0.0), 2.0)
    assert bad == 0 and K[0, 0, 0] == -np.sqrt(1.5 * (16.0 * np.pi * 2.0 * 0.25))


def test_restatements_hybrid_loop_on_the_V0_case():
    """V0 = 0.01: the restatement converges in six NL iterations,
        16^3: |dpsi| 1.61e-1 1.03e-3 6.4e-6 4.0e-8 2.3e-10 1.1e-12
        32^3: |dpsi| 1.78e-1 ... 1.4e-11
    max|Ham| / max Ham_abs 2.3e-13 and 1.3e-12, max|Mom_i| 5.18e-3 5.17e-3
    4.99e-3 and 1.61e-3 1.47e-3 1.44e-3 (ratios 3.2 - 3.5); the constant-K
    loop of tests/momentum_ref.py leaves |dpsi| = 3.6e13 after one."""
    at16, at32 = _cpu_case(16, "V0"), _cpu_case(32, "V0")
    print("16^3", at16["norms"], at16["mom"], at16["ham"])
    print("32^3", at32["norms"], at32["mom"], at32["ham"])
    _assert_v0_caps(at16, at32)
    phi_g, pi = _cpu_inputs(16)
    with np.errstate(all="ignore"):
        plain = R.coupled_solve(_prm(16), 16, 2, phi_g, CASES["V0"][0], pi, momentum_on=True)
    print("constant K: |dpsi|", plain["norms"])
    assert not plain["norms"][-1] <= 1e-1


@pytest.mark.parametrize("n", [16, 32])
def test_restatements_hybrid_loop_on_the_mass_case(n):
    """mass = 1 (max|K| 0.63 and 0.67): |dpsi| contracts by 0.17 - 0.19 per NL
    iteration, 14 iterations at 16^3 and 15 at 32^3; max|Mom_i| 1.387e-2
    1.401e-2 1.395e-2 and 4.15e-3 4.09e-3 3.98e-3; with the D_i K term left out
    of S_i 0.1117 0.1129 0.1130 and 0.1275 0.1268 0.1256 (8.0 - 8.1 and 30.7 -
    31.5 times as much)."""
    r = _cpu_case(n, "mass")
    print(n, r["norms"], r["mom"], r["ham"], _cpu_case(n, "mass", False)["mom"])
    _assert_mass_caps(r, n)
    assert r["ham"] < RELATIVE_HAM_BOUND


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def comm():
    import mg_ic_code_amd as mg
    return mg.Comm()


def _download(fields):
    return [[f.download(n, with_ghosts=True) for n in range(f.grid.num_local)] for f in fields]


def run_kernel_cases(comm):
    """k_khyb_K against tests/khyb_ref.py bit for bit on random fields whose
    ghosts hold arbitrary values: with Pi and without, a potential that leaves
    every cell a real K and one that does not (with NaNs in phi), twice with the
    same bits, every ghost of K and every other field unchanged.  Shared with
    tests/khyb_worker.py.  Returns (the library's ledger, the calls made)."""
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import ScalarPotential, khyb
    from mg_ic_code_amd.decomposition import split_domain
    rng = np.random.default_rng(20271202)
    dom16 = (0, 0, 0, 15, 15, 15)
    layouts = [(KDOM, KBOXES, KDX, True)] + [
        (dom16, split_domain(dom16, parts), L / 16, False)
        for parts in ((1, 1, 1), (2, 2, 1), (2, 2, 2))]
    calls = 0
    for dom, boxes, dx, patches in layouts:
        grid = mg.Grid(comm, dom, boxes, dx, patches=patches)
        nb = grid.num_local
        assert nb == len(boxes)
        (phi, phi_a), (pi, pi_a), (K, K_a) = (_random_field(grid, rng) for _ in range(3))
        for pot, G, nans in (((0.3, 1.2, 0.7), 1.0, False), ((-0.2, 0.9, 0.0), 2.5, True)):
            if nans:
                for n in range(nb):
                    flat = phi_a[n].reshape(-1)
                    flat[rng.choice(flat.size, 12, replace=False)] = np.nan
                    phi.upload(n, phi_a[n], with_ghosts=True)
            for with_pi in (True, False):
                want, bad = [], 0
                for n in range(nb):
                    with np.errstate(invalid="ignore"):
                        k, b = H.kernel_K(R.valid(phi_a[n]), R.valid(pi_a[n]) if with_pi else None,
                                          pot, G)
                    w = K_a[n].copy()
                    w[1:-1, 1:-1, 1:-1] = k
                    want.append(w)
                    bad += b
                assert (bad > 0) == nans, (bad, nans)
                for rep in range(2):
                    for n in range(nb):  # K's cells and ghosts as they were
                        K.upload(n, K_a[n], with_ghosts=True)
                    got_bad = khyb.set_K_from_matter(phi, pi if with_pi else None,
                                                     ScalarPotential(*pot), G, K)
                    calls += 1
                    assert got_bad == bad, (got_bad, bad, dom, len(boxes), pot, with_pi)
                    got = _download([phi, pi, K])
                    for n in range(nb):
                        assert np.array_equal(got[0][n], phi_a[n], equal_nan=True)
                        assert np.array_equal(got[1][n], pi_a[n])
                        assert np.array_equal(got[2][n], want[n]), (dom, len(boxes), pot, with_pi,
                                                                    n, rep)
                        if nans:  # K = +0.0 exactly where there is no real K
                            k = R.valid(got[2][n])
                            refused = ~(1.5 * H.m16(R.valid(phi_a[n]),
                                                    R.valid(pi_a[n]) if with_pi else None, pot,
                                                    G) >= 0.0)
                            assert refused.any() and np.all(k[refused] == 0.0)
                            assert not np.signbit(k[refused]).any()
    return khyb.khyb_launch_ledger(), calls


@pytest.mark.gpu
def test_kernel_is_bit_identical_to_the_restatement(comm):
    from mg_ic_code_amd import khyb
    before = khyb.khyb_launch_ledger()
    after, calls = run_kernel_cases(comm)
    assert sorted(after) == ["k_khyb_K"]
    # one launch per call, whatever the number of boxes: 4 layouts, 2 potentials,
    # with and without Pi, twice
    assert calls == 32 and after["k_khyb_K"] - before["k_khyb_K"] == calls


@pytest.mark.gpu
def test_the_kernel_is_launched_against_its_reference_in_a_fresh_process(tmp_path):
    from mg_ic_code_amd.core import read_launch_ledger
    out = tmp_path / "khyb.ledger"
    _run_worker("kernels", out)
    assert read_launch_ledger(out) == {"k_khyb_K": 32}


@pytest.mark.gpu
def test_entry_point_refuses_with_the_ledger_unchanged(comm):
    import ctypes

    import mg_ic_code_amd as mg
    from mg_ic_code_amd import _lib, khyb
    from mg_ic_code_amd._lib import MgicError
    rng = np.random.default_rng(20271203)
    dom = (0, 0, 0, 7, 7, 7)
    grid = mg.Grid(comm, dom, [dom], 1.0)
    other = mg.Grid(comm, dom, [(0, 0, 0, 7, 7, 3), (0, 0, 4, 7, 7, 7)], 1.0)
    fields, _ = zip(*[_random_field(grid, rng) for _ in range(3)])
    alien, _ = _random_field(other, rng)
    khyb.khyb_launch_ledger()  # loads the library
    before = (khyb.khyb_launch_ledger(), _download(fields))
    phi, pi, K = (f.handle for f in fields)
    pot = (ctypes.c_double * 3)(0.1, 0.2, 0.3)
    bad = ctypes.c_longlong(-7)
    ref, c = ctypes.byref(bad), comm.handle
    cases = [
        ("null", (None, phi, pi, pot, 1.0, K, ref)),
        ("null", (c, None, pi, pot, 1.0, K, ref)),
        ("null", (c, phi, pi, None, 1.0, K, ref)),
        ("null", (c, phi, pi, pot, 1.0, None, ref)),
        ("null", (c, phi, pi, pot, 1.0, K, None)),
        ("null", (c, phi, None, pot, 1.0, None, ref)),
        ("aliased", (c, phi, pi, pot, 1.0, phi, ref)),
        ("aliased", (c, phi, pi, pot, 1.0, pi, ref)),
        ("aliased", (c, phi, None, pot, 1.0, phi, ref)),
        ("layout", (c, phi, alien.handle, pot, 1.0, K, ref)),
        ("layout", (c, phi, pi, pot, 1.0, alien.handle, ref)),
        ("layout", (c, alien.handle, pi, pot, 1.0, K, ref)),
    ]
    for what, args in cases:
        with pytest.raises(MgicError, match=what) as e:
            _lib.khyb_call("mgic_khyb_K", *args)
        assert e.value.code == -1, (what, e.value)  # MGIC_EBADARG
    assert bad.value == -7
    after = (khyb.khyb_launch_ledger(), _download(fields))
    assert after[0] == before[0]
    for a, b in zip(after[1], before[1]):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


def _matter(pot, pi_f=PI_0):
    from mg_ic_code_amd import Matter, PiProfile, ScalarPotential
    return Matter(ScalarPotential(*pot), PiProfile.from_function(pi_f))


def _grid(comm, n, length=L):
    import mg_ic_code_amd as mg
    dom = (0, 0, 0, n - 1, n - 1, n - 1)
    return mg.Grid(comm, dom, [dom], length / n)


_GPU = {}


def _solve(comm, n, case):
    """poisson_solve(hybrid_K=True) on one Dirichlet n^3 box (cached)."""
    import mg_ic_code_amd as mg
    from mg_ic_code_amd.nl import poisson_solve
    if (n, case) not in _GPU:
        t0 = time.perf_counter()
        res = poisson_solve(_grid(comm, n), _case_prm(n, case), max_depth=2,
                            matter=_matter(CASES[case][0]), constraints=True, hybrid_K=True)
        mg.device_synchronize()
        print(f"{n}^3 {case}: {time.perf_counter() - t0:.2f} s, {len(res.dpsi_norms)} NL "
              f"iterations, BiCGStab {res.linear_iterations}, momentum {res.momentum_iterations}")
        _GPU[(n, case)] = res
    return _GPU[(n, case)]


def _report(res):
    rep = res.constraints
    return dict(norms=res.dpsi_norms, mom=[rep.max_norm[f"Mom{i + 1}"] for i in range(3)],
                ham=rep.relative_ham)


def _stored_K(comm, n, pot, prm=None, pi_f=PI_0):
    """The restatement's kernel on phi_0 and Pi_0 as the device stores them."""
    from mg_ic_code_amd import PiProfile
    from mg_ic_code_amd.phi import PhiProfile
    prm = _prm(n) if prm is None else prm
    grid = _grid(comm, n, prm.domainLength[0])
    phi = PhiProfile.gaussian().fill(grid, prm).download(0)
    pi = PiProfile.from_function(pi_f).fill(grid, prm).download(0)
    K, bad = H.kernel_K(phi, pi, pot, prm.G_Newton)
    assert bad == 0
    return K


@pytest.mark.gpu
def test_plain_solve_diverges_and_the_hybrid_converges(comm):
    """The V0 case at 16^3: the parent's best effort, matter with momentum=True,
    raises NLDivergenceError; the same call with hybrid_K=True converges."""
    from mg_ic_code_amd.nl import NLDivergenceError, poisson_solve
    with pytest.raises(NLDivergenceError) as e:
        poisson_solve(_grid(comm, 16), _case_prm(16, "V0"), max_depth=2,
                      matter=_matter(CASES["V0"][0]), constraints=True, momentum=True)
    print("plain |dpsi|", e.value.result.dpsi_norms)
    assert e.value.result.K is None
    res = _solve(comm, 16, "V0")
    assert res.converged and res.momentum is not None and res.constant_K == []


@pytest.mark.gpu
def test_V0_case_end_to_end(comm):
    got = {n: _report(_solve(comm, n, "V0")) for n in (16, 32)}
    for n in (16, 32):
        res, cpu = _solve(comm, n, "V0"), _cpu_case(n, "V0")
        print(f"{n}^3 V0: {got[n]} k_max {res.k_max}")
        assert res.converged
        np.testing.assert_allclose(got[n]["mom"], cpu["mom"], rtol=1e-6)
        K = res.K.download(0)
        assert np.array_equal(K, _stored_K(comm, n, CASES["V0"][0]))
        print(f"{n}^3 V0: cells where K is not the K of the restatement's loop:",
              int(np.count_nonzero(K != cpu["K"])))
        assert res.k_max == float(np.abs(K).max())
    _assert_v0_caps(got[16], got[32])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [16, 32])
def test_mass_case_end_to_end(comm, n):
    res, cpu = _solve(comm, n, "mass"), _cpu_case(n, "mass")
    got = _report(res)
    print(f"{n}^3 mass: {got} k_max {res.k_max}")
    assert res.converged
    _assert_mass_caps(got, n)
    assert got["ham"] < RELATIVE_HAM_BOUND
    np.testing.assert_allclose(got["mom"], cpu["mom"], rtol=1e-6)
    K = res.K.download(0)
    assert np.array_equal(K, _stored_K(comm, n, CASES["mass"][0]))
    # (the loop's own K is numpy's Gaussian's: the same bits wherever the
    # device's exp gives numpy's)
    print(f"{n}^3 mass: cells where K is not the K of numpy's own Gaussian:",
          int(np.count_nonzero(K != cpu["K"])))
    # K's ghosts across the domain faces: 2 K(face) - K(next)
    g = res.K.download(0, with_ghosts=True)
    assert np.array_equal(g[1:-1, 1:-1, 0], 2.0 * g[1:-1, 1:-1, 1] - g[1:-1, 1:-1, 2])
    assert np.array_equal(g[-1, 1:-1, 1:-1], 2.0 * g[-2, 1:-1, 1:-1] - g[-3, 1:-1, 1:-1])


@pytest.mark.gpu
def test_a_negative_rho_raises(comm):
    from mg_ic_code_amd import HybridKError, PiProfile
    from mg_ic_code_amd.nl import poisson_solve
    # V0 = -1e-5 against Pi_0^2 / 2 <= 1.25e-3: negative away from the peak
    pi = PiProfile.from_function(PI_0).fill(_grid(comm, 16), _prm(16)).download(0)
    bad = int(np.count_nonzero(~(1.5 * H.m16(0.0 * pi, pi, (-1e-5, 0.0, 0.0), 1.0) >= 0.0)))
    assert 0 < bad < 16 ** 3
    with pytest.raises(HybridKError, match=f"{bad} cells of level 0") as e:
        poisson_solve(_grid(comm, 16), _prm(16), max_depth=2, matter=_matter((-1e-5, 0.0, 0.0)),
                      hybrid_K=True)
    assert (e.value.bad_cells, e.value.level) == (bad, 0)


@pytest.mark.gpu
def test_with_holes_and_the_final_file(comm, tmp_path):
    """The deck itself (two holes, L = 100) at 32^3, V0 = 4e-4, Pi_0 = 0.08 PI_0
    stretched: the plain solve diverges; the hybrid one ends with |dpsi| <
    1e-8 (the restatement stalls near 2.4e-10, where the linear solve takes no
    iteration) and Ham at rounding; the final file carries K, the corrected
    constraints and the total tensor."""
    from mg_ic_code_amd.nl import NLDivergenceError, poisson_solve
    n = 32
    prm = _prm(n, holes=True)
    LD = prm.domainLength[0]
    with pytest.raises(NLDivergenceError) as e:
        poisson_solve(_grid(comm, n, LD), prm, max_depth=2, matter=_matter(POT_DECK, PI_DECK),
                      constraints=True, momentum=True)
    print("holes, plain |dpsi|", e.value.result.dpsi_norms)
    t0 = time.perf_counter()
    on = poisson_solve(_grid(comm, n, LD), prm, max_depth=2, matter=_matter(POT_DECK, PI_DECK),
                       constraints=True, hybrid_K=True, output_dir=str(tmp_path))
    print(f"holes, hybrid: {time.perf_counter() - t0:.2f} s |dpsi| {on.dpsi_norms} BiCGStab "
          f"{on.linear_iterations} Ham {on.constraints.relative_ham} "
          f"Mom {on.constraints.max_norm} k_max {on.k_max}")
    assert on.dpsi_norms[-1] < 1e-8
    assert on.constraints.relative_ham < RELATIVE_HAM_BOUND
    K = on.K.download(0)
    assert np.array_equal(K, _stored_K(comm, n, POT_DECK, prm, PI_DECK))
    lo, hi, dx = (0, 0, 0), (n - 1,) * 3, LD / n
    table = P.deck_table(prm.bh())
    d = h5read.dataset(str(tmp_path / "vcPoissonFinal.3d.hdf5"), "/level_0/data:datatype=0",
                       "<f8").reshape((31, n, n, n))
    assert np.array_equal(d[7], K) and float(np.abs(K).min()) > 0.0
    A, psi_bh = P.bowen_york(table, LD, lo, hi, dx)
    psi_0 = on.psi.download(0) + psi_bh
    np.testing.assert_allclose(d[0], psi_0 ** -4.0, rtol=1e-13, atol=0)
    LW = [f.download(0) for f in on.momentum.lw(0)]
    assert max(float(np.abs(x).max()) for x in LW) > 1e-5
    for c, ij in enumerate(P.IJ):
        want = (A[ij] + LW[c]) * psi_0 ** -6.0
        bar = (np.abs(A[ij]) + np.abs(LW[c])) * psi_0 ** -6.0
        assert np.max(np.abs(d[8 + c] - want) / bar) <= 1e-13, ij
    for c in range(4):
        assert np.array_equal(d[27 + c], on.constraints.fields[0].fields()[c].download(0))
    assert float(np.abs(d[27]).max()) == on.constraints.max_norm["Ham"]


@pytest.mark.gpu
def test_hierarchy_solve_and_the_ghosts_of_K(comm):
    """A 16^3 base and tests/test_momentum.py's fine patch, mass case: the
    solve converges, Ham is at rounding, the fine K's face ghosts are cf_interp
    of the coarse K, the base's are extrapolated; max|Mom_i| over the uncovered
    cells is held to the one-level 16^3 value."""
    import mg_ic_code_amd as mg
    from mg_ic_code_amd.core import AMRSolver, OperatorParams, SolverParams
    from mg_ic_code_amd.nl import poisson_solve
    prm = _case_prm(16, "mass")
    dom = (0, 0, 0, 15, 15, 15)
    grids = [mg.Grid(comm, dom, [dom], L / 16),
             mg.Grid(comm, (0, 0, 0, 31, 31, 31), [PATCH], L / 32, patches=True)]
    t0 = time.perf_counter()
    res = poisson_solve(grids, prm, max_depth=2, matter=_matter(CASES["mass"][0]),
                        constraints=True, hybrid_K=True)
    print(f"hierarchy: {time.perf_counter() - t0:.2f} s |dpsi| {res.dpsi_norms} BiCGStab "
          f"{res.linear_iterations} momentum {res.momentum_iterations}")
    assert res.converged and len(res.dpsi_norms) <= 20
    assert res.constraints.relative_ham < RELATIVE_HAM_BOUND
    assert isinstance(res.K, list) and len(res.K) == 2
    one = _report(_solve(comm, 16, "mass"))
    got = [res.constraints.max_norm[f"Mom{i + 1}"] for i in range(3)]
    print("hierarchy max|Mom_i|", got, "one level 16^3", one["mom"])
    for i in range(3):
        assert got[i] <= one["mom"][i], (i, got, one["mom"])
    # the fine K's ghosts: every face of the patch is a coarse-fine face
    a, b = [mg.LevelData(g) for g in grids], [mg.LevelData(g) for g in grids]
    for l in range(2):
        a[l].set_zero()
        b[l].set_val(1.0)
    amr = AMRSolver(list(zip(grids, a, b)), OperatorParams(), SolverParams())

    def faces(x):
        return [x[0, 1:-1, 1:-1], x[-1, 1:-1, 1:-1], x[1:-1, 0, 1:-1], x[1:-1, -1, 1:-1],
                x[1:-1, 1:-1, 0], x[1:-1, 1:-1, -1]]

    fine = res.K[1].download(0, with_ghosts=True)
    poisoned = np.full_like(fine, -7.0)
    poisoned[1:-1, 1:-1, 1:-1] = R.valid(fine)
    again = mg.LevelData(grids[1])
    again.upload(0, poisoned, with_ghosts=True)
    amr.cf_interp(1, again, res.K[0])
    new = again.download(0, with_ghosts=True)
    for x, y in zip(faces(fine), faces(new)):
        assert np.all(y != -7.0) and np.array_equal(x, y)
    base = res.K[0].download(0, with_ghosts=True)
    for ax in range(3):
        g = np.moveaxis(base, ax, 0)
        assert np.array_equal(g[0, 1:-1, 1:-1], 2.0 * g[1, 1:-1, 1:-1] - g[2, 1:-1, 1:-1])
        assert np.array_equal(g[-1, 1:-1, 1:-1], 2.0 * g[-2, 1:-1, 1:-1] - g[-3, 1:-1, 1:-1])
    # max|K| over the hierarchy (covered coarse cells masked)
    assert 0.0 < res.k_max <= max(float(np.abs(k.download(0)).max()) for k in res.K)


def run_off_means_off():
    """hybrid_K=False, the keyword left out and the deck's hybrid_K = 0 are one
    solve (psi bits, iteration counts, libmgic's ledger), and libmgic_khyb.so
    stays unloaded.  Run by tests/khyb_worker.py in a fresh process."""
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import _lib
    from mg_ic_code_amd.nl import poisson_solve
    from tests.test_momentum import _matter as plain_matter
    comm = mg.Comm()
    runs = []
    for how in (False, None, "deck"):
        mg.launch_ledger_reset()
        prm = dataclasses.replace(_prm(16), hybrid_K=0) if how == "deck" else _prm(16)
        kw = {"hybrid_K": False} if how is False else {}
        res = poisson_solve(_grid(comm, 16), prm, max_depth=2, matter=plain_matter(),
                            constraints=True, momentum=True, **kw)
        runs.append((res.psi.download(0, with_ghosts=True), res.linear_iterations, res.dpsi_norms,
                     res.momentum_iterations, mg.launch_ledger()))
        assert not _lib.khyb_loaded() and not _lib.cttk_loaded(), how
        assert res.K is None and res.k_max == 0.0
    for r in runs[1:]:
        assert np.array_equal(r[0], runs[0][0]) and r[1:] == runs[0][1:]
    assert runs[0][1] and sum(runs[0][4].values()) > 0
    names = sorted(mg.launch_ledger())
    res = poisson_solve(_grid(comm, 16), _prm(16), max_depth=2, matter=plain_matter(),
                        hybrid_K=True)
    assert _lib.khyb_loaded() and _lib.cttk_loaded() and res.K is not None
    assert sorted(mg.launch_ledger()) == names


@pytest.mark.gpu
def test_hybrid_K_off_is_the_solve_it_was_and_loads_nothing():
    out = _run_worker("off")
    assert out.strip().splitlines()[-1] == "ok off"


@pytest.mark.gpu
def test_run_poisson_cli_hybrid_K(tmp_path):
    with open(PARAMS) as f:
        txt = f.read().replace("max_NL_iterations = 6", "max_NL_iterations = 2")
    decks = {"key": tmp_path / "key.txt", "flag": tmp_path / "flag.txt"}
    decks["key"].write_text(txt + "\nhybrid_K = 1\n")
    decks["flag"].write_text(txt)
    tool = os.path.join(ROOT, "tools", "run_poisson.py")
    common = ["--size", "16", "--max-depth", "2", "--pi", "0.004", "--potential", "4e-4 0 0",
              "--constraints"]
    outs, texts = {}, {}
    for how, extra in (("key", []), ("flag", ["--hybrid-K"])):
        r = subprocess.run([sys.executable, tool, str(decks[how])] + extra + common,
                           capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs[how], texts[how] = json.loads(r.stdout.strip().splitlines()[-1]), r.stdout
    key, flag = outs["key"], outs["flag"]
    assert flag["dpsi_norms"] == key["dpsi_norms"] and len(key["dpsi_norms"]) == 2
    assert flag["momentum_iterations"] == key["momentum_iterations"]
    assert flag["hybrid_K"] == key["hybrid_K"]
    # K = -sqrt(24 pi G (Pi^2/2 + V0)) is one number on this deck
    k = float(np.sqrt(1.5 * (16.0 * np.pi * 1.0 * (0.5 * 0.004 * 0.004 + 4e-4))))
    assert key["hybrid_K"]["k_max"] == k
    assert set(key["hybrid_K"]["max_norm"]) == {"Ham", "Mom1", "Mom2", "Mom3"}
    assert key["hybrid_K"]["relative_ham"] > 0.0
    for text in texts.values():
        assert f"hybrid K: max|K| = {k:.16e}" in text
        assert text.count("constraint Mom") == 3 and "constraint max|Ham| / max Ham_abs" in text
