"""Periodic decks closed by the CTTK method (mg_ic_code_amd/cttk.py, DESIGN.md
3q): psi is chosen, K varies in space, the momentum constraint carries
(2/3) D_i K as a source.

CPU: the numpy restatement (tests/cttk_ref.py) on the cases of
tests/test_momentum_periodic.py -- the loop contracts, the momentum constraint
falls against the first pass's data, Ham is at rounding with the final K, the
unbalanced case's net current stays, a psi that asks too much is refused --
the deck keys, the refusals (raised before anything is loaded or launched),
libmgic_cttk.so's ledger without a device, the binding against the header.
GPU: the three kernels bit for bit against the restatement; the ledger in a
fresh worker; the entry points' refusals; the solve end to end against the
restatement; the output file; poisson_solve untouched; the command line.

The per-cell bound on Ham (HAM_C, in units of eps Ham_abs) is counted from the
roundings of the two expressions that cancel, with u = eps / 2 and A the sum of
the absolute terms at K = 0 (both kernels read the same lap, rho_grad, A2, rho
and powers of psi_0):

    libmgic's Ham at K = 0     the products of the four terms carry 2, 1, 3, 1
                               roundings (16 pi and 8 lap are exact), at most
                               3 u A together; its three subtractions 3 u A
    the integrand I            its products carry 3, 2, 4, 2 roundings on terms
                               1.5 times as large, at most 6 u A; its three
                               additions 4.5 u A; (2/3) of that: 7 u A
    (2/3) K^2 from I           sqrt, K * K, the product with 2/3 and the
                               rounded constants 2/3 and 1.5: 5 u |Ham| <= 5 u A
    Ham + (2/3) K^2            1 u A

19 u A = 9.5 eps A, and the corrected Ham_abs is no smaller than A.
"""
import dataclasses
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import cttk_ref as C
from tests import momentum_periodic_ref as Q
from tests import momentum_ref as R
from tests import phi_ref
from tests.test_momentum_periodic import (B_PI, EPS, K_SINE, PI_BAL, PI_UNB, POT, _cpu_inputs,
                                          _prm, mean_order_bound)
from tests.test_phi_field import PARAMS, _boxes, _shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAM_C = 10.0
KERNELS = ["k_cttk_K", "k_cttk_constraints", "k_cttk_source"]


def _psi_sine(n, amp):
    prm, lo, hi, dx, _, _ = _cpu_inputs(n, PI_BAL)
    x, y, z = phi_ref.centres(lo, hi, dx, prm.domainLength[0], grow=0)
    return np.ascontiguousarray(np.broadcast_to(1.0 + amp * np.sin(K_SINE * x) + 0.0 * (y + z),
                                                (n, n, n)))


_CPU = {}


def _cpu_case(n, pi_f=PI_BAL, amp=0.0):
    """The restatement's loop (computed once, shared, left unchanged)."""
    key = (n, pi_f.__name__, amp)
    if key not in _CPU:
        prm, _, _, _, phi_g, pi = _cpu_inputs(n, pi_f)
        _CPU[key] = C.cttk_loop(prm, n, phi_g, POT, pi, psi=_psi_sine(n, amp) if amp else None)
    return _CPU[key]


def _mom_max(d):
    return [float(np.abs(m).max()) for m in d["mom"]]


# ------------------------------------------------------------------ CPU
@pytest.mark.parametrize("n,fall", [(16, 8.0), (32, 20.0)])
def test_restatements_loop_on_the_balanced_case(n, fall):
    r = _cpu_case(n)
    steps = r["k_steps"]
    print(n, "passes", r["iterations"], "min I", min(r["min_I"]), "steps", steps)
    assert r["converged"] and min(r["min_I"]) > 0.0
    assert len(steps) == r["iterations"] >= 5
    for i in range(1, len(steps) - 1):
        assert steps[i + 1] <= 0.5 * steps[i], (i, steps)
    first, final = max(_mom_max(r["first"])), max(_mom_max(r["final"]))
    print(n, "max|Mom_i| first pass", first, "final", final, first / final)
    assert final * fall <= first
    ham, ham_abs = r["final"]["ham"], r["final"]["ham_abs"]
    print(n, "max|Ham| / max Ham_abs", float(np.abs(ham).max() / ham_abs.max()),
          "per cell, in eps", float((np.abs(ham) / ham_abs).max() / EPS))
    assert np.all(np.abs(ham) <= HAM_C * EPS * ham_abs)
    assert max(abs(v) for it in r["nets_relative"] for v in it) < 1e-12
    # the returned K belongs to the returned tensor
    prm, lo, hi, dx, phi_g, pi = _cpu_inputs(n, PI_BAL)
    I = R.nl_integrand(prm.bh(), lo, hi, dx, np.ones((n + 2,) * 3), phi_g, POT, pi,
                       [R.valid(a) for a in r["LW_g"]])
    assert np.array_equal(C.kernel_K(I)[0], r["K"])


def test_restatements_unbalanced_case_keeps_its_net_current():
    r = _cpu_case(16, PI_UNB)
    prm, lo, hi, dx, phi_g, pi = _cpu_inputs(16, PI_UNB)
    step = Q.momentum_step(prm.bh(), lo, hi, dx, np.ones((18,) * 3), phi_g, POT, pi)
    nets = [it[0] for it in r["nets"]]
    print("net current along x per pass", nets)
    assert r["converged"] and abs(step["net"][0] + 1.54e-4) < 1e-6
    for m in nets:  # D_i K sums to zero on the torus: only rounding moves the mean
        assert abs(m - step["net"][0]) <= 1e-12 * abs(step["net"][0])


def test_restatement_with_a_psi_that_varies():
    r = _cpu_case(32, PI_BAL, 0.002)
    print("psi = 1 + 0.002 sin kx: min I per pass", r["min_I"], "steps", r["k_steps"])
    assert min(r["min_I"]) > 0.0  # first, so that the case cannot hide a refusal
    assert abs(r["min_I"][0] - 9.8e-5) < 1e-6
    assert r["converged"]
    steps = r["k_steps"]
    for i in range(1, len(steps) - 1):
        assert steps[i + 1] <= 0.5 * steps[i], (i, steps)
    ham, ham_abs = r["final"]["ham"], r["final"]["ham_abs"]
    assert np.all(np.abs(ham) <= HAM_C * EPS * ham_abs)


def test_restatement_refuses_a_psi_without_a_real_K():
    with pytest.raises(C.BadCells) as e:
        _cpu_case(16, PI_BAL, 0.05)
    assert (e.value.count, e.value.iteration) == (496, 0)


def test_restated_kernels_on_their_special_values():
    I = np.array([[[4.0, 0.0, -0.0, -1.0, np.nan, np.inf, -np.inf, 2.25]]])
    K, bad = C.kernel_K(I)
    assert bad == 3 and np.array_equal(K[0, 0], [-2.0, -0.0, -0.0, 0.0, 0.0, -np.inf, 0.0, -1.5])
    assert not np.signbit(K[0, 0, 3]) and not np.signbit(K[0, 0, 4]) and np.signbit(K[0, 0, 1])


def test_deck_keys_cttk():
    from mg_ic_code_amd.params import read_params
    with open(PARAMS) as f:
        txt = f.read()
    assert "cttk" not in txt
    p = read_params(txt)
    assert (p.cttk, p.cttk_tolerance, p.cttk_max_iterations) == (0, 1e-10, 50)
    p = read_params(txt + "\ncttk = 1\ncttk_tolerance = 1e-8\ncttk_max_iterations = 7\n")
    assert (p.cttk, p.cttk_tolerance, p.cttk_max_iterations) == (1, 1e-8, 7)
    p = read_params(txt, {"cttk": "1", "cttk_tolerance": "2.5e-9", "cttk_max_iterations": "3"})
    assert (p.cttk, p.cttk_tolerance, p.cttk_max_iterations) == (1, 2.5e-9, 3)
    for key, bad in (("cttk", "2"), ("cttk", "-1"), ("cttk_tolerance", "0"),
                     ("cttk_tolerance", "-1e-3"), ("cttk_tolerance", "nan"),
                     ("cttk_tolerance", "inf"), ("cttk_max_iterations", "0"),
                     ("cttk_max_iterations", "-4")):
        with pytest.raises(ValueError, match=key):
            read_params(txt + f"\n{key} = {bad}\n")
        with pytest.raises(ValueError, match=key):
            read_params(txt, {key: bad})
    for key, bad in (("cttk", "yes"), ("cttk_tolerance", "small"), ("cttk_max_iterations", "1.5")):
        with pytest.raises(ValueError):
            read_params(txt + f"\n{key} = {bad}\n")
    # whatever its is_periodic, a deck may carry the keys
    assert read_params(txt + "\ncttk = 1\n").is_periodic == 0


def test_refusals_are_raised_before_anything_is_loaded_or_launched():
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import Matter, PiProfile, ScalarPotential, _lib, cttk_solve
    from mg_ic_code_amd.matter import MatterArgumentError
    prm = _prm(16)
    matter = Matter(ScalarPotential(), PiProfile.from_function(PI_BAL))
    loaded = (_lib.cttk_loaded(), _lib.ctt_loaded(), _lib.zm_loaded())
    ledger = mg.launch_ledger()
    with pytest.raises(ValueError, match="periodic deck"):
        cttk_solve(None, dataclasses.replace(prm, is_periodic=0), matter=matter)
    with pytest.raises(ValueError, match="one level.*hierarchies"):
        cttk_solve([None, None], prm, matter=matter)
    with pytest.raises(ValueError, match="one level"):
        cttk_solve([], prm, matter=matter)
    for kw in ({"bh1_bare_mass": 0.5}, {"bh2_momentum": -0.05}, {"bh2_spin": 0.1}):
        with pytest.raises(ValueError, match="without holes: puncture [12]"):
            cttk_solve(None, dataclasses.replace(prm, **kw), matter=matter)
    zero = [0.0, 1.0, 2.0, 3.0] + [0.0] * 6
    for col in (0, 5, 9):
        row = list(zero)
        row[col] = 0.25
        with pytest.raises(ValueError, match="without holes: puncture 2"):
            cttk_solve(None, dataclasses.replace(prm, punctures=[zero, row]), matter=matter)
    with pytest.raises(ValueError, match="psi must be a LevelData"):
        cttk_solve(None, prm, matter=matter, psi=np.ones((16, 16, 16)))
    with pytest.raises(MatterArgumentError, match="needs matter"):
        cttk_solve(None, prm)
    with pytest.raises(MatterArgumentError, match="Pi_0"):
        cttk_solve(None, prm, matter=Matter(ScalarPotential()))
    for kw in ({"tol": 0.0}, {"tol": -1.0}, {"max_iterations": 0}, {"max_iterations": 2.5}):
        with pytest.raises(ValueError, match="cttk: "):
            cttk_solve(None, prm, matter=matter, **kw)
    assert (_lib.cttk_loaded(), _lib.ctt_loaded(), _lib.zm_loaded()) == loaded
    assert mg.launch_ledger() == ledger


def test_cttk_library_loads_without_a_device_and_lists_its_three_kernels(tmp_path):
    out = tmp_path / "cttk.ledger"
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import mg_ic_code_amd as mg\n"
            "from mg_ic_code_amd import _lib, cttk, momentum\n"
            "assert not _lib.cttk_loaded() and not _lib.zm_loaded() and not _lib.ctt_loaded()\n"
            "d = cttk.cttk_launch_ledger()\n"
            "assert _lib.cttk_loaded() and not _lib.zm_loaded() and not _lib.ctt_loaded()\n"
            "assert _lib.cttk_call('mgic_cttk_launch_ledger_dump', %r) == 0\n"
            "assert d == {'k_cttk_K': 0, 'k_cttk_constraints': 0, 'k_cttk_source': 0}, d\n"
            "assert not any(n.startswith('k_cttk') for n in mg.launch_ledger())\n"
            "assert not any(n.startswith('k_cttk') for n in momentum.zm_launch_ledger())\n"
            % (ROOT, str(out).encode()))
    env = dict(os.environ, MGIC_NO_TORCH_PRELOAD="1")
    env.pop("MGIC_LAUNCH_LEDGER", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(out) as f:
        assert f.read() == "k_cttk_K\t0\nk_cttk_constraints\t0\nk_cttk_source\t0\n"


def test_binding_covers_the_cttk_header():
    from mg_ic_code_amd import _lib
    with open(os.path.join(ROOT, "include", "mgic_cttk.h")) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    names = set(re.findall(r"MGIC_CTTK_API\s+[\w\s\*]+?\b(mgic_cttk_\w+)\s*\(", txt))
    assert len(names) == 6 and names == set(_lib.CTTK_SIGNATURES)
    assert "mgic_io_write_final_data_cttk" in _lib.IO_SIGNATURES


def test_no_kernel_of_the_cttk_library_is_launched_around_its_ledger():
    for name in ("cttk.hip", "cttk_capi.cpp", "cttk.hpp"):
        with open(os.path.join(ROOT, "mg_ic_code_amd", "csrc", name)) as f:
            assert "<<<" not in f.read(), name
    with open(os.path.join(ROOT, "mg_ic_code_amd", "csrc", "cttk.hip")) as f:
        txt = f.read()
    assert txt.count("__global__") == txt.count("ledger::launch<k_cttk_") == 3
    assert "__shared__" not in txt


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def comm():
    import mg_ic_code_amd as mg
    return mg.Comm()


def _download(fields):
    return [[f.download(n, with_ghosts=True) for n in range(f.grid.num_local)] for f in fields]


def run_kernel_cases(comm):
    """The three kernels against tests/cttk_ref.py bit for bit on random fields
    whose ghosts hold arbitrary finite values, read as stored; twice, with the
    same bits; every ghost and every other field unchanged.  Shared with
    tests/cttk_worker.py.  Returns the library's ledger."""
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import cttk
    from mg_ic_code_amd.constraints import ConstraintFields
    from mg_ic_code_amd.decomposition import split_domain
    from tests.test_momentum import _random_field
    rng = np.random.default_rng(20271101)
    layouts = [((0, 0, 0, 11, 7, 15), (1, 1, 1)), ((0, 0, 0, 15, 15, 15), (1, 1, 1)),
               ((0, 0, 0, 15, 15, 15), (2, 2, 1)), ((0, 0, 0, 15, 15, 15), (2, 2, 2))]
    launches = 0
    for dom, parts in layouts:
        boxes = split_domain(dom, parts)
        dx = 100.0 / (dom[3] + 1)
        grid = mg.Grid(comm, dom, boxes, dx, periodic=(1, 1, 1))
        nb = grid.num_local
        assert nb == parts[0] * parts[1] * parts[2]
        # 0 I, 1 K, 2 psi, 3-5 S, 6 Ham, 7-9 Mom, 10 Ham_abs
        fields, arrs = map(list, zip(*[_random_field(grid, rng) for _ in range(11)]))
        for n in range(nb):  # I of either sign, with zeros, -0.0 and NaNs; psi near one
            a = arrs[0][n]
            flat = a.reshape(-1)
            flat[rng.choice(flat.size, 40, replace=False)] = np.repeat(
                [0.0, -0.0, np.nan, -1e-300], 10)
            fields[0].upload(n, a, with_ghosts=True)
            arrs[2][n][...] = 1.0 + 0.1 * arrs[2][n]
            fields[2].upload(n, arrs[2][n], with_ghosts=True)
        cf = ConstraintFields(grid)
        cf.ham, cf.mom1, cf.mom2, cf.mom3, cf.ham_abs = fields[6:11]

        def expect(which):
            want = [[a.copy() for a in per] for per in arrs]
            bad = 0
            for n in range(nb):
                if which == "K":
                    k, b = C.kernel_K(R.valid(arrs[0][n]))
                    want[1][n][1:-1, 1:-1, 1:-1] = k
                    bad += b
                elif which == "source":
                    S = C.kernel_source(R.valid(arrs[2][n]), arrs[1][n],
                                        [R.valid(arrs[3 + d][n]) for d in range(3)], dx)
                    for d in range(3):
                        want[3 + d][n][1:-1, 1:-1, 1:-1] = S[d]
                else:
                    ham, mom, ham_abs = C.kernel_constraints(
                        arrs[1][n], R.valid(arrs[6][n]),
                        [R.valid(arrs[7 + d][n]) for d in range(3)], R.valid(arrs[10][n]), dx)
                    want[6][n][1:-1, 1:-1, 1:-1] = ham
                    want[10][n][1:-1, 1:-1, 1:-1] = ham_abs
                    for d in range(3):
                        want[7 + d][n][1:-1, 1:-1, 1:-1] = mom[d]
            return want, bad

        def same(got, want, what):
            for q in range(11):
                for n in range(nb):
                    assert np.array_equal(got[q][n], want[q][n], equal_nan=True), (what, dom, parts,
                                                                                   q, n)

        for which in ("K", "source", "constraints"):
            start = [[a.copy() for a in per] for per in arrs]
            want, bad = expect(which)
            runs = []
            for rep in range(2):
                if rep:  # the same inputs again
                    for q in range(11):
                        for n in range(nb):
                            fields[q].upload(n, start[q][n], with_ghosts=True)
                if which == "K":
                    got_bad = cttk.set_K(fields[0], fields[1])
                    # the inserted NaNs and negatives, and every negative random value
                    assert got_bad == bad > 0, (got_bad, bad)
                elif which == "source":
                    cttk.add_source(fields[2], fields[1], fields[3:6])
                else:
                    cttk.correct_constraints(fields[1], cf)
                launches += 1
                runs.append(_download(fields))
                same(runs[-1], want, which)
            arrs = [[a.copy() for a in per] for per in want]
            if which == "K":  # K = 0 exactly where I is negative or NaN
                for n in range(nb):
                    I, k = R.valid(arrs[0][n]), R.valid(arrs[1][n])
                    refused = ~(I >= 0.0)
                    assert refused.any() and np.all(k[refused] == 0.0)
                    assert not np.signbit(k[refused]).any()
    return cttk.cttk_launch_ledger(), launches


@pytest.mark.gpu
def test_kernels_are_bit_identical_to_the_restatement(comm):
    from mg_ic_code_amd import cttk
    before = cttk.cttk_launch_ledger()
    after, launches = run_kernel_cases(comm)
    assert sorted(after) == KERNELS
    # one launch per call, whatever the number of boxes: 4 layouts, 2 runs each
    assert launches == 24
    for k in KERNELS:
        assert after[k] - before[k] == 8, (k, before, after)


@pytest.mark.gpu
def test_every_kernel_of_the_cttk_library_is_launched_against_its_reference(tmp_path):
    from mg_ic_code_amd.core import read_launch_ledger
    out = tmp_path / "cttk.ledger"
    env = dict(os.environ)
    env.pop("MGIC_LAUNCH_LEDGER", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cttk_worker.py"), str(out)],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, f"{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    ledger = read_launch_ledger(out)
    assert sorted(ledger) == KERNELS, ledger
    missing = sorted(n for n, c in ledger.items() if c == 0)
    assert not missing, f"{len(missing)} of {len(ledger)} kernels never launched:\n" + "\n".join(missing)


@pytest.mark.gpu
def test_entry_points_refuse_with_the_ledger_unchanged(comm):
    import ctypes

    import mg_ic_code_amd as mg
    from mg_ic_code_amd import _lib, cttk
    from mg_ic_code_amd._lib import MgicError
    from mg_ic_code_amd.constraints import ConstraintFields
    from tests.test_momentum import _random_field
    rng = np.random.default_rng(20271102)
    dom = (0, 0, 0, 7, 7, 7)
    grid = mg.Grid(comm, dom, [dom], 1.0, periodic=(1, 1, 1))
    other = mg.Grid(comm, dom, [(0, 0, 0, 7, 7, 3), (0, 0, 4, 7, 7, 7)], 1.0, periodic=(1, 1, 1))
    fields, _ = zip(*[_random_field(grid, rng) for _ in range(7)])
    alien, _ = _random_field(other, rng)
    cf = ConstraintFields(grid)
    cf.ham, cf.mom1, cf.mom2, cf.mom3, cf.ham_abs = fields[2:7]
    cttk.cttk_launch_ledger()  # loads the library
    before = (cttk.cttk_launch_ledger(), _download(fields))
    h = lambda f: f.handle
    three = lambda fs: (ctypes.c_void_p * 3)(*[f.handle.value for f in fs])
    bad = ctypes.c_longlong(-7)
    c = comm.handle
    cases = [
        ("null", "mgic_cttk_K", (c, None, h(fields[1]), ctypes.byref(bad))),
        ("null", "mgic_cttk_K", (c, h(fields[0]), None, ctypes.byref(bad))),
        ("null", "mgic_cttk_K", (c, h(fields[0]), h(fields[1]), None)),
        ("null", "mgic_cttk_K", (None, h(fields[0]), h(fields[1]), ctypes.byref(bad))),
        ("aliased", "mgic_cttk_K", (c, h(fields[0]), h(fields[0]), ctypes.byref(bad))),
        ("layout", "mgic_cttk_K", (c, h(fields[0]), h(alien), ctypes.byref(bad))),
        ("null", "mgic_cttk_source", (c, None, h(fields[1]), three(fields[2:5]))),
        ("null", "mgic_cttk_source", (c, h(fields[0]), h(fields[1]), None)),
        ("null", "mgic_cttk_source", (c, h(fields[0]), h(fields[1]),
                                      (ctypes.c_void_p * 3)(fields[2].handle.value, None,
                                                            fields[4].handle.value))),
        ("aliased", "mgic_cttk_source", (c, h(fields[0]), h(fields[1]),
                                         three([fields[2], fields[3], fields[2]]))),
        ("aliased", "mgic_cttk_source", (c, h(fields[0]), h(fields[1]),
                                         three([fields[2], fields[1], fields[4]]))),
        ("layout", "mgic_cttk_source", (c, h(fields[0]), h(alien), three(fields[2:5]))),
        ("null", "mgic_cttk_constraints", (c, None, h(fields[2]), three(fields[3:6]),
                                           h(fields[6]))),
        ("null", "mgic_cttk_constraints", (c, h(fields[1]), h(fields[2]), None, h(fields[6]))),
        ("null", "mgic_cttk_constraints", (c, h(fields[1]), h(fields[2]), three(fields[3:6]),
                                           None)),
        ("aliased", "mgic_cttk_constraints", (c, h(fields[1]), h(fields[2]), three(fields[3:6]),
                                              h(fields[2]))),
        ("aliased", "mgic_cttk_constraints", (c, h(fields[1]), h(fields[1]), three(fields[3:6]),
                                              h(fields[6]))),
        ("layout", "mgic_cttk_constraints", (c, h(fields[1]), h(fields[2]), three(fields[3:6]),
                                             h(alien))),
    ]
    for what, name, args in cases:
        with pytest.raises(MgicError, match=what) as e:
            _lib.cttk_call(name, *args)
        assert e.value.code == -1, (name, what, e.value)  # MGIC_EBADARG
    assert bad.value == -7
    after = (cttk.cttk_launch_ledger(), _download(fields))
    assert after[0] == before[0]
    for a, b in zip(after[1], before[1]):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


_GPU = {}


def _grid(comm, n, parts=(1, 1, 1)):
    import mg_ic_code_amd as mg
    from mg_ic_code_amd.decomposition import split_domain
    dom = (0, 0, 0, n - 1, n - 1, n - 1)
    return mg.Grid(comm, dom, split_domain(dom, parts), 100.0 / n, periodic=(1, 1, 1))


def _matter(pi_f):
    from mg_ic_code_amd import Matter, PiProfile, ScalarPotential
    return Matter(ScalarPotential(), PiProfile.from_function(pi_f))


def _solve(comm, n, pi_f=PI_BAL, parts=(1, 1, 1)):
    import time

    import mg_ic_code_amd as mg
    from mg_ic_code_amd.phi import PhiProfile
    key = (n, pi_f.__name__, parts)
    if key not in _GPU:
        t0 = time.perf_counter()
        _GPU[key] = mg.cttk_solve(_grid(comm, n, parts), _prm(n), matter=_matter(pi_f),
                                  phi0=PhiProfile.sine(), constraints=True, max_depth=2)
        mg.device_synchronize()
        res = _GPU[key]
        print(f"{n}^3 {pi_f.__name__} {parts}: {time.perf_counter() - t0:.2f} s, "
              f"{res.iterations} passes, BiCGStab iterations {res.momentum_iterations}")
    return _GPU[key]


def _whole(field, n, parts):
    from mg_ic_code_amd.decomposition import split_domain
    out = np.empty((n, n, n))
    for i, b in enumerate(split_domain((0, 0, 0, n - 1, n - 1, n - 1), parts)):
        out[b[2]:b[5] + 1, b[1]:b[4] + 1, b[0]:b[3] + 1] = field.download(i)
    return out


def _rep_mom(rep):
    return [rep.max_norm[f"Mom{i + 1}"] for i in range(3)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [16, 32])
def test_balanced_case_end_to_end(comm, n):
    cpu = _cpu_case(n)
    res = _solve(comm, n)
    rep = res.constraints
    print(f"{n}^3: k_max {res.k_max} k_mean {res.k_mean} steps {res.k_steps} Mom {_rep_mom(rep)} "
          f"Ham {rep.relative_ham} residuals {res.momentum_residuals[-1]}")
    assert res.converged and res.iterations <= 50
    assert len(res.k_steps) == res.iterations == len(res.momentum_iterations)
    assert all(len(its) == 4 for its in res.momentum_iterations)
    np.testing.assert_allclose([res.k_max, res.k_mean], [cpu["k_max"], cpu["k_mean"]], rtol=1e-6)
    np.testing.assert_allclose(res.k_steps[:4], cpu["k_steps"][:4], rtol=1e-6)
    np.testing.assert_allclose(_rep_mom(rep), _mom_max(cpu["final"]), rtol=1e-6)
    ham = rep.fields[0].ham.download(0)
    ham_abs = rep.fields[0].ham_abs.download(0)
    print(f"{n}^3: per-cell |Ham| / Ham_abs, in eps: {float((np.abs(ham) / ham_abs).max() / EPS)}")
    assert np.all(np.abs(ham) <= HAM_C * EPS * ham_abs)
    # nothing to carry on the balanced case
    assert max(abs(v) for it in res.momentum_net_relative for v in it) < 1e-12
    np.testing.assert_allclose([rep.max_norm_net[f"Mom{i + 1}"] for i in range(3)], _rep_mom(rep),
                               rtol=1e-9)
    # the returned K is the returned tensor's
    from mg_ic_code_amd import cttk, momentum
    from mg_ic_code_amd.phi import PhiProfile, resolve_phi0
    from mg_ic_code_amd.matter import fill_matter
    import mg_ic_code_amd as mg
    grid = res.K.grid
    prm = _prm(n)
    mat = fill_matter(_matter(PI_BAL), [grid], prm)
    phis = resolve_phi0(PhiProfile.sine(), [grid], prm)
    I, K2 = mg.LevelData(grid), mg.LevelData(grid)
    momentum.set_nl_integrand_ctt(res.psi, I, prm.bh(constant_K=0.0), mat.potential,
                                  res.momentum.lw(0), mat.level(0), None, phis[0])
    assert cttk.set_K(I, K2) == 0
    assert np.array_equal(K2.download(0), res.K.download(0))
    # K's ghost layer holds the wrapped values
    assert np.array_equal(res.K.download(0, with_ghosts=True)[1:-1, 1:-1, 0],
                          res.K.download(0)[:, :, -1])


@pytest.mark.gpu
def test_four_boxes_agree_with_one(comm):
    n, parts = 16, (2, 2, 1)
    one, four = _solve(comm, n), _solve(comm, n, parts=parts)
    assert four.converged
    np.testing.assert_allclose([four.k_max, four.k_mean], [one.k_max, one.k_mean], rtol=1e-6)
    np.testing.assert_allclose(four.k_steps[:4], one.k_steps[:4], rtol=1e-6)
    np.testing.assert_allclose(_rep_mom(four.constraints), _rep_mom(one.constraints), rtol=1e-6)
    np.testing.assert_allclose(_whole(four.K, n, parts), one.K.download(0), rtol=1e-6)
    for i in range(4):
        ham = four.constraints.fields[0].ham.download(i)
        ham_abs = four.constraints.fields[0].ham_abs.download(i)
        assert np.all(np.abs(ham) <= HAM_C * EPS * ham_abs)


@pytest.mark.gpu
def test_unbalanced_case_reports_the_net_current(comm):
    n = 16
    cpu = _cpu_case(n, PI_UNB)
    res = _solve(comm, n, PI_UNB)
    print("net", res.momentum_net, cpu["nets"])
    assert res.converged and len(res.momentum_net) == res.iterations
    smax = abs(res.momentum_net[0][0] / res.momentum_net_relative[0][0])
    for got, want in zip(res.momentum_net, cpu["nets"]):
        assert abs(got[0] - want[0]) <= mean_order_bound(n ** 3) * smax
        assert max(abs(got[1]), abs(got[2])) <= 1e-12 * smax
    assert res.constraints.momentum_net == res.momentum_net[-1]
    assert any("Mom1 + m psi_0^-6" in line for line in res.constraints.lines())


@pytest.mark.gpu
def test_a_psi_without_a_real_K_raises(comm):
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import CTTKError
    from mg_ic_code_amd.phi import PhiProfile
    n = 16
    grid = _grid(comm, n)
    psi = mg.LevelData(grid)
    psi.set_zero()
    psi.upload(0, _psi_sine(n, 0.05))
    with pytest.raises(CTTKError, match="496 cells on pass 0") as e:
        mg.cttk_solve(grid, _prm(n), matter=_matter(PI_BAL), phi0=PhiProfile.sine(), psi=psi,
                      max_depth=2)
    assert (e.value.bad_cells, e.value.iteration) == (496, 0)
    # a psi on another layout is refused before anything runs
    with pytest.raises(ValueError, match="layout of psi"):
        mg.cttk_solve(_grid(comm, n, (2, 1, 1)), _prm(n), matter=_matter(PI_BAL), psi=psi)


@pytest.mark.gpu
def test_output_carries_K_and_the_corrected_constraints(comm, tmp_path):
    import mg_ic_code_amd as mg
    from mg_ic_code_amd.output import GRCHOMBO_VARS, output_final_data
    from mg_ic_code_amd.phi import PhiProfile, resolve_phi0
    from tests import h5read
    n = 16
    grid, prm = _grid(comm, n), _prm(n)
    phis = resolve_phi0(PhiProfile.sine(), [grid], prm)
    res = mg.cttk_solve(grid, prm, matter=_matter(PI_BAL), phi0=phis, constraints=True,
                        output_dir=str(tmp_path), max_depth=2)
    got = h5read.dataset(str(tmp_path / "vcPoissonFinal.3d.hdf5"), "/level_0/data:datatype=0",
                         "<f8").reshape(31, n, n, n)
    other = str(tmp_path / "ctt.hdf5")
    output_final_data([res.psi], prm.bh(constant_K=0.0), prm.max_level, [2], other, phi=phis,
                      matter=_matter(PI_BAL), constraints=True, momentum=res.momentum)
    want = h5read.dataset(other, "/level_0/data:datatype=0", "<f8").reshape(31, n, n, n)
    assert GRCHOMBO_VARS[7] == "K" and GRCHOMBO_VARS[27:] == ("Ham", "Mom1", "Mom2", "Mom3")
    assert np.array_equal(got[7], res.K.download(0)) and np.all(want[7] == 0.0)
    for c, f in zip(range(27, 31), res.constraints.fields[0].fields()):
        assert np.array_equal(got[c], f.download(0)), c
        assert not np.array_equal(got[c], want[c]), c
    for c in range(31):
        if c != 7 and c < 27:
            assert np.array_equal(got[c], want[c]), GRCHOMBO_VARS[c]
    assert float(np.abs(got[8:14]).max()) > 0.0  # the total tensor, not zeros
    assert h5read.contents(str(tmp_path / "vcPoissonFinal.3d.hdf5")) == h5read.contents(other)


@pytest.mark.gpu
def test_poisson_solve_never_loads_the_library(tmp_path):
    code = """
import sys
sys.path.insert(0, %r)
import mg_ic_code_amd as mg
from mg_ic_code_amd import _lib
from mg_ic_code_amd.nl import poisson_solve
from mg_ic_code_amd.phi import PhiProfile
from tests import test_cttk as T
comm = mg.Comm()
res = poisson_solve(T._grid(comm, 16), T._prm(16), max_depth=2, phi0=PhiProfile.sine(),
                    matter=T._matter(T.PI_BAL), constraints=True, momentum=True,
                    zero_mode="project", max_NL_iterations=2)
assert not _lib.cttk_loaded()
assert len(res.dpsi_norms) == 2 and len(res.constant_K) == 2
assert not any("cttk" in k for k in mg.launch_ledger())
print("ok", res.constant_K)
""" % ROOT
    env = dict(os.environ)
    env.pop("MGIC_LAUNCH_LEDGER", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env,
                       timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1].startswith("ok")


@pytest.mark.gpu
def test_run_poisson_cli_cttk(comm, tmp_path):
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import Matter, PiProfile, ScalarPotential
    from mg_ic_code_amd.params import read_params
    from mg_ic_code_amd.phi import PhiProfile
    with open(PARAMS) as f:
        txt = f.read()
    for old, new in (("is_periodic = 0", "is_periodic = 1"),
                     ("bh1_bare_mass = 0.5", "bh1_bare_mass = 0.0"),
                     ("bh2_bare_mass = 0.5", "bh2_bare_mass = 0.0"),
                     ("bh1_spin = 0.1", "bh1_spin = 0.0"), ("bh2_spin = 0.1", "bh2_spin = 0.0"),
                     ("bh1_momentum = 0.05", "bh1_momentum = 0.0"),
                     ("bh2_momentum = -0.05", "bh2_momentum = 0.0")):
        assert txt.count(old) == 1, old
        txt = txt.replace(old, new)
    deck = tmp_path / "periodic.txt"
    deck.write_text(txt + "\ncttk_max_iterations = 3\n")
    prm = read_params(txt)
    n = 16
    want = mg.cttk_solve(_grid(comm, n), prm, phi0=PhiProfile.sine(), constraints=True,
                         matter=Matter(ScalarPotential(), PiProfile.constant(B_PI)), max_depth=2,
                         tol=1e-6, max_iterations=3)
    assert want.iterations == 3 and not want.converged
    tool = os.path.join(ROOT, "tools", "run_poisson.py")
    r = subprocess.run([sys.executable, tool, str(deck), "--cttk", "--cttk-tol", "1e-6", "--size",
                        "16", "--max-depth", "2", "--phi", "sine", "--pi", repr(B_PI),
                        "--constraints"], capture_output=True, text=True, timeout=300,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["cttk"]["k_steps"] == want.k_steps and out["cttk"]["iterations"] == 3
    assert (out["cttk"]["k_max"], out["cttk"]["k_mean"]) == (want.k_max, want.k_mean)
    assert out["cttk"]["max_norm"] == want.constraints.max_norm
    assert out["cttk"]["relative_ham"] == want.constraints.relative_ham
    assert out["converged"] is False
    assert out["momentum_iterations"] == want.momentum_iterations
    assert out["momentum_net"] == want.momentum_net
    assert f"CTTK K: max|K| = {want.k_max:.16e} mean = {want.k_mean:.16e}; 3 passes" in r.stdout
    for i, s in enumerate(want.k_steps):
        assert f"CTTK pass {i + 1}: max|K - K_prev| = {s:.16e}" in r.stdout
    for line in want.constraints.lines():
        assert line in r.stdout
