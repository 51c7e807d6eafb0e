"""The momentum constraint on a periodic one-level base, the zero mode projected
(mg_ic_code_amd/momentum.py, zero_mode="project").

CPU: the deck key, the refusals (raised before anything is loaded or
launched), libmgic_zm.so's ledger without a device, and the numpy restatement
(tests/momentum_periodic_ref.py): the projected system is consistent, LW stays
symmetric and trace-free, the balanced case has no net current, and the
coupled loop stays inside the caps the GPU solve is held to.  GPU: k_zm_shift
bit for bit against numpy; the ghosts of W_i and LW_ij on a periodic level of
two boxes; V_i and U against the exact inverse; the balanced and the
unbalanced case end to end; no effect on a Dirichlet base; the command line.

The two cases: params.txt made periodic with one sine period of phi_0 per
direction (tests/test_phi_field.py::_sine_case), no holes, one box, and

    balanced     Pi_0 = B (sin kx + sin ky + sin kz), k the profile's own
    unbalanced   Pi_0 = B cos kx: a net current along x of about A B k / 2

B = 0.002.  "Converged" below means the last |dpsi| is under CONVERGED times
the first.  The deck's tolerance, 1e-10, is also its BiCGStab tolerance, and
the reference's loop keeps dpsi between NL iterations: once a linear solve
finds its initial residual good enough it takes no iteration, dpsi stays, and
the volume-weighted |dpsi| (dx^1.5, L = 100) repeats at about 2e-8 for ever,
the solve without the momentum step included; that is 4e-9 of the first
|dpsi|, and what the NL loop's own criterion can never see as converged.
"""
import dataclasses
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from mg_ic_code_amd.matter import ScalarPotential
from tests import momentum_periodic_ref as Q
from tests import momentum_ref as R
from tests import phi_ref
from tests.test_momentum import KBOXES, KDOM, KDX, RELATIVE_HAM_BOUND, _random_field
from tests.test_phi_field import PARAMS, _boxes, _shape, _sine_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(float).eps)

B_PI = 0.002
K_SINE = 2.0 * np.pi * 1.0 / 100.0  # MyPhiFunction's 2 pi w / L of the sine deck
POT = (0.0, 0.0, 0.0)
CONVERGED = 1e-7

# The mean of N values summed in two different orders: each sum carries at most
# (N - 1) eps sum|f| of rounding, so the two means differ by at most 2 N eps
# max|f|.  Per unit of max|f|:
def mean_order_bound(cells):
    return 2.0 * cells * EPS


def PI_BAL(x, y, z):
    return B_PI * (np.sin(K_SINE * x) + np.sin(K_SINE * y) + np.sin(K_SINE * z))


def PI_UNB(x, y, z):
    return B_PI * np.cos(K_SINE * x) + 0.0 * (y + z)


def _prm(n):
    """The periodic sine deck with no holes, n cells a side."""
    prm, _, _ = _sine_case()
    assert (prm.is_periodic, prm.phi_wavelength, prm.L, prm.tolerance) == (1, 1.0, 100.0, 1e-10)
    return dataclasses.replace(prm, N=[n] * 3, coarsestDx=prm.L / n, max_level=0,
                               bh1_bare_mass=0.0, bh2_bare_mass=0.0, bh1_spin=0.0, bh2_spin=0.0,
                               bh1_momentum=0.0, bh2_momentum=0.0)


def _cpu_inputs(n, pi_f):
    prm = _prm(n)
    lo, hi, dx = (0, 0, 0), (n - 1,) * 3, prm.domainLength[0] / n
    phi_g = phi_ref.phi_on_box(phi_ref.sine, prm.bh(), lo, hi, dx)
    x, y, z = phi_ref.centres(lo, hi, dx, prm.domainLength[0], grow=0)
    pi = np.ascontiguousarray(np.broadcast_to(pi_f(x, y, z), (n, n, n)))
    return prm, lo, hi, dx, phi_g, pi


_CPU = {}


def _cpu_case(n, pi_f=PI_BAL):
    """The restatement's coupled loop at n^3 without and with the step (computed
    once, shared, left unchanged)."""
    key = (n, pi_f.__name__)
    if key not in _CPU:
        prm, _, _, _, phi_g, pi = _cpu_inputs(n, pi_f)
        _CPU[key] = {on: Q.coupled_solve(prm, n, 2, phi_g, POT, pi, momentum_on=on)
                     for on in (False, True)}
    return _CPU[key]


def _maxes(fields):
    return [float(np.abs(f).max()) for f in fields]


# ------------------------------------------------------------------ CPU
def test_deck_key_momentum_zero_mode():
    from mg_ic_code_amd.params import read_params
    with open(PARAMS) as f:
        txt = f.read()
    assert "momentum_zero_mode" not in txt
    assert read_params(txt).momentum_zero_mode == "refuse"
    for v in ("refuse", "project"):
        assert read_params(txt + f"\nmomentum_zero_mode = {v}\n").momentum_zero_mode == v
        assert read_params(txt, {"momentum_zero_mode": v}).momentum_zero_mode == v
    for bad in ("Project", "1", "drop"):
        with pytest.raises(ValueError, match="momentum_zero_mode.*refuse.*project"):
            read_params(txt + f"\nmomentum_zero_mode = {bad}\n")
        with pytest.raises(ValueError, match="momentum_zero_mode"):
            read_params(txt, {"momentum_zero_mode": bad})
    # whatever its is_periodic, a deck may carry the key
    assert read_params(txt + "\nmomentum_zero_mode = project\n").is_periodic == 0


def test_refusals_are_raised_before_anything_is_loaded_or_launched():
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import Matter, PiProfile, _lib
    from mg_ic_code_amd.nl import poisson_solve
    prm = _prm(16)
    matter = Matter(ScalarPotential(), PiProfile.from_function(PI_BAL))
    loaded = (_lib.ctt_loaded(), _lib.zm_loaded())
    ledger = mg.launch_ledger()
    # the default on a periodic base: today's message
    for kw in ({}, {"zero_mode": "refuse"}, {"zero_mode": None}):
        with pytest.raises(ValueError, match="periodic.*sum S_i = 0"):
            poisson_solve(None, prm, matter=matter, momentum=True, **kw)
    # a bad value, with or without the momentum solve, from the keyword or the deck
    for kw in ({"momentum": True}, {}):
        with pytest.raises(ValueError, match="'refuse' or 'project'"):
            poisson_solve(None, prm, matter=matter, zero_mode="drop", **kw)
    with pytest.raises(ValueError, match="'refuse' or 'project'"):
        poisson_solve(None, dataclasses.replace(prm, momentum_zero_mode="yes"), matter=matter,
                      momentum=True)
    # project on a periodic hierarchy, from the keyword or the deck
    with pytest.raises(ValueError, match="periodic hierarchy.*no refluxing.*sum to zero"):
        poisson_solve([None, None], prm, matter=matter, momentum=True, zero_mode="project")
    with pytest.raises(ValueError, match="periodic hierarchy"):
        poisson_solve([None, None], dataclasses.replace(prm, momentum_zero_mode="project"),
                      matter=matter, momentum=True)
    assert (_lib.ctt_loaded(), _lib.zm_loaded()) == loaded
    assert mg.launch_ledger() == ledger


def test_zm_library_loads_without_a_device_and_lists_its_two_kernels(tmp_path):
    out = tmp_path / "zm.ledger"
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import mg_ic_code_amd as mg\n"
            "from mg_ic_code_amd import _lib, momentum\n"
            "assert not _lib.zm_loaded() and not _lib.ctt_loaded()\n"
            "d = momentum.zm_launch_ledger()\n"
            "assert _lib.zm_loaded() and not _lib.ctt_loaded()\n"
            "assert _lib.zm_call('mgic_zm_launch_ledger_dump', %r) == 0\n"
            "assert d == {'k_zm_shift<1>': 0, 'k_zm_shift<3>': 0}, d\n"
            "assert not any(n.startswith('k_zm') for n in mg.launch_ledger())\n"
            "assert not any(n.startswith('k_zm') for n in momentum.ctt_launch_ledger())\n"
            % (ROOT, str(out).encode()))
    env = dict(os.environ, MGIC_NO_TORCH_PRELOAD="1")
    env.pop("MGIC_LAUNCH_LEDGER", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(out) as f:
        assert f.read() == "k_zm_shift<1>\t0\nk_zm_shift<3>\t0\n"


def test_binding_covers_the_zm_header():
    from mg_ic_code_amd import _lib
    with open(os.path.join(ROOT, "include", "mgic_zm.h")) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    names = set(re.findall(r"MGIC_ZM_API\s+[\w\s\*]+?\b(mgic_zm_\w+)\s*\(", txt))
    assert len(names) == 4 and names == set(_lib.ZM_SIGNATURES)


def test_no_kernel_of_the_zm_library_is_launched_around_its_ledger():
    for name in ("zm.hip", "zm_capi.cpp", "zm.hpp"):
        with open(os.path.join(ROOT, "mg_ic_code_amd", "csrc", name)) as f:
            assert "<<<" not in f.read(), name
    with open(os.path.join(ROOT, "mg_ic_code_amd", "csrc", "zm.hip")) as f:
        assert f.read().count("ledger::launch<k_zm_shift<N>>") == 1


def test_restatements_projected_system_is_consistent():
    """The removed mean plus the Laplacian of the solved part reproduces S_i
    (and U's right-hand side), the solutions have mean zero, and LW stays
    symmetric and trace-free -- on the unbalanced case, whose mean is not
    small."""
    n = 16
    prm, lo, hi, dx, phi_g, pi = _cpu_inputs(n, PI_UNB)
    psi_g = np.ones((n + 2,) * 3)
    step = Q.momentum_step(prm.bh(), lo, hi, dx, psi_g, phi_g, POT, pi)
    assert abs(step["net_relative"][0]) > 0.1  # about A B k / 2 * 8 pi G against max|S_x|
    # the FFT pair and the 13 flops of the stencil per cell: a few tens of eps
    tol = 64 * EPS
    for i in range(3):
        S, V = step["S"][i], step["V"][i]
        assert np.abs(step["net"][i] + Q.laplacian(V, dx) - S).max() <= tol * np.abs(S).max()
        assert abs(Q.mean(V)) <= tol * np.abs(V).max()
    rhs_u = R.div_rhs([Q.pad_wrap(v) for v in step["V"]], dx)
    assert np.abs(step["u_mean"] + Q.laplacian(step["U"], dx) - rhs_u).max() <= tol * np.abs(rhs_u).max()
    assert abs(Q.mean(step["U"])) <= tol * np.abs(step["U"]).max()
    # a centred difference of a periodic field sums to zero up to rounding
    assert abs(step["u_mean"]) <= tol * np.abs(rhs_u).max()
    LW = [R.valid(a) for a in step["LW_g"]]
    size = max(_maxes(LW))
    assert size > 1e-6
    assert float(np.abs(LW[0] + LW[3] + LW[5]).max()) <= 8 * EPS * size
    Wg = [Q.pad_wrap(a) for a in step["W"]]
    for c, (i, j) in ((1, (0, 1)), (2, (0, 2)), (4, (1, 2))):
        assert np.array_equal(LW[c], R.cdiff(Wg[i], j, dx) + R.cdiff(Wg[j], i, dx))
    # the wrapped ghosts are the opposite side's valid cells, edges and corners too
    g = step["LW_g"][1]
    assert np.array_equal(g[0, 1:-1, 1:-1], LW[1][-1]) and np.array_equal(g[-1, 1:-1, 1:-1], LW[1][0])
    assert g[0, 0, 0] == LW[1][-1, -1, -1]


def test_balanced_case_has_no_net_current_on_the_restatement():
    """A condition on the choice of input, not a measurement: Pi d_i phi is odd
    under the reflection that leaves phi, Pi, rho and so psi unchanged."""
    for n in (16, 32):
        r = _cpu_case(n)[True]
        assert len(r["nets_relative"]) == len(r["norms"])
        worst = max(abs(v) for it in r["nets_relative"] for v in it)
        print(n, "balanced: worst |momentum_net_relative|", worst)
        assert worst < 1e-12


def _assert_converged(norms):
    assert norms[-1] <= CONVERGED * norms[0], norms


def _assert_caps(at16, at32):
    """at[on] = max|Mom_i| over i.  The restatement gives, for every i,
        without / with at 16^3:   24.0    (cap: at least 20)
        the same at 32^3:         101.3   (cap: at least 85)
        with, 16^3 over 32^3:     4.008   (cap: at least 3.4)
    the caps below the measured values by the margin of test_momentum's."""
    for i in range(3):
        assert at16[True][i] <= at16[False][i] / 20.0, (i, at16)
        assert at32[True][i] <= at32[False][i] / 85.0, (i, at32)
        assert at32[True][i] <= at16[True][i] / 3.4, (i, at16, at32)


def test_restatements_coupled_loop_stays_inside_the_caps():
    """The amplitude is small enough for the oracle's periodic solve without the
    momentum step to converge (and with it); the caps of _assert_caps; max|Ham|
    / max Ham_abs of 1.3e-9 and 9.0e-10 without, 4.9e-10 and 1.4e-10 with."""
    got = {}
    for n in (16, 32):
        c = _cpu_case(n)
        for on in (False, True):
            _assert_converged(c[on]["norms"])
            assert float(np.abs(c[on]["ham"]).max() / c[on]["ham_abs"].max()) < RELATIVE_HAM_BOUND
            # balanced: nothing is removed, so nothing is subtracted
            np.testing.assert_allclose(_maxes(c[on]["mom_net"]), _maxes(c[on]["mom"]), rtol=1e-9)
        got[n] = {on: _maxes(c[on]["mom"]) for on in (False, True)}
        # K moves with the total tensor
        assert abs(c[True]["ks"][-1] / c[False]["ks"][-1] - 1.0) > 1e-3
    print("16^3", got[16], "32^3", got[32])
    _assert_caps(got[16], got[32])


# what the unbalanced case is held to at 16^3 (the restatement: 15.2, 26.5, 26.5
# for max|Mom_i| without over max|Mom_i + m_i psi_0^-6| with; raw max|Mom_x| with
# is 8.9 times max|Mom_x + m_x psi_0^-6|)
UNB_CAPS = (12.5, 22.0, 22.0)


def _assert_unbalanced(off, on, on_net, m_x, psi6inv_max):
    for i in range(3):
        assert on_net[i] <= off[i] / UNB_CAPS[i], (i, off, on_net)
    # Mom_x = -m_x psi_0^-6 + (Mom_x + m_x psi_0^-6): the raw violation is the
    # offset to within what is left after subtracting it, and dominates it
    assert abs(on[0] - abs(m_x) * psi6inv_max) <= on_net[0], (on, m_x, psi6inv_max, on_net)
    assert on[0] >= 5.0 * on_net[0] and on[0] >= 0.5 * off[0], (off, on, on_net)


def test_restatements_unbalanced_case():
    c = _cpu_case(16, PI_UNB)
    for on in (False, True):
        _assert_converged(c[on]["norms"])
    m = c[True]["nets"][-1]
    # A B k / 2 times 8 pi G, psi_0^6 of order one
    assert 0.5 < abs(m[0]) / (8.0 * np.pi * 0.1 * B_PI * K_SINE / 2.0) < 2.0
    assert max(abs(v) for it in c[True]["nets_relative"] for v in it[1:]) < 1e-12
    _assert_unbalanced(_maxes(c[False]["mom"]), _maxes(c[True]["mom"]), _maxes(c[True]["mom_net"]),
                       m[0], float(c[True]["psi6inv"].max()))


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def comm():
    import mg_ic_code_amd as mg
    return mg.Comm()


def run_kernel_cases(comm):
    """k_zm_shift<1> and <3> on the two-box level of tests/test_momentum.py
    against numpy's f - c, bit for bit, ghosts included (every ghost and every
    other field stays as it was).  Shared with tests/zm_worker.py."""
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import momentum as mom
    rng = np.random.default_rng(20271001)
    grid = mg.Grid(comm, KDOM, KBOXES, KDX, patches=True)
    assert [_shape(b) for b in _boxes(grid)] == [(8, 10, 12), (6, 10, 12)]
    fields, arrs = zip(*[_random_field(grid, rng) for _ in range(5)])

    def check(shifted, consts, step):
        for q, f in enumerate(fields):
            for n in range(grid.num_local):
                want = arrs[q][n]
                if q in shifted:
                    want = want.copy()
                    want[1:-1, 1:-1, 1:-1] = R.valid(want) - consts[shifted.index(q)]
                    arrs[q][n][...] = want
                assert np.array_equal(f.download(n, with_ghosts=True), want), (step, q, n)

    for consts in ([0.0, -0.37, 0.625], [1e-3, 0.0, -2.5]):
        mom.shift(comm, [fields[0], fields[2], fields[3]], consts)
        check([0, 2, 3], consts, ("<3>", consts))
    for q, c in ((1, 0.0), (1, -0.75), (4, 0.1)):
        mom.shift(comm, [fields[q]], [c])
        check([q], [c], ("<1>", q, c))
    # two fields, an aliased field: refused by the library, nothing written
    from mg_ic_code_amd._lib import MgicError
    with pytest.raises(MgicError, match="1 or 3"):
        mom.shift(comm, [fields[0], fields[1]], [1.0, 1.0])
    with pytest.raises(MgicError, match="aliased"):
        mom.shift(comm, [fields[0], fields[1], fields[0]], [1.0, 1.0, 1.0])
    check([], [], "refused")
    return mom.zm_launch_ledger()


@pytest.mark.gpu
def test_shift_kernels_are_bit_identical_to_numpy(comm):
    from mg_ic_code_amd import momentum as mom
    before = mom.zm_launch_ledger()
    after = run_kernel_cases(comm)
    assert sorted(after) == ["k_zm_shift<1>", "k_zm_shift<3>"]
    # two boxes per call: 2 calls of <3>, 3 of <1>
    assert after["k_zm_shift<3>"] - before["k_zm_shift<3>"] == 4
    assert after["k_zm_shift<1>"] - before["k_zm_shift<1>"] == 6


@pytest.mark.gpu
def test_every_kernel_of_the_zm_library_is_launched_against_its_reference(tmp_path):
    from mg_ic_code_amd.core import read_launch_ledger
    out = tmp_path / "zm.ledger"
    env = dict(os.environ)
    env.pop("MGIC_LAUNCH_LEDGER", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "zm_worker.py"), str(out)],
                       capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, f"{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    ledger = read_launch_ledger(out)
    assert sorted(ledger) == ["k_zm_shift<1>", "k_zm_shift<3>"], ledger
    missing = sorted(n for n, c in ledger.items() if c == 0)
    assert not missing, f"{len(missing)} of {len(ledger)} kernels never launched:\n" + "\n".join(missing)


def _solver(comm, n, boxes=None):
    """(prm, grid, MomentumSolver with the projection on, bh, filled matter of
    the balanced case, stored phi_0) as poisson_solve builds them."""
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import Matter, PiProfile
    from mg_ic_code_amd.core import OperatorParams, SolverParams
    from mg_ic_code_amd.matter import fill_matter
    from mg_ic_code_amd.momentum import MomentumSolver
    from mg_ic_code_amd.phi import PhiProfile, resolve_phi0
    prm = _prm(n)
    dom = (0, 0, 0, n - 1, n - 1, n - 1)
    grid = mg.Grid(comm, dom, boxes or [dom], prm.domainLength[0] / n, periodic=(1, 1, 1))
    op = OperatorParams(alpha=prm.alpha, beta=prm.beta, bc_lo=tuple(prm.bc_lo),
                        bc_hi=tuple(prm.bc_hi), bc_value=prm.bc_value,
                        coefficient_average_type=prm.coefficient_average_type, prolong_type=1,
                        relax_mode=1)
    sp = SolverParams(max_depth=2, n_pre=prm.numMGsmooth, n_post=prm.numMGsmooth,
                      n_bottom=prm.numMGsmooth, bottom_solver=1)
    ms = MomentumSolver([grid], prm, op, sp, "project")
    assert ms.project
    mat = fill_matter(Matter(ScalarPotential(), PiProfile.from_function(PI_BAL)), [grid], prm)
    phis = resolve_phi0(PhiProfile.sine(), [grid], prm)
    return prm, grid, ms, prm.bh(constant_K=0.0), mat, phis


@pytest.mark.gpu
def test_ghosts_on_a_periodic_level_of_two_boxes_are_the_wrapped_values(comm):
    """Two boxes split in z: after set_longitudinal the ghost layer of W_i and
    LW_ij across every face (the periodic x and y faces of each box, the face
    between the boxes, the periodic z face) equals the wrapped valid values
    bit for bit, and k_ctt_extrap was not launched."""
    from mg_ic_code_amd import momentum as mom
    n = 16
    boxes = [(0, 0, 0, n - 1, n - 1, 7), (0, 0, 8, n - 1, n - 1, n - 1)]
    _, grid, ms, _, _, _ = _solver(comm, n, boxes)
    rng = np.random.default_rng(20271002)
    mf = mom.MomentumFields([grid])
    for f in mf.V[0] + [mf.U[0]] + mf.W[0] + mf.LW[0]:
        for b_n, b in enumerate(_boxes(grid)):
            f.upload(b_n, rng.uniform(-1, 1, _shape(b, 1)), with_ghosts=True)
    before = mom.ctt_launch_ledger()
    mom.set_longitudinal(ms, mf)
    after = mom.ctt_launch_ledger()
    assert after["k_ctt_extrap"] == before["k_ctt_extrap"]
    assert after["k_ctt_w"] == before["k_ctt_w"] + 2 and after["k_ctt_lw"] == before["k_ctt_lw"] + 2

    def faces(x):
        return [x[0, 1:-1, 1:-1], x[-1, 1:-1, 1:-1], x[1:-1, 0, 1:-1], x[1:-1, -1, 1:-1],
                x[1:-1, 1:-1, 0], x[1:-1, 1:-1, -1]]

    for f in mf.W[0] + mf.LW[0]:
        got = [f.download(b_n, with_ghosts=True) for b_n in range(2)]
        whole = Q.pad_wrap(np.concatenate([R.valid(g) for g in got], axis=0))
        for g, (k0, k1) in zip(got, ((0, 8), (8, 16))):
            want = whole[k0:k1 + 2]
            assert np.array_equal(R.valid(g), R.valid(want))
            for a, b in zip(faces(g), faces(want)):
                assert np.array_equal(a, b)
    # LW is the restatement's from those W
    Wg = [Q.pad_wrap(np.concatenate([f.download(b_n) for b_n in range(2)], axis=0)) for f in mf.W[0]]
    for c, want in enumerate(R.lw(Wg, grid.dx)):
        got = np.concatenate([mf.LW[0][c].download(b_n) for b_n in range(2)], axis=0)
        assert np.array_equal(got, want), c


def _oracle_solve(prm, n, rhs, parts=(1, 1, 1)):
    """The issue's probe on the oracle: one periodic level, alpha aCoef = 0,
    bCoef = 1, the deck's outer solve from a guess of zero.  (iterations, the
    solution with its mean removed)."""
    import oracle
    from mg_ic_code_amd.decomposition import split_domain
    dom = (0, 0, 0, n - 1, n - 1, n - 1)
    boxes = split_domain(dom, parts)
    o = oracle.OracleMG(boxes, dom, prm.domainLength[0] / n, alpha=prm.alpha, beta=prm.beta,
                        periodic=(1, 1, 1), nlevels=3, avg_type=prm.coefficient_average_type,
                        prolong_type=1, bottom_solver=1, n_pre=prm.numMGsmooth,
                        n_post=prm.numMGsmooth, n_bottom=prm.numMGsmooth)
    cut = [np.s_[b[2]:b[5] + 1, b[1]:b[4] + 1, b[0]:b[3] + 1] for b in boxes]
    for bi, s in enumerate(cut):
        o.set(0, oracle.ACOEF, bi, np.zeros_like(rhs[s]))
        o.set(0, oracle.BCOEF, bi, np.ones_like(rhs[s]))
        o.set(0, oracle.RHS, bi, -prm.beta * rhs[s])
        o.set(0, oracle.PHI, bi, np.zeros_like(rhs[s]))
    o.setup()
    it, _ = o.solve(mg_iters=prm.numMGIterations, imax=prm.max_iterations, eps=prm.tolerance,
                    norm_type=0)
    u = np.zeros_like(rhs)
    for bi, s in enumerate(cut):
        u[s] = o.get(0, oracle.PHI, bi)
    return it, u - Q.mean(u)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [16, 32])
def test_first_iterations_potentials_against_the_exact_inverse(comm, n):
    """V_i and U of the first NL iteration of the balanced case (psi = 1, guesses
    of zero) against the FFT inverse of the device's own projected right-hand
    sides.  The oracle's BiCGStab on the same right-hand sides at the same
    tolerance sets the scale: the device may exceed its relative max error by
    at most 10 times (the allowance for another reduction order); its iteration
    count is one the oracle takes on one of its decompositions, which change
    only the order of its reductions (tests/bicg_cases.py)."""
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import momentum as mom
    prm, grid, ms, bh, mat, phis = _solver(comm, n)
    psi = mg.LevelData(grid)
    psi.set_val_all(1.0)
    mf = mom.MomentumFields([grid])
    mom.momentum_source(psi, ms.rhs[0], bh, mat.potential, mat.level(0), None, phis[0])
    S = [f.download(0) for f in ms.rhs[0]]
    its = ms.solve_three([[mf.V[0][i]] for i in range(3)], [[ms.rhs[0][i]] for i in range(3)])
    net = ms.removed[:3]
    cases = [(f"V{i + 1}", ms.rhs[0][i].download(0), mf.V[0][i].download(0), its[i]) for i in range(3)]
    # the means of S_i the device removed are numpy's, to the order of summation
    for i in range(3):
        assert abs(net[i] - Q.mean(S[i])) <= mean_order_bound(n ** 3) * np.abs(S[i]).max()
        assert np.array_equal(cases[i][1], S[i] - net[i])
    mom.div_rhs(comm, mf.V[0], ms.rhs[0][0])
    it_u = ms.solve([mf.U[0]], [ms.rhs[0][0]])
    cases.append(("U", ms.rhs[0][0].download(0), mf.U[0].download(0), it_u))
    assert len(ms.removed) == 4
    for name, rhs, got, it in cases:
        exact, left = Q.solve_periodic(rhs, grid.dx)
        scale = float(np.abs(exact).max())
        assert scale > 0.0
        # the projected right-hand side sums to zero, the solution too
        assert abs(left) <= mean_order_bound(n ** 3) * np.abs(rhs).max(), (name, left)
        mean_ulps = abs(Q.mean(got)) / (EPS * float(np.abs(got).max()))
        runs = {p: _oracle_solve(prm, n, rhs, p) for p in ((1, 1, 1), (2, 2, 2), (2, 1, 1), (1, 2, 4))}
        err_o = float(np.abs(runs[1, 1, 1][1] - exact).max()) / scale
        err_d = float(np.abs(got - exact).max()) / scale
        counts = sorted({r[0] for r in runs.values()})
        print(f"{n}^3 {name}: relative max error device {err_d:.3e} oracle {err_o:.3e}; "
              f"iterations device {it} oracle {counts}; |mean| {mean_ulps:.2f} ulp of max|f|")
        assert err_d <= 10.0 * err_o, (name, err_d, err_o)
        assert it in counts, (name, it, counts)
        assert mean_ulps <= 4.0, (name, mean_ulps)


_GPU = {}


def _solve(comm, n, pi_f, momentum):
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import Matter, PiProfile
    from mg_ic_code_amd.nl import poisson_solve
    from mg_ic_code_amd.phi import PhiProfile
    key = (n, pi_f.__name__, momentum)
    if key not in _GPU:
        prm = _prm(n)
        dom = (0, 0, 0, n - 1, n - 1, n - 1)
        grid = mg.Grid(comm, dom, [dom], prm.domainLength[0] / n, periodic=(1, 1, 1))
        kw = dict(momentum=True, zero_mode="project") if momentum else {}
        _GPU[key] = poisson_solve(grid, prm, max_depth=2, phi0=PhiProfile.sine(),
                                  matter=Matter(ScalarPotential(), PiProfile.from_function(pi_f)),
                                  constraints=True, **kw)
    return _GPU[key]


def _mom(rep, which="max_norm"):
    return [getattr(rep, which)[f"Mom{i + 1}"] for i in range(3)]


@pytest.mark.gpu
def test_balanced_case_end_to_end(comm):
    """The caps of test_restatements_coupled_loop_stays_inside_the_caps on the
    device's own solve and report; max|Mom_i| and K per iteration against the
    restatement at 1e-6, the bar of the Dirichlet test and of the periodic
    sine solve; max|Ham| / max Ham_abs under the bound of a converged solve
    and within ten times the solve's without the step."""
    got = {}
    for n in (16, 32):
        cpu = _cpu_case(n)
        got[n] = {}
        for on in (False, True):
            res = _solve(comm, n, PI_BAL, on)
            rep = res.constraints
            print(f"{n}^3 on={on}: |dpsi| {res.dpsi_norms} K {res.constant_K} Mom {_mom(rep)} "
                  f"Ham {rep.relative_ham} net {res.momentum_net_relative}")
            _assert_converged(res.dpsi_norms)
            got[n][on] = _mom(rep)
            np.testing.assert_allclose(got[n][on], _maxes(cpu[on]["mom"]), rtol=1e-6)
            assert len(res.constant_K) == len(res.dpsi_norms) <= len(cpu[on]["ks"])
            np.testing.assert_allclose(res.constant_K, cpu[on]["ks"][:len(res.constant_K)], rtol=1e-6)
        off, on = (_solve(comm, n, PI_BAL, k) for k in (False, True))
        assert on.constraints.relative_ham < RELATIVE_HAM_BOUND
        assert on.constraints.relative_ham <= 10.0 * off.constraints.relative_ham
        # nothing to carry: nothing removed, nothing subtracted
        assert len(on.momentum_net) == len(on.momentum_net_relative) == len(on.dpsi_norms)
        assert max(abs(v) for it in on.momentum_net_relative for v in it) < 1e-12
        np.testing.assert_allclose(_mom(on.constraints, "max_norm_net"), got[n][True], rtol=1e-9)
        assert off.momentum_net == [] and off.constraints.max_norm_net == {}
        assert all(len(its) == 4 for its in on.momentum_iterations)
        assert all(v >= 1 for v in on.momentum_iterations[0])
    _assert_caps(got[16], got[32])


@pytest.mark.gpu
def test_unbalanced_case_reports_what_the_torus_cannot_carry(comm):
    n = 16
    cpu = _cpu_case(n, PI_UNB)
    off, on = (_solve(comm, n, PI_UNB, k) for k in (False, True))
    for res in (off, on):
        _assert_converged(res.dpsi_norms)
    print("net", on.momentum_net, cpu[True]["nets"], "Mom", _mom(off.constraints),
          _mom(on.constraints), _mom(on.constraints, "max_norm_net"))
    # momentum_net: the restatement's, per iteration; S_x moves with psi, which
    # the two loops agree on to the solvers' tolerance (1e-6, as above)
    smax = abs(on.momentum_net[0][0] / on.momentum_net_relative[0][0])
    for got, want in zip(on.momentum_net, cpu[True]["nets"]):
        assert abs(got[0] - want[0]) <= 1e-6 * abs(want[0])
        assert max(abs(got[1]), abs(got[2])) <= 1e-12 * smax
    # the first iteration is at psi = 1 on both sides: only the order of the sum differs
    assert abs(on.momentum_net[0][0] - cpu[True]["nets"][0][0]) <= mean_order_bound(n ** 3) * smax
    rep = on.constraints
    assert rep.momentum_net == on.momentum_net[-1]
    np.testing.assert_allclose(_mom(rep, "max_norm_net"), _maxes(cpu[True]["mom_net"]), rtol=1e-6)
    np.testing.assert_allclose(_mom(rep), _maxes(cpu[True]["mom"]), rtol=1e-6)
    psi6inv_max = float((on.psi.download(0) ** -6.0).max())
    _assert_unbalanced(_mom(off.constraints), _mom(rep), _mom(rep, "max_norm_net"),
                       rep.momentum_net[0], psi6inv_max)
    assert any("Mom1 + m psi_0^-6" in line for line in rep.lines())


@pytest.mark.gpu
def test_project_changes_nothing_on_a_dirichlet_base(comm, tmp_path):
    # in a fresh process: the 16^3 no-holes momentum solve of tests/test_momentum.py
    # as it is, with zero_mode="project" and with the deck's key: one solve (psi
    # bits, iteration counts, both ledgers' counts), libmgic_zm.so never loaded
    code = """
import sys
sys.path.insert(0, %r)
import dataclasses
import numpy as np
import mg_ic_code_amd as mg
from mg_ic_code_amd import _lib, momentum
from mg_ic_code_amd.nl import poisson_solve
from tests import test_momentum as T
comm = mg.Comm()
dom = (0, 0, 0, 15, 15, 15)
runs = []
for how in ("plain", "keyword", "deck"):
    mg.launch_ledger_reset()
    if _lib.ctt_loaded():
        _lib.ctt_call("mgic_ctt_launch_ledger_reset")
    prm, kw = T._prm(16), {}
    if how == "keyword":
        kw = dict(zero_mode="project")
    if how == "deck":
        prm = dataclasses.replace(prm, momentum_zero_mode="project")
    res = poisson_solve(mg.Grid(comm, dom, [dom], T.L / 16), prm, max_depth=2, matter=T._matter(),
                        constraints=True, momentum=True, **kw)
    runs.append((res.psi.download(0, with_ghosts=True), res.linear_iterations, res.dpsi_norms,
                 res.momentum_iterations, mg.launch_ledger(), momentum.ctt_launch_ledger(),
                 res.momentum_net, res.constraints.max_norm, res.constraints.max_norm_net))
    assert not _lib.zm_loaded(), how
for r in runs[1:]:
    assert np.array_equal(r[0], runs[0][0]) and r[1:] == runs[0][1:]
assert runs[0][1] and sum(runs[0][4].values()) > 0 and sum(runs[0][5].values()) > 0
assert runs[0][6] == [] and runs[0][8] == {}
print("ok", runs[0][1], runs[0][3])
""" % ROOT
    env = dict(os.environ)
    env.pop("MGIC_LAUNCH_LEDGER", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env,
                       timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().startswith("ok")


@pytest.mark.gpu
def test_run_poisson_cli_momentum_zero_mode(comm, tmp_path):
    # the periodic sine deck without holes at 16^3, a constant Pi: the flag gives
    # the in-process solve, the removed means printed next to the momentum solve
    # counts and in the JSON line (the deck's key: the CPU tests and the
    # Dirichlet case above)
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import Matter, PiProfile
    from mg_ic_code_amd.nl import poisson_solve
    from mg_ic_code_amd.params import read_params
    from mg_ic_code_amd.phi import PhiProfile
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
    tool = os.path.join(ROOT, "tools", "run_poisson.py")
    common = ["--momentum", "--size", "16", "--max-depth", "2", "--phi", "sine", "--pi",
              repr(B_PI), "--constraints"]
    prm = read_params(txt)
    n = 16
    dom = (0, 0, 0, n - 1, n - 1, n - 1)
    grid = mg.Grid(comm, dom, [dom], prm.domainLength[0] / n, periodic=(1, 1, 1))
    want = poisson_solve(grid, prm, max_depth=2, phi0=PhiProfile.sine(), constraints=True,
                         matter=Matter(ScalarPotential(), PiProfile.constant(B_PI)),
                         momentum=True, zero_mode="project")
    assert len(want.momentum_net) == 2
    r = subprocess.run([sys.executable, tool, str(deck), "--momentum-zero-mode", "project"] + common,
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["momentum_net"] == want.momentum_net
    assert out["momentum_net_relative"] == want.momentum_net_relative
    assert out["momentum_iterations"] == want.momentum_iterations
    assert out["dpsi_norms"] == want.dpsi_norms and out["constant_K"] == want.constant_K
    lines = [l for l in r.stdout.splitlines() if "momentum solves V1 V2 V3 U:" in l]
    assert len(lines) == 2
    for line, net in zip(lines, want.momentum_net):
        assert "removed means of S1 S2 S3: " + " ".join(f"{m:.16e}" for m in net) in line
    assert r.stdout.count("+ m psi_0^-6") == 3
