"""The momentum constraint solved by the conformal transverse-traceless step
(mg_ic_code_amd/momentum.py).

CPU: the deck key, the three refusals (raised before anything is loaded or
launched), the numpy restatement's own consistency (tests/momentum_ref.py),
libmgic_ctt.so's ledger without a device, and the restatement's coupled loop
against the caps the GPU solve is held to.  GPU: the four kernels bit for bit
against numpy; the *_ctt consumers against the *_matter ones (fields of
zeros) and against the restatement (random fields); the solve with and
without `momentum`, on one level, on a hierarchy and with holes.
"""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

from mg_ic_code_amd.matter import MatterArgumentError, ScalarPotential
from tests import constraints_ref as C
from tests import h5read
from tests import momentum_ref as R
from tests import phi_ref
from tests import puncture_ref as P
from tests.test_matter import BH_M, PI_F, POT, SP, _of_max, _rel
from tests.test_phi_field import L, PARAMS, _boxes, _shape
from tests.test_punctures import SMALL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# a converged solve's max|Ham| / max Ham_abs: below the 1.3e-7 DESIGN.md 3j
# records for a solve stopped after two NL iterations (a converged one must do
# better than that); the restatement's coupled loop gives 5e-12 to 8e-12
RELATIVE_HAM_BOUND = 1e-7

# the kernels' level: two boxes of 12x10x8 and 12x10x6 stacked in z on a
# domain whose low corner is not the boxes'.  z-lo of the first and z-hi of
# the second are domain faces, as is x-hi of both; x-lo and both y faces lie
# inside the domain; the face between the boxes is an exchange face
KDOM = (0, 0, 0, 13, 12, 13)
KBOXES = [(2, 1, 0, 13, 10, 7), (2, 1, 8, 13, 10, 13)]
KDX = L / 14


def PHI_0(x, y, z):
    return 0.1 * np.exp(-(x * x + y * y + z * z) / 8.0)


def PI_0(x, y, z):
    return 0.05 * np.exp(-((x - 1.0) ** 2 + (y + 0.5) ** 2 + z * z) / 12.5)


# the same two profiles stretched into the deck's own box of length 100 (the
# case with the deck's holes), Pi_0 at 0.004: aCoef's 10 pi G Pi^2 psi_0^4 has
# to stay below the Dirichlet Laplacian's lowest eigenvalue, 3 pi^2 / L^2 =
# 3e-3 there, for the NL loop to converge, and 0.05 does not
STRETCH = 100.0 / L


def PI_DECK(x, y, z):
    return 0.08 * PI_0(x / STRETCH, y / STRETCH, z / STRETCH)


def _prm(n, holes=False):
    """No holes: params.txt in the box of length 16 with n cells a side, bare
    masses, momenta and spins 0, the wide Gaussian phi_0 above as the deck's
    own (phi_wavelength = 8).  holes: params.txt itself, its two holes in its
    box of length 100, n cells a side, the same Gaussian stretched into it."""
    from mg_ic_code_amd.params import read_params_file
    prm = read_params_file(PARAMS)
    assert (prm.alpha, prm.beta, prm.is_periodic, prm.max_NL_iterations) == (1.0, -1.0, 0, 6)
    assert (prm.L, prm.G_Newton, prm.phi_amplitude) == (100.0, 1.0, 0.1)
    if holes:
        return dataclasses.replace(prm, N=[n] * 3, coarsestDx=prm.L / n, max_level=0,
                                   phi_wavelength=8.0 * STRETCH * STRETCH)
    return dataclasses.replace(prm, L=L, N=[n] * 3, coarsestDx=L / n, domainLength=[L] * 3,
                               max_level=0, phi_wavelength=8.0, bh1_bare_mass=0.0,
                               bh2_bare_mass=0.0, bh1_spin=0.0, bh2_spin=0.0, bh1_momentum=0.0,
                               bh2_momentum=0.0)


def _rows(table):
    return [[float(v) for v in r] for r in P.as_table(table)]


# ------------------------------------------------------------------ CPU
def test_deck_key_solve_momentum():
    from mg_ic_code_amd.params import read_params
    with open(PARAMS) as f:
        txt = f.read()
    assert "solve_momentum" not in txt
    assert read_params(txt).solve_momentum == 0
    assert read_params(txt + "\nsolve_momentum = 1\n").solve_momentum == 1
    assert read_params(txt + "\nsolve_momentum = 0\n").solve_momentum == 0
    assert read_params(txt, {"solve_momentum": "1"}).solve_momentum == 1
    with pytest.raises(ValueError, match="solve_momentum"):
        read_params(txt + "\nsolve_momentum = 2\n")


def test_the_three_refusals_are_raised_before_anything_is_launched():
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import Matter, PiProfile, _lib
    from mg_ic_code_amd.nl import poisson_solve
    prm = _prm(16)
    pi = PiProfile.from_function(PI_0)
    # no grid is needed to be refused: nothing is stored, loaded or launched
    with pytest.raises(MatterArgumentError, match="needs matter"):
        poisson_solve(None, prm, momentum=True)
    with pytest.raises(MatterArgumentError, match="Pi_0"):
        poisson_solve(None, prm, matter=Matter(ScalarPotential()), momentum=True)
    with pytest.raises(MatterArgumentError, match="Pi_0"):
        poisson_solve([None, None], prm, matter=ScalarPotential(1e-3), momentum=True)
    with pytest.raises(ValueError, match="periodic.*sum S_i = 0"):
        poisson_solve(None, dataclasses.replace(prm, is_periodic=1),
                      matter=Matter(ScalarPotential(), pi), momentum=True)
    # the deck's switch asks for the same
    with pytest.raises(MatterArgumentError, match="needs matter"):
        poisson_solve(None, dataclasses.replace(prm, solve_momentum=1))
    assert not _lib.ctt_loaded()
    assert set(mg.launch_ledger().values()) == {0}


def test_restatement_lw_is_symmetric_and_trace_free():
    n, dx = 16, L / 16
    x, y, z = phi_ref.centres((0, 0, 0), (n - 1,) * 3, dx, L)
    shape = (n + 2,) * 3
    full = lambda a: np.ascontiguousarray(np.broadcast_to(a, shape))  # noqa: E731
    U_g = full(0.3 * np.exp(-(x * x + y * y + z * z) / 20.0) * np.sin(0.4 * x + 0.2 * z))
    V = [R.valid(full(0.2 * np.sin(0.3 * x + 0.1 * (i + 1) * y) * np.cos(0.25 * z - 0.2 * i)))
         for i in range(3)]
    W = R.w(V, U_g, dx)
    LW = R.lw([R.pad_extrap(a) for a in W], dx)
    size = max(float(np.abs(a).max()) for a in LW)
    assert size > 1e-2
    # trace-free to rounding; symmetric: the six stored components are the tensor,
    # and the off-diagonal ones do not depend on the order of their two terms
    assert float(np.abs(LW[0] + LW[3] + LW[5]).max()) <= 8 * np.finfo(float).eps * size
    Wg = [R.pad_extrap(a) for a in W]
    for c, (i, j) in ((1, (0, 1)), (2, (0, 2)), (4, (1, 2))):
        assert np.array_equal(LW[c], R.cdiff(Wg[i], j, dx) + R.cdiff(Wg[j], i, dx))
    # the extrapolation is exact on a linear field, and writes faces only
    lin = full(0.5 * x - 0.25 * y + 2.0 * z + 1.0)
    got = R.pad_extrap(R.valid(lin))
    np.testing.assert_allclose(got[1:-1, 1:-1, 0], lin[1:-1, 1:-1, 0], rtol=0, atol=1e-13)
    np.testing.assert_allclose(got[-1, 1:-1, 1:-1], lin[-1, 1:-1, 1:-1], rtol=0, atol=1e-13)
    assert got[0, 0, 5] == 0.0 and got[0, 5, 0] == 0.0 and got[-1, -1, -1] == 0.0
    # D_j LW_ij = Lap W_i + (1/3) D_i D_k W_k holds for the wide (2 dx) differences
    # the stencils compose to: checked through the solve it is built for, below


def test_ctt_library_loads_without_a_device_and_lists_its_four_kernels(tmp_path):
    out = tmp_path / "ctt.ledger"
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import mg_ic_code_amd as mg\n"
            "from mg_ic_code_amd import _lib, momentum\n"
            "assert not _lib.ctt_loaded()\n"
            "d = momentum.ctt_launch_ledger()\n"
            "assert _lib.ctt_loaded()\n"
            "assert _lib.ctt_call('mgic_ctt_launch_ledger_dump', %r) == 0\n"
            "assert d == {'k_ctt_div_rhs': 0, 'k_ctt_extrap': 0, 'k_ctt_lw': 0, 'k_ctt_w': 0}, d\n"
            "assert not any(n.startswith('k_ctt') for n in mg.launch_ledger())\n"
            % (ROOT, str(out).encode()))
    env = dict(os.environ, MGIC_NO_TORCH_PRELOAD="1")
    env.pop("MGIC_LAUNCH_LEDGER", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(out) as f:
        assert f.read() == "k_ctt_div_rhs\t0\nk_ctt_extrap\t0\nk_ctt_lw\t0\nk_ctt_w\t0\n"


def test_binding_covers_the_ctt_header():
    import re

    from mg_ic_code_amd import _lib
    with open(os.path.join(ROOT, "include", "mgic_ctt.h")) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    names = set(re.findall(r"MGIC_CTT_API\s+[\w\s\*]+?\b(mgic_ctt_\w+)\s*\(", txt))
    assert len(names) == 7 and names == set(_lib.CTT_SIGNATURES)


def test_no_kernel_of_the_ctt_library_is_launched_around_its_ledger():
    for name in ("ctt.hip", "ctt_capi.cpp", "ctt.hpp"):
        with open(os.path.join(ROOT, "mg_ic_code_amd", "csrc", name)) as f:
            assert "<<<" not in f.read(), name
    with open(os.path.join(ROOT, "mg_ic_code_amd", "csrc", "ctt.hip")) as f:
        assert f.read().count("ledger::launch<k_ctt_") == 4


_CPU = {}


def _cpu_case(n):
    """The restatement's coupled loop on the issue's case at n^3, with and
    without the momentum step: max|Mom_i| and max|Ham| / max Ham_abs."""
    if n not in _CPU:
        prm = _prm(n)
        lo, hi, dx = (0, 0, 0), (n - 1,) * 3, L / n
        phi_g = phi_ref.phi_on_box(phi_ref.gaussian, prm.bh(), lo, hi, dx)
        x, y, z = phi_ref.centres(lo, hi, dx, L, grow=0)
        assert np.array_equal(phi_g, np.broadcast_to(PHI_0(*phi_ref.centres(lo, hi, dx, L)),
                                                     phi_g.shape))
        pi = np.ascontiguousarray(np.broadcast_to(PI_0(x, y, z), (n, n, n)))
        _CPU[n] = {}
        for on in (False, True):
            r = R.coupled_solve(prm, n, 2, phi_g, (0.0, 0.0, 0.0), pi, momentum_on=on)
            assert r["norms"][-1] < prm.tolerance
            _CPU[n][on] = ([float(np.abs(m).max()) for m in r["mom"]],
                           float(np.abs(r["ham"]).max() / r["ham_abs"].max()))
    return _CPU[n]


def _assert_caps(at16, at32):
    """The caps of the issue on (max|Mom_i| without, with) at 16^3 and 32^3."""
    for i in range(3):
        assert at16[True][0][i] <= at16[False][0][i] / 5.0, (i, at16)
        assert at32[True][0][i] <= at32[False][0][i] / 20.0, (i, at32)
        assert at32[True][0][i] <= at16[True][0][i] / 3.0, (i, at16, at32)
    for r in (at16, at32):
        assert r[True][1] < RELATIVE_HAM_BOUND, r


def test_restatements_coupled_loop_stays_inside_the_caps():
    """No holes, L = 16, phi_0 = 0.1 exp(-r^2/8), Pi_0 = 0.05 exp(-((x-1)^2 +
    (y+0.5)^2 + z^2)/12.5), G = 1, V = 0, Dirichlet.  The restatement (exact
    DST solves for V_i and U, the oracle's NL loop for psi) gives, over i,
        max|Mom_i| without / with at 16^3:   6.14 - 6.40   (cap: at least 5)
        the same at 32^3:                    23.5 - 24.4   (cap: at least 20)
        with, 16^3 over 32^3:                3.37 - 3.38   (cap: at least 3)
    and max|Ham| / max Ham_abs of 5e-12 and 8e-12."""
    at16, at32 = _cpu_case(16), _cpu_case(32)
    print("16^3", at16, "32^3", at32)
    _assert_caps(at16, at32)


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def comm():
    import mg_ic_code_amd as mg
    return mg.Comm()


def _kgrid(comm):
    import mg_ic_code_amd as mg
    return mg.Grid(comm, KDOM, KBOXES, KDX, patches=True)


def _random_field(grid, rng, scale=1.0):
    """A field of random values, ghosts included; returns (field, the boxes'
    arrays over the box grown by one)."""
    import mg_ic_code_amd as mg
    f = mg.LevelData(grid)
    arrs = []
    for n, b in enumerate(_boxes(grid)):
        a = scale * rng.uniform(-1, 1, _shape(b, 1))
        f.upload(n, a, with_ghosts=True)
        arrs.append(a)
    return f, arrs


def _with_interior(ghosted, interior):
    out = ghosted.copy()
    out[1:-1, 1:-1, 1:-1] = interior
    return out


def run_kernel_cases(comm):
    """Each of the four kernels on the two-box level against momentum_ref, bit
    for bit, ghosts included (an output's ghosts stay as they were).  Shared
    with tests/momentum_worker.py."""
    from mg_ic_code_amd import momentum as mom
    rng = np.random.default_rng(20270101)
    grid = _kgrid(comm)
    assert [_shape(b) for b in _boxes(grid)] == [(8, 10, 12), (6, 10, 12)]
    V, Vg = zip(*[_random_field(grid, rng) for _ in range(3)])
    U, Ug = _random_field(grid, rng)
    out, outg = _random_field(grid, rng)
    # k_ctt_div_rhs
    mom.div_rhs(comm, V, out)
    for n in range(grid.num_local):
        want = _with_interior(outg[n], R.div_rhs([Vg[i][n] for i in range(3)], KDX))
        assert np.array_equal(out.download(n, with_ghosts=True), want), ("div_rhs", n)
    # k_ctt_w
    W, Wg = zip(*[_random_field(grid, rng) for _ in range(3)])
    mom.set_w(comm, V, U, W)
    for n in range(grid.num_local):
        want = R.w([R.valid(Vg[i][n]) for i in range(3)], Ug[n], KDX)
        for i in range(3):
            assert np.array_equal(W[i].download(n, with_ghosts=True),
                                  _with_interior(Wg[i][n], want[i])), ("w", n, i)
    # k_ctt_lw, from W with the ghosts it has now
    Wnow = [[W[i].download(n, with_ghosts=True) for n in range(grid.num_local)] for i in range(3)]
    LW, LWg = zip(*[_random_field(grid, rng) for _ in range(6)])
    mom.set_lw(comm, W, LW)
    for n in range(grid.num_local):
        want = R.lw([Wnow[i][n] for i in range(3)], KDX)
        for c in range(6):
            assert np.array_equal(LW[c].download(n, with_ghosts=True),
                                  _with_interior(LWg[c][n], want[c])), ("lw", n, c)
    # k_ctt_extrap: domain faces only, every other cell untouched
    f, fg = _random_field(grid, rng)
    mom.extrapolate(comm, f)
    touched = 0
    for n, b in enumerate(_boxes(grid)):
        want = R.extrap(fg[n], b, KDOM)
        got = f.download(n, with_ghosts=True)
        assert np.array_equal(got, want), ("extrap", n)
        touched += int(np.count_nonzero(want != fg[n]))
    # x-hi of both boxes, z-lo of the first, z-hi of the second
    assert touched == 10 * 8 + 10 * 6 + 2 * 12 * 10
    # fill_ghosts: the exchange face carries the neighbour's cells, the domain
    # faces the extrapolation of the box's own
    mom.fill_ghosts([f])
    lo_box, hi_box = (f.download(n, with_ghosts=True) for n in range(2))
    assert np.array_equal(lo_box[-1, 1:-1, 1:-1], hi_box[1, 1:-1, 1:-1])
    assert np.array_equal(hi_box[0, 1:-1, 1:-1], lo_box[-2, 1:-1, 1:-1])
    for n, b in enumerate(_boxes(grid)):
        got = f.download(n, with_ghosts=True)
        assert np.array_equal(got[1:-1, 1:-1, -1], 2.0 * got[1:-1, 1:-1, -2] - got[1:-1, 1:-1, -3])
        assert np.array_equal(got[1:-1, 1:-1, 0], fg[n][1:-1, 1:-1, 0])  # x-lo: inside the domain
    return mom.ctt_launch_ledger()


@pytest.mark.gpu
def test_kernels_are_bit_identical_to_numpy(comm):
    from mg_ic_code_amd import momentum as mom
    before = mom.ctt_launch_ledger()
    after = run_kernel_cases(comm)
    assert sorted(after) == ["k_ctt_div_rhs", "k_ctt_extrap", "k_ctt_lw", "k_ctt_w"]
    assert all(after[k] > before[k] for k in after), (before, after)


# ---- the consumers on one 12x10x8 box in the box of length 16
CDOM = (0, 0, 0, 11, 9, 7)
CDX = L / 12


def _consumer_case(comm, rng):
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import PiProfile
    from mg_ic_code_amd.phi import PhiProfile
    grid = mg.Grid(comm, CDOM, [CDOM], CDX)
    psi = mg.LevelData(grid)
    psi.upload(0, 1.0 + 0.05 * rng.uniform(-1, 1, _shape(CDOM, 1)), with_ghosts=True)
    pi = PiProfile.from_function(PI_F).fill(grid, BH_M)
    stored = PhiProfile.gaussian().fill(grid, BH_M)
    glo, ghi = (-1, -1, -1), tuple(v + 1 for v in CDOM[3:])
    for table in (P.deck_table(BH_M), SMALL):
        assert P.min_distance(table, L, glo, ghi, CDX) > 0.05
    return grid, psi, pi, stored


def _sources():
    """(stored phi_0?, table): the deck's two holes and a 3-puncture table,
    analytic and stored phi_0."""
    return [(False, None), (True, None), (False, SMALL), (True, SMALL)]


@pytest.mark.gpu
def test_consumers_with_fields_of_zeros_give_the_matter_entry_points_values(comm):
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import Matter, PunctureSet
    from mg_ic_code_amd.constraints import ConstraintFields, set_constraints
    from mg_ic_code_amd.matter import set_nl_coefs_matter, set_nl_integrand_matter
    from mg_ic_code_amd.momentum import set_nl_coefs_ctt, set_nl_integrand_ctt
    from mg_ic_code_amd.output import grchombo_vars
    rng = np.random.default_rng(20270102)
    grid, psi, pi, stored = _consumer_case(comm, rng)
    zeros = [mg.LevelData(grid) for _ in range(6)]
    for f in zeros:
        f.set_zero()
    matter = Matter(SP, [pi])
    a0, r0, a1, r1, i0, i1 = (mg.LevelData(grid) for _ in range(6))
    c0, c1 = ConstraintFields(grid), ConstraintFields(grid)
    for use_stored, table in _sources():
        kw = dict(pi=pi, phi=stored if use_stored else None,
                  punctures=PunctureSet(_rows(table)) if table is not None else None)
        set_nl_coefs_matter(psi, a0, r0, BH_M, SP, **kw)
        set_nl_coefs_ctt(psi, a1, r1, BH_M, SP, zeros, **kw)
        set_nl_integrand_matter(psi, i0, BH_M, SP, **kw)
        set_nl_integrand_ctt(psi, i1, BH_M, SP, zeros, **kw)
        for x, y in ((a0, a1), (r0, r1), (i0, i1)):
            assert np.array_equal(x.download(0), y.download(0)), (use_stored, table is None)
        set_constraints(psi, c0, BH_M, potential=SP, **kw)
        set_constraints(psi, c1, BH_M, potential=SP, abar=zeros, **kw)
        for x, y in zip(c0.fields(), c1.fields()):
            assert np.array_equal(x.download(0), y.download(0)), (use_stored, table is None)
        okw = dict(phi=kw["phi"], punctures=kw["punctures"], matter=matter, constraints=True)
        assert np.array_equal(grchombo_vars(psi, 0, BH_M, **okw),
                              grchombo_vars(psi, 0, BH_M, abar=zeros, **okw))


@pytest.mark.gpu
def test_consumers_with_random_fields_match_the_restatement(comm):
    """The comparisons of tests/test_matter.py and tests/test_constraints.py
    for the same quantities: aCoef relative, rhs and the integrand of the
    field's largest magnitude, Ham, Ham_abs and Mom_i per cell of the cell's sum
    of absolute terms, all at 1e-13; S_i = -(psi_0^6) Mom_i of the
    Bowen-York-only restatement under Mom_i's comparison; the A_ij of the output
    at 1e-13 of (|Abar^BY_ij| + |abar_ij|) chi^1.5."""
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import Matter, PunctureSet
    from mg_ic_code_amd.constraints import ConstraintFields, set_constraints
    from mg_ic_code_amd.momentum import (momentum_source, set_nl_coefs_ctt,
                                         set_nl_integrand_ctt)
    from mg_ic_code_amd.output import grchombo_vars
    rng = np.random.default_rng(20270103)
    grid, psi, pi, stored = _consumer_case(comm, rng)
    lo, hi = CDOM[:3], CDOM[3:]
    # of the size of the Bowen-York components away from the punctures
    A_by, _ = P.bowen_york(P.deck_table(BH_M), L, lo, hi, CDX)
    size = float(np.median(np.abs(np.stack([A_by[ij] for ij in P.IJ]))))
    assert 1e-4 < size < 1.0
    abar, abar_g = zip(*[_random_field(grid, rng, size) for _ in range(6)])
    abar_g = [a[0] for a in abar_g]
    abar_v = [R.valid(a) for a in abar_g]
    psi_g, piv = psi.download(0, with_ghosts=True), pi.download(0)
    a, r, integ = (mg.LevelData(grid) for _ in range(3))
    cf = ConstraintFields(grid)
    S = [mg.LevelData(grid) for _ in range(3)]
    worst = {}

    def note(key, v):
        worst[key] = max(worst.get(key, 0.0), float(v))

    for use_stored, table in _sources():
        phi = stored if use_stored else None
        punct = PunctureSet(_rows(table)) if table is not None else None
        kw = dict(pi=pi, phi=phi, punctures=punct)
        phi_g = (phi.download(0, with_ghosts=True) if use_stored
                 else P.gaussian_on_box(BH_M, lo, hi, CDX))
        set_nl_coefs_ctt(psi, a, r, BH_M, SP, abar, **kw)
        set_nl_integrand_ctt(psi, integ, BH_M, SP, abar, **kw)
        ao, ro = R.nl_coefs(BH_M, lo, hi, CDX, psi_g, phi_g, POT, piv, abar_v, table)
        io = R.nl_integrand(BH_M, lo, hi, CDX, psi_g, phi_g, POT, piv, abar_v, table)
        note("acoef", _rel(a.download(0), ao))
        note("rhs", _of_max(r.download(0), ro))
        note("integrand", _of_max(integ.download(0), io))
        # the stored tensor does reach them
        a_by, _ = R.nl_coefs(BH_M, lo, hi, CDX, psi_g, phi_g, POT, piv,
                             [np.zeros_like(v) for v in abar_v], table)
        assert _rel(ao, a_by) > 1e-6
        set_constraints(psi, cf, BH_M, potential=SP, abar=abar, **kw)
        ref = R.constraints(BH_M, lo, hi, CDX, psi_g, phi_g, POT, piv, abar_g, table)
        got = [f.download(0) for f in cf.fields()]
        note("Ham", np.max(np.abs(got[0] - ref["ham"]) / ref["ham_abs"]))
        note("Ham_abs", np.max(np.abs(got[4] - ref["ham_abs"]) / ref["ham_abs"]))
        plain = C.constraints(BH_M, lo, hi, CDX, psi_g, phi_g, POT, piv, table)
        for i in range(3):
            note(f"Mom{i + 1}", np.max(np.abs(got[1 + i] - ref["mom"][i]) / ref["scale"][i]))
            assert np.abs(ref["mom"][i] - plain["mom"][i]).max() > 1e-6 * ref["scale"][i].max()
        # S_i against -(psi_0^6) Mom_i of the Bowen-York-only restatement
        momentum_source(psi, S, BH_M, SP, **kw)
        _, psi_bh = P.bowen_york(C._table(BH_M, table), L, lo, hi, CDX)
        p6 = (R.valid(psi_g) + psi_bh) ** 6.0
        for i in range(3):
            note(f"S{i + 1}", np.max(np.abs(S[i].download(0) - -(p6 * plain["mom"][i]))
                                     / (p6 * plain["scale"][i])))
        want_S, _ = R.source(BH_M, lo, hi, CDX, R.valid(psi_g), phi_g, POT, piv, table)
        for i in range(3):
            note(f"S{i + 1}", np.max(np.abs(S[i].download(0) - want_S[i]) / (p6 * plain["scale"][i])))
        # the output's A_ij: (Abar^BY + abar) chi^1.5; chi is the file's own
        out = grchombo_vars(psi, 0, BH_M, phi=phi, punctures=punct, matter=Matter(SP, [pi]),
                            abar=abar, constraints=True)
        A, _ = P.bowen_york(C._table(BH_M, table), L, lo, hi, CDX)
        factor = out[0] ** 1.5
        for c, ij in enumerate(P.IJ):
            bar = (np.abs(A[ij]) + np.abs(abar_v[c])) * factor
            note("A_ij", np.max(np.abs(out[8 + c] - (A[ij] + abar_v[c]) * factor) / bar))
        for c in range(4):  # components 27-30: the constraint fields' own values
            assert np.array_equal(out[27 + c], got[c])
    print("worst ratios", worst)
    assert all(v <= 1e-13 for v in worst.values()), worst


# ---- the solve
def _matter(pi_f=PI_0):
    from mg_ic_code_amd import Matter, PiProfile
    return Matter(ScalarPotential(), PiProfile.from_function(pi_f))


_SOLVES = {}


def _solve(comm, n, momentum, holes=False, pi_f=PI_0, out=None):
    """poisson_solve on one Dirichlet n^3 box (cached per argument set)."""
    import mg_ic_code_amd as mg
    from mg_ic_code_amd.nl import poisson_solve
    key = (n, momentum, holes, pi_f.__name__, out)
    if key not in _SOLVES:
        prm = _prm(n, holes)
        dom = (0, 0, 0, n - 1, n - 1, n - 1)
        grid = mg.Grid(comm, dom, [dom], prm.domainLength[0] / n)
        kw = {} if momentum is None else dict(momentum=momentum)
        _SOLVES[key] = (prm, poisson_solve(grid, prm, max_depth=2, matter=_matter(pi_f),
                                           constraints=True, output_dir=out, **kw))
    return _SOLVES[key]


def _gpu_case(comm, n):
    out = {}
    for on in (False, True):
        _, res = _solve(comm, n, on)
        assert res.converged, (n, on, res.dpsi_norms)
        rep = res.constraints
        out[on] = ([rep.max_norm[f"Mom{i + 1}"] for i in range(3)], rep.relative_ham)
    return out


@pytest.mark.gpu
def test_momentum_solve_removes_the_violation_at_second_order(comm):
    """The caps of test_restatements_coupled_loop_stays_inside_the_caps (whose
    docstring has the restatement's figures) on the device's own solve and its
    own report; and the solver counts it returns."""
    at16, at32 = _gpu_case(comm, 16), _gpu_case(comm, 32)
    print("16^3", at16, "32^3", at32)
    _assert_caps(at16, at32)
    # the device's solve is the restatement's, to the solvers' tolerance
    for n, got in ((16, at16), (32, at32)):
        for on in (False, True):
            np.testing.assert_allclose(got[on][0], _cpu_case(n)[on][0], rtol=1e-6)
    _, res = _solve(comm, 16, True)
    assert len(res.momentum_iterations) == len(res.dpsi_norms)
    # (a later iteration may find its initial guess, the last solution, good enough: 0)
    assert all(len(its) == 4 and all(0 <= v <= 100 for v in its)
               for its in res.momentum_iterations), res.momentum_iterations
    assert all(v >= 1 for v in res.momentum_iterations[0])
    assert _solve(comm, 16, False)[1].momentum is None
    assert _solve(comm, 16, False)[1].momentum_iterations == []


def ZERO_PI(x, y, z):
    return 0.0 * (x + y + z)


@pytest.mark.gpu
def test_zero_pi_gives_zero_fields_and_the_same_psi(comm):
    _, off = _solve(comm, 16, False, pi_f=ZERO_PI)
    _, on = _solve(comm, 16, True, pi_f=ZERO_PI)
    mf = on.momentum
    for f in mf.V[0] + [mf.U[0]] + mf.LW[0]:
        assert not np.any(f.download(0, with_ghosts=True))
    assert np.array_equal(on.psi.download(0, with_ghosts=True),
                          off.psi.download(0, with_ghosts=True))
    assert on.linear_iterations == off.linear_iterations and on.dpsi_norms == off.dpsi_norms
    assert on.momentum_iterations == [[0, 0, 0, 0]] * len(on.dpsi_norms)


@pytest.mark.gpu
def test_momentum_false_is_todays_solve_and_loads_nothing(comm, tmp_path):
    # in a fresh process: the solve with momentum=False, with the keyword left
    # out and with the deck's solve_momentum = 0 are one solve (psi bits,
    # iteration counts, the ledger's counts), and libmgic_ctt.so stays unloaded;
    # then momentum=True adds no entry to libmgic.so's ledger
    code = """
import sys
sys.path.insert(0, %r)
import dataclasses
import numpy as np
import mg_ic_code_amd as mg
from mg_ic_code_amd import _lib
from tests import test_momentum as T
comm = mg.Comm()
names = sorted(mg.launch_ledger())
runs = []
for how in (False, None, "deck"):
    mg.launch_ledger_reset()
    T._SOLVES.clear()
    if how == "deck":
        prm = dataclasses.replace(T._prm(16), solve_momentum=0)
        from mg_ic_code_amd.nl import poisson_solve
        dom = (0, 0, 0, 15, 15, 15)
        res = poisson_solve(mg.Grid(comm, dom, [dom], T.L / 16), prm, max_depth=2,
                            matter=T._matter(), constraints=True)
    else:
        res = T._solve(comm, 16, how)[1]
    runs.append((res.psi.download(0, with_ghosts=True), res.linear_iterations, res.dpsi_norms,
                 mg.launch_ledger()))
    assert not _lib.ctt_loaded(), how
for r in runs[1:]:
    assert np.array_equal(r[0], runs[0][0]) and r[1:] == runs[0][1:]
assert runs[0][1] and sum(runs[0][3].values()) > 0
res = T._solve(comm, 16, True)[1]
assert _lib.ctt_loaded() and res.momentum is not None
assert sorted(mg.launch_ledger()) == names
print("ok", runs[0][1])
""" % ROOT
    env = dict(os.environ)
    env.pop("MGIC_LAUNCH_LEDGER", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env,
                       timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().startswith("ok")


@pytest.mark.gpu
def test_hierarchy_solve_and_coarse_fine_ghosts(comm):
    """A 16^3 base and one 16^3 fine patch (ratio 2) around the Pi_0 peak: the
    solve converges, max|Mom_i| over the uncovered cells of both levels is at
    most 1/5 of the value without the momentum solve, and W's coarse-fine ghosts
    are cf_interp of the coarse W."""
    import mg_ic_code_amd as mg
    from mg_ic_code_amd.core import AMRSolver, OperatorParams, SolverParams
    from mg_ic_code_amd.nl import poisson_solve
    prm = _prm(16)
    dom = (0, 0, 0, 15, 15, 15)
    patch = (8, 8, 8, 23, 23, 23)  # coarse cells 4..11: x, y, z in [-4, 4], the peak inside
    grids = [mg.Grid(comm, dom, [dom], L / 16),
             mg.Grid(comm, (0, 0, 0, 31, 31, 31), [patch], L / 32, patches=True)]
    res = {}
    for on in (False, True):
        res[on] = poisson_solve(grids, prm, max_depth=2, matter=_matter(), constraints=True,
                                momentum=on)
        assert res[on].converged, (on, res[on].dpsi_norms)
    for i in range(3):
        off, on = (res[k].constraints.max_norm[f"Mom{i + 1}"] for k in (False, True))
        print("hierarchy Mom", i + 1, off, on, off / on)
        assert on <= off / 5.0, (i, off, on)
    assert res[True].constraints.relative_ham < RELATIVE_HAM_BOUND
    assert all(len(its) == 4 for its in res[True].momentum_iterations)
    # W's ghosts on the fine level: every face of the patch is a coarse-fine face
    mf = res[True].momentum
    a, b = [mg.LevelData(g) for g in grids], [mg.LevelData(g) for g in grids]
    for l in range(2):
        a[l].set_zero()
        b[l].set_val(1.0)
    amr = AMRSolver(list(zip(grids, a, b)), OperatorParams(), SolverParams())
    def faces(x):
        return [x[0, 1:-1, 1:-1], x[-1, 1:-1, 1:-1], x[1:-1, 0, 1:-1], x[1:-1, -1, 1:-1],
                x[1:-1, 1:-1, 0], x[1:-1, 1:-1, -1]]

    again = mg.LevelData(grids[1])
    for i in range(3):
        got = mf.W[1][i].download(0, with_ghosts=True)
        poisoned = np.full_like(got, -7.0)
        poisoned[1:-1, 1:-1, 1:-1] = R.valid(got)
        again.upload(0, poisoned, with_ghosts=True)
        amr.cf_interp(1, again, mf.W[0][i])
        new = again.download(0, with_ghosts=True)
        for x, y in zip(faces(got), faces(new)):
            assert np.all(y != -7.0) and np.array_equal(x, y), i


@pytest.mark.gpu
def test_with_holes_and_the_final_file(comm, tmp_path):
    """The deck itself (two holes, L = 100) at 32^3 with the stretched phi_0 and
    Pi_0: away from the punctures (tests/test_constraints.py's far mask, 3.0)
    max|Mom_i| with the momentum solve is below the value without it, for every
    i (the restatement's coupled loop: 1.51e-3, 1.06e-3, 1.11e-3 without and
    7.8e-4, 9.1e-4, 7.0e-4 with; what is left is the truncation error of the
    stencils next to the punctures, three cells from them at this dx); and the
    final file's A11..A33 are psi_0^-6 (Abar^BY + LW) of the downloaded fields."""
    n = 32
    on_dir = tmp_path / "on"
    os.mkdir(on_dir)
    prm, off = _solve(comm, n, False, holes=True, pi_f=PI_DECK)
    _, on = _solve(comm, n, True, holes=True, pi_f=PI_DECK, out=str(on_dir))
    LD = prm.domainLength[0]
    lo, hi, dx = (0, 0, 0), (n - 1,) * 3, LD / n
    table = P.deck_table(prm.bh())
    assert P.min_distance(table, LD, (-1,) * 3, (n,) * 3, dx) > 0.05
    mask = C.far_mask(table, LD, lo, hi, dx, 3.0)
    assert 0.5 * mask.size < mask.sum() < mask.size
    for i in range(3):
        a, b = (np.abs(r.constraints.fields[0].fields()[1 + i].download(0))[mask].max()
                for r in (off, on))
        print("holes: far max|Mom", i + 1, "| without, with:", a, b)
        assert b < a, (i, a, b)
    # the file: 31 components, A11..A33 in 8..13, Ham and Mom_i in 27..30
    d = h5read.dataset(str(on_dir / "vcPoissonFinal.3d.hdf5"), "/level_0/data:datatype=0",
                       "<f8").reshape((31, n, n, n))
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


@pytest.mark.gpu
def test_run_poisson_cli_momentum(tmp_path):
    # the deck with solve_momentum = 1 and the flag on the plain deck: the same
    # solve, its four counts per NL iteration printed and in the JSON line
    import json
    with open(PARAMS) as f:
        txt = f.read().replace("max_NL_iterations = 6", "max_NL_iterations = 2")
    decks = {"key": tmp_path / "key.txt", "flag": tmp_path / "flag.txt"}
    decks["key"].write_text(txt + "\nsolve_momentum = 1\n")
    decks["flag"].write_text(txt)
    tool = os.path.join(ROOT, "tools", "run_poisson.py")
    common = ["--size", "16", "--max-depth", "2", "--pi", "0.004", "--constraints"]
    outs = {}
    for how, extra in (("key", []), ("flag", ["--momentum"])):
        r = subprocess.run([sys.executable, tool, str(decks[how])] + extra + common,
                           capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs[how] = json.loads(r.stdout.strip().splitlines()[-1])
        assert r.stdout.count("momentum solves V1 V2 V3 U:") == 2
    assert len(outs["key"]["momentum_iterations"]) == 2
    assert all(len(its) == 4 for its in outs["key"]["momentum_iterations"])
    assert outs["flag"]["momentum_iterations"] == outs["key"]["momentum_iterations"]
    assert outs["flag"]["dpsi_norms"] == outs["key"]["dpsi_norms"]
