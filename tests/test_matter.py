"""The scalar field's kinetic and potential energy in the sources
(mg_ic_code_amd/matter.py; the slot set_m_value leaves at zero,
SetLevelData.cpp:266-278).

1. the pin: a zero potential and a zero Pi_0 give today's entry points' bits
   (generators, all 31 output components, poisson_solve, set_grids);
2. where no pow intervenes (no holes, psi = 1) the integrand equals the numpy
   restatement (tests/matter_ref.py) bit for bit, and the final data carry
   Pi_0 in component 26 as uploaded;
3. general values against the restatement at DESIGN section 4's 1e-13 bars;
4. the nonlinear solve against the oracle loop fed by the restatement
   (checked on the CPU first);
5. homogeneous matter only moves K;
6. set_grids; 7. refusals; 8. the command line.

Layouts: those of tests/test_phi_field.py -- a ragged single box, 2 x 2 x 1
boxes, a 16^3 base with a 16^3 level-1 patch and a periodic 16^3 base.
"""
import ctypes
import dataclasses
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from mg_ic_code_amd.matter import ScalarPotential
from tests import h5read, phi_ref
from tests import matter_ref as M
from tests import puncture_ref as P
from tests.test_phi_field import (BH, BH_BARE, L, LAYOUTS, PARAMS, _all, _bhv, _boxes, _grids,
                                  _same, _shape, _sine_case, _sine_reference)
from tests.test_punctures import LAYOUT_BOXES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# test 3: params.txt's two holes moved into the layouts' box of length 16 as
# tests/test_punctures.py moves its table (positions times 0.16; masses,
# momenta and spins as they are), as the bh dict and as a table
BH_M = dict(BH, bh1_bare_mass=0.5, bh2_bare_mass=0.5, bh1_spin=0.1, bh2_spin=0.1,
            bh1_offset=10.0 * L / 100.0, bh2_offset=-10.0 * L / 100.0, bh1_momentum=0.05,
            bh2_momentum=-0.05)
TABLE_M = P.deck_table(BH_M)
# ... and a matter whose rho stays below 1e-4, a third of (2/3) K^2 / (16 pi G)
# = 3.0e-4 (BH has K = -0.3, G = 4): m = 0.06 - 201 rho stays above 0.04, so
# aCoef's negative terms (0.625 m psi_0^4 >= 0.025 and A2 psi_0^-8) do not
# cancel against 2 pi G rho_grad <= 0.015
# (test_general_matter_is_well_conditioned_and_changes_acoef), while rho >=
# 3e-5 moves aCoef by far more than the bar of the GPU comparison
SP = ScalarPotential(V0=3e-5, mass=0.02, self_coupling=0.01)
POT = tuple(SP.pot())  # (V0, mass, lambda), as the restatement and the C ABI take them


def PI_F(x, y, z):
    return 0.005 * (1.0 + 0.5 * np.cos(2 * np.pi * x / L)) + 0.0 * (y + z)


# test 2: a stored phi_0 that is no profile of the library
def PHI_F(x, y, z):
    return 0.2 * np.sin(2 * np.pi * x / L) * np.cos(2 * np.pi * y / L) + 0.05 * z / L


SP_2 = ScalarPotential(V0=1e-3, mass=0.2, self_coupling=0.1)
POT_2 = tuple(SP_2.pot())

# test 4 (the issue's case): the periodic sine deck of tests/test_phi_field.py
SP_4 = ScalarPotential(V0=1e-5, mass=0.02, self_coupling=0.01)
POT_4 = tuple(SP_4.pot())
# test 5: homogeneous matter
V0_5, PI_5 = 1e-5, 0.005
# test 6: the smallest of the V0 tried on the CPU (1e-5 ... 1e-2) at which the
# hierarchy of the one-hole deck differs from the matter-free one with every
# tagging margin above 1e-4 (measured: 6.3e-4 and 6.1e-4)
V0_6 = 4e-5


def _pi_4(prm):
    Lp = prm.domainLength[0]
    return lambda x, y, z: 0.005 * (1.0 + 0.5 * np.cos(2 * np.pi * x / Lp)) + 0.0 * (y + z)


def _rows(table):
    return [[float(v) for v in r] for r in P.as_table(table)]


# ------------------------------------------------------------------ CPU
def test_restatement_with_zero_matter_gives_todays_restatements_bits():
    rng = np.random.default_rng(2)
    for lo, hi, dx in LAYOUT_BOXES[:3]:
        pg = P.gaussian_on_box(BH, lo, hi, dx)
        for psi in (None, 1.0 + 0.05 * rng.uniform(-1, 1, _shape(lo + hi, 1))):
            for table in (None, TABLE_M):
                ref = (phi_ref.nl_coefs_phi(BH, lo, hi, dx, psi, pg) if table is None
                       else P.nl_coefs(BH, table, lo, hi, dx, psi, pg))
                got = M.nl_coefs(BH, lo, hi, dx, psi, pg, (0.0, 0.0, 0.0), 0.0, table)
                assert np.array_equal(ref[0], got[0]) and np.array_equal(ref[1], got[1])
            pv = None if psi is None else psi[1:-1, 1:-1, 1:-1]
            assert np.array_equal(P.regrid_condition(BH, TABLE_M, lo, hi, dx, pv),
                                  M.regrid_condition(BH, lo, hi, dx, (0.0, 0.0, 0.0), 0.0, pv,
                                                     table=TABLE_M))
    # the association: V0 + (((0.5 m) m) phi) phi + ((((0.25 l) phi) phi) phi) phi
    phi = rng.uniform(-1, 1, 50)
    V0, m, lam = 0.3, 0.7, 0.9
    want = np.array([(V0 + 0.5 * m * m * p * p) + 0.25 * lam * p * p * p * p for p in phi])
    assert np.array_equal(M.potential((V0, m, lam), phi), want)
    assert np.array_equal(M.rho((V0, m, lam), phi[::-1], phi), 0.5 * phi[::-1] * phi[::-1] + want)


def test_general_matter_is_well_conditioned_and_changes_acoef():
    # the relative bars of the GPU comparison presuppose that no cell has its
    # terms cancel (tests/test_punctures.py): a device pow, exp or log an ulp
    # from numpy's moves one term by 1e-16 relative and the sum by that times
    # this ratio.  And the matter must matter: without it aCoef is elsewhere.
    changed = 0.0
    for lo, hi, dx in LAYOUT_BOXES:
        assert P.min_distance(TABLE_M, L, lo, hi, dx) > 0.05
        pg = P.gaussian_on_box(BH_M, lo, hi, dx)
        pi = M.pi_on_box(PI_F, L, lo, hi, dx)
        rho = M.rho(POT, pi, pg[1:-1, 1:-1, 1:-1])
        assert 3e-5 < rho.min() and rho.max() < 1.0e-4
        assert np.all(M.m_value(BH_M, BH_M["constant_K"], rho) > 0.04)
        for psi in (0.95, 1.0, 1.05):
            ca, cc = M.conditioning(BH_M, lo, hi, dx, POT, pi, pg, psi)
            assert ca < 10 and cc < 10, (lo, hi, psi, ca, cc)
        a = M.nl_coefs(BH_M, lo, hi, dx, None, pg, POT, pi)[0]
        a0 = phi_ref.nl_coefs_phi(BH_M, lo, hi, dx, None, pg)[0]
        changed = max(changed, float(np.max(np.abs(a - a0) / np.abs(a0))))
    print("aCoef moves by", changed)
    assert changed > 1e-3


_REF = {}


def _solve_case():
    prm, n, pg = _sine_case()
    pi = M.pi_on_box(_pi_4(prm), prm.domainLength[0], (0, 0, 0), (n - 1,) * 3,
                     prm.domainLength[0] / n)
    return prm, n, pg, pi


def _solve_reference():
    if "solve" not in _REF:
        prm, n, pg, pi = _solve_case()
        _REF["solve"] = M.oracle_poisson_solve(prm, n, 2, 2, pg, POT_4, pi)
    return _REF["solve"]


def _cli_reference():
    if "cli" not in _REF:
        prm, n, pg = _sine_case()
        _REF["cli"] = M.oracle_poisson_solve(prm, n, 2, 2, pg, POT_4, PI_5)
    return _REF["cli"]


def test_matter_reference_solve_is_insensitive_to_rounding():
    prm, n, pg, pi = _solve_case()
    psi, norms, iters, ks = _solve_reference()
    print("iterations", iters, "norms", norms, "K", ks)
    assert iters == [2, 2]
    np.testing.assert_allclose(norms, [17.7139, 0.073184], rtol=1e-5)
    np.testing.assert_allclose(ks, [-0.0638626, -0.0638375], rtol=1e-5)
    assert norms[-1] < 1e-1  # below the divergence bar: the final data are written
    pert = 1e-13 * np.random.default_rng(3).uniform(-1, 1, (n, n, n))
    for p in (pert, -pert):
        psi_p, norms_p, iters_p, ks_p = M.oracle_poisson_solve(prm, n, 2, 2, pg, POT_4, pi,
                                                               perturb=p)
        print("perturbed: norms move by", np.abs(np.array(norms_p) / norms - 1.0), "K by",
              np.abs(np.array(ks_p) / ks - 1.0), "psi rel-L2",
              np.linalg.norm(psi_p - psi) / np.linalg.norm(psi))
        assert iters_p == iters
        # measured: norms 6e-13, K 2e-16, psi 3e-16; asserted: a hundredth of
        # what the GPU comparison allows (1e-6, 1e-6, 1e-10)
        np.testing.assert_allclose(norms_p, norms, rtol=1e-8)
        np.testing.assert_allclose(ks_p, ks, rtol=1e-8)
        assert np.linalg.norm(psi_p - psi) / np.linalg.norm(psi) < 1e-12
    # the constant-Pi solve lies far outside the bar of the GPU comparison
    psi_c = M.oracle_poisson_solve(prm, n, 2, 2, pg, POT_4, PI_5)[0]
    assert np.linalg.norm(psi_c - psi) / np.linalg.norm(psi) > 1e-3
    # and the matter-free one further still
    assert np.linalg.norm(_sine_reference()[0] - psi) / np.linalg.norm(psi) > 1e-3


def test_homogeneous_matter_only_moves_K_on_the_oracle():
    prm, n, pg = _sine_case()
    psi0, _, iters0, ks0 = _sine_reference()
    psi1, _, iters1, ks1 = M.oracle_poisson_solve(prm, n, 2, 2, pg, (V0_5, 0.0, 0.0), PI_5)
    assert iters1 == iters0
    assert np.linalg.norm(psi1 - psi0) / np.linalg.norm(psi0) < 1e-12
    add = 24.0 * np.pi * prm.G_Newton * (0.5 * PI_5 * PI_5 + V0_5)
    np.testing.assert_allclose(np.square(ks1), np.square(ks0) + add, rtol=1e-12)
    np.testing.assert_allclose([ks0[0], ks1[0]], [-0.0439538, -0.0602362], rtol=1e-5)


def _grids_prm():
    # the off-centre-hole deck of tests/test_regrid.py and test_phi_field.py
    from mg_ic_code_amd.params import read_params_file
    return read_params_file(PARAMS, overrides=dict(
        bh1_offset="10.0", bh2_bare_mass="0.0", bh2_spin="0.0", bh2_momentum="0.0",
        block_factor="8", max_grid_size="16", fill_ratio="0.5"))


def _grids_reference():
    if "grids" not in _REF:
        prm = _grids_prm()
        _REF["grids"] = (M.reference_hierarchy(prm, 16, 2, (V0_6, 0.0, 0.0), 0.0),
                         M.reference_hierarchy(prm, 16, 2, (0.0, 0.0, 0.0), 0.0))
    return _REF["grids"]


def test_reference_hierarchy_with_a_potential_differs_by_a_safe_margin():
    (levels, margins), (free, free_margins) = _grids_reference()
    print("margins", margins, "matter-free", free_margins, "boxes", [len(b) for b in levels],
          [len(b) for b in free])
    assert len(levels) == 3 and levels != free
    # a device condition within 1e-13 of the restatement's cannot flip a tag
    assert sorted(margins) == [0, 1] and all(m >= 1e-4 for m in margins.values()), margins
    # the zero matter is the restatement every other test uses
    assert free == P.reference_hierarchy(_grids_prm(), P.deck_table(_grids_prm().bh()), 16, 2)[0]


def test_params_keys_and_matter_classes():
    from mg_ic_code_amd import Matter, MgicError, PiProfile
    from mg_ic_code_amd.grids import set_grids
    from mg_ic_code_amd.matter import MatterArgumentError, resolve_matter
    from mg_ic_code_amd.params import read_params
    with open(PARAMS) as f:
        txt = f.read()
    prm = read_params(txt)
    assert prm.matter is None and resolve_matter(None, prm) is None
    assert Matter.from_params(prm) is None
    deck = read_params(txt + "\nscalar_V0 = 1e-5\nscalar_mass = 0.02\n"
                             "scalar_self_coupling = 0.01\npi_amplitude = 0.005\n")
    m = resolve_matter(None, deck)
    assert m.potential == ScalarPotential(1e-5, 0.02, 0.01) and m.pi.value == 0.005
    assert list(m.potential.pot()) == [1e-5, 0.02, 0.01]
    # everything else of the deck is untouched, and any one key is enough
    assert dataclasses.replace(deck, matter=None) == prm
    one = resolve_matter(None, read_params(txt + "\nscalar_mass = 0.5\n"))
    assert one.potential == ScalarPotential(0.0, 0.5, 0.0) and one.pi is None
    # the caller's matter wins over the deck's
    mine = Matter(ScalarPotential(V0=3.0))
    assert resolve_matter(mine, deck) is mine
    assert ScalarPotential() == ScalarPotential(0.0, 0.0, 0.0)
    # refused on the host, with the library's bad-argument status
    for bad in (lambda: ScalarPotential(V0=float("nan")),
                lambda: ScalarPotential(mass=float("inf")),
                lambda: ScalarPotential(self_coupling="x"),
                lambda: PiProfile.constant(float("nan")),
                lambda: Matter(potential=(1.0, 2.0, 3.0)),
                lambda: resolve_matter(3.0),
                # set_grids takes a profile only: levels appear and must be filled
                lambda: set_grids(None, prm, None, matter=Matter(ScalarPotential(), [object()]))):
        with pytest.raises(MgicError) as ei:
            bad()
        assert ei.value.code == -1 and isinstance(ei.value, MatterArgumentError)
    with pytest.raises(TypeError):
        PiProfile.from_function(3.0)


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def comm():
    import mg_ic_code_amd as mg
    return mg.Comm()


def _psi(grid, rng, with_psi):
    import mg_ic_code_amd as mg
    if not with_psi:
        return None
    psi = mg.LevelData(grid)
    for n, b in enumerate(_boxes(grid)):
        psi.upload(n, 1.0 + 0.05 * rng.uniform(-1, 1, _shape(b, 1)), with_ghosts=True)
    return psi


def _today(kind, psi, phi, table, out, bh):
    """Today's entry point for a generator: `out` a field, or two for coefs."""
    from mg_ic_code_amd._lib import call
    h = lambda f: f.handle if f is not None else None  # noqa: E731
    outs = [f.handle for f in out]
    if table is not None:
        n, t = len(table), (ctypes.c_double * (10 * len(table)))(*np.ravel(table))
        call(f"mgic_field_{kind}_punct", h(psi), h(phi), *outs, _bhv(bh), n, t)
    elif phi is not None:
        call(f"mgic_field_{kind}_phi", h(psi), phi.handle, *outs, _bhv(bh))
    else:
        call(f"mgic_field_{kind}", h(psi), *outs, _bhv(bh))


@pytest.mark.gpu
@pytest.mark.parametrize("stored", [False, True], ids=["phi=analytic", "phi=stored"])
@pytest.mark.parametrize("with_psi", [False, True], ids=["psi=None", "psi=random"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_zero_matter_is_bit_identical_to_todays_entry_points(comm, layout, with_psi, stored):
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import Matter, PunctureSet
    from mg_ic_code_amd.matter import (set_nl_coefs_matter, set_nl_integrand_matter,
                                       set_regrid_condition_matter)
    from mg_ic_code_amd.output import grchombo_vars
    from mg_ic_code_amd.phi import PhiProfile
    rng = np.random.default_rng(20261101)
    zero = ScalarPotential()
    deck = P.deck_table(BH)
    for grid in _grids(comm, layout):
        phi = PhiProfile.gaussian().fill(grid, BH) if stored else None
        psi = _psi(grid, rng, with_psi)
        ones, pi0 = mg.LevelData(grid), mg.LevelData(grid)
        ones.set_val_all(1.0)
        pi0.set_zero()
        u = psi if psi is not None else ones
        a0, r0, a1, r1 = (mg.LevelData(grid) for _ in range(4))
        for table in (None, deck):
            punct = PunctureSet(_rows(table)) if table is not None else None
            for pi in (pi0, None):
                kw = dict(pi=pi, punctures=punct, phi=phi)
                _today("nl_coefs", psi, phi, table, (a0, r0), BH)
                set_nl_coefs_matter(psi, a1, r1, BH, zero, **kw)
                assert _same(_all(a0), _all(a1)) and _same(_all(r0), _all(r1))
                _today("nl_integrand", psi, phi, table, (a0,), BH)
                set_nl_integrand_matter(psi, a1, BH, zero, **kw)
                assert _same(_all(a0), _all(a1))
                _today("regrid_condition", psi, phi, table, (a0,), BH)
                set_regrid_condition_matter(psi, a1, BH, zero, **kw)
                assert _same(_all(a0), _all(a1))
                for n in range(grid.num_local):
                    g0 = grchombo_vars(u, n, BH, phi=phi, punctures=punct)
                    g1 = grchombo_vars(u, n, BH, phi=phi, punctures=punct,
                                       matter=Matter(zero, pi))
                    assert g0.shape[0] == 31 and np.array_equal(g0, g1)
                    assert not np.any(np.signbit(g1[26]))  # +0.0, as today


def _solve(grid, prm, **kw):
    from mg_ic_code_amd.nl import NLDivergenceError, poisson_solve
    try:
        return poisson_solve(grid, prm, max_depth=2, max_NL_iterations=2, **kw)
    except NLDivergenceError as e:  # |dpsi| > 1e-1 after two steps: the state travels with it
        return e.result


def _hierarchy(comm, prm, case):
    import mg_ic_code_amd as mg
    per = (1, 1, 1) if prm.is_periodic else (0, 0, 0)
    dom = (0, 0, 0, 15, 15, 15)
    dx = prm.domainLength[0] / 16
    grids = [mg.Grid(comm, dom, [dom], dx, periodic=per)]
    if case == "base+patch":
        grids.append(mg.Grid(comm, (0, 0, 0, 31, 31, 31), [(8, 8, 8, 23, 23, 23)], dx / 2,
                             periodic=per, patches=True))
    return grids


def _psis(res, nlev):
    return [res.psi[l] for l in range(nlev)] if nlev > 1 else [res.psi]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["one level", "base+patch", "periodic"])
def test_solve_with_zero_matter_is_bit_identical(comm, case):
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import Matter, PiProfile
    from tests.test_phi_field import _wide_gaussian_prm
    prm = _wide_gaussian_prm(is_periodic=int(case == "periodic"))
    grids = _hierarchy(comm, prm, case)
    arg = grids if len(grids) > 1 else grids[0]
    ref = _solve(arg, prm)
    zeros = []
    for g in grids:
        zeros.append(mg.LevelData(g))
        zeros[-1].set_zero()
    for matter in (Matter(ScalarPotential(), PiProfile.constant(0.0)),
                   Matter(ScalarPotential(), zeros)):
        got = _solve(arg, prm, matter=matter)
        assert got.linear_iterations == ref.linear_iterations and len(ref.linear_iterations) == 2
        assert got.dpsi_norms == ref.dpsi_norms and np.all(np.isfinite(ref.dpsi_norms))
        assert got.constant_K == ref.constant_K
        assert (len(ref.constant_K) == 2) == (case == "periodic")
        for p0, p1 in zip(_psis(ref, len(grids)), _psis(got, len(grids))):
            assert _same(_all(p0, True), _all(p1, True))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_integrand_without_pow_is_bit_identical_to_numpy(comm, layout):
    # no holes and psi = 1: A2 = 0, psi_0 = 1, every pow(1, .) = 1 and the
    # Laplacian of psi is 0, so the integrand is -1.5 m + 24 pi G rho_grad in
    # + - x alone
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import Matter, PiProfile
    from mg_ic_code_amd.matter import set_nl_integrand_matter
    from mg_ic_code_amd.output import grchombo_vars
    from mg_ic_code_amd.phi import PhiProfile
    pot = SP_2
    for grid in _grids(comm, layout):
        phi = PhiProfile.from_function(PHI_F).fill(grid, BH_BARE)
        pi = PiProfile.from_function(PI_F).fill(grid, BH_BARE)
        ones, out, out0 = (mg.LevelData(grid) for _ in range(3))
        ones.set_val_all(1.0)
        for psi in (None, ones):
            set_nl_integrand_matter(psi, out, BH_BARE, pot, pi=pi, phi=phi)
            set_nl_integrand_matter(psi, out0, BH_BARE, ScalarPotential(), phi=phi)
            for n, b in enumerate(_boxes(grid)):
                lo, hi = b[:3], b[3:]
                pg = phi.download(n, with_ghosts=True)
                pv = pi.download(n)
                # the fields are the functions at the cell centres
                assert np.array_equal(pv, M.pi_on_box(PI_F, L, lo, hi, grid.dx))
                assert np.array_equal(pg, phi_ref.phi_on_box(
                    lambda bh, x, y, z: PHI_F(x, y, z), BH_BARE, lo, hi, grid.dx))
                assert np.ptp(pv) > 0 and np.ptp(pg) > 0
                want = M.nl_integrand(BH_BARE, lo, hi, grid.dx, None, pg, POT_2, pv)
                got = out.download(n)
                assert np.array_equal(got, want)
                # ... and is not the matter-free integrand
                assert np.min(np.abs(got - out0.download(n))) > 1e-3 * np.abs(got).max()
                g = grchombo_vars(ones, n, BH_BARE, phi=phi, matter=Matter(pot, pi))
                assert np.array_equal(g[26], pv) and np.array_equal(g[25], pg[1:-1, 1:-1, 1:-1])
                g0 = grchombo_vars(ones, n, BH_BARE, phi=phi)
                other = [c for c in range(31) if c != 26]
                assert np.array_equal(g[other], g0[other]) and not np.any(g0[26])


def _rel(got, ref):
    return float(np.max(np.abs(got - ref) / np.abs(ref)))


def _of_max(got, ref):
    return float(np.max(np.abs(got - ref)) / np.abs(ref).max())


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_general_matter_matches_restatement(comm, layout):
    # DESIGN section 4's 1e-13 for this generator, applied as
    # tests/test_punctures.py applies it: aCoef and the regrid condition
    # relative (their terms do not cancel, checked on the CPU above), rhs and
    # the integrand (which change sign) of the field's largest magnitude
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import PiProfile, PunctureSet
    from mg_ic_code_amd.matter import (set_nl_coefs_matter, set_nl_integrand_matter,
                                       set_regrid_condition_matter)
    from mg_ic_code_amd.phi import PhiProfile
    rng = np.random.default_rng(20261102)
    pot = SP
    worst = dict(acoef=0.0, cond=0.0, rhs=0.0, integrand=0.0)
    for grid in _grids(comm, layout):
        pi = PiProfile.from_function(PI_F).fill(grid, BH_M)
        stored = PhiProfile.gaussian().fill(grid, BH_M)
        ones = mg.LevelData(grid)
        ones.set_val_all(1.0)
        a, r, integ, cond = (mg.LevelData(grid) for _ in range(4))
        for with_psi in (False, True):
            psi = _psi(grid, rng, with_psi)
            u = psi if psi is not None else ones
            # the deck's holes and the analytic Gaussian; the same holes as a
            # table and the stored Gaussian
            for phi, table in ((None, None), (stored, TABLE_M)):
                kw = dict(pi=pi, phi=phi,
                          punctures=PunctureSet(_rows(table)) if table is not None else None)
                set_nl_coefs_matter(psi, a, r, BH_M, pot, **kw)
                set_nl_integrand_matter(psi, integ, BH_M, pot, **kw)
                set_regrid_condition_matter(psi, cond, BH_M, pot, **kw)
                for n, b in enumerate(_boxes(grid)):
                    lo, hi, dx = b[:3], b[3:], grid.dx
                    pg = u.download(n, with_ghosts=True)
                    pv = pg[1:-1, 1:-1, 1:-1]
                    phi_g = (P.gaussian_on_box(BH_M, lo, hi, dx) if phi is None
                             else phi.download(n, with_ghosts=True))
                    piv = pi.download(n)
                    ao, ro = M.nl_coefs(BH_M, lo, hi, dx, pg if with_psi else None, phi_g, POT, piv,
                                        table)
                    io = M.nl_integrand(BH_M, lo, hi, dx, pg, phi_g, POT, piv, table)
                    co = M.regrid_condition(BH_M, lo, hi, dx, POT, piv, pv if with_psi else None,
                                            phi_g, table)
                    e = dict(acoef=_rel(a.download(n), ao), cond=_rel(cond.download(n), co),
                             rhs=_of_max(r.download(n), ro),
                             integrand=_of_max(integ.download(n), io))
                    worst = {k: max(worst[k], v) for k, v in e.items()}
    print(layout, "worst ratios", worst)
    assert all(v <= 1e-13 for v in worst.values()), worst


@pytest.mark.gpu
def test_periodic_solve_with_matter_matches_oracle_loop(comm, tmp_path):
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import Matter, PiProfile
    from mg_ic_code_amd.nl import poisson_solve
    from mg_ic_code_amd.phi import PhiProfile
    prm, n, _, pi_ref = _solve_case()
    dom = (0, 0, 0, n - 1, n - 1, n - 1)
    grid = mg.Grid(comm, dom, [dom], prm.domainLength[0] / n, periodic=(1, 1, 1))
    pi = PiProfile.from_function(_pi_4(prm))
    res = poisson_solve(grid, prm, max_depth=2, max_NL_iterations=2, phi0=PhiProfile.sine(),
                        matter=Matter(SP_4, pi), output_dir=str(tmp_path))
    psi_o, norms_o, iters_o, ks_o = _solve_reference()
    print("iterations", res.linear_iterations, iters_o, "norms", res.dpsi_norms, norms_o,
          "K", res.constant_K, ks_o)
    assert res.linear_iterations == iters_o == [2, 2]
    np.testing.assert_allclose(res.dpsi_norms, norms_o, rtol=1e-6)
    np.testing.assert_allclose(res.constant_K, ks_o, rtol=1e-6)
    g = res.psi.download(0)
    c = psi_o[1:-1, 1:-1, 1:-1]
    err = np.linalg.norm(g - c) / np.linalg.norm(c)
    print("psi rel-L2", err)
    assert err <= 1e-10
    # the files of that solve: Pi_0 in component 26 of the final data, as
    # uploaded; phi still the stored sine; the solver data keep 10 components
    want = pi.fill(grid, prm).download(0)
    assert np.array_equal(want, pi_ref) and np.ptp(want) > 0
    final = h5read.dataset(str(tmp_path / "vcPoissonFinal.3d.hdf5"), "/level_0/data:datatype=0",
                           "<f8").reshape((31, n, n, n))
    assert np.array_equal(final[26], want)
    assert np.array_equal(final[25], PhiProfile.sine().fill(grid, prm).download(0))
    assert np.array_equal(final[7], np.full((n, n, n), res.constant_K[-1]))
    for i in range(2):
        data = h5read.dataset(str(tmp_path / f"vcPoissonOut.3d_{i}.hdf5"),
                              "/level_0/data:datatype=0", "<f8")
        assert data.size == 10 * n ** 3
    assert sorted(os.listdir(tmp_path)) == ["vcPoissonFinal.3d.hdf5", "vcPoissonOut.3d_0.hdf5",
                                            "vcPoissonOut.3d_1.hdf5"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["one level", "base+patch"])
def test_homogeneous_matter_only_moves_K(comm, case):
    from mg_ic_code_amd import Matter, PiProfile
    from mg_ic_code_amd.phi import PhiProfile
    prm, _, _ = _sine_case()
    grids = _hierarchy(comm, prm, case)
    arg = grids if len(grids) > 1 else grids[0]
    ref = _solve(arg, prm, phi0=PhiProfile.sine())
    got = _solve(arg, prm, phi0=PhiProfile.sine(),
                 matter=Matter(ScalarPotential(V0=V0_5), PiProfile.constant(PI_5)))
    print(case, "iterations", ref.linear_iterations, got.linear_iterations, "K", ref.constant_K,
          got.constant_K)
    assert got.linear_iterations == ref.linear_iterations and len(ref.linear_iterations) == 2
    for p0, p1 in zip(_psis(ref, len(grids)), _psis(got, len(grids))):
        x = np.concatenate([v.ravel() for v in _all(p0)])
        y = np.concatenate([v.ravel() for v in _all(p1)])
        err = np.linalg.norm(y - x) / np.linalg.norm(x)
        print("psi rel-L2", err)
        assert err <= 1e-10
    add = 24.0 * np.pi * prm.G_Newton * (0.5 * PI_5 * PI_5 + V0_5)
    assert len(got.constant_K) == 2
    np.testing.assert_allclose(np.square(got.constant_K), np.square(ref.constant_K) + add,
                               rtol=1e-12)
    if case == "one level":
        np.testing.assert_allclose([ref.constant_K[0], got.constant_K[0]],
                                   [-0.0439538, -0.0602362], rtol=1e-5)


@pytest.mark.gpu
def test_set_grids_with_a_potential_matches_restatement(comm):
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import Matter, PiProfile
    from mg_ic_code_amd.grids import set_grids
    from mg_ic_code_amd.matter import set_regrid_condition_matter
    prm = _grids_prm()
    (levels, margins), (free, _) = _grids_reference()
    assert all(m >= 1e-4 for m in margins.values()), margins
    dom0 = (0, 0, 0, 15, 15, 15)
    base = mg.Grid(comm, dom0, [dom0], prm.L / 16)
    # the condition that drives the tags, against the restatement
    cond = mg.LevelData(base)
    set_regrid_condition_matter(None, cond, prm.bh(), ScalarPotential(V0=V0_6))
    want = M.regrid_condition(prm.bh(), dom0[:3], dom0[3:], base.dx, (V0_6, 0.0, 0.0), 0.0)
    err = _rel(cond.download(0), want)
    print("regrid condition worst relative error", err)
    assert err <= 1e-13
    grids = set_grids(comm, prm, base, max_level=2, matter=Matter(ScalarPotential(V0=V0_6)))
    assert [g.boxes for g in grids] == levels and len(grids) == 3
    # AMRSolver's CFLevel checks the proper nesting of every level
    fields = [(g, mg.LevelData(g), mg.LevelData(g)) for g in grids]
    for _, a, b in fields:
        a.set_val(-1.0)
        b.set_val(1.0)
    amr = mg.AMRSolver(fields, mg.OperatorParams(alpha=1.0, beta=-1.0),
                       mg.SolverParams(max_depth=2, bottom_solver=0))
    assert amr.num_levels == 3
    # the zero matter: today's boxes
    ref = set_grids(comm, prm, base, max_level=2)
    got = set_grids(comm, prm, base, max_level=2,
                    matter=Matter(ScalarPotential(), PiProfile.constant(0.0)))
    assert [g.boxes for g in got] == [g.boxes for g in ref] == free != levels
    # and the deck's keys are read
    deck = set_grids(comm, dataclasses.replace(prm, matter=dict(scalar_V0=V0_6)), base,
                     max_level=2)
    assert [g.boxes for g in deck] == levels


@pytest.mark.gpu
def test_bad_matter_is_refused_before_any_launch_or_file(comm, tmp_path):
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import Matter, PiProfile
    from mg_ic_code_amd._lib import call, io_call
    from mg_ic_code_amd.grids import set_grids
    from mg_ic_code_amd.matter import (MatterArgumentError, set_nl_coefs_matter,
                                       set_nl_integrand_matter, set_regrid_condition_matter)
    from mg_ic_code_amd.output import grchombo_vars, output_final_data
    g0, g1 = _grids(comm, "base+patch")
    a, r = mg.LevelData(g0), mg.LevelData(g0)
    a.set_val(7.0)
    pi1 = PiProfile.constant(0.1).fill(g1, BH)
    pot = ScalarPotential(1e-3)
    ok = (ctypes.c_double * 3)(1e-3, 0.0, 0.0)
    hs = (ctypes.c_void_p * 1)(a.handle)
    h1 = (ctypes.c_void_p * 1)(pi1.handle)
    rr = (ctypes.c_int * 1)(2)
    path = str(tmp_path / "x.hdf5")
    out = np.empty((31,) + _shape(g0.local_box(0)))
    optr = out.ctypes.data_as(ctypes.c_void_p)
    cases = []
    for c in range(3):  # a non-finite coefficient, in each place
        nan = (ctypes.c_double * 3)(*[float("nan") if i == c else 0.0 for i in range(3)])
        cases += [
            (lambda nan=nan: call("mgic_field_nl_coefs_matter", None, None, a.handle, r.handle,
                                  _bhv(BH), 0, None, None, nan), "finite"),
            (lambda nan=nan: call("mgic_field_nl_integrand_matter", None, None, a.handle, _bhv(BH),
                                  0, None, None, nan), "finite"),
            (lambda nan=nan: call("mgic_field_regrid_condition_matter", None, None, a.handle,
                                  _bhv(BH), 0, None, None, nan), "finite"),
            (lambda nan=nan: call("mgic_field_grchombo_vars_matter", a.handle, None, 0, 0, 1,
                                  _bhv(BH), 0, None, None, nan, optr, 0), "finite"),
            (lambda nan=nan: io_call("mgic_io_write_final_data_matter", path.encode(), 1, hs, None,
                                     _bhv(BH), 0, None, None, nan, 0, rr), "finite")]
    inf = (ctypes.c_double * 3)(0.0, float("inf"), 0.0)
    cases += [
        (lambda: call("mgic_field_nl_coefs_matter", None, None, a.handle, r.handle, _bhv(BH), 0,
                      None, None, inf), "finite"),
        (lambda: call("mgic_field_nl_coefs_matter", None, None, a.handle, r.handle, _bhv(BH), 0,
                      None, None, None), "null argument"),
        # a count without a table
        (lambda: call("mgic_field_nl_coefs_matter", None, None, a.handle, r.handle, _bhv(BH), 2,
                      None, None, ok), "null argument"),
        (lambda: io_call("mgic_io_write_final_data_matter", path.encode(), 1, hs, None, _bhv(BH),
                         2, None, None, ok, 0, rr), "null argument"),
        # a Pi_0 of another layout
        (lambda: set_nl_coefs_matter(None, a, r, BH, pot, pi=pi1), "pi"),
        (lambda: set_nl_integrand_matter(None, a, BH, pot, pi=pi1), "pi"),
        (lambda: set_regrid_condition_matter(None, a, BH, pot, pi=pi1), "pi"),
        (lambda: grchombo_vars(a, 0, BH, matter=Matter(pot, pi1)), "pi"),
        (lambda: output_final_data([a], BH, 0, [2], path, matter=Matter(pot, [pi1])), "pi"),
        (lambda: io_call("mgic_io_write_final_data_matter", path.encode(), 1, hs, None, _bhv(BH),
                         0, None, h1, ok, 0, rr), "pi")]
    for fn, what in cases:
        with pytest.raises(mg.MgicError) as ei:
            fn()
        assert ei.value.code == -1 and what in str(ei.value), str(ei.value)
    # set_grids needs a profile: a filled LevelData is refused on the host
    with pytest.raises(MatterArgumentError) as ei:
        set_grids(comm, _grids_prm(), g0, max_level=1, matter=Matter(pot, pi1))
    assert ei.value.code == -1 and "PiProfile" in str(ei.value)
    # and a count of fields that is not the count of levels
    with pytest.raises(MatterArgumentError):
        from mg_ic_code_amd.nl import poisson_solve
        from tests.test_phi_field import _wide_gaussian_prm
        poisson_solve([g0, g1], _wide_gaussian_prm(), matter=Matter(pot, [pi1]))
    assert os.listdir(tmp_path) == []       # no file was created
    assert np.all(a.download(0) == 7.0)     # nothing was launched


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["flags", "deck keys", "flags over deck keys"])
def test_run_poisson_cli_with_matter(tmp_path, how):
    deck = tmp_path / "periodic.txt"
    with open(PARAMS) as f:
        txt = f.read()
    assert "is_periodic = 0" in txt and "max_NL_iterations = 6" in txt
    txt = (txt.replace("is_periodic = 0", "is_periodic = 1")
           .replace("max_NL_iterations = 6", "max_NL_iterations = 2"))
    V0, mass, lam = POT_4
    keys = (f"scalar_V0 = {V0!r}\nscalar_mass = {mass!r}\nscalar_self_coupling = {lam!r}\n"
            f"pi_amplitude = {PI_5!r}\n")
    wrong = "scalar_V0 = 1.0\nscalar_mass = 1.0\nscalar_self_coupling = 1.0\npi_amplitude = 1.0\n"
    flags = ["--potential", f"{V0!r} {mass!r} {lam!r}", "--pi", repr(PI_5)]
    deck.write_text(txt + {"flags": "", "deck keys": keys, "flags over deck keys": wrong}[how])
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_poisson.py"), str(deck),
                          "--size", "16", "--max-depth", "2", "--phi", "sine"]
                         + (flags if how != "deck keys" else []),
                         capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    print(out.stdout)
    lines = out.stdout.splitlines()
    assert sum(line.startswith("matter: ") for line in lines) == 1
    got = json.loads(lines[-1])
    assert got["matter"] == dict(V0=V0, mass=mass, self_coupling=lam, pi=PI_5)
    _, norms_o, iters_o, ks_o = _cli_reference()
    assert got["linear_iterations"] == iters_o
    np.testing.assert_allclose(got["dpsi_norms"], norms_o, rtol=1e-6)
    np.testing.assert_allclose(got["constant_K"], ks_o, rtol=1e-6)
    assert math.isclose(ks_o[0], -0.06293, rel_tol=1e-3)  # against -0.04395 without matter
