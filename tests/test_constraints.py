"""The Hamiltonian and momentum constraints of the solved data
(mg_ic_code_amd/constraints.py).

CPU: the numpy restatement (tests/constraints_ref.py) against the integrand's
restatement, against its own evaluation in extended precision, and its order
of convergence.  GPU: k_constraints pinned across its instantiations, against
numpy bit for bit where no pow remains, against the restatement to DESIGN
section 4's 1e-13 of the cell's sum of absolute terms, against the device's
own integrand kernel; the norms, the order of convergence, the solve's report
and final file, and the refusals.
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from mg_ic_code_amd.matter import ScalarPotential
from tests import constraints_ref as C
from tests import h5read
from tests import matter_ref as M
from tests import puncture_ref as P
from tests.test_matter import (BH_M, PHI_F, PI_5, PI_F, POT, POT_4, SP, SP_2, SP_4, TABLE_M,
                               _pi_4)
from tests.test_phi_field import (BH, BH_BARE, L, LAYOUTS, PARAMS, _all, _bhv, _boxes, _grids,
                                  _same, _shape, _sine_case)
from tests.test_punctures import LAYOUT_BOXES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the box whose rows cross the 64-wide tile, in the layouts' domain of length 16
WIDE = ((0, 0, 0), (71, 11, 9), L / 72)
CLAYOUTS = LAYOUTS + ["72x12x10"]
# two punctures with every vector component set, none on a cell centre of the
# boxes used with it (asserted in the tests)
TABLE_C = P.as_table([[0.5, 1.3, 0.4, -0.7, 0.1, 0.2, -0.15, 0.05, -0.1, 0.2],
                      [0.4, -2.1, -0.9, 1.1, -0.1, 0.05, 0.1, 0.0, 0.1, -0.05]])


def _rows(table):
    return [[float(v) for v in r] for r in P.as_table(table)]


def _grown(lo, hi):
    return tuple(v - 1 for v in lo), tuple(v + 1 for v in hi)


# ------------------------------------------------------------------ CPU
def test_ham_is_two_thirds_K2_minus_two_thirds_of_the_integrand_in_numpy():
    rng = np.random.default_rng(20261201)
    worst = 0.0
    for lo, hi, dx in LAYOUT_BOXES[:3]:
        glo, ghi = _grown(lo, hi)
        assert P.min_distance(TABLE_M, L, glo, ghi, dx) > 0.05
        psi_g = 1.0 + 0.05 * rng.uniform(-1, 1, _shape(lo + hi, 1))
        phi_g = P.gaussian_on_box(BH_M, lo, hi, dx)
        pi = M.pi_on_box(PI_F, L, lo, hi, dx)
        K = BH_M["constant_K"]
        for table in (None, TABLE_M):
            ham, ham_abs = C.hamiltonian(BH_M, lo, hi, dx, psi_g, phi_g, POT, pi, table)
            integ = M.nl_integrand(BH_M, lo, hi, dx, psi_g, phi_g, POT, pi, table)
            r = np.abs(ham - (2.0 / 3.0) * (K * K) + (2.0 / 3.0) * integ) / ham_abs
            worst = max(worst, float(r.max()))
    print("worst |Ham - (2/3)K^2 + (2/3) integrand| / Ham_abs", worst)
    assert worst <= 1e-13


def test_momentum_in_float64_against_longdouble():
    # the headroom the GPU bar of 1e-13 rests on: the float64 restatement is
    # within 1e-14 of each cell's sum of absolute terms of the same
    # expressions in extended precision
    assert np.finfo(np.longdouble).eps < 1e-3 * np.finfo(np.float64).eps
    rng = np.random.default_rng(20261202)
    cube = ((0, 0, 0), (31, 31, 31), L / 32)
    for lo, hi, dx in (WIDE, cube):
        glo, ghi = _grown(lo, hi)
        assert P.min_distance(TABLE_C, L, glo, ghi, dx) > 0.05
        psi = 1.0 + 0.05 * rng.uniform(-1, 1, _shape(lo + hi))
        phi_g = 0.2 * rng.uniform(-1, 1, _shape(lo + hi, 1))
        pi = 0.005 * rng.uniform(-1, 1, _shape(lo + hi))
        m64, s64 = C.momentum(BH, lo, hi, dx, psi, phi_g, POT, pi, TABLE_C)
        mld, _ = C.momentum(BH, lo, hi, dx, psi, phi_g, POT, pi, TABLE_C, dtype=np.longdouble)
        worst = max(float(np.max(np.abs(a - b) / s)) for a, b, s in zip(m64, mld, s64))
        print(hi, "worst |float64 - longdouble| / scale", worst)
        assert worst <= 1e-14


_CONV = {}


def _conv_case(n):
    lo, hi, dx = (0, 0, 0), (n - 1,) * 3, L / n
    assert P.min_distance(TABLE_C, L, *_grown(lo, hi), dx) > 0.01  # the norm's cells are 3 away
    return lo, hi, dx, C.far_mask(TABLE_C, L, lo, hi, dx, 3.0)


def _conv_reference(n):
    """The restatement's L2 norms of Mom_i at psi = 1 without matter, away from
    the punctures, on one n^3 box."""
    if n not in _CONV:
        lo, hi, dx, mask = _conv_case(n)
        mom, _ = C.momentum(BH, lo, hi, dx, np.ones(_shape(lo + hi)), None, None, None, TABLE_C)
        _CONV[n] = [C.l2(m, mask, dx) for m in mom]
    return _CONV[n]


def test_bowen_york_divergence_converges_at_second_order():
    c, f = _conv_reference(32), _conv_reference(64)
    ratios = [a / b for a, b in zip(c, f)]
    print("32^3 : 64^3 ratios of |Mom_i|_2", ratios)
    assert all(3.5 <= r <= 4.5 for r in ratios), ratios


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def comm():
    import mg_ic_code_amd as mg
    return mg.Comm()


def _cgrids(comm, layout):
    import mg_ic_code_amd as mg
    if layout == "72x12x10":
        dom = WIDE[0] + WIDE[1]
        return [mg.Grid(comm, dom, [dom], WIDE[2])]
    return _grids(comm, layout)


def _psi(grid, rng):
    import mg_ic_code_amd as mg
    psi = mg.LevelData(grid)
    for n, b in enumerate(_boxes(grid)):
        psi.upload(n, 1.0 + 0.05 * rng.uniform(-1, 1, _shape(b, 1)), with_ghosts=True)
    return psi


def _run(psi, bh, out=None, **kw):
    """set_constraints into fresh (or the given) fields, poisoned first so an
    unwritten cell shows; returns the five fields' boxes."""
    from mg_ic_code_amd.constraints import ConstraintFields, set_constraints
    out = ConstraintFields(psi.grid) if out is None else out
    for f in out.fields():
        f.set_val_all(-7.0)
    set_constraints(psi, out, bh, **kw)
    return [_all(f) for f in out.fields()]


def _same5(a, b):
    return all(_same(x, y) for x, y in zip(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", CLAYOUTS)
def test_instantiations_are_pinned_to_each_other(comm, layout):
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import PiProfile, PunctureSet
    from mg_ic_code_amd.constraints import constraint_vars
    from mg_ic_code_amd.phi import PhiProfile
    rng = np.random.default_rng(20261203)
    deck = PunctureSet(_rows(P.deck_table(BH)))
    zero = ScalarPotential()
    for grid in _cgrids(comm, layout):
        psi = _psi(grid, rng)
        stored = PhiProfile.gaussian().fill(grid, BH)
        pi = PiProfile.from_function(PI_F).fill(grid, BH)
        pi0 = mg.LevelData(grid)
        pi0.set_zero()
        # the analytic Gaussian against the same Gaussian stored; the deck's two
        # holes against the deck as a table (with matter, so dphi is compared)
        ref = _run(psi, BH, potential=SP, pi=pi)
        assert all(np.all(x != -7.0) for f in ref for x in f)  # every valid cell is written
        assert _same5(ref, _run(psi, BH, potential=SP, pi=pi, phi=stored))
        assert _same5(ref, _run(psi, BH, potential=SP, pi=pi, punctures=deck))
        assert _same5(ref, _run(psi, BH, potential=SP, pi=pi, punctures=deck, phi=stored))
        # a zero potential without Pi, and with a zero-filled Pi, against no matter
        for kw in (dict(), dict(phi=stored), dict(punctures=deck, phi=stored)):
            bare = _run(psi, BH, **kw)
            assert _same5(bare, _run(psi, BH, potential=zero, **kw))
            assert _same5(bare, _run(psi, BH, potential=zero, pi=pi0, **kw))
        assert not _same5(ref[1:4], _run(psi, BH)[1:4])  # the matter does reach Mom_i
        # the slab form: the first four fields, planes k0 > 0, nk < nz
        for n, b in enumerate(_boxes(grid)):
            nz = b[5] - b[2] + 1
            for k0, nk, kw in ((1, nz - 2, dict(potential=SP, pi=pi)),
                               (2, 3, dict(potential=SP, pi=pi, punctures=deck, phi=stored)),
                               (nz - 1, 1, dict())):
                got = constraint_vars(psi, n, BH, k0=k0, nk=nk, **kw)
                want = ref if kw else _run(psi, BH)
                assert got.shape == (4, nk) + _shape(b)[1:]
                for c in range(4):
                    assert np.array_equal(got[c], want[c][n][k0:k0 + nk]), (n, k0, c)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", CLAYOUTS)
def test_momentum_source_without_holes_is_bit_identical_to_numpy(comm, layout):
    # no holes: every Abar_ij is a signed zero, so d_j Abar_ij is +0 and Mom_i is
    # the source alone, in + - x and the one division 0.5/dx
    from mg_ic_code_amd import PiProfile
    from mg_ic_code_amd.phi import PhiProfile
    rng = np.random.default_rng(20261204)
    G = BH_BARE["G_Newton"]
    for grid in _cgrids(comm, layout):
        psi = _psi(grid, rng)
        phi = PhiProfile.from_function(PHI_F).fill(grid, BH_BARE)
        pi = PiProfile.from_function(PI_F).fill(grid, BH_BARE)
        got = _run(psi, BH_BARE, potential=SP_2, pi=pi, phi=phi)
        dx = grid.dx
        for n, b in enumerate(_boxes(grid)):
            pg, pv = phi.download(n, with_ghosts=True), pi.download(n)
            assert np.ptp(pg) > 0 and np.ptp(pv) > 0
            for i in range(3):
                phi_p, phi_m = C._shift(pg, i, +1), C._shift(pg, i, -1)
                want = 8.0 * np.pi * G * pv * (0.5 / dx * (phi_p - phi_m))
                assert np.array_equal(got[1 + i][n], want), (n, i)
                assert np.count_nonzero(want) > want.size // 2


def _reference(grid, n, b, psi, phi, pi, bh, pot, table):
    lo, hi, dx = b[:3], b[3:], grid.dx
    assert P.min_distance(C._table(bh, table), L, *_grown(lo, hi), dx) > 0.05
    phi_g = (P.gaussian_on_box(bh, lo, hi, dx) if phi is None
             else phi.download(n, with_ghosts=True))
    return C.constraints(bh, lo, hi, dx, psi.download(n, with_ghosts=True), phi_g, pot,
                         pi.download(n) if pi is not None else None, table)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", CLAYOUTS)
def test_general_case_matches_restatement(comm, layout):
    """Per cell |got - ref| <= 1e-13 of the cell's sum of absolute terms:
    Ham_abs for Ham, psi_0^-6 sum_j 0.5/dx (|A(+)| + |A(-)|) + |8 pi G Pi
    dphi_i| for Mom_i; Ham_abs itself relative.  DESIGN section 4's bar for the
    generator family."""
    from mg_ic_code_amd import PiProfile, PunctureSet
    from mg_ic_code_amd.phi import PhiProfile
    rng = np.random.default_rng(20261205)
    worst = dict(Ham=0.0, Mom1=0.0, Mom2=0.0, Mom3=0.0, Ham_abs=0.0)
    for grid in _cgrids(comm, layout):
        psi = _psi(grid, rng)
        pi = PiProfile.from_function(PI_F).fill(grid, BH_M)
        stored = PhiProfile.gaussian().fill(grid, BH_M)
        for phi, table in ((None, None), (stored, TABLE_M), (stored, None), (None, TABLE_M)):
            punct = PunctureSet(_rows(table)) if table is not None else None
            got = _run(psi, BH_M, potential=SP, pi=pi, punctures=punct, phi=phi)
            for n, b in enumerate(_boxes(grid)):
                ref = _reference(grid, n, b, psi, phi, pi, BH_M, POT, table)
                e = dict(Ham=np.abs(got[0][n] - ref["ham"]) / ref["ham_abs"],
                         Ham_abs=np.abs(got[4][n] - ref["ham_abs"]) / ref["ham_abs"])
                for i in range(3):
                    e[f"Mom{i + 1}"] = np.abs(got[1 + i][n] - ref["mom"][i]) / ref["scale"][i]
                worst = {k: max(worst[k], float(v.max())) for k, v in e.items()}
                # the comparison is not vacuous: the fields are far above the bar
                assert np.abs(ref["ham"]).max() > 1e-6 * ref["ham_abs"].max()
                assert all(np.abs(m).max() > 1e-6 * s.max()
                           for m, s in zip(ref["mom"], ref["scale"]))
    print(layout, "worst ratios", worst)
    assert all(v <= 1e-13 for v in worst.values()), worst


@pytest.mark.gpu
@pytest.mark.parametrize("layout", CLAYOUTS)
def test_ham_is_the_devices_own_integrand(comm, layout):
    # Ham = (2/3) K^2 - (2/3) * set_nl_integrand_matter's value (pinned to the
    # compiled reference), to 1e-13 Ham_abs per cell
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import PiProfile, PunctureSet
    from mg_ic_code_amd.matter import set_nl_integrand_matter
    from mg_ic_code_amd.phi import PhiProfile
    rng = np.random.default_rng(20261206)
    K = BH_M["constant_K"]
    worst = 0.0
    for grid in _cgrids(comm, layout):
        psi = _psi(grid, rng)
        pi = PiProfile.from_function(PI_F).fill(grid, BH_M)
        stored = PhiProfile.gaussian().fill(grid, BH_M)
        integ = mg.LevelData(grid)
        for phi, table in ((None, None), (stored, TABLE_M)):
            punct = PunctureSet(_rows(table)) if table is not None else None
            got = _run(psi, BH_M, potential=SP, pi=pi, punctures=punct, phi=phi)
            set_nl_integrand_matter(psi, integ, BH_M, SP, pi=pi, punctures=punct, phi=phi)
            for n in range(grid.num_local):
                r = (np.abs(got[0][n] - (2.0 / 3.0) * (K * K) + (2.0 / 3.0) * integ.download(n))
                     / got[4][n])
                worst = max(worst, float(r.max()))
    print(layout, "worst |Ham - (2/3)K^2 + (2/3) integrand| / Ham_abs", worst)
    assert worst <= 1e-13


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["base+patch", "2x2x1"])
def test_norms_are_numpys_over_the_uncovered_cells(comm, layout):
    from mg_ic_code_amd import Matter, PiProfile
    from mg_ic_code_amd.constraints import COMPONENTS, constraints
    rng = np.random.default_rng(20261207)
    grids = _grids(comm, layout)
    psis = [_psi(g, rng) for g in grids]
    rep = constraints(psis if len(grids) > 1 else psis[0], BH_M,
                      matter=Matter(SP, PiProfile.from_function(PI_F)))
    assert len(rep.fields) == len(grids)
    mx, sq, cells = np.zeros(5), np.zeros(4), 0
    for l, g in enumerate(grids):
        for c, f in enumerate(rep.fields[l].fields()):
            for n, b in enumerate(_boxes(g)):
                x = f.download(n)
                keep = np.ones(x.shape, dtype=bool)
                if l + 1 < len(grids):  # cells under the finer level's boxes
                    for fb in grids[l + 1].boxes:
                        lo = [max(fb[d] // 2, b[d]) - b[d] for d in range(3)]
                        hi = [min(fb[3 + d] // 2, b[3 + d]) - b[d] for d in range(3)]
                        keep[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = False
                mx[c] = max(mx[c], np.abs(x[keep]).max())
                if c < 4:
                    sq[c] += np.sum(x[keep] ** 2) * g.dx ** 3
                if c == 0:
                    cells += int(keep.sum())
    assert cells <= 8192 and (layout != "base+patch" or cells == 16 ** 3 - 8 ** 3 + 16 ** 3)
    for c, name in enumerate(COMPONENTS):
        assert rep.max_norm[name] == mx[c] and mx[c] > 0, name
        np.testing.assert_allclose(rep.l2_norm[name], np.sqrt(sq[c]), rtol=1e-11)
    assert rep.max_ham_abs == mx[4]
    assert rep.relative_ham == mx[0] / mx[4]


@pytest.mark.gpu
def test_bowen_york_divergence_converges_at_second_order_on_the_device(comm):
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import PunctureSet
    norms = {}
    for n in (32, 64):
        lo, hi, dx, mask = _conv_case(n)
        grid = mg.Grid(comm, lo + hi, [lo + hi], dx)
        psi = mg.LevelData(grid)
        psi.set_val_all(1.0)
        got = _run(psi, BH, punctures=PunctureSet(_rows(TABLE_C)))
        norms[n] = [C.l2(got[1 + i][0], mask, dx) for i in range(3)]
        np.testing.assert_allclose(norms[n], _conv_reference(n), rtol=1e-9)
    ratios = [a / b for a, b in zip(norms[32], norms[64])]
    print("32^3 : 64^3 ratios of |Mom_i|_2 on the device", ratios)
    assert all(3.5 <= r <= 4.5 for r in ratios), ratios


def _attributes(fname):
    """Every attribute and the structure of a file, as h5dump -A prints them."""
    return h5read._run(["-A", fname]).split("\n", 1)[1]


@pytest.mark.gpu
def test_solve_reports_and_writes_the_constraints(comm, tmp_path):
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import Matter, PiProfile
    from mg_ic_code_amd.constraints import COMPONENTS, constraints
    from mg_ic_code_amd.nl import poisson_solve
    from mg_ic_code_amd.output import grchombo_vars
    from mg_ic_code_amd.phi import PhiProfile
    prm, n, _ = _sine_case()
    dom = (0, 0, 0, n - 1, n - 1, n - 1)
    grid = mg.Grid(comm, dom, [dom], prm.domainLength[0] / n, periodic=(1, 1, 1))
    matter = Matter(SP_4, PiProfile.from_function(_pi_4(prm)))
    plain, flagged = tmp_path / "plain", tmp_path / "flagged"
    res = {}
    for d, flag in ((plain, False), (flagged, True)):
        os.mkdir(d)
        res[flag] = poisson_solve(grid, prm, max_depth=2, max_NL_iterations=2,
                                  phi0=PhiProfile.sine(), matter=matter, output_dir=str(d),
                                  constraints=flag)
    # the solve itself does not change
    assert res[False].constraints is None
    assert res[True].linear_iterations == res[False].linear_iterations == [2, 2]
    assert res[True].dpsi_norms == res[False].dpsi_norms
    assert res[True].constant_K == res[False].constant_K and len(res[True].constant_K) == 2
    assert np.array_equal(res[True].psi.download(0, with_ghosts=True),
                          res[False].psi.download(0, with_ghosts=True))
    # the report is that of the returned psi
    rep = res[True].constraints
    K = res[True].constant_K[-1]
    again = constraints(res[True].psi, prm, phi0=PhiProfile.sine(), matter=matter, constant_K=K)
    assert again.max_norm == rep.max_norm and again.l2_norm == rep.l2_norm
    assert again.max_ham_abs == rep.max_ham_abs
    assert all(_same(_all(a), _all(b)) for a, b in zip(again.fields[0].fields(),
                                                       rep.fields[0].fields()))
    assert set(rep.max_norm) == set(COMPONENTS) and all(v > 0 for v in rep.max_norm.values())
    print("constraints of the 16^3 periodic solve:", rep.lines())
    # components 27-30 of the final file; everything else as without the flag
    shape = (31, n, n, n)
    files = [str(d / "vcPoissonFinal.3d.hdf5") for d in (plain, flagged)]
    d0, d1 = (h5read.dataset(f, "/level_0/data:datatype=0", "<f8").reshape(shape) for f in files)
    bh = prm.bh(constant_K=K)
    phi = PhiProfile.sine().fill(grid, prm)
    want = grchombo_vars(res[True].psi, 0, bh, phi=phi, matter=matter, constraints=True)
    assert np.array_equal(d1, want)
    for c in range(4):
        assert np.array_equal(d1[27 + c], rep.fields[0].fields()[c].download(0))
    assert np.array_equal(d1[:27], d0[:27]) and not np.any(d0[27:])
    assert h5read.contents(files[0]) == h5read.contents(files[1])
    assert _attributes(files[0]) == _attributes(files[1])
    assert h5read.boxes(files[0], 0) == h5read.boxes(files[1], 0)
    assert sorted(os.listdir(plain)) == sorted(os.listdir(flagged))


@pytest.mark.gpu
def test_run_poisson_cli_reports_the_constraints(comm, tmp_path):
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import Matter, PiProfile
    from mg_ic_code_amd.constraints import COMPONENTS
    from mg_ic_code_amd.nl import poisson_solve
    from mg_ic_code_amd.params import read_params_file
    from mg_ic_code_amd.phi import PhiProfile
    deck = tmp_path / "periodic.txt"
    with open(PARAMS) as f:
        txt = f.read()
    assert "is_periodic = 0" in txt and "max_NL_iterations = 6" in txt
    deck.write_text(txt.replace("is_periodic = 0", "is_periodic = 1")
                    .replace("max_NL_iterations = 6", "max_NL_iterations = 2"))
    V0, mass, lam = POT_4
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_poisson.py"), str(deck),
                          "--size", "16", "--max-depth", "2", "--phi", "sine", "--potential",
                          f"{V0!r} {mass!r} {lam!r}", "--pi", repr(PI_5), "--constraints"],
                         capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    print(out.stdout)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("constraint ")]
    num = r"([0-9]\.[0-9]{16}e[+-][0-9]{2})"
    # the same solve through the library
    prm = read_params_file(str(deck))
    n = 16
    dom = (0, 0, 0, n - 1, n - 1, n - 1)
    grid = mg.Grid(comm, dom, [dom], prm.domainLength[0] / n, periodic=(1, 1, 1))
    rep = poisson_solve(grid, prm, max_depth=2, phi0=PhiProfile.sine(),
                        matter=Matter(SP_4, PiProfile.constant(PI_5)), constraints=True).constraints
    assert len(lines) == 5
    for line, name in zip(lines, COMPONENTS):
        m = re.fullmatch(rf"constraint {name}: max = {num} L2 = {num}", line)
        assert m, line
        assert float(m.group(1)) == rep.max_norm[name] and float(m.group(2)) == rep.l2_norm[name]
    m = re.fullmatch(rf"constraint max\|Ham\| / max Ham_abs = {num}", lines[4])
    assert m and float(m.group(1)) == rep.relative_ham, lines[4]


@pytest.mark.gpu
def test_bad_arguments_are_refused_before_any_launch_or_file(comm, tmp_path):
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import Matter, PiProfile
    from mg_ic_code_amd._lib import call, io_call
    from mg_ic_code_amd.constraints import ConstraintFields, constraint_vars, set_constraints
    from mg_ic_code_amd.output import output_final_data
    g0, g1 = _grids(comm, "base+patch")
    psi, phi = mg.LevelData(g0), mg.LevelData(g0)
    psi.set_val_all(1.0)
    phi.set_val_all(0.1)
    out = ConstraintFields(g0)
    for f in out.fields():
        f.set_val(7.0)
    o = [f.handle for f in out.fields()]
    foreign, pi1 = mg.LevelData(g1), PiProfile.constant(0.1).fill(g1, BH)
    pi0 = PiProfile.constant(0.1).fill(g0, BH)
    ok = (ctypes.c_double * 3)(1e-3, 0.0, 0.0)
    nan = (ctypes.c_double * 3)(0.0, float("nan"), 0.0)
    bad_table = (ctypes.c_double * 10)(*([float("inf")] + [0.0] * 9))
    hs = (ctypes.c_void_p * 1)(psi.handle)
    h1 = (ctypes.c_void_p * 1)(pi1.handle)
    h0 = (ctypes.c_void_p * 1)(pi0.handle)
    rr = (ctypes.c_int * 1)(2)
    path = str(tmp_path / "x.hdf5")
    slab = np.full((4,) + _shape(g0.local_box(0)), 7.0)
    sptr = slab.ctypes.data_as(ctypes.c_void_p)

    def fields(*hh, table=(0, None), pi=None, pot=ok, p=psi.handle, ph=None):
        return lambda: call("mgic_field_constraints", p, ph, *hh, _bhv(BH), *table, pi, pot)

    def vars_(table=(0, None), pi=None, pot=ok, optr=sptr, box=0, k0=0, nk=1):
        return lambda: call("mgic_field_constraint_vars", psi.handle, None, box, k0, nk, _bhv(BH),
                            *table, pi, pot, optr, 0)

    def writer(table=(0, None), pi=None, pot=ok):
        return lambda: io_call("mgic_io_write_final_data_constraints", path.encode(), 1, hs, None,
                               _bhv(BH), *table, pi, pot, 0, rr)

    cases = [
        # what the _matter forms refuse: a non-finite coefficient, a count
        # without a table, a bad table, a Pi_0 of another layout
        (fields(*o, pot=nan), "finite"), (vars_(pot=nan), "finite"), (writer(pot=nan), "finite"),
        (fields(*o, table=(2, None)), "null argument"), (vars_(table=(2, None)), "null argument"),
        (writer(table=(2, None)), "null argument"),
        (fields(*o, table=(1, bad_table)), "finite"), (vars_(table=(1, bad_table)), "finite"),
        (writer(table=(1, bad_table)), "finite"),
        (fields(*o, table=(9, bad_table)), "puncture count"),
        (fields(*o, pi=pi1.handle), "pi"), (vars_(pi=pi1.handle), "pi"), (writer(pi=h1), "pi"),
        (lambda: set_constraints(psi, out, BH, potential=ScalarPotential(1e-3), pi=pi1), "pi"),
        (lambda: output_final_data([psi], BH, 0, [2], path, matter=Matter(SP, [pi1]),
                                   constraints=True), "pi"),
        # a Pi_0 without a potential
        (fields(*o, pi=pi0.handle, pot=None), "pi without pot"),
        (vars_(pi=pi0.handle, pot=None), "pi without pot"),
        (writer(pi=h0, pot=None), "pi without pot"),
        # a null psi or output, an output of another layout
        (fields(*o, p=None), "null argument"),
        (vars_(optr=None), "null argument"),
        (fields(*o, ph=foreign.handle), "phi"),
        (vars_(box=1), "box"), (vars_(k0=15, nk=2), "plane range"),
    ]
    for c in range(5):
        cases.append((fields(*(o[:c] + [None] + o[c + 1:])), "null argument"))
        cases.append((fields(*(o[:c] + [foreign.handle] + o[c + 1:])), "layout"))
        # aliased: an output that is an input, two outputs that are one field
        cases.append((fields(*(o[:c] + [psi.handle] + o[c + 1:])), "aliased"))
        cases.append((fields(*(o[:c] + [phi.handle] + o[c + 1:]), ph=phi.handle), "aliased"))
        cases.append((fields(*(o[:c] + [pi0.handle] + o[c + 1:]), pi=pi0.handle), "aliased"))
        cases.append((fields(*(o[:c] + [o[(c + 1) % 5]] + o[c + 1:])), "aliased"))
    for fn, what in cases:
        with pytest.raises(mg.MgicError) as ei:
            fn()
        assert ei.value.code == -1 and what in str(ei.value), (what, str(ei.value))
    assert os.listdir(tmp_path) == []                                   # no file was created
    assert all(np.all(f.download(0) == 7.0) for f in out.fields())      # nothing was launched
    assert np.all(slab == 7.0)
    assert np.all(psi.download(0) == 1.0) and np.all(phi.download(0) == 0.1)
    # and the calls these were made from do work
    fields(*o)()
    assert all(np.all(f.download(0) != 7.0) for f in out.fields())
    assert constraint_vars(psi, 0, BH, nk=1).shape == (4, 1, 16, 16)
