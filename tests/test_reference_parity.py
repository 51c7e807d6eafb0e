"""The oracle and the HIP drop-ins against the COMPILED reference.

Every other parity test of this suite ends at the oracle, a restatement of the
reference by the authors of the kernels it checks.  Here the other end is the
reference's own code, compiled: the seven ChomboFortran subroutines and
Source/SetLevelData.cpp with its headers (oracle/reference.py binds
oracle/_ref/libmgic_ref.so, built by oracle/ref/Makefile from a checkout of
the reference).

CPU    the oracle's kernels and level-data functions against the library, bit
       for bit (both sides use the same libm), on tests/reference_cases.py's
       case table; the numpy restatements of tests/ against it too.
fixture  tests/golden/reference_kernels.npz holds what the library wrote for a
       subset of the cases: the library reproduces it (needs the library), the
       oracle reproduces it (needs nothing -- this one protects a checkout that
       has neither the reference nor flang).
GPU    the six ChomboFortran drop-ins of include/mgic_chf.h bit for bit, and
       the device level-data functions to the tolerances the suite already
       uses for device transcendentals, against the library -- or, where the
       library did not travel, against the fixture (and, for the kernel cases
       the fixture does not hold, against the oracle the tests above pin).

A test that needs the library FAILS when the reference checkout is present
and the library is not; it skips only when both are absent.

Measured on the CPU: every oracle comparison is bit-identical;
the numpy restatements differ from the reference only through numpy's own exp,
log and pow: by at most 2 ULP of phi_0 and 1 ULP of the regrid condition.
"""
import numpy as np
import pytest

import oracle
from oracle import reference as ref
from tests import phi_ref, puncture_ref, regrid_ref
from tests import reference_cases as RC

KERNEL_CASES = [pytest.param(c.name, k, id=f"{c.name}-{k}")
                for c in RC.CASES for k in RC.KERNELS if RC.applies(k, c)]
DECKS = ("deck", "second")


def _need_library():
    if ref.available():
        return
    if ref.checkout_present():
        pytest.fail("the reference checkout is at " + ref.reference_dir() + " but " + ref.LIB +
                    " is not built: run __graft_entry__.build()")
    pytest.skip("neither a reference checkout (" + ref.reference_dir() +
                ", MGIC_REFERENCE_DIR) nor " + ref.LIB)


@pytest.fixture
def library():
    _need_library()
    ref.mayday_reset()
    yield ref
    assert ref.mayday_count() == 0, "the reference called MayDay / CH_assert"


@pytest.fixture(scope="module")
def fixture_file():
    with np.load(RC.FIXTURE) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def decks():
    return RC.decks()


def assert_bits(got, want, what=""):
    """NaN where NaN, and the same bits everywhere else (so -0.0 is not 0.0)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN in different cells"
    g, w = got.view(np.uint64)[~nan], want.view(np.uint64)[~nan]
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (f"{what}: {bad.size} of {g.size} values differ, first "
                           f"{got[~nan][bad[0]]!r} != {want[~nan][bad[0]]!r}")


def ulps(a, b):
    """Largest distance of two finite arrays in units in the last place."""
    def ordered(x):
        i = np.ascontiguousarray(x, dtype=np.float64).view(np.int64)
        return np.where(i < 0, np.int64(-2 ** 63) - i, i)
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
    return int(np.max(np.abs(ordered(a) - ordered(b))))


# ------------------------------------------------------------------ CPU: kernels
@pytest.mark.parametrize("case, kernel", KERNEL_CASES)
def test_oracle_kernel_is_the_compiled_fortran(library, case, kernel):
    c = RC.CASE[case]
    d = RC.inputs(c)
    want = RC.run_abi(kernel, c, d)
    assert_bits(RC.run_oracle(kernel, c, d), want, f"{case} {kernel}")
    # the case does what it is there for: a region with cells writes, an empty
    # one leaves everything alone, and restriction adds to what res held
    if kernel in ("gsrb0", "gsrb1"):
        before = d["u"]
    elif kernel in ("lap", "grad"):
        before = d["out0"][0]
    else:
        before = {"restrict_zero": np.zeros_like(want), "restrict_nonzero": d["res0"]}.get(
            kernel, d["out0"])
    assert np.array_equal(want, before, equal_nan=True) == c.empty
    if kernel == "restrict_nonzero" and not c.empty:
        zero = RC.run_abi("restrict_zero", c, d)
        assert not np.array_equal(want, zero, equal_nan=True)


def test_thin_region_has_rows_without_a_cell_of_one_colour(library):
    # 1 x 5 x 4: every row holds one cell, so each colour skips half the rows
    c = RC.CASE["1x5x4-thin"]
    d = RC.inputs(c)
    for rb in (0, 1):
        changed = (RC.run_abi(f"gsrb{rb}", c, d) != d["u"])[0, 1:-1, 1:-1, 1]
        j, k = np.meshgrid(np.arange(c.n[1]) + c.lo[1], np.arange(c.n[2]) + c.lo[2])
        assert np.array_equal(changed, (c.lo[0] + j + k + rb) % 2 == 0)


def test_sumfaces_translates_and_runs(library):
    # dead in the reference, translated all the same: lhs += scale * beta * (b(i + e_dir) + b(i))
    rng = np.random.default_rng(3)
    lo, n = (2, -1, 3), (5, 4, 3)
    hi = tuple(lo[d] + n[d] - 1 for d in range(3))
    lhs0 = rng.uniform(-1, 1, (2,) + n[::-1])
    for direction in range(3):
        b = rng.uniform(0.5, 2, (2,) + tuple(n[d] + (d == direction) for d in (2, 1, 0)))
        lhs = lhs0.copy()
        ref.sumfaces(ref.Fab(lhs, lo), -1.3, ref.Fab(b, lo), lo, hi, direction, 0.25)
        up = b[(slice(None),) + tuple(slice(1, None) if d == direction else slice(None)
                                      for d in (2, 1, 0))]
        low = b[(slice(None),) + tuple(slice(0, -1) if d == direction else slice(None)
                                       for d in (2, 1, 0))]
        assert_bits(lhs, lhs0 + 0.25 * -1.3 * (up + low), f"sumfaces dir {direction}")


def test_mayday_is_recorded_and_does_not_abort():
    # GSRBHELMHOLTZVC3D with rhs of another ncomp: the Fortran calls MAYDAYERROR,
    # which here sets a flag the binding reads, and the sweep still runs on
    # the one component dpsi has
    _need_library()
    c = RC.CASE["8x6x4-at-0"]
    d = RC.inputs(c)
    rlo, rhi = RC.region(c)
    F = ref.Fab
    ref.mayday_reset()
    rhs = F(np.stack([d["rhs"][0]] * 2), c.lo)
    u = F(d["u"].copy(), tuple(l - 1 for l in c.lo))
    ref.gsrb(u, rhs, rlo, rhi, c.dx, c.alpha, F(d["a"].copy(), c.lo), c.beta, F(d["b"].copy(), c.lo),
             F(d["lam"].copy(), c.lo), 0)
    assert ref.mayday_count() == 1
    ref.mayday_reset()
    assert ref.mayday_count() == 0
    assert_bits(u.arr, RC.run_abi("gsrb0", c, d), "the sweep after MAYDAYERROR")


_CHF_SAMPLE = """\
C     a comment
#include "CONSTANTS.H"
#if CH_SPACEDIM == 2
      subroutine WRONGDIM(CHF_FRA1[a])
#elif CH_SPACEDIM == 3
      subroutine SAMPLE(
     &     CHF_FRA[a],
     &     CHF_CONST_FRA1[b],
     $     CHF_BOX[region],
     &     CHF_CONST_REAL[dx],
     &     CHF_CONST_INT[dir])
#endif
      REAL_T s
      integer n, CHF_DDECL[i;j;k], CHF_AUTODECL[ii]
      CHF_DTERM[
      ii0 = CHF_ID(0,dir);
      ii1 = CHF_ID(1,dir);
      ii2 = CHF_ID(2,dir)]
      do n = 0, CHF_NCOMP[a]-1
        CHF_MULTIDO[region; i; j; k]
          s = half*dx * CHF_DTERM[
     &        b(CHF_IX[i+1;j;k]) ;
     &      + b(CHF_OFFSETIX[i;-2*ii]) ;
     &      + b(CHF_IX[i;j;CHF_UBOUND[region;2]])] / D_TERM(2, *2, *2)
          a(CHF_IX[i;j;k],n) = a(CHF_IX[i;j;k],n) + s + two*b(CHF_LBOUND[b;0],j,k) + a_very_long_name_that_runs_past_column_72
        CHF_ENDDO
      enddo
      return
      end
"""


def test_translator_expands_the_documented_macros():
    # needs neither the reference nor a compiler: the ChomboFortran-to-Fortran
    # translator on a sample of ours that uses every construct it covers
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location(
        "chf2f", os.path.join(os.path.dirname(oracle.__file__), "ref", "chf2f.py"))
    chf2f = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chf2f)
    out = chf2f.translate(_CHF_SAMPLE)
    lines = out.splitlines()
    assert all(len(ln) <= 72 for ln in lines)
    # continuation lines joined again, blanks dropped: what a compiler reads
    flat = ""
    for ln in lines[1:]:
        flat += ("" if ln[5] != " " else "\n") + ln[6:]
    flat = flat.replace(" ", "").lower()
    assert "wrongdim" not in flat and "chf_" not in flat and "#" not in flat
    # the argument order of the generated C ABI: pointer, lo0..2, hi0..2, ncomp
    assert ("subroutinesample(a,ialo0,ialo1,ialo2,iahi0,iahi1,iahi2,nacomp,"
            "b,iblo0,iblo1,iblo2,ibhi0,ibhi1,ibhi2,"
            "iregionlo0,iregionlo1,iregionlo2,iregionhi0,iregionhi1,iregionhi2,dx,dir)") in flat
    assert "real*8a(ialo0:iahi0,ialo1:iahi1,ialo2:iahi2,0:nacomp-1)" in flat
    assert "real*8b(iblo0:ibhi0,iblo1:ibhi1,iblo2:ibhi2)\n" in flat
    assert "integern,i,j,k,ii0,ii1,ii2\n" in flat and "real*8s\n" in flat
    assert "\nii1=(1-min(1,abs((1)-(dir))))\n" in flat
    assert "don=0,nacomp-1\ndok=iregionlo2,iregionhi2\ndoj=iregionlo1,iregionhi1\ndoi=iregionlo0,iregionhi0\n" in flat
    assert ("s=0.500d0*dx*b(i+1,j,k)+b(i0-2*ii0,i1-2*ii1,i2-2*ii2)+b(i,j,iregionhi2)/2*2*2\n") in flat
    assert "+2.0d0*b(iblo0,j,k)+a_very_long_name_that_runs_past_column_72\n" in flat
    assert flat.count("enddo") == 4
    with pytest.raises(chf2f.ChFError):
        chf2f.translate("      x = CHF_UNHEARD_OF[a]\n")


# ------------------------------------------------------------------ CPU: level data
def _level(bh, part="full"):
    lo, hi = RC.level_box(part)
    return lo, hi, bh["domain_length"] / RC.LEVEL_N


@pytest.fixture(scope="module")
def level_ref(decks):
    """The compiled reference's level data for both decks, computed once."""
    if not ref.available():
        return None
    return {name: RC.level_reference(bh, *RC.level_box("full")) for name, bh in decks.items()}


@pytest.mark.parametrize("deck", DECKS)
def test_oracle_level_data_is_the_compiled_setleveldata(library, level_ref, decks, deck):
    bh = decks[deck]
    lo, hi, dx = _level(bh)
    R = level_ref[deck]
    pg, pv = RC.psi_on(lo, hi), RC.psi_on(lo, hi, 0)
    a, r = oracle.nl_coefs(bh, lo, hi, dx, pg)
    assert_bits(a, R["acoef"], "set_a_coef")
    assert_bits(r, R["rhs"], "set_rhs")
    assert_bits(oracle.nl_integrand(bh, lo, hi, dx, pg), R["integrand"], "set_constant_K_integrand")
    assert_bits(oracle.output_vars(0, bh, lo, hi, dx, pv), R["output"], "set_output_data")
    # psi = 1, as set_initial_conditions leaves it: oracle.binary_bh
    a1, r1 = ref.nl_coefs(bh, lo, hi, dx, None)
    a0, r0 = oracle.binary_bh(bh, lo, hi, dx)
    assert_bits(a0, a1, "set_a_coef at psi = 1")
    assert_bits(r0, r1, "set_rhs at psi = 1")
    # the solver output's multigrid_vars components (kind 1): A_ij_0 and phi_0
    s = oracle.output_vars(1, bh, lo, hi, dx, pv, pv, pv)
    mv = R["multigrid_vars"][:, 1:-1, 1:-1, 1:-1]
    assert_bits(s[3:10], mv[1:8], "set_initial_conditions A_ij_0, phi_0")
    assert bh["constant_K"] == 0.0 or np.all(R["output"][7] == bh["constant_K"])


@pytest.mark.parametrize("deck", DECKS)
def test_numpy_restatements_are_the_compiled_setleveldata(library, level_ref, decks, deck):
    bh = decks[deck]
    lo, hi, dx = _level(bh)
    R = level_ref[deck]
    L = bh["domain_length"]
    mv = R["multigrid_vars"]
    inner = mv[:, 1:-1, 1:-1, 1:-1]
    # set_initial_conditions leaves psi = 1 (replaced by the caller's psi here)
    # and dpsi = 0, and writes every cell of its box, ghosts included
    mv1, dpsi = ref.initial_conditions(bh, [l - 1 for l in lo], [h + 1 for h in hi], dx)
    assert np.all(mv1[0] == 1.0) and np.all(dpsi == 0.0) and not np.any(np.isnan(mv1))
    assert_bits(mv1[1:], mv[1:], "multigrid_vars")
    # Bowen-York A_ij and psi_bh: +, -, *, / and sqrt only -- bit for bit, from
    # the two-row table and from the two-hole form
    table = puncture_ref.deck_table(bh)
    A, psi_bh = puncture_ref.bowen_york(table, L, lo, hi, dx)
    for n, ij in enumerate(puncture_ref.IJ):  # the enum's order: A11 A12 A13 A22 A23 A33
        assert_bits(A[ij], inner[1 + n], f"A{ij[0] + 1}{ij[1] + 1}_0")
    assert np.any(inner[1:7] != 0.0)
    assert_bits(psi_bh, R["psi_bh"], "set_binary_bh_psi (table)")
    A2, psi_bh2 = phi_ref.bowen_york(bh, lo, hi, dx)
    assert_bits(psi_bh2, R["psi_bh"], "set_binary_bh_psi (two holes)")
    assert_bits(A2, puncture_ref.contract({ij: inner[1 + n] for n, ij in enumerate(puncture_ref.IJ)}),
                "A_ij A^ij")
    # phi_0, ghosts included: numpy's exp against libm's -- the same text, two
    # implementations of exp, and a multiplication that can double their distance
    phi = phi_ref.phi_on_box(phi_ref.gaussian, bh, lo, hi, dx)
    d = ulps(phi, mv[ref.C_PHI_0])
    print(deck, "phi_0: numpy against the reference, ULPs", d)
    assert d <= PHI0_ULPS + 1
    assert np.any(phi != 0.0) and (deck == "deck" or np.all(phi != 0.0))
    # the regrid condition: pow(psi_0, -7), log(psi_0) through numpy, the rest
    # as the reference writes it
    pv = RC.psi_on(lo, hi, 0)
    for name, cond in (("regrid_ref", regrid_ref.regrid_condition(bh, lo, hi, dx, pv)),
                       ("puncture_ref", puncture_ref.regrid_condition(bh, table, lo, hi, dx, pv))):
        d = ulps(cond, R["regrid"])
        print(deck, name, "regrid condition: numpy against the reference, ULPs", d)
        assert d <= REGRID_ULPS + 1


def test_small_functions_of_the_compiled_setleveldata(library, decks):
    bh = decks["second"]
    # set_m_value: m = 2/3 K^2 - 16 pi G rho with rho = 0 (phi_here is unused)
    for K in (0.0, 0.12, -3.5):
        want = (2.0 / 3.0) * (K * K) - 16.0 * np.pi * bh["G_Newton"] * 0.0
        assert ref.m_value(bh, 0.3, K) == want
    # set_update_psi0: psi += dpsi over the whole multigrid_vars box, nothing else touched
    rng = np.random.default_rng(8)
    lo, n = (-2, 3, 1), (5, 4, 3)
    mv = rng.uniform(-1, 1, (8,) + n[::-1])
    dpsi = rng.uniform(-1, 1, tuple(v + 2 for v in n[::-1]))
    got = mv.copy()
    ref.update_psi0(got, lo, dpsi, [l - 1 for l in lo])
    assert_bits(got[0], mv[0] + dpsi[1:-1, 1:-1, 1:-1], "set_update_psi0")
    assert_bits(got[1:], mv[1:], "set_update_psi0 leaves the other components")
    # get_Aij on its own, every component, against the loops of tests/phi_ref.py
    r1, r2 = 1.7, 0.9
    n1, n2 = np.array([0.6, -0.48, 0.64]), np.array([-0.28, 0.96, 0.0])
    J1, J2, P1, P2 = (0.1, -0.2, 0.3), (0.0, 0.05, -0.4), (0.03, 0.2, -0.1), (-0.3, 0.0, 0.07)
    for i in range(3):
        for j in range(3):
            want = phi_ref._get_Aij(i, j, r1, r2, n1, n2, J1, J2, P1, P2)
            assert ref.get_Aij(bh, i, j, r1, r2, n1, n2, J1, J2, P1, P2) == want, (i, j)
    # my_phi_function and set_binary_bh_psi at one point
    loc = (3.125, -9.375, 15.625)
    assert ref.binary_bh_psi(bh, loc) == float(phi_ref.bowen_york(
        bh, (8, 6, 10), (8, 6, 10), bh["domain_length"] / RC.LEVEL_N)[1][0, 0, 0])
    assert ulps(np.array([ref.my_phi_function(loc, 0.05, 40.0, 100.0)]),
                np.array([phi_ref.gaussian(bh, *loc)])) <= PHI0_ULPS + 1


# the largest distances measured on the CPU between the numpy restatements and
# the compiled reference, over both decks (cause: numpy's own exp, log and pow
# against libm's); the assertions add one ULP of margin for a
# libm build that differs
PHI0_ULPS = 2    # phi_ref.gaussian against my_phi_function (0 on params.txt's deck)
REGRID_ULPS = 1  # regrid_ref / puncture_ref against set_regrid_condition


# ------------------------------------------------------------------ the fixture
def _fixture_kernel_items(fixture_file):
    for name in RC.FIXTURE_KERNEL_CASES:
        c = RC.CASE[name]
        d = RC.inputs(c)
        for k, v in d.items():  # the inputs the file records are the ones the cases generate
            assert_bits(v, fixture_file[RC.fixture_key("kernel", name, "in", k)], f"{name} input {k}")
        for kernel in RC.KERNELS:
            if RC.applies(kernel, c):
                yield c, d, kernel, fixture_file[RC.fixture_key("kernel", name, "out", kernel)]


def test_fixture_holds_one_case_per_kernel_and_level_function(fixture_file):
    for name in RC.FIXTURE_KERNEL_CASES:
        for kernel in RC.KERNELS:
            assert RC.fixture_key("kernel", name, "out", kernel) in fixture_file
    for deck in DECKS:
        for func in RC.LEVEL_FUNCS:
            assert RC.fixture_key("level", deck, func) in fixture_file
    import os
    assert os.path.getsize(RC.FIXTURE) <= 204 * 1024


def test_library_reproduces_the_fixture(library, fixture_file, decks):
    for c, d, kernel, want in _fixture_kernel_items(fixture_file):
        assert_bits(RC.run_abi(kernel, c, d), want, f"{c.name} {kernel}")
    lo, hi = RC.LEVEL_FIXTURE_BOX
    for deck in DECKS:
        got = RC.level_reference(decks[deck], lo, hi)
        got["multigrid_vars"] = got["multigrid_vars"][:, 1:-1, 1:-1, 1:-1]
        for func in RC.LEVEL_FUNCS:
            assert_bits(got[func], fixture_file[RC.fixture_key("level", deck, func)], f"{deck} {func}")


def test_oracle_reproduces_the_fixture(fixture_file, decks):
    # needs neither the reference nor flang: never skips
    for c, d, kernel, want in _fixture_kernel_items(fixture_file):
        assert_bits(RC.run_oracle(kernel, c, d), want, f"{c.name} {kernel}")
    lo, hi = RC.LEVEL_FIXTURE_BOX
    pg, pv = RC.psi_on(lo, hi), RC.psi_on(lo, hi, 0)
    assert_bits(pg, fixture_file[RC.fixture_key("level", "in", "psi")], "psi")
    for deck in DECKS:
        bh = decks[deck]
        dx = bh["domain_length"] / RC.LEVEL_N
        want = {f: fixture_file[RC.fixture_key("level", deck, f)] for f in RC.LEVEL_FUNCS}
        a, r = oracle.nl_coefs(bh, lo, hi, dx, pg)
        assert_bits(a, want["acoef"], f"{deck} set_a_coef")
        assert_bits(r, want["rhs"], f"{deck} set_rhs")
        assert_bits(oracle.nl_integrand(bh, lo, hi, dx, pg), want["integrand"], f"{deck} integrand")
        assert_bits(oracle.output_vars(0, bh, lo, hi, dx, pv), want["output"], f"{deck} output")
        s = oracle.output_vars(1, bh, lo, hi, dx, pv, pv, pv)
        assert_bits(s[3:10], want["multigrid_vars"][1:8], f"{deck} A_ij_0, phi_0")
        assert_bits(s[2], want["multigrid_vars"][0], f"{deck} psi")
        table = puncture_ref.deck_table(bh)
        _, psi_bh = puncture_ref.bowen_york(table, bh["domain_length"], lo, hi, dx)
        assert_bits(psi_bh, want["psi_bh"], f"{deck} psi_bh")
        cond = regrid_ref.regrid_condition(bh, lo, hi, dx, pv)
        assert ulps(cond, want["regrid"]) <= REGRID_ULPS + 1


# ------------------------------------------------------------------ GPU
class _Expected:
    """What the compiled reference gives: from the library where it travelled
    with the tree, else from the fixture."""

    def __init__(self):
        self.library = ref.available()
        if not self.library and ref.checkout_present():
            pytest.fail("reference checkout present, " + ref.LIB + " not built")
        with np.load(RC.FIXTURE) as f:
            self.file = {k: f[k] for k in f.files}
        print("\nreference parity on the GPU: expected values from",
              "the compiled library " + ref.LIB if self.library else "the fixture " + RC.FIXTURE)

    def kernel(self, c, d, kernel):
        if self.library:
            return RC.run_abi(kernel, c, d)
        key = RC.fixture_key("kernel", c.name, "out", kernel)
        if key not in self.file:
            # neither the library nor a recorded output: the oracle, which the
            # CPU tests and the fixture hold to the reference bit for bit
            return RC.run_oracle(kernel, c, d)
        for k, v in d.items():
            assert_bits(v, self.file[RC.fixture_key("kernel", c.name, "in", k)], "fixture input " + k)
        return self.file[key]

    def level(self, decks, deck):
        """(box, values): the whole 16^3 lattice from the library, the
        fixture's part of it otherwise; multigrid_vars over the box itself."""
        part = "full" if self.library else "fixture"
        lo, hi = RC.level_box(part)
        if self.library:
            v = RC.level_reference(decks[deck], lo, hi)
            v["multigrid_vars"] = v["multigrid_vars"][:, 1:-1, 1:-1, 1:-1]
        else:
            v = {f: self.file[RC.fixture_key("level", deck, f)] for f in RC.LEVEL_FUNCS}
        return (lo, hi), v


@pytest.fixture(scope="module")
def expected():
    return _Expected()


@pytest.fixture(scope="module")
def mg():
    return pytest.importorskip("mg_ic_code_amd")


@pytest.fixture(scope="module")
def comm(mg):
    return mg.Comm()


@pytest.mark.gpu
@pytest.mark.parametrize("case, kernel", KERNEL_CASES)
def test_hip_dropin_is_the_compiled_fortran(mg, expected, case, kernel):
    c = RC.CASE[case]
    d = RC.inputs(c)
    want = expected.kernel(c, d, kernel)
    assert_bits(RC.run_abi(kernel, c, d, abi=mg.lib), want, f"{case} {kernel}")


def _cut(arr, box):
    (lo, hi) = box
    return arr[..., lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1]


@pytest.fixture(scope="module")
def device_level(mg, comm, decks):
    """The device's level data on the 16^3 lattice at level_psi(), per deck."""
    from mg_ic_code_amd.grids import set_regrid_condition
    from mg_ic_code_amd.nl import set_nl_integrand
    from mg_ic_code_amd.output import grchombo_vars
    from mg_ic_code_amd.phi import PhiProfile
    from mg_ic_code_amd.punctures import (PunctureSet, set_nl_coefs_punct, set_nl_integrand_punct,
                                          set_regrid_condition_punct)
    n = RC.LEVEL_N
    dom = (0, 0, 0, n - 1, n - 1, n - 1)
    out = {}
    for deck, bh in decks.items():
        grid = mg.Grid(comm, dom, [dom], bh["domain_length"] / n)
        psi = mg.LevelData(grid)
        psi.upload(0, RC.level_psi(), with_ghosts=True)
        f = {k: mg.LevelData(grid) for k in ("acoef", "rhs", "integrand", "regrid", "acoef_t",
                                             "rhs_t", "integrand_t", "regrid_t")}
        mg.set_nl_coefs(psi, f["acoef"], f["rhs"], bh)
        set_nl_integrand(psi, f["integrand"], bh)
        set_regrid_condition(psi, f["regrid"], bh)
        table = PunctureSet.from_params(bh)
        assert np.array_equal(np.asarray(table.table()).reshape(-1, 10), puncture_ref.deck_table(bh))
        set_nl_coefs_punct(psi, f["acoef_t"], f["rhs_t"], bh, table)
        set_nl_integrand_punct(psi, f["integrand_t"], bh, table)
        set_regrid_condition_punct(psi, f["regrid_t"], bh, table)
        v = {k: x.download(0) for k, x in f.items()}
        v["output"] = grchombo_vars(psi, 0, bh)
        v["output_t"] = grchombo_vars(psi, 0, bh, punctures=table)
        v["phi"] = PhiProfile.gaussian().fill(grid, bh).download(0, with_ghosts=True)
        out[deck] = v
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["two_holes", "table"])
@pytest.mark.parametrize("deck", DECKS)
def test_device_level_data_matches_compiled_setleveldata(expected, device_level, decks, deck, form):
    box, want = expected.level(decks, deck)
    t = "_t" if form == "table" else ""
    got = {k: _cut(device_level[deck][k + t], box) for k in ("acoef", "rhs", "integrand", "regrid",
                                                            "output")}
    for k in ("acoef", "rhs", "integrand", "regrid"):
        scale = np.abs(want[k]).max()
        print(deck, form, k, "max |err| / max |ref|", np.max(np.abs(got[k] - want[k])) / scale,
              "max rel err", np.max(np.abs(got[k] - want[k]) / np.abs(want[k])))
    # the tolerances of test_nl_coefs_on_device_match_oracle (aCoef, rhs),
    # test_phi_field.py (integrand), test_regrid.py and test_output.py
    np.testing.assert_allclose(got["acoef"], want["acoef"], rtol=1e-13, atol=1e-300)
    np.testing.assert_allclose(got["rhs"], want["rhs"], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(got["integrand"], want["integrand"], rtol=0,
                               atol=1e-13 * np.abs(want["integrand"]).max())
    np.testing.assert_allclose(got["regrid"], want["regrid"], rtol=1e-13, atol=1e-300)
    exact = [c for c in range(31) if c not in (0, 8, 9, 10, 11, 12, 13, 25)]
    assert_bits(got["output"][exact], want["output"][exact], "set_output_data's constants")
    np.testing.assert_allclose(got["output"], want["output"], rtol=1e-13, atol=1e-300)


@pytest.mark.gpu
@pytest.mark.parametrize("deck", DECKS)
def test_device_fill_phi_matches_compiled_my_phi_function(expected, device_level, decks, deck):
    # test_phi_field.py's bound for the Gaussian: 1e-13 relative
    box, want = expected.level(decks, deck)
    phi = _cut(device_level[deck]["phi"][1:-1, 1:-1, 1:-1], box)
    ref_phi = want["multigrid_vars"][ref.C_PHI_0]
    with np.errstate(divide="ignore", invalid="ignore"):
        print(deck, "fill_phi (Gaussian) max rel err where phi_0 is a normal number",
              np.nanmax(np.where(np.abs(ref_phi) > 2.3e-308, np.abs(phi - ref_phi) / np.abs(ref_phi), 0)))
    # the deck's narrow Gaussian underflows far from the centre: there one
    # step of the subnormal grid (2^-1074) is all the precision the format has
    np.testing.assert_allclose(phi, ref_phi, rtol=1e-13, atol=2.0 ** -1074)
    if expected.library:  # the ghost layer too: set_initial_conditions fills its whole box
        lo, hi = box
        bh = decks[deck]
        mv, _ = ref.multigrid_vars(bh, lo, hi, bh["domain_length"] / RC.LEVEL_N)
        np.testing.assert_allclose(device_level[deck]["phi"], mv[ref.C_PHI_0], rtol=1e-13,
                                   atol=2.0 ** -1074)
