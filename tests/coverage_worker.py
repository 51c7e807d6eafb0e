"""Worker for tests/test_launch_coverage.py: one fresh interpreter per kernel
family (and per environment a family needs).  Runs the family's cases, each
against its reference with the suite's own bars (== / np.array_equal against
oracle.OracleMG and oracle.mixed.MixedOracle; the host loop for the device
BiCGStab), then dumps the launch ledger.  Any mismatch is an AssertionError:
the exit code is non-zero.

    python tests/coverage_worker.py FAMILY PART LEDGER_PATH

FAMILIES maps a family to the pattern its kernel names match: every ledger
entry belongs to exactly one family (test_ledger_loads_without_a_device).
PARTS lists, per family with cases here, the (part name, environment) runs
whose ledgers together must reach every entry of the family.
"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FAMILIES = {
    "tb2_fp64": r"k_gsrb_tb2<double,",
    "tb2_fp32": r"k_gsrb_tb2<float,",
    "sweep": r"k_gsrb(_fused6|_block|_fused_rst)?<",
    "stencil": r"k_(apply_op|residual_zl|restrict_zl|prolong|average|lambda|fill_bc_face|"
               r"copy_items|to_float|incr_f|copy_f|incr_grown)\b",
    "blas": r"k_(blas|reduce_partial|reduce_final|reduce_final_wide|axpy2_reduce|dot2|bicg_p)\b",
    "bicgd": r"k_bicgd_",
    "generators": r"k_(binary_bh|output_vars|constraints|fill_phi|lap_psi|rho_grad_phi)\b",
    "amr": r"k_(cf_interp|regrid_condition|tag_lattice)\b",
    # (k_publish: Comm::allreduce's last step on the RCCL transport, the
    # counterpart of k_ipc_allreduce; only a run of several ranks launches it)
    "transport": r"k_(exchange|ipc_allreduce|publish)\b",
}

# family -> ((part, environment), ...)
PARTS = {
    "tb2_fp64": (("untrimmed", {}), ("trimmed", {"MGIC_TB2_TRIM": "15"})),
    "tb2_fp32": (("all", {}),),
    "sweep": (("all", {}),),
    "stencil": (("all", {}),),
    "bicgd": (("all", {}),),
    "blas": (("all", {}),),
    "generators": (("all", {}),),
    "amr": (("all", {}),),
}
# the transport family's kernels need several ranks: tests/mp_worker.py, from
# test_launch_coverage.py::test_transport_family_launches_every_instantiation
MULTI_RANK = ("transport",)


def family_of(name):
    """The families whose pattern matches a ledger entry's name."""
    return [f for f, pat in FAMILIES.items() if re.match(pat, name)]


# ------------------------------------------------------------------ builders
DIRI0 = dict(bc_lo=(0, 0, 0), bc_hi=(0, 0, 0), bc_value=0.0)         # one ghost rule
MIXED = dict(bc_lo=(0, 1, 1), bc_hi=(1, 0, 0), bc_value=0.5)         # several, with a value


def _dom(shape):
    return (0, 0, 0, shape[0] - 1, shape[1] - 1, shape[2] - 1)


def _arrays(rng, shape, bvar, bval=1.0):
    nx, ny, nz = shape
    a = rng.uniform(-2.0, -0.5, (nz, ny, nx))
    b = rng.uniform(0.5, 2.0, (nz, ny, nx)) if bvar else np.full((nz, ny, nx), bval)
    rhs = rng.uniform(-1, 1, (nz, ny, nx))
    return a, b, rhs


def _slab(arr, bx):
    return np.ascontiguousarray(arr[bx[2]:bx[5] + 1, bx[1]:bx[4] + 1, bx[0]:bx[3] + 1])


def _upload(f, grid, arr):
    for n in range(grid.num_local):
        f.upload(n, _slab(arr, grid.local_box(n)))


def _download(f, grid, shape):
    out = np.zeros(shape[::-1])
    for n in range(grid.num_local):
        b = grid.local_box(n)
        out[b[2]:b[5] + 1, b[1]:b[4] + 1, b[0]:b[3] + 1] = f.download(n)
    return out


def _gpu(comm, shape, dx, a, b, rhs, *, alpha, beta, bc, fused, avg=1, prolong=1, boxes=None):
    dom = _dom(shape)
    grid = mg.Grid(comm, dom, boxes or [dom], dx)
    fa, fb, frhs, fphi, fres = (mg.LevelData(grid) for _ in range(5))
    for f, arr in ((fa, a), (fb, b), (frhs, rhs)):
        _upload(f, grid, arr)
    fphi.set_zero()
    prm = mg.OperatorParams(alpha=alpha, beta=beta, coefficient_average_type=avg,
                            prolong_type=prolong, fused_smoother=fused, **bc)
    fac = mg.defineOperatorFactory(grid, fa, fb, prm)
    return dict(grid=grid, fa=fa, fb=fb, frhs=frhs, fphi=fphi, fres=fres, fac=fac, shape=shape)


def _oracle(shape, dx, a, b, rhs, *, alpha, beta, bc, levels, avg=1, prolong=1, n_pre=4, n_post=4,
            n_bottom=4):
    dom = _dom(shape)
    o = oracle.OracleMG([dom], dom, dx, alpha=alpha, beta=beta, nlevels=levels, avg_type=avg,
                        prolong_type=prolong, n_pre=n_pre, n_post=n_post, n_bottom=n_bottom,
                        bottom_solver=0, **bc)
    for f, arr in ((oracle.ACOEF, a), (oracle.BCOEF, b), (oracle.RHS, rhs)):
        o.set(0, f, 0, arr)
    o.setup()
    return o


def vcycle64(comm, rng, shape, *, alpha=1.0, beta=-1.0, bc=DIRI0, bvar=False, fused=2, levels=2,
             n_pre=4, n_post=4, avg=1, prolong=1, boxes=None, iters=2):
    """AMRMultiGrid iterations against the oracle: every norm and phi bit for bit."""
    dx = 0.7
    a, b, rhs = _arrays(rng, shape, bvar)
    S = _gpu(comm, shape, dx, a, b, rhs, alpha=alpha, beta=beta, bc=bc, fused=fused, avg=avg,
             prolong=prolong, boxes=boxes)
    sp = mg.SolverParams(max_depth=levels - 1, bottom_solver=0, n_pre=n_pre, n_post=n_post,
                         n_bottom=n_pre + n_post)
    amg = mg.AMRMultiGrid(S["fac"], sp)
    assert amg.num_depths == levels, (shape, amg.num_depths)
    o = _oracle(shape, dx, a, b, rhs, alpha=alpha, beta=beta, bc=bc, levels=levels, avg=avg,
                prolong=prolong, n_pre=n_pre, n_post=n_post, n_bottom=n_pre + n_post)
    what = ("vcycle64", shape, alpha, beta, bc, bvar, fused, n_pre, n_post, avg, prolong)
    assert amg.init_residual(S["fphi"], S["frhs"], S["fres"], 0) == o.init_residual(0), what
    for _ in range(iters):
        assert amg.iteration(S["fphi"], S["frhs"], S["fres"], 0) == o.iteration(0), what
    assert np.array_equal(_download(S["fphi"], S["grid"], shape), o.get(0, oracle.PHI, 0)), what


def vcycle32(comm, rng, shape, *, alpha=1.0, beta=-1.0, bc=DIRI0, bvar=False, fused=2, levels=2,
             n_pre=4, n_post=4, n_bottom=None, avg=1, prolong=1, boxes=None, iters=2):
    """MixedMultiGrid iterations against the float32 restatement, bit for bit.
    With `boxes`, the multi-box layout against the same single-box restatement."""
    dx = 0.3
    n_bottom = n_pre + n_post if n_bottom is None else n_bottom
    a, b, rhs = _arrays(rng, shape, bvar)
    S = _gpu(comm, shape, dx, a, b, rhs, alpha=alpha, beta=beta, bc=bc, fused=fused, avg=avg,
             prolong=prolong, boxes=boxes)
    sp = mg.SolverParams(max_depth=levels - 1, bottom_solver=0, n_pre=n_pre, n_post=n_post,
                         n_bottom=n_bottom)
    mm = mg.MixedMultiGrid(S["fac"], sp)
    assert mm.num_depths == levels, (shape, mm.num_depths)
    o = _oracle(shape, dx, a, b, rhs, alpha=alpha, beta=beta, bc=bc, levels=levels, avg=avg,
                prolong=prolong)
    m = MixedOracle(o, alpha, beta, bc["bc_lo"], bc["bc_hi"], n_pre=n_pre, n_post=n_post,
                    n_bottom=n_bottom, prolong_type=prolong)
    what = ("vcycle32", shape, alpha, beta, bc, bvar, fused, n_pre, n_post, avg, prolong)
    assert mm.init_residual(S["fphi"], S["frhs"], S["fres"], 0) == \
        np.abs(m.init_residual(np.zeros(shape[::-1]))).max(), what
    for _ in range(iters):
        assert mm.iteration(S["fphi"], S["frhs"], S["fres"], 0) == np.abs(m.iteration()).max(), what
    assert np.array_equal(_download(S["fphi"], S["grid"], shape), m.phi), what


def relax64(comm, rng, shape, nsweeps, *, alpha=1.0, beta=-1.0, bc=DIRI0, bvar=False, fused=2,
            big=0.0):
    """op.relax alone (nothing need be coarsenable) against the oracle's relax.
    big: a few aCoef cells whose lambda leaves the short reciprocal's range."""
    dx = 0.7
    a, b, rhs = _arrays(rng, shape, bvar)
    if big:
        a.flat[rng.choice(a.size, 37, replace=False)] = big
    u0 = rng.uniform(-1, 1, a.shape)
    S = _gpu(comm, shape, dx, a, b, rhs, alpha=alpha, beta=beta, bc=bc, fused=fused)
    S["fphi"].upload(0, u0)
    op = S["fac"].AMRnewOp()
    op.relax(S["fphi"], S["frhs"], nsweeps)
    o = _oracle(shape, dx, a, b, rhs, alpha=alpha, beta=beta, bc=bc, levels=1)
    o.set(0, oracle.PHI, 0, u0)
    o.relax(0, oracle.PHI, oracle.RHS, nsweeps)
    assert np.array_equal(S["fphi"].download(0), o.get(0, oracle.PHI, 0), equal_nan=True), \
        ("relax64", shape, nsweeps, alpha, beta, bc, bvar, fused, big)


# ------------------------------------------------------------------ families
GEN = dict(alpha=0.75, beta=-1.3)  # outside the kernels' exact specialisation (FAST off)
# 3 x 3 tiles of 64 x 22 with one interior tile and ragged last tiles: every
# tile class (EM 0, 3, 12, 15) in one launch; every side a multiple of 4, so
# a 2-depth cycle exists (ZIN: the first pair from zero; ACC: phi += e)
TB2_SHAPE = (136, 52, 12)


def tb2_fp64(comm, rng, part):
    # (with MGIC_TB2_TRIM=15 the FAST one-rule launches below are the TRIM ones)
    assert (os.environ.get("MGIC_TB2_TRIM") == "15") == (part == "trimmed")
    vcycle64(comm, rng, TB2_SHAPE)                       # FAST, UBC: ZIN, plain, ACC
    if part == "trimmed":
        return
    vcycle64(comm, rng, TB2_SHAPE, bc=MIXED)             # FAST, several ghost rules
    vcycle64(comm, rng, TB2_SHAPE, **GEN)                # general coefficients, UBC
    vcycle64(comm, rng, TB2_SHAPE, bc=MIXED, **GEN)
    relax64(comm, rng, TB2_SHAPE, 4, big=-1.0e160)       # FAST off by the lambda range
    relax64(comm, rng, TB2_SHAPE, 4, big=-1.0e308)


def tb2_fp32(comm, rng, part):
    vcycle32(comm, rng, TB2_SHAPE)
    vcycle32(comm, rng, TB2_SHAPE, bc=MIXED)
    vcycle32(comm, rng, TB2_SHAPE, **GEN)
    vcycle32(comm, rng, TB2_SHAPE, bc=MIXED, **GEN)
    # the issue's general-coefficient mixed cycle: a non-zero Dirichlet value
    nz_diri = dict(bc_lo=(0, 0, 0), bc_hi=(0, 0, 0), bc_value=-0.5)
    for prolong, avg in ((1, 1), (0, 0)):
        vcycle32(comm, rng, (72, 48, 40), bc=nz_diri, prolong=prolong, avg=avg, **GEN)


def sweep(comm, rng, part):
    # streaming single sweeps (fused_smoother=2), per tile shape: variable b
    # takes ZIN, plain + restriction, plain, ACC as single sweeps; constant b
    # takes them where a pair cannot (n = 1 from zero, n = 1 with phi += e, the
    # odd sweep of relax(3), the odd last pre-sweep + restriction)
    for shape in ((136, 24, 16), (132, 24, 16)):         # 128 x 16 and 132 x 17 tiles
        vcycle64(comm, rng, shape, bvar=True, n_pre=2, n_post=2, bc=MIXED)
        vcycle64(comm, rng, shape, n_pre=1, n_post=1, bc=MIXED)
        relax64(comm, rng, shape, 3, bc=MIXED)
    vcycle64(comm, rng, (136, 32, 16), n_pre=3, n_post=2, bc=MIXED)   # sweep + restrict, constant b
    vcycle64(comm, rng, (136, 32, 16), bvar=True, n_pre=3, n_post=2)  # ... variable b
    # fp32 128 x 32 tiles
    vcycle32(comm, rng, (264, 40, 16), bvar=True, n_pre=2, n_post=2, bc=MIXED)
    vcycle32(comm, rng, (264, 40, 16), n_pre=1, n_post=1, bc=MIXED)
    vcycle32(comm, rng, (264, 40, 16), n_pre=3, n_post=1, bc=MIXED)
    # the 3D-block kernel (fused_smoother=3), fp64 and fp32
    for bvar in (True, False):
        vcycle64(comm, rng, (40, 24, 16), bvar=bvar, fused=3, n_pre=2, n_post=2, bc=MIXED)
        vcycle32(comm, rng, (40, 24, 16), bvar=bvar, fused=3, n_pre=2, n_post=2, bc=MIXED)
    # the per-colour pass (fused_smoother=0), lambda recomputed in registers
    for bvar in (True, False):
        relax64(comm, rng, (37, 9, 40), 2, bvar=bvar, fused=0, bc=MIXED)
    chf_gsrb(rng)                                         # ... and lambda read (the drop-in)


def chf_gsrb(rng):
    """The ChomboFortran GSRB drop-in (a stored lambda) against the oracle's."""
    import ctypes

    def dbl(p):
        return p.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def ints(*v):
        return [ctypes.byref(ctypes.c_int(int(x))) for x in v]

    def fab_args(arr, lo):
        nz, ny, nx = arr.shape
        return [dbl(arr)] + ints(*lo) + ints(lo[0] + nx - 1, lo[1] + ny - 1, lo[2] + nz - 1) + \
            ints(1)

    # dpsi with 3 ghosts, rhs / coefficients with none, an odd global offset
    lo, n = (5, -3, 2), (20, 14, 9)
    g3 = tuple(x - 3 for x in lo)
    hi = tuple(lo[d] + n[d] - 1 for d in range(3))
    dx, alpha, beta = 100.0 / 64, 1.0, -1.0
    for rb in (0, 1):
        u = rng.uniform(-1, 1, (n[2] + 6, n[1] + 6, n[0] + 6))
        rhs = rng.uniform(-1, 1, n[::-1])
        a = rng.uniform(-2, -0.5, n[::-1])
        b = rng.uniform(0.5, 2, n[::-1])
        lam = rng.uniform(0.1, 0.3, n[::-1])
        got, want = u.copy(), u.copy()
        mg.lib.gsrbhelmholtzvc3d_(*fab_args(got, g3), *fab_args(rhs, lo), *ints(*lo), *ints(*hi),
                                  ctypes.byref(ctypes.c_double(dx)),
                                  ctypes.byref(ctypes.c_double(alpha)), *fab_args(a, lo),
                                  ctypes.byref(ctypes.c_double(beta)), *fab_args(b, lo),
                                  *fab_args(lam, lo), ctypes.byref(ctypes.c_int(rb)))
        oracle.gsrb(oracle.Fab(want, g3), oracle.Fab(rhs, lo), lo, hi, dx, alpha,
                    oracle.Fab(a, lo), beta, oracle.Fab(b, lo), oracle.Fab(lam, lo), rb)
        assert np.array_equal(got, want), ("chf gsrb", rb)


def stencil(comm, rng, part):
    from mg_ic_code_amd.decomposition import split_domain
    shape = (40, 24, 16)
    # residual (+ norm), restriction, prolongation of either type, both
    # coefficient averages, lambda: the fp64 and the mixed cycle, variable and
    # constant b (the block smoother: the restriction is a launch of its own)
    for bvar in (True, False):
        for prolong, avg in ((1, 1), (0, 0)):
            vcycle64(comm, rng, shape, bvar=bvar, fused=3, prolong=prolong, avg=avg, bc=MIXED)
            vcycle32(comm, rng, shape, bvar=bvar, fused=3, prolong=prolong, avg=avg, bc=MIXED)
    # box-to-box copies (fp64 and fp32 ghost exchanges, the coarse-level gathers)
    boxes = split_domain(_dom(shape), (2, 1, 2))
    vcycle64(comm, rng, shape, bvar=True, fused=3, boxes=boxes, bc=MIXED)
    vcycle32(comm, rng, shape, bvar=True, fused=3, boxes=boxes, bc=MIXED)
    # an odd number of fp32 launches leaves the result in the scratch buffer (a copy)
    vcycle32(comm, rng, shape, bvar=True, fused=3, n_pre=3, n_post=2, bc=MIXED)
    # a one-depth mixed cycle of one sweep: the sweep from zero, then phi += e
    # as a launch of its own
    vcycle32(comm, rng, shape, levels=1, n_bottom=1, fused=3, bc=MIXED)
    operator_methods(comm, rng)


def operator_methods(comm, rng):
    """applyOp / residual with the inhomogeneous BC (fill-bc faces), both b
    kinds, against the oracle; psi += dpsi over the grown box against numpy."""
    shape, dx = (20, 12, 16), 0.7
    bc = dict(bc_lo=(0, 1, 0), bc_hi=(1, 0, 2), bc_value=0.25)
    for bvar in (True, False):
        a, b, rhs = _arrays(rng, shape, bvar)
        S = _gpu(comm, shape, dx, a, b, rhs, alpha=1.0, beta=-1.0, bc=bc, fused=1)
        o = _oracle(shape, dx, a, b, rhs, alpha=1.0, beta=-1.0, bc=bc, levels=1)
        op = S["fac"].AMRnewOp()
        u = rng.uniform(-1, 1, a.shape)
        fu, out = mg.LevelData(S["grid"]), mg.LevelData(S["grid"])
        fu.upload(0, u)
        o.set(0, oracle.PHI, 0, u)
        for hom in (0, 1):
            op.residualI(out, fu, S["frhs"], homogeneous=hom)
            o.residual(0, oracle.RESID, oracle.PHI, oracle.RHS, hom)
            assert np.array_equal(out.download(0), o.get(0, oracle.RESID, 0)), ("residual", bvar, hom)
            op.applyOpI(out, fu, homogeneous=hom)
            o.apply_op(0, oracle.TMP, oracle.PHI, hom)
            assert np.array_equal(out.download(0), o.get(0, oracle.TMP, 0)), ("applyOp", bvar, hom)
        assert np.array_equal(op.m_lambda.download(0), o.get(0, oracle.LAMBDA, 0)), ("lambda", bvar)
        op.fillBC(fu, homogeneous=False)
        o.fill_bc(0, oracle.PHI, 0)
        g, c = fu.download(0, with_ghosts=True), o.get(0, oracle.PHI, 0, full=True)
        for sl in (np.s_[1:-1, 1:-1, 0], np.s_[1:-1, 1:-1, -1], np.s_[1:-1, 0, 1:-1],
                   np.s_[1:-1, -1, 1:-1], np.s_[0, 1:-1, 1:-1]):
            assert np.array_equal(g[sl], c[sl]), ("fillBC", bvar)
        # set_update_psi0: psi += dpsi over the valid cells and ghost layer 1
        psi = mg.LevelData(S["grid"])
        psi.upload(0, rng.uniform(-1, 1, a.shape))
        before = psi.download(0, with_ghosts=True)
        op.update_psi(psi, fu)
        assert np.array_equal(psi.download(0, with_ghosts=True),
                              before + fu.download(0, with_ghosts=True)), ("update_psi", bvar)


def bicgd(comm, rng, part):
    """The device BiCGStab loop (constant bCoef, one two-sweep launch per
    preCond) against the host loop, bit for bit in every norm, the iteration
    counts and phi, for each norm type of the stop test (tests/bicg_cases.py's
    rnd64_2l inputs and its norm-type variants)."""
    from tests import bicg_cases
    for name in ("rnd64_2l", "rnd64_nt0", "rnd64_nt1"):
        case = bicg_cases.BY_NAME[name]
        runs = []
        for dev in ("0", "1"):
            os.environ["MGIC_BICG_DEVICE"] = dev
            S = bicg_cases.make_gpu(mg, comm, case)
            amg = S["amg"]
            amg.init_residual(S["fphi"], S["frhs"], S["fres"], bicg_cases.NORM_TYPE)
            norms, iters = [], []
            for _ in range(2):
                norms.append(amg.iteration(S["fphi"], S["frhs"], S["fres"], bicg_cases.NORM_TYPE))
                on_dev, it, _ = amg.bottom_info()
                assert on_dev == (dev == "1"), (name, dev)
                iters.append(it)
            runs.append((norms, iters, bicg_cases.download(S["fphi"], S["grid"], case)))
        assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1], (name, runs[0][:2], runs[1][:2])
        assert np.array_equal(runs[0][2], runs[1][2]), name
        assert max(runs[0][1]) >= bicg_cases.MIN_ITERS, (name, runs[0][1])


# The three families below run cases the suite already states, as the plain
# functions they are, with this process's communicator: the references
# (tests/reduce_ref.py, phi_ref, puncture_ref, matter_ref, constraints_ref,
# regrid_ref, oracle.amr) and their bounds are those test files' own, imported
# and not restated.  One layout each: the smallest that reaches the entry.
def _levels(comm):
    from tests import test_level_algebra as la
    made = {}

    def get(case):
        if case not in made:
            made[case] = la.Level(comm, case)
        return made[case]

    return get


def blas(comm, rng, part):
    from tests import reduce_ref as rr
    from tests import test_level_algebra as la
    levels = _levels(comm)
    # the finals' loops wrap (6144 partials, three boxes); multi-box, ragged
    for case in (rr.SHAPES[3], rr.SHAPES[10], rr.SHAPES[11]):
        la.test_reductions_equal_the_stated_order(levels, rng, case)   # dot, 1-, 2-, max norm
        la.test_blas1_matches_numpy_and_keeps_ghosts(levels, rng, case)  # every k_blas kind
        la.test_fused_bicgstab_updates(levels, rng, case)              # axpy2 + norm, dot2, P update
    la.test_max_norm_keeps_the_maximum_past_a_nan(levels, rng)
    # max / min of bCoef and the lambda range behind resetLambda (the wide finals)
    la.test_bcoef_detector_sees_one_outlier(levels, la.GUARD_CASES[2], "last_row_tail")
    la.test_lambda_range_guard_sees_a_zero_denominator(levels, la.GUARD_CASES[2], "row0_tail")
    # preCond (res * lambda) and levelJacobi (residual * lambda) against the oracle
    from tests import test_gpu_parity as gp
    gp.test_operator_methods_bitwise(comm, rng, (1, 1, 1))


def _entry_point_cases(comm):
    """Every generator entry point (coefficients, integrand, regrid condition,
    output variables) x phi analytic / stored x punctures deck / table x matter
    absent / zero / general, each against its restatement or its twin."""
    from tests import test_matter as ma
    from tests import test_phi_field as pf
    from tests import test_punctures as pu
    layout = "ragged"
    for with_psi in (False, True):
        pf.test_stored_gaussian_path_is_bit_identical_to_analytic_path(comm, layout, with_psi)
        for stored in (False, True):
            pu.test_deck_as_table_is_bit_identical_to_todays_entry_points(comm, layout, with_psi,
                                                                          stored)
            ma.test_zero_matter_is_bit_identical_to_todays_entry_points(comm, layout, with_psi,
                                                                        stored)
    pf.test_analytic_generators_match_oracle_on_the_wide_gaussian(comm, layout, True)
    pf.test_any_stored_field_acoef_is_rho_grad_of_the_stored_values(comm, layout)
    pu.test_general_table_matches_restatement(comm, layout)
    ma.test_integrand_without_pow_is_bit_identical_to_numpy(comm, layout)
    ma.test_general_matter_matches_restatement(comm, layout)


def generators(comm, rng, part):
    import pathlib
    import tempfile

    from tests import test_constraints as co
    from tests import test_gpu_parity as gp
    from tests import test_phi_field as pf
    from tests import test_punctures as pu
    _entry_point_cases(comm)
    pf.test_fill_matches_analytic_phi0_and_numpy(comm, "ragged")           # Gaussian and sine
    for layout in ("ragged", "base+patch"):
        co.test_instantiations_are_pinned_to_each_other(comm, layout)
        co.test_momentum_source_without_holes_is_bit_identical_to_numpy(comm, layout)
        co.test_general_case_matches_restatement(comm, layout)
    co.test_ham_is_the_devices_own_integrand(comm, "ragged")
    co.test_bowen_york_divergence_converges_at_second_order_on_the_device(comm)  # a table alone
    gp.test_chf_dropin_setleveldata_bitwise(rng)                           # Laplacian, rho_grad
    with tempfile.TemporaryDirectory() as d:                               # the solver's variables
        pf.test_output_files_carry_the_stored_field(comm, pathlib.Path(d))
    with tempfile.TemporaryDirectory() as d:
        pu.test_solve_and_files_match_the_oracle_loop(comm, pathlib.Path(d))


def amr(comm, rng, part):
    from tests import test_amr as ta
    from tests import test_regrid as tr
    ta.test_amr_cf_interp_matches_oracle(comm)                 # inhomogeneous CF ghosts
    ta.test_amr_vcycle_matches_oracle_bitwise(comm, False)     # homogeneous, in the cycle
    tr.test_regrid_condition_single_box(comm)
    for with_psi in (False, True):
        tr.test_regrid_condition_patch_level(comm, with_psi)
    tr.test_tag_lattice_single_box(comm, 4, 2)
    tr.test_tag_lattice_three_boxes(comm, 2, 3)
    _entry_point_cases(comm)                                   # the regrid condition's instantiations


RUN = dict(tb2_fp64=tb2_fp64, tb2_fp32=tb2_fp32, sweep=sweep, stencil=stencil, bicgd=bicgd,
           blas=blas, generators=generators, amr=amr)


def main():
    global mg, np, oracle, MixedOracle
    family, part, out = sys.argv[1:4]
    import numpy as np
    import mg_ic_code_amd as mg
    import oracle
    from oracle.mixed import MixedOracle

    comm = mg.Comm()
    rng = np.random.default_rng(20261020)
    RUN[family](comm, rng, part)
    comm.synchronize()
    mg.lib.mgic_launch_ledger_dump(out.encode())
    counts = mg.launch_ledger()
    assert counts == mg.core.read_launch_ledger(out) and any(counts.values())
    mg.launch_ledger_reset()
    assert set(mg.launch_ledger().values()) == {0}, "reset leaves every count at zero"
    print("coverage worker OK", family, part, flush=True)


if __name__ == "__main__":
    main()
