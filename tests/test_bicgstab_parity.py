"""GPU parity of the BiCGStab solvers against the CPU oracle, where they iterate.

The bottom solver of the V-cycle (BiCGStabSolver::solve / solveDevice), the
direct level solve (mg.bicgstab) and the outer solve over MultilevelLinearOp
with the reference's own BiCGStab bottom, each against the one-box oracle on
the cases of tests/bicg_cases.py.  Every case passes the CPU gate of
tests/test_oracle.py (test_bicgstab_cases_hold_still_over_decompositions):
on the oracle alone, changing only the order of the reductions keeps the
iteration counts and moves phi and the L2 residual norms by <= 1e-12.  So
the bars here are the project's own and are not widened by conditioning:

  * phi: rel-L2 <= 1e-10 (BASELINE.json);
  * every residual norm within 1e-10 x the initial residual norm;
  * BiCGStab iterations per solve equal to the oracle's.

Which loop ran (device / host) is asserted for every run, never assumed.
"""
import functools

import numpy as np
import pytest

import oracle
from tests import bicg_cases as bc

pytestmark = pytest.mark.gpu

mg = pytest.importorskip("mg_ic_code_amd")

ENV_KEYS = ("MGIC_BICG_DEVICE", "MGIC_BICG_BATCH", "MGIC_BICG_PIPE")
# the device loop as shipped, the device loop publishing after every
# iteration, the host loop
PATHS = {"device": {}, "batch1": {"MGIC_BICG_BATCH": "1"}, "host": {"MGIC_BICG_DEVICE": "0"}}


@pytest.fixture(scope="module")
def comm():
    return mg.Comm()


def set_env(monkeypatch, env):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def run_vcycles(comm, case, parts=(1, 1, 1), agglomerate_below=0):
    S = bc.make_gpu(mg, comm, case, parts, agglomerate_below)
    amg = S["amg"]
    r0 = amg.init_residual(S["fphi"], S["frhs"], S["fres"], norm_type=bc.NORM_TYPE)
    norms, iters, dev = [], [], []
    for _ in range(bc.VCYCLES):
        norms.append(amg.iteration(S["fphi"], S["frhs"], S["fres"], norm_type=bc.NORM_TYPE))
        d, it, _ = amg.bottom_info()
        dev.append(d)
        iters.append(it)
    return dict(r0=r0, norms=norms, iters=iters, dev=dev,
                phi=bc.download(S["fphi"], S["grid"], case))


def check_vcycles(case, run, label):
    ref = bc.reference(case.name)
    err = bc.rel_l2(run["phi"], ref["phi"])
    nerr = max(abs(x - y) for x, y in zip([run["r0"]] + run["norms"],
                                          [ref["r0"]] + ref["norms"])) / ref["r0"]
    print(f"{case.name} [{label}]: its {run['iters']} (oracle {ref['iters']}) dev {run['dev']} "
          f"phi rel-L2 {err:.2e} norm err / r0 {nerr:.2e}")
    assert run["iters"] == ref["iters"]
    assert err <= bc.GPU_PHI_TOL
    assert nerr <= bc.GPU_NORM_TOL


# --------------------------------------- (a) V-cycles with the BiCGStab bottom
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", [c.name for c in bc.VCYCLE_CASES if c.group == "a"])
def test_vcycle_bicgstab_bottom_matches_oracle(comm, monkeypatch, name, path):
    """Three AMRMultiGrid iterations with an iterating BiCGStab bottom (16^3,
    32^3, 36 x 10 x 14 with Dirichlet / Neumann faces; SetBinaryBH inputs at
    alpha = 1, random ones at alpha = 0) against the oracle, on the device
    loop, the device loop with one iteration per batch and the host loop.
    rnd64_smooth_b has a variable bCoef, so preCond is not one two-sweep
    launch and every path is the host loop."""
    case = bc.BY_NAME[name]
    set_env(monkeypatch, PATHS[path])
    run = run_vcycles(comm, case)
    want_dev = case.device and path != "host"
    assert run["dev"] == [want_dev] * bc.VCYCLES, run["dev"]
    check_vcycles(case, run, path)


# ---------------------- (b) restarts, the restart limit, imax, norm types 0 / 1
@pytest.mark.parametrize("name", [c.name for c in bc.VCYCLE_CASES if c.group == "b"])
def test_vcycle_bicgstab_stops_and_restarts_match_oracle_and_each_other(comm, monkeypatch, name):
    """The stops the plain cases never take: |m| <= small |rho| restarts
    (phi += E, fresh residual, re-upload with init = 1, split between device
    and host), the restart limit, the imax stop and norm types 0 and 1 of the
    device loop.  Each of the device loop at batch sizes 1, 3, 16 and as
    shipped and the host loop is compared with the oracle; and the runs are
    bit-identical to each other in phi, every norm and every count, whichever
    batch the stop fell into.  (In these cases a restart is followed at once
    by the next, up to the limit; the restart that recovers is
    direct24x12x16_restart below.)"""
    case = bc.BY_NAME[name]
    ref = bc.reference(name)
    # the oracle side takes the path the case is about (also gated on the CPU)
    if case.expect == "restarts":
        assert max(ref["restarts"]) >= 1
    elif case.expect == "limit":
        assert any(ref["limit"])
    runs = []
    for label, env in (("batch1", {"MGIC_BICG_BATCH": "1"}), ("batch3", {"MGIC_BICG_BATCH": "3"}),
                       ("batch16", {"MGIC_BICG_BATCH": "16"}), ("device", {}),
                       ("host", {"MGIC_BICG_DEVICE": "0"})):
        set_env(monkeypatch, env)
        run = run_vcycles(comm, case)
        assert run["dev"] == [label != "host"] * bc.VCYCLES, (label, run["dev"])
        check_vcycles(case, run, label)
        runs.append((label, run))
    for label, r in runs[1:]:
        first = runs[0][1]
        assert r["iters"] == first["iters"], label
        assert r["r0"] == first["r0"] and r["norms"] == first["norms"], label
        assert np.array_equal(r["phi"], first["phi"]), label


# ------------------------------------------------------ (c) the gathered bottom
def test_vcycle_bicgstab_gathered_bottom_matches_oracle(comm, monkeypatch):
    """64^3 on 2 x 2 x 2 boxes with agglomerate_below = 32: the eight 16^3
    coarse boxes gather to one 32^3 box, whose BiCGStab runs on the device
    loop; against the one-box oracle."""
    case = bc.BY_NAME["rnd64_2l"]
    set_env(monkeypatch, {})
    run = run_vcycles(comm, case, parts=(2, 2, 2), agglomerate_below=32)
    assert run["dev"] == [True] * bc.VCYCLES, run["dev"]
    check_vcycles(case, run, "gathered")


# ------------------------------- (d) the outer solve with the reference's bottom
@pytest.mark.parametrize("name,parts", [("outer_bh64_2l", (1, 1, 1)), ("outer_rnd64_2l", (1, 1, 1)),
                                        ("outer_rnd128_3l", (1, 1, 1)),
                                        ("outer_rnd128_3l", (2, 2, 2))])
def test_outer_solve_with_bicgstab_bottom_matches_oracle(comm, monkeypatch, name, parts):
    """solver.solve(dpsi, rhs) of Main_PoissonSolver.cpp:174-184 as the
    reference configures it: BiCGStab over MultilevelLinearOp (two
    AMRMultiGrid iterations) with the BiCGStab bottom.  The final norm is
    rounding noise (1e-13), so it is bounded, not compared."""
    case = bc.BY_NAME[name]
    ref = bc.reference(name)
    set_env(monkeypatch, {})
    S = bc.make_gpu(mg, comm, case, parts)
    solver = mg.BiCGStabSolver(mg.MultilevelLinearOp(S["amg"], bc.OUTER["mg_iters"]),
                               tolerance=bc.OUTER["eps"], max_iterations=bc.OUTER["imax"],
                               norm_type=bc.OUTER["norm_type"])
    it = solver.solve(S["fphi"], S["frhs"])
    dev, bit, _ = S["amg"].bottom_info()
    # one box: the device loop; 2 x 2 x 2: eight coarse boxes, the host loop
    assert dev == (parts == (1, 1, 1))
    err = bc.rel_l2(bc.download(S["fphi"], S["grid"], case), ref["phi"])
    print(f"{name} {parts}: its {it} (oracle {ref['iters']}) last bottom its {bit} dev {dev} "
          f"phi rel-L2 {err:.2e} final norm {solver.final_norm:.2e}")
    assert [it] == ref["iters"]
    assert err <= bc.GPU_PHI_TOL
    assert solver.final_norm <= 1e-9 * np.max(np.abs(S["rhs"]))


@functools.lru_cache(maxsize=None)
def _oracle_precond(name):
    case = bc.BY_NAME[name]
    o, _ = bc.make_oracle(case)
    o.amr_precond(oracle.TMP, oracle.RHS, bc.OUTER["mg_iters"])
    return o.get(0, oracle.TMP, 0), o.last_bicg_iters()


@pytest.mark.parametrize("name", [c.name for c in bc.OUTER_CASES])
def test_mg_preconditioner_with_bicgstab_bottom_matches_oracle(comm, monkeypatch, name):
    """MultilevelLinearOp::preCond (e = 0 + two AMRMultiGrid iterations,
    homogeneous BC) with the BiCGStab bottom against the oracle's."""
    case = bc.BY_NAME[name]
    e_o, bit_o = _oracle_precond(name)
    set_env(monkeypatch, {})
    S = bc.make_gpu(mg, comm, case)
    e = mg.LevelData(S["grid"])
    mg.MultilevelLinearOp(S["amg"], bc.OUTER["mg_iters"]).preCond(e, S["frhs"])
    dev, bit, _ = S["amg"].bottom_info()
    err = bc.rel_l2(bc.download(e, S["grid"], case), e_o)
    print(f"{name}: last bottom its {bit} (oracle {bit_o}) dev {dev} e rel-L2 {err:.2e}")
    assert dev
    assert bit == bit_o and bit >= bc.MIN_ITERS
    assert err <= bc.GPU_PHI_TOL


# ------------------------------------------------- (e) the direct level solve
@pytest.mark.parametrize("path", ["device", "host"])
@pytest.mark.parametrize("name", [c.name for c in bc.DIRECT_CASES])
def test_direct_level_bicgstab_matches_oracle(comm, monkeypatch, name, path):
    """mg.bicgstab(op, phi, rhs, homogeneous, params) (mgic_op_bicgstab) on a
    one-level operator from a random phi, with homogeneous and inhomogeneous
    BCs, against o.bicgstab.  40 x 9 x 14 has ny * nz = 126 rows, so the
    last 4-row block of every reduction is partial; the non-cubic shapes
    carry Dirichlet / Neumann faces with a BC value.  direct24x12x16_restart
    restarts twice and then converges, so what the device loop does after a
    restart (fresh residual, init = 1 re-upload) reaches phi."""
    case = bc.BY_NAME[name]
    ref = bc.reference(name)
    set_env(monkeypatch, PATHS[path])
    S = bc.make_gpu(mg, comm, case)
    op = S["fac"].AMRnewOp()
    it = mg.bicgstab(op, S["fphi"], S["frhs"], homogeneous=bool(case.hom), params=S["params"])
    dev = mg.bicgstab_on_device()
    err = bc.rel_l2(bc.download(S["fphi"], S["grid"], case), ref["phi"])
    print(f"{name} [{path}]: its {it} (oracle {ref['iters']}) dev {dev} phi rel-L2 {err:.2e}")
    assert dev == (path == "device")
    assert [it] == ref["iters"] and it >= bc.MIN_ITERS
    assert err <= bc.GPU_PHI_TOL
