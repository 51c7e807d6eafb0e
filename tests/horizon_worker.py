"""Worker for tests/test_horizon.py: one fresh interpreter.

    python tests/horizon_worker.py kernel LEDGER_PATH
        runs the kernel cases of libmgic_horizon.so (one case without LW and one
        with, against tests/horizon_ref.py) and dumps that library's launch
        ledger.  Any mismatch is an AssertionError: the exit code is non-zero.

    python tests/horizon_worker.py solve | solve2
        the Dirichlet 16^3 deck (solve2: with the 16^3 patch over coarse cells
        4..11 of tests/test_adm.py) without the switch, then with
        horizons="punctures", then with the deck's horizons = punctures; prints
        one JSON line: whether libmgic_horizon.so was loaded after each, whether
        psi, the norms, the iteration counts and libmgic's ledger are the same,
        whether NLResult.horizons is find_horizon(res.psi, ...) bit for bit,
        M_irr, M_chr and 3o's M_i, and M_irr from the numpy evaluator fed the
        restatement on the CPU oracle's psi, with dM_irr/du measured by shifting
        the device's psi.

    python tests/horizon_worker.py cli TMP_DIR
        tools/run_poisson.py --horizons-at-punctures --puncture-masses and
        --horizon (twice) against the same solves through the library.

    python tests/horizon_worker.py nonlocal RANK PORT OUT_DIR
        one rank of two (as tests/sample_worker.py nonlocal): each rank holds a
        box that is not local; the library's call and the package's are made
        and refused; writes OUT_DIR/rank<R>.json.
"""
import dataclasses
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def kernel(path):
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import _lib
    from tests import test_horizon as T
    comm = mg.Comm()
    T.run_kernel_cases(comm)
    mg.device_synchronize()
    _lib.horizon_call("mgic_horizon_launch_ledger_dump", path.encode())
    assert not any("horizon" in n for n in mg.launch_ledger())
    assert not _lib.sample_loaded() and not _lib.adm_loaded()
    return 0


def same_result(a, b):
    """Two HorizonResults equal bit for bit (NaN equal to NaN)."""
    import numpy as np
    for f in dataclasses.fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        if isinstance(x, np.ndarray) or f.name == "steps":
            if not np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True):
                return False
        elif isinstance(x, float) and x != x:
            if y == y:
                return False
        elif x != y:
            return False
    return True


def _grids(mg, comm, prm, two_levels):
    from tests import test_sample as TS
    dx = prm.domainLength[0] / 16
    boxes = [(0, 0, 0, 15, 15, 15)] + ([TS.PATCH[0]] if two_levels else [])
    grids = [mg.Grid(comm, boxes[0], [boxes[0]], dx)]
    if two_levels:
        grids.append(mg.Grid(comm, (0, 0, 0, 31, 31, 31), [boxes[1]], dx / 2, patches=True))
    return grids, boxes, dx


def solve(two_levels):
    import numpy as np
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import _lib
    from mg_ic_code_amd.horizon import SurfaceBasis, expansion_points, find_horizon
    from mg_ic_code_amd.nl import poisson_solve
    from mg_ic_code_amd.punctures import PunctureSet
    from mg_ic_code_amd.sample import puncture_masses
    from tests import horizon_ref as H
    from tests import nl_ref
    from tests import test_sample as TS
    comm = mg.Comm()
    prm = TS._deck(16)
    grids, boxes, dx = _grids(mg, comm, prm, two_levels)
    grid = grids if two_levels else grids[0]
    out = {}

    def fields(res):
        return res.psi if two_levels else [res.psi]

    def state(res):
        return ([f.download(0, with_ghosts=True) for f in fields(res)], res.dpsi_norms,
                res.linear_iterations, res.converged)

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and a[1:] == b[1:]

    mg.launch_ledger_reset()
    plain = poisson_solve(grid, prm, max_depth=2)
    ledger_plain = mg.launch_ledger()
    out["loaded_after_plain_solve"] = _lib.horizon_loaded()
    assert plain.horizons is None
    mg.launch_ledger_reset()
    flag = poisson_solve(grid, prm, max_depth=2, horizons="punctures")
    ledger_flag = mg.launch_ledger()
    out["loaded_after_flag_solve"] = _lib.horizon_loaded()
    assert not _lib.sample_loaded()
    a, b = state(plain), state(flag)
    out["same_solve"] = bool(same(a, b) and ledger_plain == ledger_flag)
    table = PunctureSet.from_params(prm)
    direct = [find_horizon(flag.psi, prm, p.position, p.mass) for p in table]
    out["same_report"] = bool(len(flag.horizons) == 2
                              and all(same_result(x, y) for x, y in zip(flag.horizons, direct)))
    key = poisson_solve(grid, dataclasses.replace(prm, horizons="punctures"), max_depth=2)
    out["deck_key_same"] = bool(all(same_result(x, y) for x, y in zip(key.horizons, flag.horizons))
                                and same(state(key), a))
    hz = flag.horizons
    out["found"] = [h.found for h in hz]
    out["enclosed"] = [h.enclosed for h in hz]
    out["iterations"] = [h.iterations for h in hz]
    out["degraded"] = [h.degraded_points for h in hz]
    out["M_irr"] = [h.irreducible_mass for h in hz]
    out["M_chr"] = [h.christodoulou_mass for h in hz]
    out["M_i"] = puncture_masses(flag.psi, prm).adm_masses
    out["lines"] = [ln for h in hz for ln in h.lines()]
    B = SurfaceBasis(8)
    levels = set()
    for h in hz:
        geo = B.geometry(h.coeffs, h.centre)
        levels |= set(int(v) for v in expansion_points(flag.psi, geo.points, geo.normal, geo.divn,
                                                       prm).level)
    out["levels"] = sorted(levels)
    # dM_irr/du: the device's psi shifted by a constant on every level
    shift = 1e-6
    shifted = []
    for f in fields(flag):
        g = mg.LevelData(f.grid)
        g.set_val_all(1e300)
        for n in range(f.grid.num_local):
            g.upload(n, f.download(n) + shift)
        shifted.append(g)
    moved = [find_horizon(shifted if two_levels else shifted[0], prm, p.position, p.mass)
             for p in table]
    out["sensitivity"] = [(m.irreducible_mass - h.irreducible_mass) / shift
                          for m, h in zip(moved, hz)]
    # the CPU oracle's psi through the restatement and the numpy finder
    n_nl = prm.max_NL_iterations
    if two_levels:
        psi_o = nl_ref.oracle_poisson_solve_amr(prm, boxes, 16, max_depth=2, n_nl=n_nl)[0]
    else:
        psi_o = [nl_ref.oracle_poisson_solve(prm, 16, max_depth=2, n_nl=n_nl)[0]]
    inner = [p[1:-1, 1:-1, 1:-1] for p in psi_o]
    ref = H.Hierarchy((16,) * 3, dx, [[(bx[:3], bx[3:], arr)] for bx, arr in zip(boxes, inner)])
    ev = H.restatement_evaluator(ref)
    oracle = [find_horizon(None, prm, p.position, p.mass, evaluator=ev, basis=B) for p in table]
    out["M_irr_oracle"] = [h.irreducible_mass for h in oracle]
    assert [h.status for h in oracle] == [h.status for h in hz]
    out["psi_scale"] = float(max(np.max(np.abs(c)) for c in inner))
    out["psi_rel_l2"] = [float(np.linalg.norm(f.download(0) - c) / np.linalg.norm(c))
                         for f, c in zip(fields(flag), inner)]
    print(json.dumps(out))
    return 0


def cli(tmp):
    import mg_ic_code_amd as mg
    from mg_ic_code_amd.horizon import horizon_lines
    from mg_ic_code_amd.nl import poisson_solve
    from mg_ic_code_amd.params import read_params_file
    from tests import test_sample as TS
    deck = os.path.join(tmp, "deck.txt")
    with open(deck, "w") as f:
        f.write(TS._deck_text().replace("max_NL_iterations = 6", "max_NL_iterations = 2"))
    tool = os.path.join(ROOT, "tools", "run_poisson.py")

    def run(*flags):
        r = subprocess.run([sys.executable, tool, deck, "--size", "16", "--max-depth", "2", *flags],
                           capture_output=True, text=True, timeout=300, cwd=tmp)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines = r.stdout.splitlines()
        return [ln for ln in lines if ln.startswith("horizon ")], json.loads(lines[-1])

    def summary(hz):
        return [h.summary() for h in hz]

    prm = read_params_file(deck)
    dom = (0, 0, 0, 15, 15, 15)
    grid = mg.Grid(mg.Comm(), dom, [dom], prm.domainLength[0] / 16)
    out = {}
    got, js = run("--horizons-at-punctures", "--puncture-masses")
    res = poisson_solve(grid, prm, max_depth=2, horizons="punctures", puncture_masses=True)
    want = horizon_lines(res.horizons, res.puncture_masses)
    out["punctures_lines_same"] = got == want
    out["punctures_json_same"] = js["horizons"] == summary(res.horizons)
    out["n_lines"] = len(got)
    out["mirr_next_to_mi"] = sum(1 for ln in got if " M_irr = " in ln and " M_1 = " in ln
                                 or " M_irr = " in ln and " M_2 = " in ln)
    # explicit surfaces: one that is found and one that collapses (nothing at the origin)
    got, js = run("--horizon", "10 0 0 0.6", "--horizon=0 0 0 1.0")
    res = poisson_solve(grid, prm, max_depth=2, horizons=[(10, 0, 0, 0.6), "0 0 0 1.0"])
    out["explicit_lines_same"] = got == horizon_lines(res.horizons)
    out["explicit_json_same"] = js["horizons"] == summary(res.horizons) and \
        [h.found for h in res.horizons] == [True, False] and \
        js["horizons"][1]["area"] is None and js["horizons"][0]["area"] > 0.0
    print(json.dumps(out))
    return 0


def nonlocal_box(rank, port, out_dir):
    import ctypes
    import datetime
    import numpy as np
    import torch  # noqa: F401  (before the library: one HIP runtime)
    import torch.distributed as dist
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import _lib
    from mg_ic_code_amd.core import read_launch_ledger
    from mg_ic_code_amd.horizon import HorizonArgumentError, expansion_points
    _lib.check_single_hip_runtime()
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank,
                            world_size=2, timeout=datetime.timedelta(seconds=120))
    mg.set_device(0)
    comm = mg.Comm(rank, 2, transport="ipc")
    dom = (0, 0, 0, 15, 15, 15)
    grid = mg.Grid(comm, dom, [(0, 0, 0, 7, 15, 15), (8, 0, 0, 15, 15, 15)], 1.0, owners=[0, 1])
    assert grid.num_local == 1
    psi = mg.LevelData(grid)
    psi.set_val_all(1.0)
    pts = np.array([[0.5, 0.25, -0.75], [-3.0, 2.0, 1.0]])
    nrm, dv = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]), np.ones(2)
    table = np.array([1.0, 0.2, 0.1, -0.15, 0, 0, 0, 0, 0, 0], dtype=np.float64)
    res, level, order = np.zeros((2, 6)), np.zeros(2, np.int32), np.zeros(2, np.int32)
    PD, PI = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    out = {"rank": rank, "code": None, "message": "", "value_error": False}
    try:
        _lib.horizon_call("mgic_horizon_expansion", comm.handle, 1,
                          (ctypes.c_void_p * 1)(psi.handle.value), None, 1, table.ctypes.data_as(PD),
                          2, pts.ctypes.data_as(PD), nrm.ctypes.data_as(PD), dv.ctypes.data_as(PD),
                          res.ctypes.data_as(PD), level.ctypes.data_as(PI), order.ctypes.data_as(PI))
    except mg.MgicError as e:
        out["code"], out["message"] = e.code, str(e)
    try:
        expansion_points(psi, pts, nrm, dv, None, punctures=[list(table)])
    except HorizonArgumentError as e:
        out["value_error"] = isinstance(e, ValueError) and e.code == -1
    path = os.path.join(out_dir, f"rank{rank}.ledger")
    _lib.horizon_call("mgic_horizon_launch_ledger_dump", path.encode())
    out["ledger"] = read_launch_ledger(path)
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump(out, f)
    comm.synchronize()
    dist.barrier()
    del psi, grid
    dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "kernel":
        sys.exit(kernel(sys.argv[2]))
    if mode == "cli":
        sys.exit(cli(sys.argv[2]))
    if mode == "nonlocal":
        sys.exit(nonlocal_box(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]))
    sys.exit(solve(mode == "solve2"))
