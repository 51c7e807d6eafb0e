"""Worker for tests/test_sample.py: one fresh interpreter.

    python tests/sample_worker.py kernel LEDGER_PATH
        runs the kernel cases of libmgic_sample.so (every instantiation of
        k_sample_points against tests/sample_ref.py) and dumps that library's
        launch ledger.  Any mismatch is an AssertionError: the exit code is
        non-zero.

    python tests/sample_worker.py solve | solve2
        the Dirichlet 16^3 deck (solve2: with the 16^3 patch over coarse cells
        4..11 of tests/test_adm.py) without the flag, then with
        puncture_masses=True, then with the deck's puncture_masses = 1; prints
        one JSON line: whether libmgic_sample.so was loaded after each, whether
        psi, the norms, the iteration counts and libmgic's ledger are the same,
        whether NLResult.puncture_masses is puncture_masses(res.psi, ...) bit
        for bit, and psi at the punctures next to the restatement applied to
        the CPU oracle's psi.

    python tests/sample_worker.py nonlocal RANK PORT OUT_DIR
        one rank of two (peer-mapped transport, both on device 0; gloo on
        127.0.0.1 is the control plane): a 16^3 level of two boxes, one per
        rank, so each rank holds a box that is not local.  The library's call
        and the package's are made and refused; writes OUT_DIR/rank<R>.json:
        the status code, whether the package raised its ValueError, and the
        library's launch ledger afterwards.
"""
import dataclasses
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def kernel(path):
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import _lib
    from tests import test_sample as T
    comm = mg.Comm()
    T.run_kernel_cases(comm)
    mg.device_synchronize()
    _lib.sample_call("mgic_sample_launch_ledger_dump", path.encode())
    assert not any("sample" in n for n in mg.launch_ledger())
    return 0


def solve(two_levels):
    import numpy as np
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import _lib
    from mg_ic_code_amd.nl import poisson_solve
    from mg_ic_code_amd.punctures import PunctureSet
    from mg_ic_code_amd.sample import puncture_masses
    from tests import nl_ref
    from tests import sample_ref as R
    from tests import test_sample as T
    comm = mg.Comm()
    prm = T._deck(16)
    dx = prm.domainLength[0] / 16
    boxes = [(0, 0, 0, 15, 15, 15)] + ([T.PATCH[0]] if two_levels else [])
    grids = [mg.Grid(comm, boxes[0], [boxes[0]], dx)]
    if two_levels:
        grids.append(mg.Grid(comm, (0, 0, 0, 31, 31, 31), [boxes[1]], dx / 2, patches=True))
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
    out["loaded_after_plain_solve"] = _lib.sample_loaded()
    assert plain.puncture_masses is None
    mg.launch_ledger_reset()
    flag = poisson_solve(grid, prm, max_depth=2, puncture_masses=True)
    ledger_flag = mg.launch_ledger()
    out["loaded_after_flag_solve"] = _lib.sample_loaded()
    a, b = state(plain), state(flag)
    out["same_solve"] = bool(same(a, b) and ledger_plain == ledger_flag)
    out["same_report"] = flag.puncture_masses == puncture_masses(flag.psi, prm)
    key = poisson_solve(grid, dataclasses.replace(prm, puncture_masses=1), max_depth=2)
    out["deck_key_same"] = bool(key.puncture_masses == flag.puncture_masses
                                and same(state(key), a))
    rows = flag.puncture_masses.punctures
    out["u"] = [p.u for p in rows]
    out["levels"] = [p.level for p in rows]
    out["orders"] = [p.order for p in rows]
    out["masses"] = flag.puncture_masses.adm_masses
    out["lines"] = flag.puncture_masses.lines()
    # the CPU oracle's psi through the restatement
    n_nl = prm.max_NL_iterations
    if two_levels:
        psi_o = nl_ref.oracle_poisson_solve_amr(prm, boxes, 16, max_depth=2, n_nl=n_nl)[0]
    else:
        psi_o = [nl_ref.oracle_poisson_solve(prm, 16, max_depth=2, n_nl=n_nl)[0]]
    inner = [p[1:-1, 1:-1, 1:-1] for p in psi_o]
    h = R.Hierarchy((16,) * 3, dx, [[(bx[:3], bx[3:], arr)] for bx, arr in zip(boxes, inner)])
    u, lev, used = R.sample(h, [p.position for p in PunctureSet.from_params(prm)], 4)
    out["u_oracle"] = [float(v) for v in u]
    assert list(lev) == out["levels"] and list(used) == out["orders"]
    out["psi_rel_l2"] = [float(np.linalg.norm(f.download(0) - c) / np.linalg.norm(c))
                         for f, c in zip(fields(flag), inner)]
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
    from mg_ic_code_amd.sample import SampleArgumentError, sample_points
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
    values, level, order = np.zeros(2), np.zeros(2, np.int32), np.zeros(2, np.int32)
    PD, PI = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    out = {"rank": rank, "code": None, "message": "", "value_error": False}
    try:
        _lib.sample_call("mgic_sample_points", comm.handle, 1, (ctypes.c_void_p * 1)(psi.handle.value),
                         2, pts.ctypes.data_as(PD), 4, values.ctypes.data_as(PD),
                         level.ctypes.data_as(PI), order.ctypes.data_as(PI))
    except mg.MgicError as e:
        out["code"], out["message"] = e.code, str(e)
    try:
        sample_points(psi, pts, 4)
    except SampleArgumentError as e:
        out["value_error"] = isinstance(e, ValueError) and e.code == -1
    path = os.path.join(out_dir, f"rank{rank}.ledger")
    _lib.sample_call("mgic_sample_launch_ledger_dump", path.encode())
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
    if mode == "nonlocal":
        sys.exit(nonlocal_box(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]))
    sys.exit(solve(mode == "solve2"))
