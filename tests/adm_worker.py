"""Worker for tests/test_adm.py: one fresh interpreter.

    python tests/adm_worker.py kernel LEDGER_PATH
        runs the kernel cases of libmgic_adm.so (both instantiations of
        k_adm_surface and k_adm_finish against tests/adm_ref.py) and dumps that
        library's launch ledger.  Any mismatch is an AssertionError: the exit
        code is non-zero.

    python tests/adm_worker.py solve
        a Dirichlet 16^3 deck solve without the flag, then with adm=[5, 7], then
        with the deck's adm_half_widths; prints one JSON line: whether
        libmgic_adm.so was loaded after each, whether psi, the norms and the
        iteration counts are the same, and whether NLResult.adm is
        adm_charges(res.psi, ...) bit for bit.
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
    from tests import test_adm as T
    comm = mg.Comm()
    T.run_kernel_cases(comm)
    mg.device_synchronize()
    _lib.adm_call("mgic_adm_launch_ledger_dump", path.encode())
    assert not any("adm" in n for n in mg.launch_ledger())
    return 0


def solve():
    import numpy as np
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import _lib
    from mg_ic_code_amd.adm import adm_charges
    from mg_ic_code_amd.nl import poisson_solve
    from tests import test_adm as T
    comm = mg.Comm()
    prm = T._deck(16)
    dom = (0, 0, 0, 15, 15, 15)
    grid = mg.Grid(comm, dom, [dom], prm.domainLength[0] / 16)
    out = {}

    def state(res):
        return (res.psi.download(0, with_ghosts=True), res.dpsi_norms, res.linear_iterations,
                res.converged)

    mg.launch_ledger_reset()
    plain = poisson_solve(grid, prm, max_depth=2)
    ledger_plain = mg.launch_ledger()
    out["loaded_after_plain_solve"] = _lib.adm_loaded()
    assert plain.adm is None
    mg.launch_ledger_reset()
    flag = poisson_solve(grid, prm, max_depth=2, adm=[5, 7])
    ledger_flag = mg.launch_ledger()
    out["loaded_after_adm_solve"] = _lib.adm_loaded()
    a, b = state(plain), state(flag)
    out["same_solve"] = bool(np.array_equal(a[0], b[0]) and a[1:] == b[1:]
                             and ledger_plain == ledger_flag)
    out["same_report"] = flag.adm == adm_charges(flag.psi, prm, [5, 7])
    key = poisson_solve(grid, dataclasses.replace(prm, adm_half_widths=[5, 7]), max_depth=2)
    out["deck_key_same"] = key.adm == flag.adm and bool(np.array_equal(state(key)[0], a[0]))
    out["converged"] = bool(flag.converged)
    out["masses"] = [s.mass for s in flag.adm.surfaces]
    out["lines"] = flag.adm.lines()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(kernel(sys.argv[2]) if sys.argv[1] == "kernel" else solve())
