"""Worker for tests/test_cttk.py: one fresh interpreter that runs its kernel
cases (the three kernels of libmgic_cttk.so against tests/cttk_ref.py, bit for
bit) and dumps that library's launch ledger.  Any mismatch is an
AssertionError: the exit code is non-zero.

    python tests/cttk_worker.py LEDGER_PATH
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(path):
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import _lib
    from tests import test_cttk as T
    comm = mg.Comm()
    T.run_kernel_cases(comm)
    mg.device_synchronize()
    _lib.cttk_call("mgic_cttk_launch_ledger_dump", path.encode())
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
