"""Worker for tests/test_khyb.py: one fresh interpreter per check.  Any
mismatch is an AssertionError: the exit code is non-zero.

    python tests/khyb_worker.py kernels LEDGER_PATH   the kernel cases against
                                                      tests/khyb_ref.py, then the
                                                      library's ledger dumped
    python tests/khyb_worker.py refusals              poisson_solve(hybrid_K=True)'s
                                                      refusals; needs no device
    python tests/khyb_worker.py off                   hybrid_K off is the solve it was
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv):
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import _lib
    from tests import test_khyb as T
    what = argv[1]
    if what == "kernels":
        assert not _lib.khyb_loaded()
        T.run_kernel_cases(mg.Comm())
        mg.device_synchronize()
        _lib.khyb_call("mgic_khyb_launch_ledger_dump", argv[2].encode())
    elif what == "refusals":
        T.run_refusals()
    elif what == "off":
        T.run_off_means_off()
    else:
        raise SystemExit(f"unknown check {what!r}")
    print("ok", what)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
