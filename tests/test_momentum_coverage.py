"""Every kernel of libmgic_ctt.so is launched by a case that compares it with
its reference, as tests/test_launch_coverage.py holds libmgic.so's to.

The library counts launches per kernel on the host (csrc/launch_ledger.hpp,
its own registry).  One fresh process (tests/momentum_worker.py) runs the
kernel cases of tests/test_momentum.py against tests/momentum_ref.py and dumps
the ledger; the test fails on a mismatch (the worker's exit code) and on any
entry that was never launched, with the missing names in the message.
"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "momentum_worker.py")
# the worker takes a few seconds (interpreter start and imports included); ten
# times that ends one that hangs
WORKER_TIMEOUT = 60


@pytest.mark.gpu
def test_every_kernel_of_the_ctt_library_is_launched_against_its_reference(tmp_path):
    from mg_ic_code_amd.core import read_launch_ledger
    out = tmp_path / "ctt.ledger"
    env = dict(os.environ)
    env.pop("MGIC_LAUNCH_LEDGER", None)
    r = subprocess.run([sys.executable, WORKER, str(out)], capture_output=True, text=True, env=env,
                       timeout=WORKER_TIMEOUT)
    assert r.returncode == 0, f"{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    ledger = read_launch_ledger(out)
    assert sorted(ledger) == ["k_ctt_div_rhs", "k_ctt_extrap", "k_ctt_lw", "k_ctt_w"], ledger
    missing = sorted(n for n, c in ledger.items() if c == 0)
    assert not missing, f"{len(missing)} of {len(ledger)} kernels never launched:\n" + "\n".join(missing)
