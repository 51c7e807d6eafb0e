"""The residual formed inside the next V-cycle's first launch (k_gsrb_tb2's RES
body, AMRMultiGrid::iterations / precondition): pipelined iterations() give
phi, resid and every norm of iteration() calls and of the oracle bit for bit,
the residual launches really are gone (launch ledger), and MGIC_FUSED_RES=0
in a fresh process gives the same bits with the residual launches back.

Every case runs tests/fused_res_worker.py twice, in fresh interpreters (the
switches are read once per process): with MGIC_FUSED_RES unset and with 0.
The worker makes the comparisons and the ledger check; the test compares the
two runs' result digests.
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

mg = pytest.importorskip("mg_ic_code_amd")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_worker(case, **env):
    e = dict(os.environ, PYTHONUNBUFFERED="1")
    for k in ("MGIC_FUSED_RES", "MGIC_TB2_TRIM", "MGIC_TB2_KC"):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fused_res_worker.py"), case],
                       cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "fused res worker OK" in r.stdout, out[-3000:]
    digest = [ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith("digest ")]
    assert len(digest) == 1, out[-3000:]
    return digest[0]


@pytest.mark.parametrize("case,env", [
    ("ragged", {}),                        # 136 x 52 x 12: every tile class, 4-plane chunks
    ("ragged", {"MGIC_TB2_TRIM": "15"}),   # the edge tiles skip the domain faces' ghost lines
    ("ragged", {"MGIC_TB2_TRIM": "0"}),    # ... and load them
    ("general", {}),                       # alpha, beta = 0.75, -1.3
    ("cube", {}),                          # 64^3, 3 depths
    ("steady", {"MGIC_TB2_KC": "32"}),     # 64^3 in 32-plane chunks: steady-state steps
    ("mixed", {}),                         # 72 x 20 x 28, Dirichlet 0.375 / Neumann: not fused
    ("precond", {}),                       # precondition(e, r, 2)
])
def test_fused_residual_bitwise(case, env):
    on = run_worker(case, **env)
    off = run_worker(case, MGIC_FUSED_RES="0", **env)
    assert on == off
