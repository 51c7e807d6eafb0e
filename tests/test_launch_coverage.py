"""Every compiled kernel instantiation is launched by a test that compares it
with its reference.

The library counts launches per instantiation on the host (csrc/
launch_ledger.hpp): the entries come from the build, so an instantiation no
case reaches shows up with a count of zero.  One fresh process per kernel
family (tests/coverage_worker.py) runs the family's cases against their
references and dumps its ledger; a family's test fails on a mismatch (the
worker's exit code) and on any entry of the family that was never launched,
with the missing names in the message -- deleting a case, or adding a
template argument to a kernel without adding a case, is such a failure.

CPU tests: the ledger registers its entries without a device and every name
falls into exactly one family; no kernel is launched around the ledger.
"""
import glob
import os
import re
import subprocess
import sys

import pytest

from tests import coverage_worker as cw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mg_ic_code_amd", "csrc")
WORKER = os.path.join(ROOT, "tests", "coverage_worker.py")
# a worker takes 2 to 5.5 s on an MI355X (interpreter start and imports
# included); ten times that ends one that hangs
WORKER_TIMEOUT = 60


def read_ledger(path):
    from mg_ic_code_amd.core import read_launch_ledger
    return read_launch_ledger(path)


def test_every_family_has_a_test():
    # a family is held by the per-process test (PARTS, with a worker) or by the
    # several-rank test below: no pattern of FAMILIES is left unasserted
    assert set(cw.PARTS) | set(cw.MULTI_RANK) == set(cw.FAMILIES)
    assert not set(cw.PARTS) & set(cw.MULTI_RANK)
    assert set(cw.PARTS) == set(cw.RUN)
    assert cw.MULTI_RANK == ("transport",)
    assert callable(globals()["test_transport_family_launches_every_instantiation"])


# ------------------------------------------------------------------ CPU
def test_ledger_loads_without_a_device(tmp_path):
    # a child that only loads the library and dumps the ledger
    out = tmp_path / "ledger.txt"
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import mg_ic_code_amd as mg\n"
            "assert mg.lib.mgic_launch_ledger_dump(%r) == 0\n"
            "d = mg.launch_ledger()\n"
            "assert d and set(d.values()) == {0}, 'a launch without a device?'\n"
            % (ROOT, str(out).encode()))
    env = dict(os.environ, MGIC_NO_TORCH_PRELOAD="1", MGIC_LAUNCH_LEDGER=str(tmp_path / "unload"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(out) as f:
        names = [line.rpartition("\t")[0] for line in f]
    assert names and len(names) == len(set(names))
    assert names == sorted(names)
    for n in names:
        assert len(cw.family_of(n)) == 1, (n, cw.family_of(n))
    # names are the compiler's spelling of the instantiation, tile classes included
    for spot in ("k_gsrb_tb2<float, 64, 22, 1024, false, true, false, true, false>",
                 "k_gsrb_tb2<float, 64, 22, 1024, false, true, false, true, false>#em0",
                 "k_gsrb_tb2<double, 64, 22, 1024, true, false, true, true, true>#em12",
                 "k_gsrb_tb2<double, 64, 22, 1024, false, false, false, false, false>#em15",
                 "k_gsrb_fused6<double, 132, 17, 512, false, true, true>",
                 "k_gsrb_block<float, 32, 8, 4, 256, true, false, false>",
                 "k_prolong<float, 0>", "k_residual_zl<true, float, false>", "k_blas<6>",
                 "k_exchange<float>", "k_lambda"):
        assert spot in names, spot
    # without the one-rule edge bodies there are no x-face / y-face classes
    assert "k_gsrb_tb2<double, 64, 22, 1024, false, false, false, false, false>#em3" not in names
    # MGIC_LAUNCH_LEDGER: the same ledger, written as the library unloads
    unload = glob.glob(str(tmp_path / "unload.*"))
    assert len(unload) == 1 and unload[0].rsplit(".", 1)[1].isdigit()
    assert sorted(read_ledger(unload[0])) == names


def test_every_launch_goes_through_the_ledger():
    # the triple chevron appears in the wrapper's own definition and nowhere else
    hits = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if not path.endswith((".hip", ".hpp", ".cpp", ".h")):
            continue
        with open(path) as f:
            for i, line in enumerate(f, 1):
                if "<<<" in line:
                    hits.append((os.path.basename(path), i, line.strip()))
    assert hits, "the wrapper itself launches"
    for name, i, line in hits:
        assert name == "launch_ledger.hpp" and line.startswith("K<<<grid, block, shmem, st>>>("), \
            f"{name}:{i}: a kernel launch outside ledger::launch: {line}"
    assert len(hits) == 2  # launch and launch_tiles
    # the four kernel files do launch through it
    for name in ("kernels.hip", "smoother.hip", "smoother_tb.hip", "transport.hip"):
        with open(os.path.join(CSRC, name)) as f:
            assert re.search(r"ledger::launch(_tiles)?<", f.read()), name


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("family", sorted(cw.PARTS))
def test_family_launches_every_instantiation(family, tmp_path):
    total = {}
    for part, extra in cw.PARTS[family]:  # one after another: one GPU process at a time
        out = tmp_path / f"{family}.{part}.ledger"
        env = dict(os.environ, **extra)
        env.pop("MGIC_LAUNCH_LEDGER", None)
        r = subprocess.run([sys.executable, WORKER, family, part, str(out)], capture_output=True,
                           text=True, env=env, timeout=WORKER_TIMEOUT)
        assert r.returncode == 0, f"{family}/{part}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        for name, count in read_ledger(out).items():
            total[name] = total.get(name, 0) + count
    assert_family_launched(family, total)


def assert_family_launched(family, total):
    mine = {n: c for n, c in total.items() if cw.family_of(n) == [family]}
    assert mine, family
    missing = sorted(n for n, c in mine.items() if c == 0)
    assert not missing, f"{family}: {len(missing)} of {len(mine)} instantiations never launched:\n" \
        + "\n".join(missing)


@pytest.mark.gpu
def test_transport_family_launches_every_instantiation(tmp_path):
    # the peer-mapped transport's kernels need more than one rank: two worker
    # processes (tests/mp_worker.py, one z-slab of 64^3 each), the fp64 V-cycle
    # and the mixed cycle (fp32 messages), phi and every norm (an all-reduce
    # between the ranks) bit-identical to the single box; each rank writes its
    # ledger as its library unloads, and the union of the ranks' files counts
    # The same V-cycle over one RCCL communicator of two ranks, where the
    # all-reduced norm reaches the host through k_publish -- on a box with two
    # devices: RCCL takes one rank per device and refuses a second rank on the
    # same one (ncclCommInitRank: invalid usage), and with one rank, or on the
    # peer-mapped transport, no path leads to k_publish.  On a one-device box
    # that entry alone is held to a count of zero instead.
    import torch

    from tests import test_multiprocess as mp
    n, levels = 64, 3
    total = {}
    two_devices = torch.cuda.device_count() >= 2
    runs = [("vcycle", "ipc"), ("mixed", "ipc")] + ([("vcycle", "rccl")] if two_devices else [])
    for mode, transport in runs:
        d = tmp_path / f"{mode}-{transport}"
        d.mkdir()
        out = mp.run_workers(d, 2, n, levels, mode=mode, timeout=120, transport=transport,
                             devices=2 if transport == "rccl" else 1,
                             env_extra={"MGIC_LAUNCH_LEDGER": str(d / "ledger")})
        mp.check(out, n, levels, mode=mode, transport=transport)
        files = glob.glob(str(d / "ledger.*"))
        assert len(files) == 2, files
        for path in files:
            for name, count in read_ledger(path).items():
                total[name] = total.get(name, 0) + count
    if not two_devices:
        assert total.pop("k_publish") == 0
    assert_family_launched("transport", total)
