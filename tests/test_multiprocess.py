"""BASELINE config C4's real form on the GPU box: separate processes (one
box each, bench.py's split), halo exchange between processes through the
peer-mapped transport (csrc/transport.hpp: hipIpcOpenMemHandle-mapped
receive arenas, device-side flags), all ranks on device 0 of the one-GPU
box.  phi and every residual max norm must be bit-identical to the single
box computed in this process (itself bit-identical to the oracle:
test_gpu_parity.py::test_full_size_512_vcycle_bitwise).

The workers are fresh interpreters (tests/mp_worker.py) started with
subprocess (no fork of this GPU-initialised process, no exec).
"""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

mg = pytest.importorskip("mg_ic_code_amd")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def run_workers(tmp_path, world, n, levels=3, agglomerate_below=0, timeout=240, mode="vcycle",
                bottom_solver=0, fmg=0, env_extra=None, transport="ipc", devices=1):
    port = free_port()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", PYTHONUNBUFFERED="1", **(env_extra or {}))
    procs = []
    logs = []
    for r in range(world):
        log = open(tmp_path / f"w{r}.log", "w")
        logs.append(log)
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(ROOT, "tests", "mp_worker.py"), "--rank", str(r),
             "--world", str(world), "--port", str(port), "--n", str(n), "--levels", str(levels),
             "--agglomerate-below", str(agglomerate_below), "--out", str(tmp_path),
             "--mode", mode, "--bottom-solver", str(bottom_solver), "--fmg", str(fmg),
             "--transport", transport, "--device", str(r % devices)],
            stdout=log, stderr=subprocess.STDOUT, env=env))
    rcs = []
    try:
        for p in procs:
            rcs.append(p.wait(timeout=timeout))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
        for log in logs:
            log.close()
    texts = [(tmp_path / f"w{r}.log").read_text() for r in range(world)]
    if any(rcs) or any("double free" in x or "corruption" in x for x in texts):
        msg = "\n".join(x[-3000:] for x in texts)
        pytest.fail(f"workers exited {rcs}:\n{msg}")
    out = [dict(np.load(tmp_path / f"rank{r}.npz")) for r in range(world)]
    return out


def single_box(n, levels, iters=2, mode="vcycle", bottom_solver=0, fmg=0):
    import bench
    comm = mg.Comm()
    case = bench.build_case(mg, comm, 1, n, levels, 4, bottom_solver=bottom_solver)
    amg, fphi, frhs, fres = (case[k] for k in ("amg", "fphi", "frhs", "fres"))
    if mode == "mixed":
        amg = mg.MixedMultiGrid(case["fac"], mg.SolverParams(
            max_depth=levels - 1, n_pre=4, n_post=4, n_bottom=4, bottom_solver=0))
        norms = [amg.init_residual(fphi, frhs, fres, 0), amg.fmg(fphi, frhs, fres, 0)]
        norms += [amg.iteration(fphi, frhs, fres, 0) for _ in range(iters)]
    else:
        norms = [amg.init_residual(fphi, frhs, fres, norm_type=0)]
        if fmg:
            norms.append(amg.fmg(fphi, frhs, fres, norm_type=0))
        norms += [amg.iteration(fphi, frhs, fres, norm_type=0) for _ in range(iters)]
    return norms, fphi.download(0)


def check(out, n, levels, iters=2, mode="vcycle", bottom_solver=0, fmg=0, transport="ipc"):
    norms, phi = single_box(n, levels, iters, mode, bottom_solver, fmg)
    for o in out:
        assert str(o["transport"]) == transport
        assert bool(o["checked"])  # commcheck.check_transport passed on every rank
        assert list(o["norms"]) == norms, (list(o["norms"]), norms)
        i = 0
        while f"box{i}" in o:
            b = o[f"box{i}"]
            assert np.array_equal(o[f"phi{i}"], phi[b[2]:b[5] + 1, b[1]:b[4] + 1, b[0]:b[3] + 1])
            i += 1
    assert norms[-1] < norms[0]


def test_two_processes_bench_split_512_bitwise(tmp_path):
    # bench.py --gpus 2's exact workload: 512^3 as two 512x512x256 z-slabs, one
    # per process, deep halo (4-deep shells), 3 levels
    n, levels = 512, 3
    check(run_workers(tmp_path, 2, n, levels), n, levels)


def test_four_processes_with_agglomeration_bitwise(tmp_path):
    # bench.py --gpus 4's split (1x2x2) at 128^3, deep halo, the 32^3 depth
    # gathered to rank 0 (agglomerate_below 17: its 32x16x16 boxes), so the
    # gather / scatter plans run between processes too
    n, levels = 128, 3
    check(run_workers(tmp_path, 4, n, levels, agglomerate_below=17), n, levels)


def test_eight_processes_bench_split_512_bitwise(tmp_path):
    # BASELINE config C4 as bench.py --gpus 8 runs it: 512^3 as 2 x 2 x 2
    # boxes of 256^3, one per process, deep halo (4-deep shells), 3 levels,
    # the coarsest depth placed as bench.py places it (AGG_C4 below) -- all
    # eight ranks on this box's one GPU, so the exchange grids are capped
    # (csrc/level.cpp: every rank's exchange workgroups resident at once);
    # phi and every residual norm bit-identical to the single box
    import bench
    n, levels = 512, 3
    check(run_workers(tmp_path, 8, n, levels, agglomerate_below=bench.agglomerate_default(8, n,
                                                                                          levels),
                      timeout=420), n, levels)


@pytest.mark.parametrize("agg", [0, 9])
def test_four_processes_mixed_fmg_bitwise(tmp_path, agg):
    # BASELINE config C5's cycle between processes: the 4-level mixed fp32
    # smoother / fp64 residual FMG and two V-cycles at 128^3 on bench.py's
    # 4-rank split (1 x 2 x 2), deep halo (fp32 4-deep shells before every
    # two-sweep launch), fp32 messages through the peer-mapped transport;
    # agg 9: the coarsest depth (16 x 8 x 8 per rank) gathered onto rank 0,
    # which alone relaxes it (the fp32 restriction gathered, the correction
    # scattered) -- phi and every norm bit-identical to the single box
    # (itself bit-identical to oracle/mixed.py: test_mixed.py)
    n, levels = 128, 4
    check(run_workers(tmp_path, 4, n, levels, agglomerate_below=agg, mode="mixed"), n, levels,
          mode="mixed")


@pytest.mark.parametrize("world", [4, 8])
def test_bicgstab_bottom_on_rank0_bitwise(tmp_path, world):
    # the reference's bottom solver (BiCGStab, Main_PoissonSolver.cpp:103-117)
    # on the gathered coarsest depth: rank 0 alone runs it -- its dot products
    # and norms reduce on rank 0 with no allreduce; the other ranks go from
    # the gather straight to the scatter -- on bench.py's 4- and 8-rank
    # splits at 128^3 (coarsest depth 32^3 on rank 0, bench.py's default
    # placement).  The gathered box is the single box's coarsest box, so its
    # reductions add the same partials in the same order: phi and every norm
    # bit-identical to the single box
    import bench
    n, levels = 128, 3
    agg = bench.agglomerate_default(world, n, levels)
    check(run_workers(tmp_path, world, n, levels, agglomerate_below=agg, bottom_solver=1,
                      timeout=300), n, levels, bottom_solver=1)


@pytest.mark.parametrize("agg", [0, 9])
def test_four_processes_fp64_fmg_bitwise(tmp_path, agg):
    # MultiGrid::fmg (fp64) between processes on bench.py's 4-rank split at
    # 128^3, 4 levels, deep halo; agg 9: the coarsest depth gathered onto rank
    # 0 -- the other ranks stop the FMG's restriction loop after the gather,
    # skip the coarse solve and wait in the scatter while rank 0 runs the
    # gathered depths -- then two V-cycles: phi and every norm bit-identical
    # to the single box
    n, levels = 128, 4
    check(run_workers(tmp_path, 4, n, levels, agglomerate_below=agg, fmg=1), n, levels, fmg=1)


def test_two_processes_distributed_bicgstab_bottom_pipelines_agree(tmp_path):
    # the BiCGStab bottom NOT gathered (agglomerate_below 0): every rank runs
    # the host loop on its own half of the coarsest depth, each dot product
    # and norm an allreduce (two back-to-back ones in dot2), the preCond /
    # applyOp exchanges queued before the loop reads the norm that decides
    # whether they were needed (MGIC_BICG_PIPE=1) -- phi and every norm
    # bit-identical to the loop that waits for every reduction
    # (MGIC_BICG_PIPE=0).  Against the single box the two halves' partial sums
    # add in another order: equal to a relative 1e-9
    n, levels = 128, 3
    runs = []
    for pipe in ("1", "0"):
        d = tmp_path / f"pipe{pipe}"
        d.mkdir()
        runs.append(run_workers(d, 2, n, levels, agglomerate_below=0, bottom_solver=1,
                                env_extra={"MGIC_BICG_PIPE": pipe}))
    for a, b in zip(runs[0], runs[1]):
        assert list(a["norms"]) == list(b["norms"])
        assert np.array_equal(a["phi0"], b["phi0"])
    norms, phi = single_box(n, levels, 2, "vcycle", 1)
    for o in runs[0]:
        assert np.allclose(o["norms"], norms, rtol=1e-9, atol=0.0)
        b = o["box0"]
        ref = phi[b[2]:b[5] + 1, b[1]:b[4] + 1, b[0]:b[3] + 1]
        assert np.linalg.norm(o["phi0"] - ref) <= 1e-9 * np.linalg.norm(ref)


def test_two_processes_gathered_device_bicgstab_bottom_bitwise(tmp_path):
    # bench.py's split of 512^3 over two processes with the reference's
    # BiCGStab bottom gathered onto rank 0 (agglomerate_below 65: the two
    # 128 x 128 x 64 halves of the coarsest depth become one 128^3 box): rank
    # 0 runs it on the device (BiCGStabSolver::solveDevice, as the bench's
    # 8-GPU split does) -- phi and every norm bit-identical to the single box
    n, levels = 512, 3
    check(run_workers(tmp_path, 2, n, levels, agglomerate_below=65, bottom_solver=1, timeout=300),
          n, levels, bottom_solver=1)


def test_worker_exits_cleanly_with_one_hip_runtime(tmp_path):
    # the abort at exit of a process holding two HIP runtimes (torch's bundled
    # libamdhip64 and /opt/rocm's, "double free or corruption", status -6):
    # a fresh one-rank worker process maps one image (mp_worker checks it) and
    # exits 0 with no heap-corruption message (run_workers fails on either)
    out = run_workers(tmp_path, 1, 64, 3)
    assert len(out) == 1 and list(out[0]["norms"])


def test_transport_check_single_rank():
    # the check bench.py runs before trusting a transport, on one rank: the
    # periodic images arrive through local copies, the reduction is local
    from mg_ic_code_amd.commcheck import check_transport
    assert check_transport(mg.Comm(), 1)
