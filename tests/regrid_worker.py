#!/usr/bin/env python3
"""One rank of a multi-process set_grids run, for tests/test_regrid.py: the
32^3 base level as `world` slabs across --split-dir, one per rank (all ranks
on one device, peer-mapped transport), params.txt with one black hole at
x = --bh1-offset, max_level 2.

    regrid_worker.py --rank R --world W --port P --out DIR [--device D]
                     [--bh1-offset X] [--split-dir 0|1|2]
Writes DIR/rank<R>.json: the boxes and owners of every generated level and
this rank's local boxes.  gloo (127.0.0.1) is the control plane and carries
the tag masks; nothing touches the GPU before the process group exists.
"""
import argparse
import datetime
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--world", type=int, required=True)
    ap.add_argument("--port", type=int, required=True)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--bh1-offset", default="0.0")
    ap.add_argument("--split-dir", type=int, default=2)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()

    import torch
    import torch.distributed as dist

    import mg_ic_code_amd as mg
    from mg_ic_code_amd._lib import check_single_hip_runtime
    from mg_ic_code_amd.grids import set_grids
    from mg_ic_code_amd.params import read_params_file

    check_single_hip_runtime()
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{a.port}", rank=a.rank,
                            world_size=a.world, timeout=datetime.timedelta(seconds=120))
    mg.set_device(a.device)
    comm = mg.Comm(a.rank, a.world, transport="ipc")
    prm = read_params_file(os.path.join(ROOT, "tests", "golden", "params.txt"), overrides=dict(
        bh1_offset=a.bh1_offset, bh2_bare_mass="0.0", bh2_spin="0.0", bh2_momentum="0.0",
        block_factor="8", max_grid_size="16", fill_ratio="0.5"))
    n, w = a.n, a.world
    dom = (0, 0, 0, n - 1, n - 1, n - 1)
    slabs = []
    for r in range(w):
        b = [0, 0, 0, n - 1, n - 1, n - 1]
        b[a.split_dir], b[3 + a.split_dir] = r * n // w, (r + 1) * n // w - 1
        slabs.append(tuple(b))
    base = mg.Grid(comm, dom, slabs, prm.L / n, owners=list(range(w)))
    grids = set_grids(comm, prm, base, max_level=2)
    comm.synchronize()
    out = {"boxes": [g.boxes for g in grids[1:]], "owners": [g.owners for g in grids[1:]],
           "local": [[list(g.local_box(k)) for k in range(g.num_local)] for g in grids[1:]]}
    with open(os.path.join(a.out, f"rank{a.rank}.json"), "w") as f:
        json.dump(out, f)
    dist.barrier()
    del grids, base
    dist.destroy_process_group()
    print(json.dumps({"rank": a.rank, "levels": len(out["boxes"]) + 1}), flush=True)
    del torch


if __name__ == "__main__":
    main()
