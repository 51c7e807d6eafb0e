#!/usr/bin/env python3
"""Timing of set_grids (mg_ic_code_amd/grids.py) at an n^3 base (one box):
the whole hierarchy generation (host clock around calls that end in a device
synchronise), and its two device kernels on the base level -- the regrid
condition (8 B written per cell) and the tag kernel (8 B read per cell),
ms per call over `reps` calls.  The tag call's time includes its mask clear,
the device-to-host copy of the lattice mask and the synchronise; the kernel's
own time comes from a kernel trace of this program (k_tag_lattice).

With --periodic-ab the base is periodic in every direction and set_grids is
timed with periodic_regrid off, on and off again in this one process (DESIGN.md
3m); the kernel's own time comes from a kernel trace (k_ptag_lattice).

usage: python tools/bench_regrid.py [params.txt] [--size N] [--max-level K] [--reps R]
                                    [--periodic-ab]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("params", nargs="?", default=os.path.join(ROOT, "tests", "golden", "params.txt"))
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--max-level", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--periodic-ab", action="store_true",
                    help="a periodic base: set_grids with periodic_regrid off, on, off")
    args = ap.parse_args()
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import grids as G
    from mg_ic_code_amd.params import read_params_file
    prm = read_params_file(args.params)
    n = args.size
    comm = mg.Comm()
    dom = (0, 0, 0, n - 1, n - 1, n - 1)
    base = mg.Grid(comm, dom, [dom], prm.domainLength[0] / n)
    res = {"size": n, "max_level": args.max_level}
    if args.periodic_ab:
        pbase = mg.Grid(comm, dom, [dom], prm.domainLength[0] / n, periodic=(1, 1, 1))
        res["periodic_ab"] = []
        for on in (False, True, False):
            G.set_grids(comm, prm, pbase, max_level=args.max_level, periodic_regrid=on)  # warm-up
            comm.synchronize()
            t = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                g = G.set_grids(comm, prm, pbase, max_level=args.max_level, periodic_regrid=on)
                comm.synchronize()
                t.append(time.perf_counter() - t0)
            res["periodic_ab"].append({"periodic_regrid": on, "boxes": [len(x.boxes) for x in g],
                                       "set_grids_ms": {"min": round(min(t) * 1e3, 2),
                                                        "max": round(max(t) * 1e3, 2)}})
        print(json.dumps(res), flush=True)
        return

    def set_grids():
        g = G.set_grids(comm, prm, base, max_level=args.max_level)
        comm.synchronize()
        return g

    grids = set_grids()  # warm-up: code objects, allocations
    t = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        set_grids()
        t.append(time.perf_counter() - t0)
    res["set_grids_ms"] = {"min": round(min(t) * 1e3, 2), "max": round(max(t) * 1e3, 2)}
    res["levels"] = [{"boxes": len(g.boxes),
                      "cells": sum((b[3] - b[0] + 1) * (b[4] - b[1] + 1) * (b[5] - b[2] + 1)
                                   for b in g.boxes)} for g in grids]

    cells = n ** 3
    c, _ = G.regrid_lattice(prm.block_factor, prm.max_grid_size)
    cond = mg.LevelData(base)
    bh = prm.bh()
    G.set_regrid_condition(None, cond, bh)
    comm.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.reps):
        G.set_regrid_condition(None, cond, bh)
    comm.synchronize()
    ms = (time.perf_counter() - t0) / args.reps * 1e3
    res["condition"] = {"ms": round(ms, 4), "GBps_written": round(8 * cells / (ms * 1e-3) / 1e9, 1)}
    tag_val = G._level_max_norm(cond) * prm.refine_threshold
    for name, tv in (("tag", tag_val), ("tag_all_cells", 0.0)):
        G.tag_lattice(cond, tv, G.TAGS_GROW, c)
        t0 = time.perf_counter()
        for _ in range(args.reps):
            _, mask = G.tag_lattice(cond, tv, G.TAGS_GROW, c)
        ms = (time.perf_counter() - t0) / args.reps * 1e3
        res[name] = {"call_ms": round(ms, 4), "lattice_cells_set": int(mask.sum()),
                     "GBps_read_per_call": round(8 * cells / (ms * 1e-3) / 1e9, 1)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
