#!/usr/bin/env python3
"""Cost of the reflux term on tools/bench_regrid.py's hierarchy:
AMRSolver.applyOp over the levels set_grids generates from an n^3 base, with
the switch off and on, in one process on one device -- ms per call over
`reps` calls (host clock around calls that end in a device synchronise), and
the launches of libmgic_reflux.so's kernels per call.  No bar: the figure
goes into DESIGN.md, not into a test.

usage: python tools/bench_reflux.py [params.txt] [--size N] [--max-level K] [--reps R]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("params", nargs="?", default=os.path.join(ROOT, "tests", "golden", "params.txt"))
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--max-level", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import _lib
    from mg_ic_code_amd import grids as G
    from mg_ic_code_amd.core import read_launch_ledger
    from mg_ic_code_amd.params import read_params_file
    prm = read_params_file(args.params)
    n = args.size
    comm = mg.Comm()
    dom = (0, 0, 0, n - 1, n - 1, n - 1)
    base = mg.Grid(comm, dom, [dom], prm.domainLength[0] / n)
    grids = G.set_grids(comm, prm, base, max_level=args.max_level)
    res = {"size": n, "levels": [len(g.boxes) for g in grids]}
    a, b, x, y = ([mg.LevelData(g) for g in grids] for _ in range(4))
    for l in range(len(grids)):
        a[l].set_val(-1.0)
        b[l].set_val(1.0)
        x[l].set_val_all(1.0 + 0.25 * l)
    op = mg.OperatorParams(alpha=prm.alpha, beta=prm.beta, bc_lo=tuple(prm.bc_lo),
                           bc_hi=tuple(prm.bc_hi), bc_value=prm.bc_value, prolong_type=1)

    def ledger():
        fd, path = tempfile.mkstemp(prefix="mgic_reflux_ledger_")
        os.close(fd)
        try:
            _lib.reflux_call("mgic_reflux_launch_ledger_dump", path.encode())
            return read_launch_ledger(path)
        finally:
            os.unlink(path)

    for name, on in (("off", False), ("on", True), ("off_again", False)):
        amr = mg.AMRSolver(list(zip(grids, a, b)), op, mg.SolverParams(max_depth=2), reflux=on)
        amr.applyOp(y, x, True)  # warm-up: code objects, the flux registers
        comm.synchronize()
        before = ledger() if on else None
        t0 = time.perf_counter()
        for _ in range(args.reps):
            amr.applyOp(y, x, True)
        comm.synchronize()
        res[name + "_ms"] = round((time.perf_counter() - t0) / args.reps * 1e3, 4)
        if on:
            after = ledger()
            res["reflux_launches_per_call"] = {k: (after[k] - before[k]) / args.reps for k in after}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
