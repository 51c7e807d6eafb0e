"""Worker for tests/test_regrid_periodic.py: one fresh interpreter.

    python tests/ptag_worker.py kernel LEDGER_PATH
        runs the three-box and the single-box kernel cases of libmgic_ptag.so
        against the restatement (any mismatch is an AssertionError: the exit
        code is non-zero), dumps that library's launch ledger and prints
        {"calls": the number of tagging calls made}.
    python tests/ptag_worker.py off
        set_grids on the 16^3 base with the hole on the x-hi face: plain on a
        bounded base, the switch off on a periodic one, the switch on on a
        bounded one; prints their box lists, libmgic's k_tag_lattice count of
        each, and whether libmgic_ptag.so was ever loaded.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def kernel(path):
    import mg_ic_code_amd as mg
    from mg_ic_code_amd import _lib
    from tests import test_regrid_periodic as T
    comm = mg.Comm()
    got = T.run_kernel_cases(comm, ["three", "corner"], ["xyz", "x"])
    mg.device_synchronize()
    _lib.ptag_call("mgic_ptag_launch_ledger_dump", path.encode())
    assert not any("ptag" in n for n in mg.launch_ledger())
    print(json.dumps({"calls": len(got)}))
    return 0


def off():
    import dataclasses

    import mg_ic_code_amd as mg
    from mg_ic_code_amd import _lib, grids
    from tests import test_regrid_periodic as T
    comm = mg.Comm()
    prm = T._centred_params(T.FACE)
    dom0 = (0, 0, 0, 15, 15, 15)

    def run(periodic, max_level=2, **kw):
        base = mg.Grid(comm, dom0, [dom0], prm.L / 16, periodic=periodic)
        mg.launch_ledger_reset()
        levels = grids.set_grids(comm, kw.pop("prm", prm), base, max_level=max_level, **kw)
        return dict(boxes=[g.boxes for g in levels],
                    k_tag_lattice=mg.launch_ledger()["k_tag_lattice"])

    out = dict(plain=run((0, 0, 0)),
               off_periodic=run(T.TORUS, periodic_regrid=False),
               on_bounded=run((0, 0, 0), prm=dataclasses.replace(prm, regrid_periodic=1)))
    out["level1_after_pass1"] = len(run((0, 0, 0), max_level=1)["boxes"][1])
    out["ptag_loaded"] = _lib.ptag_loaded()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(kernel(sys.argv[2]) if sys.argv[1] == "kernel" else off())
