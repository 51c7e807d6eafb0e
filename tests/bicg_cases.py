"""The BiCGStab cases that are pinned to the oracle, and their builders.

One table serves two tests.  tests/test_oracle.py runs every case on the
oracle alone, on one box and on three other decompositions: the oracle's
stencils do not depend on the decomposition (bit for bit, test_oracle.py),
so only the order of its serial dot products and norms changes -- which is
what a GPU reduction tree changes too.  A case whose iteration counts,
phi and residual norms hold still there (CPU_PHI_TOL, CPU_NORM_TOL) is well
enough conditioned that tests/test_bicgstab_parity.py may hold the HIP
solver to GPU_PHI_TOL / GPU_NORM_TOL, 100 times wider, without a wrong
kernel hiding behind conditioning.  A case that misses the CPU gate is
replaced, never loosened ("BiCGStab: what is pinned to the
oracle", lists the ones left out: 64^3 bottoms, random bCoef at alpha = 0,
eps = 1e-9, the direct 32^3 solve with mixed BCs).

`python -m tests.bicg_cases` prints the table of measured spreads.
"""
from __future__ import annotations

import functools
import os
from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

import numpy as np

import oracle

CPU_PHI_TOL = 1e-12    # rel-L2 spread of phi over the oracle's decompositions
CPU_NORM_TOL = 1e-12   # spread of a residual norm / the initial residual norm
GPU_PHI_TOL = 1e-10    # BASELINE's bar: rel-L2 of phi against the one-box oracle
GPU_NORM_TOL = 1e-10   # |norm - oracle's| / the initial residual norm
MIN_ITERS = 8          # an "iterating" solve: the most iterations of any solve >= this
VCYCLES = 3
# The residual norms compared are L2 norms (norm type 2).  The max norm of
# the first V-cycle's residual is one cell's value and moves by up to
# 3e-12 x the initial norm over the oracle's decompositions (rnd64_2l), over
# the CPU gate; the L2 norm moves by 1.3e-14 at most.
NORM_TYPE = 2

MIXED_BC = dict(bc_lo=(0, 1, 0), bc_hi=(1, 0, 0), bc_value=0.375)
OUTER = dict(mg_iters=2, imax=100, eps=1e-10, norm_type=0)  # params.txt's outer solve


@dataclass(frozen=True)
class Case:
    name: str
    kind: str                         # "vcycle" | "direct" | "outer"
    shape: Tuple[int, int, int]       # nx, ny, nz
    levels: int
    inputs: str                       # "bh" | "rnd" | "smooth_b"
    alpha: float
    splits: Tuple[Tuple[int, int, int], ...]  # the oracle's other decompositions
    seed: int = 7
    bc: Dict = field(default_factory=dict)      # bc_lo / bc_hi / bc_value
    params: Dict = field(default_factory=dict)  # bicg_* overrides (SolverParams / OracleMG)
    expect: str = "iterates"          # "iterates" | "restarts" | "limit" | "recovers"
    hom: int = 1                      # direct solves: homogeneous BC
    device: bool = True               # the device loop takes the solve (constant bCoef)
    group: str = "a"                  # parity test: "a" paths only, "b" also bitwise over batches
    dx: Optional[float] = None        # default 100 / nx

    @property
    def spacing(self) -> float:
        return self.dx if self.dx is not None else 100.0 / self.shape[0]

    @property
    def domain(self):
        nx, ny, nz = self.shape
        return (0, 0, 0, nx - 1, ny - 1, nz - 1)


_CUBE = ((2, 2, 2), (2, 1, 1), (1, 2, 4))

# The V-cycle cases: three AMRMultiGrid iterations from phi = 0, harmonic
# averaging, linear prolongation, 4/4 sweeps, BiCGStab bottom (eps 1e-6,
# imax 80, norm type 2 unless overridden), beta = -1, dx = 100 / nx.
# alpha = 1 with random aCoef does not iterate (one or two iterations), so
# random inputs use alpha = 0 and alpha = 1 uses the SetBinaryBH inputs.
VCYCLE_CASES = (
    Case("bh64_2l", "vcycle", (64, 64, 64), 2, "bh", 1.0, _CUBE),
    Case("bh128_3l", "vcycle", (128, 128, 128), 3, "bh", 1.0, _CUBE),
    Case("bh64_3l", "vcycle", (64, 64, 64), 3, "bh", 1.0, _CUBE),            # 16^3 bottom
    Case("rnd64_2l", "vcycle", (64, 64, 64), 2, "rnd", 0.0, _CUBE),
    Case("rnd128_3l", "vcycle", (128, 128, 128), 3, "rnd", 0.0, _CUBE),
    # non-cubic bottom 36 x 10 x 14 with Dirichlet / Neumann faces and a BC
    # value.  MGnewOp gives a depth only to boxes coarsenable by 2^depth *
    # s_maxCoarse (Factory.cpp:168-172), so every side of a 2-level domain is
    # a multiple of 4: 72 x 18 x 28 (bottom 36 x 9 x 14) builds one depth only
    # and 72 x 20 x 28 is the nearest shape that builds two.  Every bottom's
    # ny * nz is therefore a multiple of the 4 rows of a reduction block; the
    # partial last block is covered by the direct 40 x 9 x 14 solve below.
    Case("rnd72x20x28_mixed", "vcycle", (72, 20, 28), 2, "rnd", 0.0,
         ((2, 1, 1), (1, 5, 1), (3, 1, 7)), bc=MIXED_BC),
    # variable bCoef: preCond is not one two-sweep launch, so the host loop
    Case("rnd64_smooth_b", "vcycle", (64, 64, 64), 2, "smooth_b", 0.0, _CUBE, device=False),
    # ---- group b: stop tests, restarts, norm types
    Case("rnd64_nt0", "vcycle", (64, 64, 64), 2, "rnd", 0.0, _CUBE,
         params=dict(bicg_norm_type=0), group="b"),
    Case("rnd64_nt1", "vcycle", (64, 64, 64), 2, "rnd", 0.0, _CUBE,
         params=dict(bicg_norm_type=1), group="b"),
    Case("rnd64_imax10", "vcycle", (64, 64, 64), 2, "rnd", 0.0, _CUBE,
         params=dict(bicg_imax=10), group="b"),
    Case("rnd64_small03", "vcycle", (64, 64, 64), 2, "rnd", 0.0, _CUBE,
         params=dict(bicg_small=0.3), expect="restarts", group="b"),
    Case("rnd64_small03_r1", "vcycle", (64, 64, 64), 2, "rnd", 0.0, _CUBE,
         params=dict(bicg_small=0.3, bicg_restarts=1), expect="limit", group="b"),
    Case("rnd64_small05", "vcycle", (64, 64, 64), 2, "rnd", 0.0, _CUBE,
         params=dict(bicg_small=0.5), expect="limit", group="b"),
)

# The direct solve on one level: phi starts from a random field, eps 1e-6,
# alpha = 0, dx = 100 / 64.  (32^3 with the mixed BCs is left out: 31
# iterations with nothing around them to damp a reduction-order difference,
# spread 2.5e-11.)
_DX = 100.0 / 64
DIRECT_CASES = (
    Case("direct32_hom1", "direct", (32, 32, 32), 1, "rnd", 0.0, _CUBE, hom=1, dx=_DX),
    Case("direct36x18x14_hom0", "direct", (36, 18, 14), 1, "rnd", 0.0,
         ((2, 1, 1), (1, 2, 1), (2, 3, 2)), bc=MIXED_BC, hom=0, dx=_DX),
    Case("direct36x18x14_hom1", "direct", (36, 18, 14), 1, "rnd", 0.0,
         ((2, 1, 1), (1, 2, 1), (2, 3, 2)), bc=MIXED_BC, hom=1, dx=_DX),
    # ny * nz = 126 rows: the last reduction block (4 rows) is partial
    Case("direct40x9x14_hom0", "direct", (40, 9, 14), 1, "rnd", 0.0,
         ((2, 1, 1), (1, 3, 1), (4, 3, 2)), bc=MIXED_BC, hom=0, dx=_DX),
    Case("direct40x9x14_hom1", "direct", (40, 9, 14), 1, "rnd", 0.0,
         ((2, 1, 1), (1, 3, 1), (4, 3, 2)), bc=MIXED_BC, hom=1, dx=_DX),
    # a restart that recovers.  In the V-cycle restart cases above every
    # restart is followed at once by the next one up to the limit (a restart
    # that fails leaves phi unchanged, so the next starts from the same state),
    # so nothing computed after a restart reaches phi there.  Here the solve
    # restarts twice and goes on to converge: the fresh residual, RT = R and
    # the P = R of init = 1 after a restart all feed the result.
    Case("direct24x12x16_restart", "direct", (24, 12, 16), 1, "rnd", 0.0,
         ((2, 1, 1), (1, 2, 1), (2, 3, 2)), seed=23, params=dict(bicg_small=0.2),
         expect="recovers", hom=1, dx=_DX),
)

# The outer solve of Main_PoissonSolver.cpp:174-184 with the reference's own
# bottom: BiCGStab over MultilevelLinearOp (two AMRMultiGrid iterations as the
# preconditioner), BiCGStab at the coarsest depth.
OUTER_CASES = (
    Case("outer_bh64_2l", "outer", (64, 64, 64), 2, "bh", 1.0, _CUBE),
    Case("outer_rnd64_2l", "outer", (64, 64, 64), 2, "rnd", 0.0, _CUBE),
    Case("outer_rnd128_3l", "outer", (128, 128, 128), 3, "rnd", 0.0, _CUBE),
)

CASES = VCYCLE_CASES + DIRECT_CASES + OUTER_CASES
BY_NAME = {c.name: c for c in CASES}


@functools.lru_cache(maxsize=None)
def _arrays(inputs: str, shape, seed: int, dx: float, direct: bool):
    nx, ny, nz = shape
    if inputs == "bh":
        from mg_ic_code_amd.params import read_params_file
        assert nx == ny == nz
        prm = read_params_file(os.path.join(os.path.dirname(__file__), "golden", "params.txt"))
        bh = prm.bh()
        bh["domain_length"] = dx * nx  # as bench.py's build_case
        a, rhs = oracle.binary_bh(bh, (0, 0, 0), (nx - 1, ny - 1, nz - 1), dx)
        b = np.ones_like(a)
        phi0 = None
    else:
        # build_pair's draws with bvar=False: aCoef, then rhs
        rng = np.random.default_rng(seed)
        a = rng.uniform(-2.0, -0.5, (nz, ny, nx))
        rhs = rng.uniform(-1, 1, (nz, ny, nx))
        phi0 = rng.uniform(-1, 1, (nz, ny, nx)) if direct else None
        if inputs == "smooth_b":
            z, y, x = np.meshgrid((np.arange(nz) + 0.5) / nz, (np.arange(ny) + 0.5) / ny,
                                  (np.arange(nx) + 0.5) / nx, indexing="ij")
            b = 1.0 + 0.5 * np.sin(2 * np.pi * x) * np.cos(2 * np.pi * y) * np.sin(4 * np.pi * z)
        else:
            b = np.ones_like(a)
    for arr in (a, b, rhs, phi0):
        if arr is not None:
            arr.setflags(write=False)
    return a, b, rhs, phi0


def arrays(case: Case):
    """(aCoef, bCoef, rhs, phi0) of the case, (nz, ny, nx), read-only and shared."""
    return _arrays(case.inputs, case.shape, case.seed, case.spacing, case.kind == "direct")


def split(case: Case, parts):
    from mg_ic_code_amd.decomposition import split_domain
    return split_domain(case.domain, parts)


def make_oracle(case: Case, parts=(1, 1, 1)):
    """(OracleMG with the case's coefficients and rhs loaded, its boxes)."""
    a, b, rhs, phi0 = arrays(case)
    boxes = split(case, parts)
    o = oracle.OracleMG(boxes, case.domain, case.spacing, alpha=case.alpha, beta=-1.0,
                        nlevels=case.levels, avg_type=1, prolong_type=1, bottom_solver=1,
                        **case.bc, **case.params)
    for bi, bx in enumerate(boxes):
        s = np.s_[bx[2]:bx[5] + 1, bx[1]:bx[4] + 1, bx[0]:bx[3] + 1]
        o.set(0, oracle.ACOEF, bi, a[s])
        o.set(0, oracle.BCOEF, bi, b[s])
        o.set(0, oracle.RHS, bi, rhs[s])
        if phi0 is not None:
            o.set(0, oracle.PHI, bi, phi0[s])
    o.setup()
    return o, boxes


def _gather(o, case: Case, nbox: int, field_id: int):
    nx, ny, nz = case.shape
    out = np.zeros((nz, ny, nx))
    for bi in range(nbox):
        bx = o.box(0, bi)
        out[bx[2]:bx[5] + 1, bx[1]:bx[4] + 1, bx[0]:bx[3] + 1] = o.get(0, field_id, bi)
    return out


def run_oracle(case: Case, parts=(1, 1, 1)):
    """The case on the oracle: dict(r0, norms, iters, restarts, limit, phi).
    iters / restarts / limit hold one entry per BiCGStab solve that can be read
    back (each V-cycle's bottom; the direct solve; the outer solve)."""
    o, boxes = make_oracle(case, parts)
    out = dict(r0=None, norms=[], iters=[], restarts=[], limit=[], final_norm=None)

    def record():
        n, lim = o.last_bicg_restarts()
        out["iters"].append(o.last_bicg_iters())
        out["restarts"].append(n)
        out["limit"].append(lim)

    if case.kind == "vcycle":
        out["r0"] = o.init_residual(NORM_TYPE)
        for _ in range(VCYCLES):
            out["norms"].append(o.iteration(NORM_TYPE))
            record()
    elif case.kind == "direct":
        it = o.bicgstab(0, oracle.PHI, oracle.RHS, case.hom)
        record()
        assert out["iters"] == [it]
    else:
        it, fin = o.solve(**OUTER)
        record()
        assert out["iters"] == [it]
        out["final_norm"] = fin
    out["phi"] = _gather(o, case, len(boxes), oracle.PHI)
    return out


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """The one-box oracle run of a case, computed once and shared (read-only)."""
    ref = run_oracle(BY_NAME[name])
    ref["phi"].setflags(write=False)
    return ref


def rel_l2(x, ref) -> float:
    return float(np.linalg.norm(x - ref) / np.linalg.norm(ref))


def spreads(case: Case):
    """The CPU gate's measurements: the one-box run against `case.splits`."""
    ref = reference(case.name)
    runs = [run_oracle(case, p) for p in case.splits]
    phi = max(rel_l2(r["phi"], ref["phi"]) for r in runs)
    nrm = 0.0
    for r in runs:
        for x, y in zip(r["norms"], ref["norms"]):
            nrm = max(nrm, abs(x - y) / ref["r0"])
    return dict(ref=ref, runs=runs, phi_spread=phi, norm_spread=nrm)


def make_gpu(mg, comm, case: Case, parts=(1, 1, 1), agglomerate_below=0, fused=2):
    """The HIP side of a case from the same arrays: grid, fields, operator
    factory and, for V-cycle and outer cases, the AMRMultiGrid."""
    a, b, rhs, phi0 = arrays(case)
    boxes = split(case, parts)
    grid = mg.Grid(comm, case.domain, boxes, case.spacing)
    fa, fb, frhs, fphi, fres = (mg.LevelData(grid) for _ in range(5))
    for f, arr in ((fa, a), (fb, b), (frhs, rhs)) + (((fphi, phi0),) if phi0 is not None else ()):
        for n in range(grid.num_local):
            bx = grid.local_box(n)
            f.upload(n, np.ascontiguousarray(arr[bx[2]:bx[5] + 1, bx[1]:bx[4] + 1,
                                                 bx[0]:bx[3] + 1]))
    if phi0 is None:
        fphi.set_zero()
    prm = mg.OperatorParams(alpha=case.alpha, beta=-1.0, coefficient_average_type=1,
                            prolong_type=1, relax_mode=1, fused_smoother=fused, **case.bc)
    fac = mg.defineOperatorFactory(grid, fa, fb, prm)
    sp = mg.SolverParams(max_depth=case.levels - 1, bottom_solver=1,
                         agglomerate_below=agglomerate_below, **case.params)
    amg = None
    if case.kind != "direct":
        amg = mg.AMRMultiGrid(fac, sp)
        assert amg.num_depths == case.levels, (case.name, amg.num_depths)
    return dict(grid=grid, boxes=boxes, fa=fa, fb=fb, frhs=frhs, fphi=fphi, fres=fres, fac=fac,
                amg=amg, params=sp, rhs=rhs)


def download(mg_field, grid, case: Case):
    nx, ny, nz = case.shape
    out = np.zeros((nz, ny, nx))
    for n in range(grid.num_local):
        bx = grid.local_box(n)
        out[bx[2]:bx[5] + 1, bx[1]:bx[4] + 1, bx[0]:bx[3] + 1] = mg_field.download(n)
    return out


def main():
    print("| case | bottom / level | its per solve | restarts (limit) | equal over 4 decomp. "
          "| phi spread | norm spread / r0 |")
    print("|---|---|---|---|---|---|---|")
    for c in CASES:
        s = spreads(c)
        ref = s["ref"]
        same = all(r["iters"] == ref["iters"] and r["restarts"] == ref["restarts"]
                   and r["limit"] == ref["limit"] for r in s["runs"])
        bottom = " x ".join(str(n >> (c.levels - 1)) for n in c.shape)
        rs = ", ".join(f"{n}{'*' if lim else ''}" for n, lim in zip(ref["restarts"], ref["limit"]))
        print(f"| {c.name} | {bottom} | {', '.join(map(str, ref['iters']))} | {rs} | "
              f"{'yes' if same else 'NO'} | {s['phi_spread']:.1e} | "
              + (f"{s['norm_spread']:.1e}" if ref["norms"] else "--") + " |")


if __name__ == "__main__":
    main()
