"""Periodic decks closed by the CTTK method: a K(x) field and its momentum source.

`poisson_solve` closes the Hamiltonian constraint of a periodic deck the
reference's way: one constant K from the integrability condition, then a
nonlinear solve for psi.  The CTTK method (Aurrekoetxea, Clough & Lim) turns
the problem round.  The conformal factor psi is the caller's choice (psi = 1
by default) and the trace K of the extrinsic curvature varies in space, so the
Hamiltonian constraint is algebraic, cell by cell,

    (2/3) K^2 = I,   I = set_nl_integrand_ctt(psi, ..., constant_K = 0, LW)

(constraints.py: Ham = (2/3) K^2 - (2/3) * the integrand's value), and the
momentum constraint gains the gradient of K as a source,

    S_i = -(D_j Abar^BY_ij + psi^6 (8 pi G Pi D_i phi - (2/3) D_i K))

solved as the vector Poisson problem of momentum.py.  K depends on the
longitudinal piece LW_ij through A2, and LW_ij on K through S_i, so the two
are iterated, from LW_ij = 0:

    1. I from psi and the current LW_ij             (libmgic's integrand kernel)
    2. K = -sqrt(I) on the valid cells, exchanged   (k_cttk_K)
    3. from the second pass on: step = max|K - K_prev|; converged when
       step <= tol * max|K| -- K is then the latest tensor's
    4. S_i = momentum_source(...) + ((2/3) psi^6) D_i K          (k_cttk_source)
    5. the projected solves for V_i and U, then LW_ij    (momentum.py, as it is)

V_i and U are kept as initial guesses between passes.  When the passes run out
K is evaluated once more from the final tensor and `converged` is False;
either way the returned K belongs to the returned tensor, so Ham is at
rounding.  A cell with I < 0 (or NaN) has no real K: the chosen psi, or a
negative potential, asks for more than the sources give; CTTKError names the
count and the pass.

The constraints of the result are libmgic's at constant_K = 0 with one
correcting launch (k_cttk_constraints): Ham += (2/3) K^2, Ham_abs +=
|(2/3) K^2|, Mom_i -= (2/3) D_i K.

One periodic level without holes; hierarchies, asymptotically flat decks and
punctures are refused (ValueError) before anything is loaded or launched.
The three kernels are libmgic_cttk.so's (include/mgic_cttk.h), loaded on first
use; `poisson_solve` never loads it.

    cttk_solve(grid, prm, ...) -> CTTKResult
    set_K / add_source / correct_constraints      the three kernels, one level
    cttk_launch_ledger()                          the library's ledger
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

from ._lib import cttk_call
from .core import Grid, LevelData, OperatorParams, SolverParams
from .matter import MatterArgumentError, fill_matter, resolve_matter
from .params import PoissonParameters
from .phi import resolve_phi0


class CTTKError(RuntimeError):
    """The integrand is negative (or NaN) somewhere: no real K closes the
    Hamiltonian constraint at the chosen psi."""

    def __init__(self, bad_cells: int, iteration: int):
        super().__init__(f"cttk_solve: K^2 < 0 in {bad_cells} cells on pass {iteration}: the "
                         "chosen psi (or a negative potential) has no real K there")
        self.bad_cells = bad_cells
        self.iteration = iteration


@dataclass
class CTTKResult:
    psi: LevelData
    K: LevelData
    momentum: object  # momentum.MomentumFields: V, U, W and the LW_ij of the result
    k_steps: List[float] = field(default_factory=list)  # max|K - K_prev| per pass
    k_max: float = 0.0   # max|K|
    k_mean: float = 0.0  # sum(K) / cells
    # per pass: the BiCGStab iterations of V1 V2 V3 U, the means removed from S_i
    # (absolute, and over max|S_i|), (final residual, max|rhs|) per solve
    momentum_iterations: List[List[int]] = field(default_factory=list)
    momentum_net: List[List[float]] = field(default_factory=list)
    momentum_net_relative: List[List[float]] = field(default_factory=list)
    momentum_residuals: List[List[tuple]] = field(default_factory=list)
    iterations: int = 0  # momentum passes taken
    converged: bool = False
    constraints: object = None  # constraints.ConstraintReport of the corrected fields


def _handles(fields: Sequence[LevelData]):
    return (ctypes.c_void_p * len(fields))(*[f.handle.value for f in fields])


def set_K(integrand: LevelData, K: LevelData) -> int:
    """K = -sqrt(integrand) on the valid cells (k_cttk_K); a cell with
    !(integrand >= 0) gets K = 0 and is counted.  Returns the count."""
    bad = ctypes.c_longlong(0)
    cttk_call("mgic_cttk_K", integrand.grid.comm.handle, integrand.handle, K.handle,
              ctypes.byref(bad))
    return int(bad.value)


def add_source(psi: LevelData, K: LevelData, S: Sequence[LevelData]) -> None:
    """S_i += ((2/3) psi^6) D_i K on the valid cells, K's ghost layer 1 read as
    stored (k_cttk_source)."""
    cttk_call("mgic_cttk_source", psi.grid.comm.handle, psi.handle, K.handle, _handles(S))


def correct_constraints(K: LevelData, fields) -> None:
    """Ham += (2/3) K^2, Ham_abs += |(2/3) K^2|, Mom_i -= (2/3) D_i K on the
    five fields of a constraints.ConstraintFields (k_cttk_constraints)."""
    cttk_call("mgic_cttk_constraints", K.grid.comm.handle, K.handle, fields.ham.handle,
              _handles([fields.mom1, fields.mom2, fields.mom3]), fields.ham_abs.handle)


def cttk_launch_ledger() -> dict:
    """{kernel: launches so far in this process} of libmgic_cttk.so."""
    import tempfile

    from .core import read_launch_ledger
    fd, path = tempfile.mkstemp(prefix="mgic_cttk_ledger_")
    os.close(fd)
    try:
        cttk_call("mgic_cttk_launch_ledger_dump", path.encode())
        return read_launch_ledger(path)
    finally:
        os.unlink(path)


def resolve_cttk(tol, max_iterations, prm):
    """cttk_solve's tol and max_iterations: None -- the deck's cttk_tolerance
    and cttk_max_iterations; a tolerance that is not positive or a count
    below 1 is a ValueError."""
    tol = getattr(prm, "cttk_tolerance", 1e-10) if tol is None else tol
    if max_iterations is None:
        max_iterations = getattr(prm, "cttk_max_iterations", 50)
    if not (isinstance(tol, (int, float)) and tol > 0.0):
        raise ValueError(f"cttk: tol must be a positive number, got {tol!r}")
    if not (isinstance(max_iterations, int) and max_iterations >= 1):
        raise ValueError(f"cttk: max_iterations must be an integer >= 1, got {max_iterations!r}")
    return float(tol), int(max_iterations)


def check_cttk_request(grid, prm, matter, psi) -> Grid:
    """The refusals of cttk_solve, raised before anything is loaded or
    launched; returns the one grid."""
    grids = list(grid) if isinstance(grid, (list, tuple)) else [grid]
    if not prm.is_periodic:
        raise ValueError("cttk_solve needs a periodic deck (is_periodic = 1): an asymptotically "
                         "flat one is not supported")
    if len(grids) != 1:
        raise ValueError("cttk_solve needs one level: K under a coarse-fine boundary is not "
                         "supported, so hierarchies are refused")
    table = getattr(prm, "punctures", None)
    rows = [list(r) for r in table] if table is not None else [
        [prm.bh1_bare_mass, prm.bh1_momentum, prm.bh1_spin],
        [prm.bh2_bare_mass, prm.bh2_momentum, prm.bh2_spin]]
    for i, r in enumerate(rows):
        vals = [r[0]] + list(r[4:10]) if table is not None else r
        if any(float(v) != 0.0 for v in vals):
            raise ValueError(f"cttk_solve needs a deck without holes: puncture {i + 1} has a "
                             "non-zero mass, momentum or spin")
    g = grids[0]
    if g is not None and not all(g.periodic):
        raise ValueError("grid periodicity must match params is_periodic")
    if psi is not None:
        if not isinstance(psi, LevelData):
            raise ValueError("cttk_solve: psi must be a LevelData on the grid, or None (psi = 1)")
        pg = psi.grid
        if g is None or not (pg is g or (pg.domain == g.domain and pg.boxes == g.boxes and
                                         pg.dx == g.dx and pg.periodic == g.periodic
                                         and pg.comm is g.comm)):
            raise ValueError("cttk_solve: the layout of psi is not the grid's")
    from .momentum import check_momentum_request
    check_momentum_request(resolve_matter(matter, prm, "cttk_solve"), True, "cttk_solve",
                           zero_mode="project", num_levels=1)
    return g


def cttk_solve(grid, prm: PoissonParameters, matter=None, phi0=None,
               psi: Optional[LevelData] = None, tol: Optional[float] = 1e-10,
               max_iterations: Optional[int] = 50, constraints: bool = False,
               output_dir: Optional[str] = None, max_depth: int = -1, bottom_solver: int = 1,
               prolong_type: int = 1) -> CTTKResult:
    """The CTTK data of a periodic one-level deck without holes (the module's
    docstring).

    matter: None -- the deck's; it needs a Pi_0 (MatterArgumentError), as the
    momentum solve does.  phi0: as poisson_solve's.  psi: None -- psi = 1;
    else a LevelData on the grid, kept as it is but for its ghost layer, which
    is exchanged (the wrapped values).  tol, max_iterations: the loop's
    criterion and the momentum passes it may take (None: the deck's
    cttk_tolerance, cttk_max_iterations).  constraints: the corrected report
    is attached (with the net-subtracted norms, as poisson_solve's).
    output_dir: vcPoissonFinal.3d.hdf5 is written there, component "K" from
    the field and, with `constraints`, components 27-30 from the corrected
    fields.  max_depth, bottom_solver, prolong_type: the momentum solves', as
    poisson_solve's."""
    tol, max_iterations = resolve_cttk(tol, max_iterations, prm)
    grid = check_cttk_request(grid, prm, matter, psi)
    # nothing above loads or launches anything
    from . import momentum as mom
    from .constraints import constraints as constraint_report
    mat = fill_matter(matter, [grid], prm, "cttk_solve")
    phis = resolve_phi0(phi0, [grid], prm)
    phi = phis[0] if phis is not None else None
    if psi is None:
        psi = LevelData(grid)
        psi.set_val_all(1.0)
    else:
        psi.exchange()
    bh = prm.bh(constant_K=0.0)
    avg = prm.coefficient_average_type if prm.coefficient_average_type >= 0 else 0
    op_params = OperatorParams(alpha=prm.alpha, beta=prm.beta, bc_lo=tuple(prm.bc_lo),
                               bc_hi=tuple(prm.bc_hi), bc_value=prm.bc_value,
                               coefficient_average_type=avg, prolong_type=prolong_type,
                               relax_mode=1)
    depth = prm.preCondSolverDepth if prm.preCondSolverDepth >= 0 else max_depth
    mf = mom.MomentumFields([grid])
    ms = mom.MomentumSolver([grid], prm, op_params, SolverParams(
        max_depth=depth, n_pre=prm.numMGsmooth, n_post=prm.numMGsmooth,
        n_bottom=prm.numMGsmooth, bottom_solver=bottom_solver,
        agglomerate_below=32 if grid.comm.size > 1 else 0), "project")
    K, K_prev, integrand = LevelData(grid), LevelData(grid), LevelData(grid)
    for f in (K, K_prev, integrand):
        f.set_zero()
    res = CTTKResult(psi=psi, K=K, momentum=mf)
    op = ms.ops[0]

    def evaluate_K(p: int) -> None:
        mom.set_nl_integrand_ctt(psi, integrand, bh, mat.potential, mf.lw(0), mat.level(0), None,
                                 phi)
        bad = set_K(integrand, K)
        if bad > 0:
            raise CTTKError(bad, p)
        K.exchange()
        res.k_max = op.norm(K, 0)

    def source_term(level: int, S) -> None:
        add_source(psi, K, S)

    for p in range(max_iterations + 1):
        if p > 0:
            K.copy_to(K_prev)
        evaluate_K(p)
        if p > 0:
            op.axby(integrand, K, K_prev, 1.0, -1.0)  # K - K_prev, into the free field
            step = op.norm(integrand, 0)
            res.k_steps.append(step)
            if step <= tol * res.k_max:
                res.converged = True
                break
        if p == max_iterations:
            break
        res.momentum_iterations.append(
            mom.solve_vector_potential(ms, mf, [psi], bh, mat, None, phis, add_source=source_term))
        mom.set_longitudinal(ms, mf)
        res.momentum_residuals.append(list(ms.final_norms))
        ms.final_norms.clear()
        net = ms.removed[:3]
        ms.removed.clear()
        res.momentum_net.append(net)
        res.momentum_net_relative.append([m / s if s != 0.0 else 0.0
                                          for m, s in zip(net, ms.source_max)])
        res.iterations += 1
    res.k_mean = ms.mean(K)
    rep = None
    if constraints:
        rep = res.constraints = constraint_report(
            psi, bh, phis, None, mat, momentum=mf,
            momentum_net=res.momentum_net[-1] if res.momentum_net else None,
            correct=lambda level, fields: correct_constraints(K, fields))
    if output_dir is not None:
        write_final_data(os.path.join(output_dir, "vcPoissonFinal.3d.hdf5"), psi, K, bh, mat, mf,
                         phis, rep.fields[0] if rep is not None else None, prm.max_level)
    return res


def write_final_data(filename: Optional[str], psi: LevelData, K: LevelData, bh: dict, mat,
                     momentum, phi=None, constraint_fields=None, max_level: int = 0) -> None:
    """The final data of one level with K from the field
    (mgic_io_write_final_data_cttk): what output_final_data(momentum=) writes
    at constant_K = 0, component "K" from K and, with constraint_fields (the
    corrected ConstraintFields), components 27-30 from them."""
    from ._lib import io_call
    from .output import _bh
    hs = _handles
    io_call("mgic_io_write_final_data_cttk", filename.encode() if filename is not None else None,
            1, hs([psi]), hs(phi) if phi is not None else None, _bh(bh), 0, None,
            hs(mat.pi) if mat.pi is not None else None, mat.potential.pot(), hs(momentum.lw(0)),
            hs([K]), hs(constraint_fields.fields()) if constraint_fields is not None else None,
            int(max_level), (ctypes.c_int * 1)(2))
