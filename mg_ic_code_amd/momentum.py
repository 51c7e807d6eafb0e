"""The momentum constraint, solved: the conformal transverse-traceless step.

With a non-zero Pi_0 and a varying phi_0 the Bowen-York data violate the
momentum constraint by 8 pi G Pi d_i phi (constraints.py reports it).  This
module removes the violation the way GRChombo's initial-data tools do: a
longitudinal piece is added to the Bowen-York tensor,

    Abar_ij = Abar^BY_ij + LW_ij
    LW_ij   = D_i W_j + D_j W_i - (2/3) delta_ij D_k W_k
    W_i     = V_i + D_i U

(flat conformal metric, constant K; D_d f = 0.5/dx*(f(+e_d) - f(-e_d)), the
project's centred difference), chosen so that D_j Abar_ij cancels the matter
current.  V_i and U come from four constant-coefficient Poisson solves,

    Lap V_i = S_i,   S_i = -(D_j Abar^BY_ij + 8 pi G psi_0^6 Pi D_i phi_0)
    Lap U   = -(1/4) D_k V_k

with the solver the NL loop uses for dpsi: the multigrid-preconditioned
BiCGStab on one level, AMRSolver over all levels on a hierarchy, the deck's
beta and boundary conditions, the alpha aCoef term zero and bCoef = 1.  The
operator is alpha aCoef - beta bCoef Lap, here -beta Lap, so each right-hand
side is scaled by -beta (the deck's beta = -1: by 1, and not at all).  S_i is
-psi_0^6 times the Mom_i of the Bowen-York-only data, so it removes the
truncation divergence of the analytic tensor too.  Pi enters with the sign
the caller stored, as in constraints.py.

Ghost layer 1.  V_i and U take the operator's homogeneous Dirichlet ghost
across a domain face, as dpsi does.  W_i and LW_ij are exchanged between
boxes, interpolated from the coarser level under a coarse-fine boundary
(AMRSolver.cf_interp), and across a domain face extrapolated linearly from
the two cells inside: g = 2 f(face cell) - f(next cell in).  Only face ghosts
are filled: no consumer reads an edge or a corner.

The four stencils between the solves (the right-hand side of U, W, LW and
the extrapolation) are the kernels of libmgic_ctt.so (include/mgic_ctt.h),
loaded on first use; the consumers of LW_ij are the *_ctt entry points of
libmgic.so.

    MomentumFields(grids)          V[3], U, W[3], LW[6] per level
    momentum_source(...)           S_i of one level
    solve_vector_potential(...)    steps 2-3 of an NL iteration: V_i, then U
    set_longitudinal(...)          steps 4-5: W_i, its ghosts, LW_ij, its ghosts
    fill_ghosts(...)               the ghost rule of W_i and LW_ij
    MomentumSolver                 the operators of the four solves, built once

`poisson_solve(..., momentum=True)` runs them inside the NL loop; periodic
bases are refused (the singular alpha = 0 problem needs sum S_i = 0, which a
varying psi_0 does not give).
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

from ._lib import call, ctt_call
from .core import (AMRMultiGrid, AMRSolver, BH_KEYS, BiCGStabSolver, Grid, LevelData,
                   MultilevelLinearOp, OperatorParams, SolverParams, defineOperatorFactory)
from .matter import FilledMatter, MatterArgumentError, ScalarPotential, _pot, table_or_null

# the order of the six stored components, as the A_ij of the output
LW_COMPONENTS = ("11", "12", "13", "22", "23", "33")


def _bh(bh: dict):
    return (ctypes.c_double * 13)(*[float(bh[k]) for k in BH_KEYS])


def _h(f: Optional[LevelData]):
    return f.handle if f is not None else None


def handles(fields: Sequence[LevelData]):
    """const mgic_field * over `fields`."""
    return (ctypes.c_void_p * len(fields))(*[f.handle.value for f in fields])


class MomentumFields:
    """The fields of the momentum solve on a hierarchy (one level: a list of
    one Grid): V[l][3], U[l], W[l][3] and LW[l][6] (LW_COMPONENTS order), all
    zero until solved for."""

    def __init__(self, grids: Sequence[Grid]):
        self.grids = list(grids)
        self.V = [[LevelData(g) for _ in range(3)] for g in self.grids]
        self.U = [LevelData(g) for g in self.grids]
        self.W = [[LevelData(g) for _ in range(3)] for g in self.grids]
        self.LW = [[LevelData(g) for _ in range(6)] for g in self.grids]
        for l in range(len(self.grids)):
            for f in self.V[l] + [self.U[l]] + self.W[l] + self.LW[l]:
                f.set_zero()

    @property
    def num_levels(self) -> int:
        return len(self.grids)

    def lw(self, level: int = 0) -> List[LevelData]:
        """The six LW_ij of one level: the `abar` of the *_ctt entry points."""
        return self.LW[level]


def check_momentum_request(mat, periodic: bool, func: str = "poisson_solve") -> None:
    """The refusals of momentum=True, raised before anything is launched:
    no matter, a matter without a Pi_0, a periodic base."""
    if mat is None:
        raise MatterArgumentError(func, "momentum=True needs matter: the source of the momentum "
                                  "constraint is the scalar field's Pi d_i phi")
    if getattr(mat, "pi", None) is None:
        raise MatterArgumentError(func, "momentum=True needs a matter with a Pi_0: with Pi = 0 "
                                  "the momentum constraint has no source to solve for")
    if periodic:
        raise ValueError("momentum=True on a periodic base is not supported: the singular "
                         "alpha = 0 problem Lap V_i = S_i needs sum S_i = 0 over the domain, "
                         "which a varying psi_0 does not give")


def momentum_source(psi: LevelData, out: Sequence[LevelData], bh: dict,
                    potential: ScalarPotential, pi: Optional[LevelData] = None, punctures=None,
                    phi: Optional[LevelData] = None) -> None:
    """S_i = -(D_j Abar^BY_ij + psi_0^6 * 8 pi G Pi D_i phi_0) of one level on the
    valid cells of out[0..2].  pi None: Pi = 0; punctures None: the deck's two
    holes; phi None: the analytic Gaussian."""
    call("mgic_field_momentum_source", psi.handle, _h(phi), out[0].handle, out[1].handle,
         out[2].handle, _bh(bh), *table_or_null(punctures), _h(pi), _pot(potential).pot())


def div_rhs(comm, v: Sequence[LevelData], out: LevelData) -> None:
    """out = -0.25 * (D_x V_x + D_y V_y + D_z V_z) (k_ctt_div_rhs)."""
    ctt_call("mgic_ctt_div_rhs", comm.handle, handles(v), out.handle)


def set_w(comm, v: Sequence[LevelData], u: LevelData, w: Sequence[LevelData]) -> None:
    """W_i = V_i + D_i U on the valid cells (k_ctt_w)."""
    ctt_call("mgic_ctt_w", comm.handle, handles(v), u.handle, handles(w))


def set_lw(comm, w: Sequence[LevelData], lw: Sequence[LevelData]) -> None:
    """The six LW_ij on the valid cells from W with its ghost layer (k_ctt_lw)."""
    ctt_call("mgic_ctt_lw", comm.handle, handles(w), handles(lw))


def extrapolate(comm, f: LevelData) -> None:
    """Ghost layer 1 of f across the domain faces by linear extrapolation
    (k_ctt_extrap); faces only."""
    ctt_call("mgic_ctt_extrap", comm.handle, f.handle)


def ctt_launch_ledger() -> dict:
    """{kernel: launches so far in this process} of libmgic_ctt.so, as
    core.launch_ledger gives libmgic.so's."""
    import os
    import tempfile

    from .core import read_launch_ledger
    fd, path = tempfile.mkstemp(prefix="mgic_ctt_ledger_")
    os.close(fd)
    try:
        ctt_call("mgic_ctt_launch_ledger_dump", path.encode())
        return read_launch_ledger(path)
    finally:
        os.unlink(path)


def fill_ghosts(fields, amr: Optional[AMRSolver] = None) -> None:
    """Ghost layer 1 of W_i or LW_ij.  fields[l]: the LevelData of level l with
    that component (coarsest first; one level: a list of one).  Per level:
    interpolated from the coarser level under a coarse-fine boundary
    (amr.cf_interp, levels > 0), exchanged between boxes, and linearly
    extrapolated across the domain faces."""
    for l, f in enumerate(fields):
        if l > 0:
            amr.cf_interp(l, f, fields[l - 1])
        f.exchange()
        extrapolate(f.grid.comm, f)


class MomentumSolver:
    """The operators of the four solves: -beta Lap with the deck's boundary
    conditions (aCoef = 0, bCoef = 1), the NL loop's multigrid and BiCGStab
    settings.  Nothing in them depends on psi, so they are built once."""

    def __init__(self, grids: Sequence[Grid], prm, op_params: OperatorParams, sp: SolverParams):
        self.grids = list(grids)
        self.prm = prm
        self.rhs_scale = -float(op_params.beta)
        self.a = [LevelData(g) for g in self.grids]
        self.b = [LevelData(g) for g in self.grids]
        self.rhs = [[LevelData(g) for _ in range(3)] for g in self.grids]
        for l in range(len(self.grids)):
            self.a[l].set_zero()
            self.b[l].set_val(1.0)
        if len(self.grids) == 1:
            self.amr = None
            fac = defineOperatorFactory(self.grids[0], self.a[0], self.b[0], op_params)
            self.amg = AMRMultiGrid(fac, sp)
            mlop = MultilevelLinearOp(self.amg, prm.numMGIterations)
            self.ops = [self.amg.op(0)]
        else:
            self.amr = AMRSolver(list(zip(self.grids, self.a, self.b)), op_params, sp)
            mlop = MultilevelLinearOp(self.amr, prm.numMGIterations)
            self.ops = [self.amr.level_op(l) for l in range(len(self.grids))]
        self.solver = BiCGStabSolver(mlop, tolerance=prm.tolerance,
                                     max_iterations=prm.max_iterations, norm_type=0)

    def _max_norm(self, rhs: List[LevelData]) -> float:
        if self.amr is None:
            return self.ops[0].norm(rhs[0], 0)
        return self.amr.norm(rhs, 0)

    def solve(self, x: List[LevelData], rhs: List[LevelData]) -> int:
        """Lap x = rhs over the hierarchy (x, rhs: one LevelData per level; rhs
        is scaled by -beta in place), x the initial guess; then x's ghost layer
        is filled as dpsi's is (coarse-fine interpolation, exchange, the
        homogeneous boundary condition).  Returns the BiCGStab iterations; a
        right-hand side of zeros has the solution zero and takes none."""
        if self._max_norm(rhs) == 0.0:
            for f in x:
                f.set_zero()
            return 0
        if self.rhs_scale != 1.0:
            for l, f in enumerate(rhs):
                self.ops[l].scale(f, self.rhs_scale)
        if self.amr is None:
            its = self.solver.solve(x[0], rhs[0])
        else:
            its = self.solver.solve(x, rhs)
        for l, f in enumerate(x):
            if l > 0:
                self.amr.cf_interp(l, f, x[l - 1])
            f.exchange()
            self.ops[l].fillBC(f, True)
        return its


def solve_vector_potential(ms: MomentumSolver, mf: MomentumFields, psi: Sequence[LevelData],
                           bh: dict, mat: FilledMatter, punctures=None,
                           phi: Optional[Sequence[LevelData]] = None) -> List[int]:
    """Steps 2-3 of an NL iteration with `momentum` on: S_i from the current
    psi and the three solves for V_i, then the right-hand side of U from V
    with its ghosts and the solve for U.  V_i and U are the initial guesses
    and keep their values between calls.  Returns the four iteration counts."""
    nlev = len(ms.grids)
    comm = ms.grids[0].comm
    for l in range(nlev):
        momentum_source(psi[l], ms.rhs[l], bh, mat.potential, mat.level(l), punctures,
                        phi[l] if phi is not None else None)
    its = []
    for i in range(3):
        its.append(ms.solve([mf.V[l][i] for l in range(nlev)],
                            [ms.rhs[l][i] for l in range(nlev)]))
    for l in range(nlev):
        div_rhs(comm, mf.V[l], ms.rhs[l][0])
    its.append(ms.solve(mf.U, [ms.rhs[l][0] for l in range(nlev)]))
    return its


def set_longitudinal(ms: MomentumSolver, mf: MomentumFields) -> None:
    """Steps 4-5: W_i on the valid cells and its ghost layer, then the six
    LW_ij on the valid cells and their ghost layer (read by the constraints)."""
    nlev = len(ms.grids)
    comm = ms.grids[0].comm
    for l in range(nlev):
        set_w(comm, mf.V[l], mf.U[l], mf.W[l])
    for i in range(3):
        fill_ghosts([mf.W[l][i] for l in range(nlev)], ms.amr)
    for l in range(nlev):
        set_lw(comm, mf.W[l], mf.LW[l])
    for c in range(6):
        fill_ghosts([mf.LW[l][c] for l in range(nlev)], ms.amr)


def set_nl_coefs_ctt(psi: Optional[LevelData], acoef: LevelData, rhs: LevelData, bh: dict,
                     potential: ScalarPotential, abar: Sequence[LevelData],
                     pi: Optional[LevelData] = None, punctures=None,
                     phi: Optional[LevelData] = None) -> None:
    """matter.set_nl_coefs_matter with A2 of the total tensor Abar^BY + abar."""
    call("mgic_field_nl_coefs_ctt", _h(psi), _h(phi), acoef.handle, rhs.handle, _bh(bh),
         *table_or_null(punctures), _h(pi), _pot(potential).pot(), handles(abar))


def set_nl_integrand_ctt(psi: Optional[LevelData], out: LevelData, bh: dict,
                         potential: ScalarPotential, abar: Sequence[LevelData],
                         pi: Optional[LevelData] = None, punctures=None,
                         phi: Optional[LevelData] = None) -> None:
    """matter.set_nl_integrand_matter with A2 of the total tensor."""
    call("mgic_field_nl_integrand_ctt", _h(psi), _h(phi), out.handle, _bh(bh),
         *table_or_null(punctures), _h(pi), _pot(potential).pot(), handles(abar))
