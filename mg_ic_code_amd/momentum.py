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

`poisson_solve(..., momentum=True)` runs them inside the NL loop.

Periodic bases.  -beta Lap on a torus is singular: constants are its null
space and a right-hand side is in its range only when it sums to zero, which
a varying psi_0 does not give S_i.  By default such a base is refused.  With
zero_mode="project" (the deck's momentum_zero_mode = project) and one level,
every one of the four solves is projected on both sides,

    m = sum(rhs) / cells,  rhs <- rhs - m      (the system becomes consistent)
    solve
    x <- x - sum(x) / cells                    (the null-space component is fixed)

with the sums the level's own dotProduct(f, ones), the mean formed on the
host in double, and the subtraction k_zm_shift of libmgic_zm.so
(include/mgic_zm.h), loaded on first use.  The removed means of S_i are the
net momentum density the torus cannot carry; they are recorded
(MomentumSolver.removed, NLResult.momentum_net).  The ghosts of every field
across a periodic face come from the exchange; fillBC and the extrapolation
have nothing to do there.  A periodic hierarchy is refused unless the solve
runs with reflux (poisson_solve(..., reflux=True)): without it
the AMR operators do no refluxing, so the composite operator's columns do not
sum to zero and a zero-sum right-hand side is not in its range.  With it the
projection is composite: m = computeSum(f) / computeSum(ones) over the
uncovered cells of every level with dx_l^3 weights, subtracted from the valid
cells of every level (k_zm_shift per level; covered cells are shifted too,
which nothing reads).
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

from ._lib import call, ctt_call, zm_call
from .core import (AMRMultiGrid, AMRSolver, BH_KEYS, BiCGStabSolver, Grid, LevelData,
                   MultilevelLinearOp, OperatorParams, SolverParams, defineOperatorFactory)
from .params import ZERO_MODES
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


def resolve_reflux(reflux, prm) -> bool:
    """poisson_solve's reflux: None -- the deck's reflux (absent: 0); True /
    False / 1 / 0; anything else is a ValueError."""
    if reflux is None:
        reflux = getattr(prm, "reflux", 0)
    if isinstance(reflux, bool) or (isinstance(reflux, int) and reflux in (0, 1)):
        return bool(reflux)
    raise ValueError(f"reflux must be 0 or 1 (False or True), got {reflux!r}")


def resolve_zero_mode(zero_mode: Optional[str], prm) -> str:
    """poisson_solve's zero_mode: None -- the deck's momentum_zero_mode (absent:
    "refuse"); anything but the two accepted values is a ValueError."""
    if zero_mode is None:
        zero_mode = getattr(prm, "momentum_zero_mode", "refuse")
    if zero_mode not in ZERO_MODES:
        raise ValueError(f"zero_mode must be 'refuse' or 'project', got {zero_mode!r}")
    return zero_mode


def check_momentum_request(mat, periodic: bool, func: str = "poisson_solve",
                           zero_mode: str = "refuse", num_levels: int = 1,
                           reflux: bool = False) -> None:
    """The refusals of momentum=True, raised before anything is launched:
    no matter, a matter without a Pi_0, a periodic base without
    zero_mode="project", a periodic hierarchy with it and without reflux."""
    if mat is None:
        raise MatterArgumentError(func, "momentum=True needs matter: the source of the momentum "
                                  "constraint is the scalar field's Pi d_i phi")
    if getattr(mat, "pi", None) is None:
        raise MatterArgumentError(func, "momentum=True needs a matter with a Pi_0: with Pi = 0 "
                                  "the momentum constraint has no source to solve for")
    if periodic and zero_mode != "project":
        raise ValueError("momentum=True on a periodic base is not supported: the singular "
                         "alpha = 0 problem Lap V_i = S_i needs sum S_i = 0 over the domain, "
                         "which a varying psi_0 does not give; zero_mode='project' (the deck's "
                         "momentum_zero_mode = project) removes the mean of S_i and reports it")
    if periodic and num_levels > 1 and not reflux:
        raise ValueError("zero_mode='project' on a periodic hierarchy is not supported: the AMR "
                         "operators do no refluxing, so the composite operator's columns do not "
                         "sum to zero and a zero-sum right-hand side is not in its range; use "
                         "one level")


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


def shift(comm, fields: Sequence[LevelData], consts: Sequence[float]) -> None:
    """fields[i] -= consts[i] on the valid cells of every local box, one or
    three fields in one pass (k_zm_shift<1>, <3>); no ghost cell is written."""
    zm_call("mgic_zm_shift", comm.handle, len(fields), handles(fields),
            (ctypes.c_double * len(fields))(*[float(c) for c in consts]))


def zm_launch_ledger() -> dict:
    """{kernel: launches so far in this process} of libmgic_zm.so."""
    import os
    import tempfile

    from .core import read_launch_ledger
    fd, path = tempfile.mkstemp(prefix="mgic_zm_ledger_")
    os.close(fd)
    try:
        zm_call("mgic_zm_launch_ledger_dump", path.encode())
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
    settings.  Nothing in them depends on psi, so they are built once.
    zero_mode "project" on a periodic base: every solve is projected (the
    module's docstring), and `removed` keeps the mean taken out of each
    right-hand side, in the order of the solves, until the caller clears it.
    On a base that is not periodic zero_mode changes nothing.  reflux: the
    hierarchy's AMRSolver is built with it (one level: no effect); a periodic
    hierarchy is projected only with it."""

    def __init__(self, grids: Sequence[Grid], prm, op_params: OperatorParams, sp: SolverParams,
                 zero_mode: str = "refuse", reflux: bool = False):
        self.grids = list(grids)
        self.prm = prm
        self.project = zero_mode == "project" and all(self.grids[0].periodic)
        if self.project and len(self.grids) > 1 and not reflux:
            raise ValueError("zero_mode='project' needs a one-level base, or reflux")
        self.removed: List[float] = []
        self.source_max: List[float] = []
        # per solve since the caller last cleared it: (the BiCGStab's final
        # residual max norm, max|rhs| as the solve took it); (0.0, 0.0) for the
        # all-zero shortcut
        self.final_norms: List[tuple] = []
        self.ones = None
        if self.project and len(self.grids) == 1:
            d = self.grids[0].domain
            self.cells = (d[3] - d[0] + 1) * (d[4] - d[1] + 1) * (d[5] - d[2] + 1)
            self.ones = LevelData(self.grids[0])
            self.ones.set_val(1.0)
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
            self.amr = AMRSolver(list(zip(self.grids, self.a, self.b)), op_params, sp,
                                 reflux=reflux)
            mlop = MultilevelLinearOp(self.amr, prm.numMGIterations)
            self.ops = [self.amr.level_op(l) for l in range(len(self.grids))]
            if self.project:  # computeSum(ones): the hierarchy's volume
                ones = [LevelData(g) for g in self.grids]
                for f in ones:
                    f.set_val(1.0)
                self.volume = self.amr.computeSum(ones)
        self.solver = BiCGStabSolver(mlop, tolerance=prm.tolerance,
                                     max_iterations=prm.max_iterations, norm_type=0)

    def _max_norm(self, rhs: List[LevelData]) -> float:
        if self.amr is None:
            return self.ops[0].norm(rhs[0], 0)
        return self.amr.norm(rhs, 0)

    def mean(self, f: LevelData) -> float:
        """sum(f) / cells over the periodic level: the level's dotProduct(f,
        ones) (reduced over the ranks), divided on the host."""
        return self.ops[0].dotProduct(f, self.ones) / self.cells

    def remove_means(self, fields: Sequence[LevelData]) -> List[float]:
        """Subtract its mean from each of one or three fields of the level
        (one pass of k_zm_shift); returns the means removed."""
        means = [self.mean(f) for f in fields]
        shift(self.grids[0].comm, fields, means)
        return means

    def _remove(self, xs: Sequence[List[LevelData]]) -> List[float]:
        """Subtract its mean from each of one or three fields over the hierarchy
        (xs[i]: one LevelData per level).  One level: remove_means.  More: the
        composite mean computeSum(f) / computeSum(ones), subtracted from the
        valid cells of every level (one pass of k_zm_shift per level)."""
        if self.amr is None:
            return self.remove_means([x[0] for x in xs])
        means = [self.amr.computeSum(x) / self.volume for x in xs]
        for l, g in enumerate(self.grids):
            shift(g.comm, [x[l] for x in xs], means)
        return means

    def _solve(self, x: List[LevelData], rhs: List[LevelData]) -> int:
        """The all-zero shortcut, the scaling by -beta and the solve."""
        rhs_max = self._max_norm(rhs)
        if rhs_max == 0.0:
            for f in x:
                f.set_zero()
            self.final_norms.append((0.0, 0.0))
            return 0
        if self.rhs_scale != 1.0:
            for l, f in enumerate(rhs):
                self.ops[l].scale(f, self.rhs_scale)
        its = self.solver.solve(x[0], rhs[0]) if self.amr is None else self.solver.solve(x, rhs)
        self.final_norms.append((self.solver.final_norm, abs(self.rhs_scale) * rhs_max))
        return its

    def _fill(self, x: List[LevelData]) -> None:
        for l, f in enumerate(x):
            if l > 0:
                self.amr.cf_interp(l, f, x[l - 1])
            f.exchange()
            self.ops[l].fillBC(f, True)

    def solve(self, x: List[LevelData], rhs: List[LevelData]) -> int:
        """Lap x = rhs over the hierarchy (x, rhs: one LevelData per level; rhs
        is scaled by -beta in place), x the initial guess; then x's ghost layer
        is filled as dpsi's is (coarse-fine interpolation, exchange, the
        homogeneous boundary condition).  Returns the BiCGStab iterations; a
        right-hand side of zeros has the solution zero and takes none.  With
        the projection on, the mean of rhs is removed first (and appended to
        `removed`), and the mean of x after the solve, before its ghosts are
        filled.  The shortcut is looked for after the projection: a field of
        zeros has the mean 0.0, stays as it is and takes it as before, and a
        constant one, which has no solution part either, takes it too."""
        if self.project:
            self.removed.extend(self._remove([rhs]))
        its = self._solve(x, rhs)
        if self.project:
            self._remove([x])
        self._fill(x)
        return its

    def solve_three(self, xs: Sequence[List[LevelData]],
                    rhss: Sequence[List[LevelData]]) -> List[int]:
        """solve for three components.  With the projection on, the three
        right-hand sides lose their means in one pass and the three solutions
        in another (k_zm_shift<3>); `source_max` keeps max|rhs_i| as they came."""
        if not self.project:
            return [self.solve(x, r) for x, r in zip(xs, rhss)]
        self.source_max = [self._max_norm(r) for r in rhss]
        self.removed.extend(self._remove(list(rhss)))
        its = [self._solve(x, r) for x, r in zip(xs, rhss)]
        self._remove(list(xs))
        for x in xs:
            self._fill(x)
        return its


def solve_vector_potential(ms: MomentumSolver, mf: MomentumFields, psi: Sequence[LevelData],
                           bh: dict, mat: FilledMatter, punctures=None,
                           phi: Optional[Sequence[LevelData]] = None,
                           add_source=None) -> List[int]:
    """Steps 2-3 of an NL iteration with `momentum` on: S_i from the current
    psi and the three solves for V_i, then the right-hand side of U from V
    with its ghosts and the solve for U.  V_i and U are the initial guesses
    and keep their values between calls.  Returns the four iteration counts.
    add_source: None, or a callable (level, S) that adds a further term to the
    three S_i of that level on their valid cells, before the scaling by -beta
    and the projection (cttk.py: the (2/3) psi^6 D_i K of a K that varies)."""
    nlev = len(ms.grids)
    comm = ms.grids[0].comm
    for l in range(nlev):
        momentum_source(psi[l], ms.rhs[l], bh, mat.potential, mat.level(l), punctures,
                        phi[l] if phi is not None else None)
        if add_source is not None:
            add_source(l, ms.rhs[l])
    its = ms.solve_three([[mf.V[l][i] for l in range(nlev)] for i in range(3)],
                         [[ms.rhs[l][i] for l in range(nlev)] for i in range(3)])
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
