"""The nonlinear solve of Main_PoissonSolver.cpp on one AMR level, on device.

`poisson_solve` mirrors `poissonSolve` (Main_PoissonSolver.cpp:51-250) for
max_level = 0:

    psi = 1, dpsi = 0                     set_initial_conditions (SetLevelData.cpp:31-72)
    for NL_iter < max_NL_iterations:      :129-220
        aCoef, rhs from psi               set_a_coef / set_rhs (:155-161)
        bCoef = 1                         set_b_coef
        factory, MG, BiCGStab             defineOperatorFactory, mlOp, solver (:163-178)
        solver.solve(dpsi, rhs)           :184 (dpsi keeps its value between NL iterations)
        psi += dpsi                       set_update_psi0 (:188-207)
        stop if |dpsi| < tolerance or > 1e5   computeNorm (:210-217)

On a periodic domain each NL iteration first sets K from the integrability
condition: K = -sqrt(|sum(integrand) dV| / volume), with the integrand of
set_constant_K_integrand (:133-147); with the momentum solve on such a
domain (zero_mode="project", momentum.py) its step comes first and the
integrand is the total tensor's.  Every field stays in HBM, and each step
is a libmgic kernel.  With output_dir set, the reference's HDF5 files are
written as it writes them: output_solver_data before every solve (:181) and
output_final_data after the loop (:229), through libmgic_io (output.py).
After the loop the reference stops with MayDay::Error when the final |dpsi|
is above 1e-1 (:221-225), before output_final_data: `poisson_solve` raises
NLDivergenceError at the same point, so a diverged solve writes no
checkpoint.

max_level > 0 (`grid` a list of Grids, coarsest first, finer ones
Grid(patches=True) properly nested -- what grids.set_grids generates from the
reference's tagging, or any hierarchy the caller gives): every step runs per
level as the reference's loops over ilev do -- coefficients on every level
(:154-160),
the outer BiCGStab over MultilevelLinearOp with AMR V-cycles as its
preconditioner (:169-184; AMRSolver), then per level QuadCFInterp of dpsi
from the coarser level before set_update_psi0 (:189-205), and computeNorm /
computeSum over the hierarchy with covered cells masked (:144-145, :208).
With reflux (the keyword, or the deck's reflux = 1) every AMRSolver of the
solve adds the reflux term at the coarse-fine faces: the
composite operator is then conservative, and a periodic hierarchy takes the
projected momentum solve.

With hybrid_K (the keyword, or the deck's hybrid_K = 1; khyb.py)
a deck that is not periodic is solved by the hybrid CTTK method: K(x) is set
from the matter's energy once before the loop, every iteration's momentum step
carries (2/3) psi^6 D_i K in its source, and the coefficients see no matter.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import ctypes
import math
import os

from .core import (AMRMultiGrid, AMRSolver, BiCGStabSolver, Grid, LevelData, MultilevelLinearOp,
                   OperatorParams, SolverParams, defineOperatorFactory, set_nl_coefs, BH_KEYS)
from ._lib import call
from . import horizon as _horizon
from . import khyb as _khyb
from . import sample as _sample
from .adm import adm_charges, check_base, check_hierarchy, parse_half_widths, resolve_table
from .constraints import constraints as constraint_report
from .output import output_final_data, output_solver_data
from .matter import fill_matter, resolve_matter, set_nl_coefs_matter, set_nl_integrand_matter
from .momentum import (MomentumFields, MomentumSolver, check_momentum_request, resolve_reflux,
                       resolve_zero_mode, set_longitudinal, set_nl_coefs_ctt, set_nl_integrand_ctt,
                       solve_vector_potential)
from .params import PoissonParameters
from .phi import PhiProfile, resolve_phi0, set_nl_coefs_phi, set_nl_integrand_phi
from .punctures import resolve_punctures, set_nl_coefs_punct, set_nl_integrand_punct


# Main_PoissonSolver.cpp:221-225: "a fairly generous threshold"
NL_DIVERGENCE_THRESHOLD = 1e-1


class NLDivergenceError(RuntimeError):
    """MayDay::Error("NL iterations did not converge - may need a better initial
    guess") of Main_PoissonSolver.cpp:223-224.  Carries the loop's result."""

    def __init__(self, result: "NLResult"):
        super().__init__("NL iterations did not converge - may need a better initial guess "
                         f"(final |dpsi| = {result.dpsi_norms[-1]!r})")
        self.result = result


@dataclass
class NLResult:
    psi: object   # LevelData, or one per AMR level (max_level > 0)
    dpsi: object
    dpsi_norms: List[float] = field(default_factory=list)
    linear_iterations: List[int] = field(default_factory=list)
    converged: bool = False
    constant_K: List[float] = field(default_factory=list)
    constraints: object = None  # constraints.ConstraintReport (poisson_solve(constraints=True))
    # poisson_solve(momentum=True): the momentum.MomentumFields of the solve (V,
    # U, W, LW per level), and per NL iteration the BiCGStab iterations of its
    # four solves (V_x, V_y, V_z, U)
    momentum: object = None
    momentum_iterations: List[List[int]] = field(default_factory=list)
    # zero_mode="project" on a periodic base: per NL iteration the three means
    # removed from S_i (the net momentum density the torus cannot carry, before
    # the -beta scaling), and each divided by that iteration's max|S_i|
    momentum_net: List[List[float]] = field(default_factory=list)
    momentum_net_relative: List[List[float]] = field(default_factory=list)
    # per NL iteration and momentum solve (V_x, V_y, V_z, U): (final residual
    # max norm of the BiCGStab, max|rhs| as it took it); (0.0, 0.0) where the
    # right-hand side was all zero
    momentum_residuals: List[List[tuple]] = field(default_factory=list)
    # poisson_solve(adm=[n_R, ...]): the adm.AdmReport of the returned psi (and
    # of the total tensor, with momentum=True)
    adm: object = None
    # poisson_solve(puncture_masses=True): the sample.PunctureMassReport of the
    # returned psi (psi at every puncture and the ADM mass it gives)
    puncture_masses: object = None
    # poisson_solve(horizons=...): one horizon.HorizonResult per requested
    # surface, found on the returned psi (and the total tensor, with momentum=True)
    horizons: object = None
    # poisson_solve(hybrid_K=True): the K(x) of the hybrid CTTK method (khyb.py)
    # with its ghost layer 1 filled, a LevelData or one per AMR level, and max|K|
    K: object = None
    k_max: float = 0.0


def set_nl_integrand(psi: LevelData, out: LevelData, bh: dict) -> None:
    """set_constant_K_integrand (SetLevelData.cpp:131-180) on device."""
    vals = (ctypes.c_double * 13)(*[float(bh[k]) for k in BH_KEYS])
    call("mgic_field_nl_integrand", psi.handle, out.handle, vals)


def _coefs(psi, phi, a, rhs, bh, punct=None, mat=None, lev=0, mom=None) -> None:
    """set_a_coef + set_rhs: analytic phi_0 (phi None) or the stored field; the
    deck's two holes (punct None) or the puncture table; no matter (mat None:
    today's calls) or the filled matter's potential and its Pi_0 of level lev;
    mom (with matter): A2 of the total tensor, the momentum fields' LW_ij of
    level lev added to the Bowen-York one.  mat is what m reads, which need not
    be the matter of the momentum source: the hybrid CTTK solve hands over a
    zero potential without a Pi_0 (khyb.HybridK.no_matter)."""
    if mom is not None:
        set_nl_coefs_ctt(psi, a, rhs, bh, mat.potential, mom.lw(lev), mat.level(lev), punct, phi)
    elif mat is not None:
        set_nl_coefs_matter(psi, a, rhs, bh, mat.potential, mat.level(lev), punct, phi)
    elif punct is not None:
        set_nl_coefs_punct(psi, a, rhs, bh, punct, phi=phi)
    elif phi is None:
        set_nl_coefs(psi, a, rhs, bh)
    else:
        set_nl_coefs_phi(psi, phi, a, rhs, bh)


def _integrand(psi, phi, out, bh, punct=None, mat=None, lev=0, mom=None) -> None:
    if mom is not None:
        set_nl_integrand_ctt(psi, out, bh, mat.potential, mom.lw(lev), mat.level(lev), punct, phi)
    elif mat is not None:
        set_nl_integrand_matter(psi, out, bh, mat.potential, mat.level(lev), punct, phi)
    elif punct is not None:
        set_nl_integrand_punct(psi, out, bh, punct, phi=phi)
    elif phi is None:
        set_nl_integrand(psi, out, bh)
    else:
        set_nl_integrand_phi(psi, phi, out, bh)


def poisson_solve(grid, prm: PoissonParameters, max_depth: int = -1,
                  prolong_type: int = 1, bottom_solver: int = 1,
                  max_NL_iterations: Optional[int] = None,
                  output_dir: Optional[str] = None, phi0=None, punctures=None,
                  matter=None, constraints: bool = False,
                  momentum: Optional[bool] = None,
                  zero_mode: Optional[str] = None, reflux=None, adm=None,
                  puncture_masses: Optional[bool] = None, horizons=None,
                  hybrid_K: Optional[bool] = None) -> NLResult:
    """phi0: None -- the analytic Gaussian, evaluated in the kernels; else a
    phi.PhiProfile, or one pre-filled LevelData per level: phi_0 is stored once
    before the NL loop (set_initial_conditions, SetLevelData.cpp:32-71) and the
    stored-field generators and writers are used throughout.
    punctures: None -- the deck's table (prm.punctures) if it has one, else
    the deck's two holes through today's entry points; else a
    punctures.PunctureSet: the table generators and writers are used
    throughout.
    matter: None -- the deck's (prm.matter) if it has one, else no matter
    (rho = 0, today's calls); else a matter.Matter: rho = 0.5 Pi^2 + V(phi_0)
    enters m in the coefficients and the K integrand, Pi_0 is stored once
    before the NL loop, and the final data carry it as "Pi".
    constraints: True -- the Hamiltonian and momentum constraints of the
    returned psi (constraints.py), with the solve's own sources and its last K,
    are attached as NLResult.constraints, and the final data carry them in
    components 27-30.  The solve itself is unchanged.
    momentum: True -- the momentum constraint is solved for the matter's
    Pi d_i phi source (momentum.py): every NL iteration solves for V_i and U,
    forms the longitudinal piece LW_ij, and takes A2 from the total tensor
    Abar^BY_ij + LW_ij; the fields are attached as NLResult.momentum, and the
    constraint report and the final data carry the total tensor.  It needs a
    matter with a Pi_0 (MatterArgumentError otherwise) and a base that is not
    periodic (ValueError) unless zero_mode says otherwise.  None: the deck's
    solve_momentum; False: nothing of it is loaded or launched.
    zero_mode: "refuse" -- momentum=True on a periodic base is a ValueError;
    "project" -- on a periodic one-level base the momentum solve removes the
    mean of each of its four right-hand sides and solutions (momentum.py), the
    means removed from S_i are NLResult.momentum_net, and each NL iteration
    runs the momentum step first so that K comes from the total tensor; a
    periodic hierarchy is refused (ValueError) unless reflux is on, and on a
    base that is not periodic it changes nothing.  None: the deck's
    momentum_zero_mode; any other value is a ValueError.
    reflux: True -- every AMRSolver the solve builds (the Hamiltonian solve,
    the momentum solves, the geometry-only ones) adds the reflux term at the
    coarse-fine faces, and the projection of the momentum solve
    on a periodic hierarchy is the composite one (momentum.py); on one level
    it changes nothing and loads nothing.  None: the deck's reflux (0 when
    absent); anything but True / False / 1 / 0 is a ValueError.
    adm: half-widths [n_R, ...] in level-0 cells -- the ADM mass, momentum and
    spin of the returned psi on those cubes (adm.py; of the total tensor with
    momentum=True) are attached as NLResult.adm.  The solve itself and the
    output files are unchanged.  A periodic base, and any surface adm_charges
    would refuse, is a ValueError before anything is stored or launched.
    None: the deck's adm_half_widths; absent there too: nothing of it is
    loaded or launched.
    puncture_masses: True -- psi at every puncture of the table (the deck's two
    holes as a table without one) and the ADM mass it gives (sample.py) are
    attached as NLResult.puncture_masses, taken from the returned psi on the
    finest level that holds each puncture.  The solve itself and the output
    files are unchanged.  Two punctures at one position are a ValueError before
    anything is stored or launched.  None: the deck's puncture_masses; absent
    or 0 there: nothing of it is loaded or launched.
    horizons: a list of (cx, cy, cz, r0), or "punctures" (one surface per
    puncture of the table, centred on it, r0 = m_i) -- the apparent horizon
    about each centre, from the sphere of radius r0 (horizon.py), is looked for
    on the returned psi (and the total tensor, with momentum=True) and attached
    as NLResult.horizons, one HorizonResult per surface, found or not.  The
    solve itself and the output files are unchanged.  A periodic deck and a bad
    centre or radius are a ValueError before anything is stored or launched.
    None: the deck's horizons; absent there too: nothing of it is loaded or
    launched.
    hybrid_K: True -- the hybrid CTTK method (khyb.py): K varies
    in space, K = -sqrt(24 pi G (Pi_0^2/2 + V(phi_0))), so that the matter's
    energy drops out of the psi equation, and every NL iteration's momentum
    step carries (2/3) psi^6 D_i K in its source.  phi_0 is stored (phi0 None:
    the deck's Gaussian as PhiProfile.gaussian() stores it), K is evaluated
    once before the loop (HybridKError where rho < 0) and attached as
    NLResult.K with NLResult.k_max; the constraint report and the final data
    carry K's terms and K itself.  It implies momentum=True and needs what that
    needs (MatterArgumentError otherwise); a periodic deck (cttk_solve is that
    path), an explicit momentum=False, and adm or horizons (both assume
    K = 0) are a ValueError before anything is stored, loaded or launched.
    None: the deck's hybrid_K; absent or 0 there: nothing of it is loaded or
    launched."""
    hybrid_K = _khyb.resolve_hybrid_K(hybrid_K, prm)
    if hybrid_K:  # refused before anything is stored, loaded or launched
        _khyb.check_hybrid_request(
            prm, resolve_matter(matter, prm), momentum,
            adm if adm is not None else getattr(prm, "adm_half_widths", None),
            horizons if horizons is not None else getattr(prm, "horizons", None))
        momentum = True
        if phi0 is None:
            phi0 = PhiProfile.gaussian()
    if horizons is None:
        horizons = getattr(prm, "horizons", None)
    if horizons is not None:  # refused before anything is stored or launched
        _horizon.check_not_periodic(prm, "poisson_solve")
        horizons = _horizon.resolve_horizons(horizons, resolve_table(punctures, prm),
                                             "poisson_solve")
    if puncture_masses is None:
        puncture_masses = bool(getattr(prm, "puncture_masses", 0))
    if puncture_masses:  # refused before anything is stored or launched
        _sample.check_distinct(resolve_table(punctures, prm), "poisson_solve")
    if adm is None:
        adm = getattr(prm, "adm_half_widths", None)
    if adm is not None:  # refused before anything is stored or launched
        adm = parse_half_widths(adm, "poisson_solve")
        glist = list(grid) if isinstance(grid, (list, tuple)) else [grid]
        if prm.is_periodic:
            raise ValueError("adm: the charges are not defined on a periodic domain")
        check_base(glist[0].domain, glist[0].periodic, adm, "poisson_solve")
        check_hierarchy(glist, adm, "poisson_solve")
    punct = resolve_punctures(punctures, prm)
    zero_mode = resolve_zero_mode(zero_mode, prm)
    reflux = resolve_reflux(reflux, prm)
    if momentum is None:
        momentum = bool(getattr(prm, "solve_momentum", 0))
    if momentum:  # refused before anything is stored or launched
        nlev = len(grid) if isinstance(grid, (list, tuple)) else 1
        check_momentum_request(resolve_matter(matter, prm), bool(prm.is_periodic),
                               zero_mode=zero_mode, num_levels=nlev, reflux=reflux)
    if isinstance(grid, (list, tuple)):
        if len(grid) > 1:
            return _poisson_solve_amr(list(grid), prm, max_depth, prolong_type, bottom_solver,
                                      max_NL_iterations, output_dir, phi0, punct, matter,
                                      constraints, momentum, zero_mode, reflux, adm,
                                      bool(puncture_masses), horizons, hybrid_K)
        grid = grid[0]
    mat = fill_matter(matter, [grid], prm)
    phis = resolve_phi0(phi0, [grid], prm)
    phi = phis[0] if phis is not None else None
    periodic = bool(prm.is_periodic)
    if periodic != all(grid.periodic):
        raise ValueError("grid periodicity must match params is_periodic")
    psi, dpsi = LevelData(grid), LevelData(grid)
    a, b, rhs = LevelData(grid), LevelData(grid), LevelData(grid)
    psi.set_val_all(1.0)
    dpsi.set_zero()
    b.set_val(1.0)  # set_b_coef (SetLevelData.cpp:330-340)
    bh = prm.bh(constant_K=0.0)
    avg = prm.coefficient_average_type if prm.coefficient_average_type >= 0 else 0
    op_params = OperatorParams(alpha=prm.alpha, beta=prm.beta, bc_lo=tuple(prm.bc_lo),
                               bc_hi=tuple(prm.bc_hi), bc_value=prm.bc_value,
                               coefficient_average_type=avg, prolong_type=prolong_type,
                               relax_mode=1)
    depth = prm.preCondSolverDepth if prm.preCondSolverDepth >= 0 else max_depth
    res = NLResult(psi=psi, dpsi=dpsi)
    mom = msolve = None
    if momentum:
        mom = res.momentum = MomentumFields([grid])
        msolve = MomentumSolver([grid], prm, op_params, SolverParams(
            max_depth=depth, n_pre=prm.numMGsmooth, n_post=prm.numMGsmooth,
            n_bottom=prm.numMGsmooth, bottom_solver=bottom_solver,
            agglomerate_below=32 if grid.comm.size > 1 else 0), zero_mode)
    hyb = extra = None
    coef_mat = mat
    if hybrid_K:  # K does not depend on psi: once, before the loop
        hyb = _khyb.HybridK([grid], mat, phis, prm.G_Newton)
        res.K, res.k_max = hyb.K[0], msolve.ops[0].norm(hyb.K[0], 0)
        extra, coef_mat = hyb.source([psi]), hyb.no_matter
    n_nl = prm.max_NL_iterations if max_NL_iterations is None else max_NL_iterations
    dx = grid.dx
    ones = integrand = None
    volume = prm.domainLength[0] * prm.domainLength[1] * prm.domainLength[2]
    for it in range(n_nl):
        if momentum and periodic:
            # the momentum step first, so that K below comes from the total
            # tensor.  S_i does not depend on K: mgic_field_momentum_source
            # (bh_constraints with `source`) reads constant_K for Ham alone,
            # which it does not write, so the order leaves S_i as it was
            _momentum_step(res, msolve, mom, [psi], bh, mat, punct, phis)
        if periodic:  # integrability condition for K (:133-147)
            if integrand is None:
                integrand, ones = LevelData(grid), LevelData(grid)
                ones.set_val(1.0)
            bh["constant_K"] = 0.0
            _integrand(psi, phi, integrand, bh, punct, mat, 0, mom)
            tmp_op = defineOperatorFactory(grid, a, b, op_params).AMRnewOp()
            integral = tmp_op.dotProduct(integrand, ones) * dx ** 3  # computeSum
            bh["constant_K"] = -math.sqrt(abs(integral) / volume)
            res.constant_K.append(bh["constant_K"])
        if momentum and not periodic:
            _momentum_step(res, msolve, mom, [psi], bh, mat, punct, phis, extra)
        _coefs(psi, phi, a, rhs, bh, punct, coef_mat, 0, mom)  # :155-161
        fac = defineOperatorFactory(grid, a, b, op_params)
        # N > 1: depths whose boxes are below 32 cells a side are gathered to
        # one box on rank 0 (the coarsest levels solved on rank 0)
        amg = AMRMultiGrid(fac, SolverParams(max_depth=depth, n_pre=prm.numMGsmooth,
                                             n_post=prm.numMGsmooth, n_bottom=prm.numMGsmooth,
                                             bottom_solver=bottom_solver,
                                             agglomerate_below=32 if grid.comm.size > 1 else 0))
        solver = BiCGStabSolver(MultilevelLinearOp(amg, prm.numMGIterations),
                                tolerance=prm.tolerance, max_iterations=prm.max_iterations,
                                norm_type=0)
        if output_dir is not None:  # :180-181
            output_solver_data([dpsi], [rhs], [psi], bh, it, [2],
                               os.path.join(output_dir, f"vcPoissonOut.3d_{it}.hdf5"), phi=phis,
                               punctures=punct)
        res.linear_iterations.append(solver.solve(dpsi, rhs))
        op0 = amg.op(0)
        op0.update_psi(psi, dpsi)
        # computeNorm (L2 over the level, dV = dx^3)
        nrm = op0.norm(dpsi, 2) * dx ** 1.5
        res.dpsi_norms.append(nrm)
        if nrm < prm.tolerance or nrm > 1e5:
            res.converged = nrm < prm.tolerance
            break
    write = None
    if output_dir is not None and hyb is None:  # :227-230
        def write():
            output_final_data([psi], bh, prm.max_level, [2],
                              os.path.join(output_dir, "vcPoissonFinal.3d.hdf5"), phi=phis,
                              punctures=punct, matter=mat, constraints=constraints, momentum=mom)
    finish_nl_loop(res, write)
    if hyb is not None:
        _finish_hybrid(res, hyb, [psi], bh, phis, punct, mat, mom, constraints, output_dir,
                       prm.max_level, [2])
    elif constraints:
        res.constraints = constraint_report(
            psi, bh, phis, punct, mat, momentum=mom,
            momentum_net=res.momentum_net[-1] if res.momentum_net else None)
    if adm is not None:
        res.adm = adm_charges(psi, prm, adm, punctures=punct, momentum=mom)
    if puncture_masses:
        res.puncture_masses = _sample.puncture_masses(psi, prm, punctures=punct)
    if horizons is not None:
        res.horizons = _horizon.horizons_of(psi, prm, horizons, punctures=punct, momentum=mom)
    return res


def _finish_hybrid(res: NLResult, hyb, psi, bh, phis, punct, mat, mom, constraints: bool,
                   output_dir: Optional[str], max_level: int, refs, reflux: bool = False) -> None:
    """After a hybrid CTTK loop that did not diverge: the constraint report
    with K's terms (bh["constant_K"] stays 0), then the final data with K from
    the field and, with the report, components 27-30 from its corrected
    fields."""
    rep = None
    if constraints:
        rep = res.constraints = constraint_report(
            psi if len(psi) > 1 else psi[0], bh, phis, punct, mat, momentum=mom, reflux=reflux,
            correct=hyb.correct)
    if output_dir is not None:
        _khyb.write_final_data(os.path.join(output_dir, "vcPoissonFinal.3d.hdf5"), psi, hyb.K, bh,
                               mat, mom, phis, punct, rep.fields if rep is not None else None,
                               max_level, refs)


def _momentum_step(res: NLResult, msolve, mom, psi, bh, mat, punct, phis, add_source=None) -> None:
    """V_i and U at the current psi (one LevelData per level), then LW_ij of the
    total tensor; with the zero mode projected, the means removed from S_i.
    add_source: solve_vector_potential's."""
    res.momentum_iterations.append(
        solve_vector_potential(msolve, mom, psi, bh, mat, punct, phis, add_source=add_source))
    set_longitudinal(msolve, mom)
    res.momentum_residuals.append(list(msolve.final_norms))
    msolve.final_norms.clear()
    if msolve.project:
        net = msolve.removed[:3]
        msolve.removed.clear()
        res.momentum_net.append(net)
        res.momentum_net_relative.append([m / s if s != 0.0 else 0.0
                                          for m, s in zip(net, msolve.source_max)])


def _op_params(prm: PoissonParameters, prolong_type: int) -> OperatorParams:
    avg = prm.coefficient_average_type if prm.coefficient_average_type >= 0 else 0
    return OperatorParams(alpha=prm.alpha, beta=prm.beta, bc_lo=tuple(prm.bc_lo),
                          bc_hi=tuple(prm.bc_hi), bc_value=prm.bc_value,
                          coefficient_average_type=avg, prolong_type=prolong_type, relax_mode=1)


def _poisson_solve_amr(grids: List[Grid], prm: PoissonParameters, max_depth: int,
                       prolong_type: int, bottom_solver: int, max_NL_iterations: Optional[int],
                       output_dir: Optional[str], phi0=None, punct=None,
                       matter=None, constraints: bool = False,
                       momentum: bool = False, zero_mode: str = "refuse",
                       reflux: bool = False, adm=None,
                       puncture_masses: bool = False, horizons=None,
                       hybrid_K: bool = False) -> NLResult:
    """poissonSolve over nlevels = len(grids) AMR levels (Main_PoissonSolver.cpp:51-250)."""
    periodic = bool(prm.is_periodic)
    if periodic != all(grids[0].periodic):
        raise ValueError("grid periodicity must match params is_periodic")
    nlev = len(grids)
    psi = [LevelData(g) for g in grids]
    dpsi = [LevelData(g) for g in grids]
    a = [LevelData(g) for g in grids]
    b = [LevelData(g) for g in grids]
    rhs = [LevelData(g) for g in grids]
    for l in range(nlev):  # set_initial_conditions / set_b_coef per level (:79-99, :157)
        psi[l].set_val_all(1.0)
        dpsi[l].set_zero()
        b[l].set_val(1.0)
    mat = fill_matter(matter, grids, prm)
    phis = resolve_phi0(phi0, grids, prm)
    phi = phis if phis is not None else [None] * nlev
    bh = prm.bh(constant_K=0.0)
    op_params = _op_params(prm, prolong_type)
    depth = prm.preCondSolverDepth if prm.preCondSolverDepth >= 0 else max_depth
    sp = SolverParams(max_depth=depth, n_pre=prm.numMGsmooth, n_post=prm.numMGsmooth,
                      n_bottom=prm.numMGsmooth, bottom_solver=bottom_solver,
                      agglomerate_below=32 if grids[0].comm.size > 1 else 0)
    res = NLResult(psi=psi, dpsi=dpsi)
    mom = msolve = None
    if momentum:
        mom = res.momentum = MomentumFields(grids)
        msolve = MomentumSolver(grids, prm, op_params, sp, zero_mode, reflux=reflux)
    hyb = extra = None
    coef_mat = mat
    if hybrid_K:  # K does not depend on psi: once, before the loop
        hyb = _khyb.HybridK(grids, mat, phis, prm.G_Newton, msolve.amr)
        res.K, res.k_max = hyb.K, msolve.amr.norm(hyb.K, 0)
        extra, coef_mat = hyb.source(psi), hyb.no_matter
    n_nl = prm.max_NL_iterations if max_NL_iterations is None else max_NL_iterations
    volume = prm.domainLength[0] * prm.domainLength[1] * prm.domainLength[2]
    integrand = geom = None
    refs = [2] * nlev
    for it in range(n_nl):
        if momentum and periodic:
            # the momentum step first, so that K below comes from the total
            # tensor (as on one level: S_i does not depend on K)
            _momentum_step(res, msolve, mom, psi, bh, mat, punct, phis)
        if periodic:  # integrability condition for K over the hierarchy (:137-150)
            if integrand is None:
                integrand = [LevelData(g) for g in grids]
                # computeSum only needs the hierarchy's geometry
                geom = AMRSolver(list(zip(grids, a, b)), op_params, sp, reflux=reflux)
            bh["constant_K"] = 0.0
            for l in range(nlev):
                _integrand(psi[l], phi[l], integrand[l], bh, punct, mat, l, mom)
            integral = geom.computeSum(integrand)
            bh["constant_K"] = -math.sqrt(abs(integral) / volume)
            res.constant_K.append(bh["constant_K"])
        if momentum and not periodic:  # V_i and U at the current psi, then LW_ij
            res.momentum_iterations.append(
                solve_vector_potential(msolve, mom, psi, bh, mat, punct, phis, add_source=extra))
            set_longitudinal(msolve, mom)
        for l in range(nlev):  # :154-160
            _coefs(psi[l], phi[l], a[l], rhs[l], bh, punct, coef_mat, l, mom)
        amr = AMRSolver(list(zip(grids, a, b)), op_params, sp, reflux=reflux)  # :163-170
        solver = BiCGStabSolver(MultilevelLinearOp(amr, prm.numMGIterations),
                                tolerance=prm.tolerance, max_iterations=prm.max_iterations,
                                norm_type=0)
        if output_dir is not None:  # :180-181
            output_solver_data(dpsi, rhs, psi, bh, it, refs,
                               os.path.join(output_dir, f"vcPoissonOut.3d_{it}.hdf5"), phi=phis,
                               punctures=punct)
        res.linear_iterations.append(solver.solve(dpsi, rhs))  # :184
        for l in range(nlev):  # :189-205
            if l > 0:
                amr.cf_interp(l, dpsi[l], dpsi[l - 1])  # QuadCFInterp::coarseFineInterp
            amr.level_op(l).update_psi(psi[l], dpsi[l])
        nrm = amr.computeNorm(dpsi, 2)  # :208-209
        res.dpsi_norms.append(nrm)
        if nrm < prm.tolerance or nrm > 1e5:
            res.converged = nrm < prm.tolerance
            break
    write = None
    if output_dir is not None and hyb is None:  # :227-230
        def write():
            output_final_data(psi, bh, nlev - 1, refs,
                              os.path.join(output_dir, "vcPoissonFinal.3d.hdf5"), phi=phis,
                              punctures=punct, matter=mat, constraints=constraints, momentum=mom)
    finish_nl_loop(res, write)
    if hyb is not None:
        _finish_hybrid(res, hyb, psi, bh, phis, punct, mat, mom, constraints, output_dir,
                       nlev - 1, refs, reflux)
    elif constraints:
        res.constraints = constraint_report(
            psi, bh, phis, punct, mat, momentum=mom,
            momentum_net=res.momentum_net[-1] if res.momentum_net else None, reflux=reflux)
    if adm is not None:
        res.adm = adm_charges(psi, prm, adm, punctures=punct, momentum=mom)
    if puncture_masses:
        res.puncture_masses = _sample.puncture_masses(psi, prm, punctures=punct)
    if horizons is not None:
        res.horizons = _horizon.horizons_of(psi, prm, horizons, punctures=punct, momentum=mom)
    return res


def finish_nl_loop(res: NLResult, write_final=None) -> NLResult:
    """The end of poissonSolve (Main_PoissonSolver.cpp:218-230): raise when the
    final |dpsi| exceeds 1e-1 (MayDay::Error, :221-225) -- before anything is
    written -- else write the final data (`write_final`, :229) and return.
    The comparison is the reference's `dpsi_norm > 1e-1`, so a NaN norm passes
    it as it does there."""
    if res.dpsi_norms and res.dpsi_norms[-1] > NL_DIVERGENCE_THRESHOLD:
        raise NLDivergenceError(res)
    if write_final is not None:
        write_final()
    return res
