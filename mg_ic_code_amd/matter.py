"""The scalar field's kinetic and potential energy in the sources.

The reference's set_m_value (SetLevelData.cpp:266-278) reads

    Real Pi_field = 0.0;  Real V_of_phi = 0.0;
    Real rho = 0.5 * Pi_field * Pi_field + V_of_phi;
    m = (2.0 / 3.0) * (constant_K * constant_K) - 16.0 * M_PI * G_Newton * rho;

with a note that V(phi) and Pi may be added later.  A `Matter` fills that
slot, and nothing else changes:

    V(phi) = V0 + 0.5 * mass * mass * phi * phi
                + 0.25 * self_coupling * phi * phi * phi * phi    (left to right)
    rho    = 0.5 * Pi * Pi + V(phi_0)

phi_0 is the cell's scalar field (the stored phi_0 where one is given, else
the analytic Gaussian) and Pi the cell's value of the stored field Pi_0: one
value per cell, like phi_0, but never differenced, so only valid cells are
read.  m keeps the reference's place in every expression, which fixes the psi
weighting of rho: K is constant_K in the coefficients and 0 in the
integrability integrand and the regrid condition (where 1.5 |m| is no longer
zero).

    ScalarPotential(V0=0, mass=0, self_coupling=0)
    PiProfile.constant(v)            LevelData.set_val_all(v)
    PiProfile.from_function(f)       the caller's f(x, y, z) over the cell centres,
                                     exactly as PhiProfile.from_function
    Matter(potential, pi=None)       pi: None (Pi = 0), a PiProfile, or one
                                     filled LevelData per level

`matter=` of poisson_solve, set_grids, output_final_data and grchombo_vars
takes a Matter; None: the deck's (scalar_V0, scalar_mass,
scalar_self_coupling, pi_amplitude), else today's calls.  With a zero
potential and a zero Pi_0 every generator gives today's bits.

Only Pi * Pi enters, so the sign of Pi (GRChombo's Pi is "(minus) conjugate
momentum") is the caller's convention; the final data carry Pi_0 as given in
component 26.  The solver-data file (the reference's multigrid_vars) has no Pi.

The momentum constraint: with a non-zero Pi_0 and a varying phi_0 the
Bowen-York data violate it by 8 pi G Pi d_i phi.  constraints.py
(`constraints`, `poisson_solve(..., constraints=True)`) reports Ham and Mom_i
of the data per cell and their norms, and momentum.py
(`poisson_solve(..., momentum=True)`) removes the violation by the conformal
transverse-traceless step; in both the sign of Pi does enter.  Without that
switch the violation stays, as before.
Not done here: no potential beyond this polynomial; no periodic images.
Convergence is not guaranteed for large potentials: with constant K the
operator's aCoef becomes indefinite when V(phi(x)) - <V> outweighs the
gradient energy.  `poisson_solve(..., hybrid_K=True)` (khyb.py,
DESIGN.md 3r) is the way round it on a deck that is not periodic: K(x) chosen
so that rho drops out of m.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Union

import numpy as np

from ._lib import MgicError, call
from .core import BH_KEYS, Grid, LevelData, box_shape
from .punctures import resolve_punctures


class MatterArgumentError(MgicError, TypeError):
    """A matter argument of the wrong kind or value, refused before anything
    is launched: the library's bad-argument status (MGIC_EBADARG), raised on
    the host."""

    def __init__(self, func: str, msg: str):
        MgicError.__init__(self, func, -1, msg)


def _bh(bh: dict):
    return (ctypes.c_double * 13)(*[float(bh[k]) for k in BH_KEYS])


def _prm_bh(prm) -> dict:
    return prm if isinstance(prm, dict) else prm.bh(constant_K=0.0)


@dataclass(frozen=True)
class ScalarPotential:
    """V(phi) = V0 + 0.5 mass^2 phi^2 + 0.25 self_coupling phi^4."""
    V0: float = 0.0
    mass: float = 0.0
    self_coupling: float = 0.0

    def __post_init__(self):
        for name in ("V0", "mass", "self_coupling"):
            try:
                v = float(getattr(self, name))
            except (TypeError, ValueError):
                raise MatterArgumentError(
                    "ScalarPotential", f"{name} must be a number, not {getattr(self, name)!r}")
            if not math.isfinite(v):
                raise MatterArgumentError("ScalarPotential", f"{name} is not finite: {v!r}")
            object.__setattr__(self, name, v)

    def pot(self):
        """const double pot[3] of the C ABI: V0, mass, lambda."""
        return (ctypes.c_double * 3)(self.V0, self.mass, self.self_coupling)


class PiProfile:
    """A profile of Pi_0: a constant, or a host function of the cell-centre
    coordinates."""

    def __init__(self, value: Optional[float] = None, function: Optional[Callable] = None):
        if function is not None:
            if not callable(function):
                raise TypeError("PiProfile.from_function needs a callable f(x, y, z)")
            self.kind, self.value = "function", None
        else:
            try:
                v = float(value)
            except (TypeError, ValueError):
                raise MatterArgumentError("PiProfile", f"a constant Pi must be a number, not {value!r}")
            if not math.isfinite(v):
                raise MatterArgumentError("PiProfile", f"Pi is not finite: {v!r}")
            self.kind, self.value = "constant", v
        self.function = function

    @classmethod
    def constant(cls, v: float) -> "PiProfile":
        return cls(value=v)

    @classmethod
    def from_function(cls, f: Callable) -> "PiProfile":
        """f(x, y, z) -> ndarray, called with broadcastable float64 arrays of
        cell-centre coordinates (shapes (1, 1, nx), (1, ny, 1), (nz, 1, 1))."""
        return cls(function=f)

    def __repr__(self) -> str:
        return f"PiProfile({self.kind if self.function else self.value!r})"

    def fill(self, grid: Grid, prm) -> LevelData:
        """Pi_0 on `grid` (prm: PoissonParameters, or the bh dict of BH_KEYS)."""
        pi = LevelData(grid)
        if self.function is None:
            pi.set_val_all(self.value)
            return pi
        bh = _prm_bh(prm)
        L, dx = float(bh["domain_length"]), grid.dx
        for n in range(grid.num_local):
            b = grid.local_box(n)
            shape = box_shape(b, 1)
            # bh_loc: ((double)iv + 0.5) * dx - L / 2.0, over the box grown by one
            ax = [(np.arange(b[d] - 1, b[3 + d] + 2, dtype=np.float64) + 0.5) * dx - L / 2.0
                  for d in range(3)]
            v = self.function(ax[0].reshape(1, 1, -1), ax[1].reshape(1, -1, 1),
                              ax[2].reshape(-1, 1, 1))
            v = np.broadcast_to(np.asarray(v, dtype=np.float64), shape)
            pi.upload(n, np.ascontiguousarray(v), with_ghosts=True)
        return pi


PiArg = Union[PiProfile, LevelData, Sequence[LevelData], None]


@dataclass
class FilledMatter:
    """A Matter on a hierarchy: the potential and Pi_0 per level (None: Pi = 0)."""
    potential: ScalarPotential
    pi: Optional[List[LevelData]] = None

    def level(self, l: int) -> Optional[LevelData]:
        return self.pi[l] if self.pi is not None else None


class Matter:
    """The potential and the field's velocity Pi_0 (None: Pi = 0; a PiProfile;
    or one pre-filled LevelData per level)."""

    def __init__(self, potential: Optional[ScalarPotential] = None, pi: PiArg = None):
        potential = ScalarPotential() if potential is None else potential
        if not isinstance(potential, ScalarPotential):
            raise MatterArgumentError("Matter", "potential must be a ScalarPotential, not "
                                      f"{type(potential).__name__}")
        self.potential = potential
        self.pi = pi

    @classmethod
    def from_params(cls, prm) -> Optional["Matter"]:
        """The deck's matter (scalar_V0, scalar_mass, scalar_self_coupling,
        pi_amplitude); None when it has none of the keys."""
        d = getattr(prm, "matter", None)
        if d is None:
            return None
        pi = d.get("pi_amplitude")
        return cls(ScalarPotential(d.get("scalar_V0", 0.0), d.get("scalar_mass", 0.0),
                                   d.get("scalar_self_coupling", 0.0)),
                   PiProfile.constant(pi) if pi is not None else None)

    def __repr__(self) -> str:
        return f"Matter({self.potential!r}, pi={self.pi!r})"

    def fill(self, grids: Sequence[Grid], prm, func: str = "Matter.fill") -> FilledMatter:
        """Pi_0 stored on every level of `grids`."""
        grids = list(grids)
        pi = self.pi
        if pi is None:
            return FilledMatter(self.potential, None)
        if isinstance(pi, PiProfile):
            return FilledMatter(self.potential, [pi.fill(g, prm) for g in grids])
        fields = [pi] if isinstance(pi, LevelData) else list(pi)
        if len(fields) != len(grids) or not all(isinstance(f, LevelData) for f in fields):
            raise MatterArgumentError(func, "pi must be a PiProfile or one LevelData per level")
        return FilledMatter(self.potential, fields)


def resolve_matter(matter, prm=None, func: str = "poisson_solve") -> Optional[Matter]:
    """A `matter=` argument: the caller's Matter, else the deck's, else None
    (no matter: today's calls)."""
    if matter is None and prm is not None and not isinstance(prm, dict):
        matter = Matter.from_params(prm)
    if matter is None:
        return None
    if isinstance(matter, ScalarPotential):
        matter = Matter(matter)
    if not isinstance(matter, (Matter, FilledMatter)):
        raise MatterArgumentError(func, "matter must be a Matter (or a ScalarPotential), not "
                                  f"{type(matter).__name__}")
    return matter


def fill_matter(matter, grids: Sequence[Grid], prm, func: str = "poisson_solve"
                ) -> Optional[FilledMatter]:
    """`matter=` resolved and stored on `grids` (None: no matter)."""
    m = resolve_matter(matter, prm, func)
    if m is None or isinstance(m, FilledMatter):
        return m
    return m.fill(grids, prm, func)


def _h(f: Optional[LevelData]):
    return f.handle if f is not None else None


def table_or_null(punctures):
    """(count, const double *) of a *_matter entry point: (0, NULL) is the
    deck's two holes."""
    ps = resolve_punctures(punctures)
    if ps is None:
        return 0, None
    t = ps.table()
    return len(ps), (ctypes.c_double * len(t))(*t)


def _pot(potential) -> ScalarPotential:
    if not isinstance(potential, ScalarPotential):
        raise MatterArgumentError("matter", "potential must be a ScalarPotential, not "
                                  f"{type(potential).__name__}")
    return potential


def set_nl_coefs_matter(psi: Optional[LevelData], acoef: LevelData, rhs: LevelData, bh: dict,
                        potential: ScalarPotential, pi: Optional[LevelData] = None,
                        punctures=None, phi: Optional[LevelData] = None) -> None:
    """set_a_coef + set_rhs (SetLevelData.cpp:73-127, :281-325) with rho from the
    potential and the stored Pi_0 (None: Pi = 0); punctures None: the deck's two
    holes; phi None: the analytic Gaussian."""
    call("mgic_field_nl_coefs_matter", _h(psi), _h(phi), acoef.handle, rhs.handle, _bh(bh),
         *table_or_null(punctures), _h(pi), _pot(potential).pot())


def set_nl_integrand_matter(psi: Optional[LevelData], out: LevelData, bh: dict,
                            potential: ScalarPotential, pi: Optional[LevelData] = None,
                            punctures=None, phi: Optional[LevelData] = None) -> None:
    """set_constant_K_integrand (SetLevelData.cpp:131-180) with rho from the matter."""
    call("mgic_field_nl_integrand_matter", _h(psi), _h(phi), out.handle, _bh(bh),
         *table_or_null(punctures), _h(pi), _pot(potential).pot())


def set_regrid_condition_matter(psi: Optional[LevelData], out: LevelData, bh: dict,
                                potential: ScalarPotential, pi: Optional[LevelData] = None,
                                punctures=None, phi: Optional[LevelData] = None) -> None:
    """set_regrid_condition (SetLevelData.cpp:190-240) with rho from the matter."""
    call("mgic_field_regrid_condition_matter", _h(psi), _h(phi), out.handle, _bh(bh),
         *table_or_null(punctures), _h(pi), _pot(potential).pot())
