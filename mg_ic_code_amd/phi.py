"""The scalar field phi_0 as a stored device field (Source/MyPhiFunction.H,
set_initial_conditions, SetLevelData.cpp:32-71).

The reference evaluates `my_phi_function` once on every box grown by its
ghosts and stores the values as the component phi_0; GETRHOGRADPHIF and the
output routines read that component.  A `PhiProfile` does the same here:

    PhiProfile.gaussian()         amplitude exp(-r^2 / wavelength)   (:14-15, "use with
                                  Dirichlet BCs"; the analytic path's profile)
    PhiProfile.sine()             amplitude sum_d sin(2 pi x_d wavelength / L)
                                  (:18-20, "use with periodic BCs")
    PhiProfile.from_function(f)   the caller's f(x, y, z) -> ndarray

`fill(grid, prm)` returns a LevelData holding the profile at every cell
centre of each local box and of the one ghost layer next to it,
loc = (iv + 0.5) dx - L/2 -- also where a ghost cell lies outside the domain
or under a coarse-fine boundary.  The field is never exchanged, BC-filled or
interpolated.  The stored-field generators below read it where the analytic
ones evaluate the Gaussian; filled by `gaussian()` they give the same bits.
"""
from __future__ import annotations

import ctypes
from typing import Callable, List, Optional, Sequence, Union

import numpy as np

from ._lib import MgicError, call
from .core import BH_KEYS, Grid, LevelData, box_shape

GAUSSIAN, SINE = 0, 1  # MGIC_PHI_GAUSSIAN, MGIC_PHI_SINE (include/mgic.h)


def _bh(bh: dict):
    return (ctypes.c_double * 13)(*[float(bh[k]) for k in BH_KEYS])


def _prm_bh(prm) -> dict:
    return prm if isinstance(prm, dict) else prm.bh(constant_K=0.0)


class PhiArgumentError(MgicError, TypeError):
    """A phi0 argument of the wrong kind, refused before anything is launched:
    the library's bad-argument status (MGIC_EBADARG), raised on the host."""

    def __init__(self, func: str, msg: str):
        MgicError.__init__(self, func, -1, msg)


class PhiProfile:
    """A scalar-field profile: a built-in one (evaluated by the fill kernel) or
    a host function of the cell-centre coordinates."""

    def __init__(self, kind: Union[str, int], function: Optional[Callable] = None):
        names = {"gaussian": GAUSSIAN, "sine": SINE}
        if function is not None:
            if not callable(function):
                raise TypeError("PhiProfile.from_function needs a callable f(x, y, z)")
            self.kind, self.profile_id = "function", None
        elif isinstance(kind, str):
            if kind not in names:
                raise ValueError(f"unknown phi profile {kind!r} (gaussian, sine)")
            self.kind, self.profile_id = kind, names[kind]
        else:  # a raw profile id: the library checks it
            self.kind, self.profile_id = f"profile {int(kind)}", int(kind)
        self.function = function

    @classmethod
    def gaussian(cls) -> "PhiProfile":
        return cls("gaussian")

    @classmethod
    def sine(cls) -> "PhiProfile":
        return cls("sine")

    @classmethod
    def from_function(cls, f: Callable) -> "PhiProfile":
        """f(x, y, z) -> ndarray, called with broadcastable float64 arrays of
        cell-centre coordinates (shapes (1, 1, nx), (1, ny, 1), (nz, 1, 1))."""
        return cls("function", f)

    def __repr__(self) -> str:
        return f"PhiProfile({self.kind})"

    def fill(self, grid: Grid, prm) -> LevelData:
        """phi_0 on `grid` (prm: PoissonParameters, or the bh dict of BH_KEYS)."""
        bh = _prm_bh(prm)
        phi = LevelData(grid)
        if self.function is None:
            call("mgic_field_fill_phi", phi.handle, int(self.profile_id), _bh(bh))
            return phi
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
            phi.upload(n, np.ascontiguousarray(v), with_ghosts=True)
        return phi


PhiArg = Union[PhiProfile, LevelData, Sequence[LevelData], None]


def resolve_phi0(phi0: PhiArg, grids: Sequence[Grid], prm) -> Optional[List[LevelData]]:
    """poisson_solve's phi0 argument as one filled LevelData per level (None:
    the analytic path)."""
    if phi0 is None:
        return None
    if isinstance(phi0, PhiProfile):
        return [phi0.fill(g, prm) for g in grids]
    fields = [phi0] if isinstance(phi0, LevelData) else list(phi0)
    if len(fields) != len(grids) or not all(isinstance(f, LevelData) for f in fields):
        raise PhiArgumentError("poisson_solve",
                               "phi0 must be a PhiProfile or one LevelData per level")
    return fields


def _h(f: Optional[LevelData]):
    return f.handle if f is not None else None


def set_nl_coefs_phi(psi: Optional[LevelData], phi: LevelData, acoef: LevelData, rhs: LevelData,
                     bh: dict) -> None:
    """set_a_coef + set_rhs (SetLevelData.cpp:73-127, :281-325) with the stored phi_0."""
    call("mgic_field_nl_coefs_phi", _h(psi), phi.handle, acoef.handle, rhs.handle, _bh(bh))


def set_nl_integrand_phi(psi: Optional[LevelData], phi: LevelData, out: LevelData,
                         bh: dict) -> None:
    """set_constant_K_integrand (SetLevelData.cpp:131-180) with the stored phi_0."""
    call("mgic_field_nl_integrand_phi", _h(psi), phi.handle, out.handle, _bh(bh))


def set_regrid_condition_phi(psi: Optional[LevelData], phi: LevelData, out: LevelData,
                             bh: dict) -> None:
    """set_regrid_condition (SetLevelData.cpp:190-240) with the stored phi_0."""
    call("mgic_field_regrid_condition_phi", _h(psi), phi.handle, out.handle, _bh(bh))
