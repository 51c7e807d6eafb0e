"""Bowen-York punctures as a table: any position, momentum and spin.

The reference's set_binary_bh_Aij / set_binary_bh_psi (SetBinaryBH.H:55-99)
place two holes on the x axis, with momentum along y and spin along z; its
get_Aij (:24-53) is written for full vectors.  A `PunctureSet` hands the
generators 1 to 8 punctures, each a `Puncture(mass, position, momentum,
spin)`, positions relative to the domain centre (the coordinates of
bh1_offset).

The table is taken in pairs, in table order: (0, 1), (2, 3), ...  One pair
contributes what get_Aij gives for two holes with these vectors, and
psi_bh = m_a / r_a + m_b / r_b; A_ij_0 and psi_bh are the sums over the
pairs, in pair order.  An odd count is completed by a puncture with
m = P = J = 0 at the last puncture's position.  Punctures get no periodic
images.  `PunctureSet.from_params(prm)` is the deck's two holes as a table:
with it every table generator gives the bits of today's entry points.

`punctures=` of poisson_solve, set_grids and the output functions takes a
PunctureSet (or a list of Punctures, or rows of ten numbers); None: today's
calls.  It composes with the stored phi_0 (phi.py).
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Iterable, Optional, Sequence, Tuple

import numpy as np

from ._lib import MgicError, call
from .core import BH_KEYS, LevelData

MAX_PUNCTURES = 8  # MGIC_MAX_PUNCTURES (include/mgic.h)
ROW = ("m", "x", "y", "z", "Px", "Py", "Pz", "Jx", "Jy", "Jz")


class PunctureArgumentError(MgicError, ValueError):
    """A punctures argument refused before anything is launched: the library's
    bad-argument status (MGIC_EBADARG), raised on the host."""

    def __init__(self, func: str, msg: str):
        MgicError.__init__(self, func, -1, msg)


def _vec3(func: str, name: str, v) -> Tuple[float, float, float]:
    try:
        t = tuple(float(c) for c in v)
    except (TypeError, ValueError):
        t = ()
    if len(t) != 3:
        raise PunctureArgumentError(func, f"{name} must be three numbers, not {v!r}")
    return t


@dataclass(frozen=True)
class Puncture:
    """One Bowen-York puncture: bare mass, position relative to the domain
    centre, linear momentum and spin."""
    mass: float
    position: Tuple[float, float, float]
    momentum: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    spin: Tuple[float, float, float] = (0.0, 0.0, 0.0)

    def __post_init__(self):
        try:
            m = float(self.mass)
        except (TypeError, ValueError):
            raise PunctureArgumentError("Puncture", f"mass must be a number, not {self.mass!r}")
        object.__setattr__(self, "mass", m)
        for name in ("position", "momentum", "spin"):
            object.__setattr__(self, name, _vec3("Puncture", name, getattr(self, name)))
        if not all(math.isfinite(v) for v in self.row()):
            raise PunctureArgumentError("Puncture", f"non-finite entry in {self.row()}")

    def row(self) -> Tuple[float, ...]:
        """m, x, y, z, Px, Py, Pz, Jx, Jy, Jz"""
        return (self.mass,) + self.position + self.momentum + self.spin

    @classmethod
    def from_row(cls, row: Sequence[float]) -> "Puncture":
        try:
            r = [float(v) for v in row]
        except (TypeError, ValueError):
            r = []
        if len(r) != len(ROW):
            raise PunctureArgumentError(
                "Puncture", f"a puncture is ten numbers ({' '.join(ROW)}), not {row!r}")
        return cls(r[0], tuple(r[1:4]), tuple(r[4:7]), tuple(r[7:10]))


class PunctureSet(list):
    """1 to MAX_PUNCTURES punctures, in table order."""

    def __init__(self, punctures: Iterable = ()):
        super().__init__(p if isinstance(p, Puncture) else Puncture.from_row(p)
                         for p in punctures)

    @classmethod
    def from_params(cls, prm) -> "PunctureSet":
        """The deck's two holes (prm: PoissonParameters, or the bh dict of
        BH_KEYS): on the x axis, momentum along y, spin along z."""
        bh = prm if isinstance(prm, dict) else prm.bh()
        return cls(Puncture(bh[f"bh{i}_bare_mass"], (bh[f"bh{i}_offset"], 0.0, 0.0),
                            (0.0, bh[f"bh{i}_momentum"], 0.0), (0.0, 0.0, bh[f"bh{i}_spin"]))
                   for i in (1, 2))

    def table(self) -> np.ndarray:
        """The flat float64 array of 10 n values the C ABI takes."""
        if not 1 <= len(self) <= MAX_PUNCTURES:
            raise PunctureArgumentError(
                "PunctureSet", f"puncture count {len(self)} outside 1..{MAX_PUNCTURES}")
        if not all(isinstance(p, Puncture) for p in self):
            raise PunctureArgumentError("PunctureSet", "every entry must be a Puncture")
        return np.array([p.row() for p in self], dtype=np.float64).ravel()

    def __repr__(self) -> str:
        return f"PunctureSet({list.__repr__(self)})"


def resolve_punctures(punctures, prm=None) -> Optional[PunctureSet]:
    """A `punctures=` argument as a checked PunctureSet: the caller's, else
    the deck's table (prm.punctures), else None (the deck's two holes through
    today's entry points)."""
    if punctures is None and prm is not None and not isinstance(prm, dict):
        punctures = getattr(prm, "punctures", None)
    if punctures is None:
        return None
    ps = punctures if isinstance(punctures, PunctureSet) else PunctureSet(punctures)
    ps.table()
    return ps


def _bh(bh: dict):
    return (ctypes.c_double * 13)(*[float(bh[k]) for k in BH_KEYS])


def table_args(punctures):
    """(count, const double *) for a *_punct entry point."""
    t = resolve_punctures(punctures).table()
    return len(t) // len(ROW), (ctypes.c_double * len(t))(*t)


def _h(f: Optional[LevelData]):
    return f.handle if f is not None else None


def set_nl_coefs_punct(psi: Optional[LevelData], acoef: LevelData, rhs: LevelData, bh: dict,
                       punctures, phi: Optional[LevelData] = None) -> None:
    """set_a_coef + set_rhs (SetLevelData.cpp:73-127, :281-325) with the holes of
    the table; phi: the stored phi_0 (None: the analytic Gaussian)."""
    call("mgic_field_nl_coefs_punct", _h(psi), _h(phi), acoef.handle, rhs.handle, _bh(bh),
         *table_args(punctures))


def set_nl_integrand_punct(psi: Optional[LevelData], out: LevelData, bh: dict, punctures,
                           phi: Optional[LevelData] = None) -> None:
    """set_constant_K_integrand (SetLevelData.cpp:131-180) with the holes of the table."""
    call("mgic_field_nl_integrand_punct", _h(psi), _h(phi), out.handle, _bh(bh),
         *table_args(punctures))


def set_regrid_condition_punct(psi: Optional[LevelData], out: LevelData, bh: dict, punctures,
                               phi: Optional[LevelData] = None) -> None:
    """set_regrid_condition (SetLevelData.cpp:190-240) with the holes of the table."""
    call("mgic_field_regrid_condition_punct", _h(psi), _h(phi), out.handle, _bh(bh),
         *table_args(punctures))
