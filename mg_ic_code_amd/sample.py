"""A field of the AMR hierarchy at points: puncture masses, line-outs, and the
solve for given puncture masses.

Every other kernel of the package works on cells.  libmgic_sample.so
(include/mgic_sample.h) interpolates a field at arbitrary real
positions, each on the finest level that holds it: cubic (4^3 cells), linear
(2^3) or the cell itself, whichever is the first whose cells are all valid
cells of that level not covered by a finer one.  Coordinates are those of the
puncture table and of adm.py: level l's cell centres are at
(iv + 0.5) dx_l - N_d dx_0 / 2.  Only valid cells are read.

    sample_points(fields, points, order=4)        values, levels and orders used
    lineout(fields, a, b, n, order=4)             n points from a to b, with arc length
    puncture_masses(psi, prm, punctures=None)     -> PunctureMassReport
    solve_for_masses(grid, prm, targets, ...)     bare masses for given ADM masses

With psi_0 = psi + sum_n m_n / r_n (geometric units, no factor G, as adm.py)
the ADM mass of puncture i, measured in its own asymptotic end, is

    M_i = 2 m_i (psi(x_i) + sum_{j != i} m_j / |x_i - x_j|)

which is algebraic once psi is known at the puncture.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from ._lib import MgicError, sample_call
from .adm import resolve_table
from .core import LevelData
from .punctures import Puncture, PunctureSet

MAX_LEVELS = 8         # MGIC_SAMPLE_MAX_LEVELS (include/mgic_sample.h)
MAX_POINTS = 1 << 20   # MGIC_SAMPLE_MAX_POINTS
ORDERS = (1, 2, 4)


class SampleArgumentError(MgicError, ValueError):
    """A sampling request refused before anything is launched: the library's
    bad-argument status (MGIC_EBADARG)."""

    def __init__(self, func: str, msg: str):
        MgicError.__init__(self, func, -1, msg)


def cubic_weights(t: float) -> List[float]:
    """The order-4 weights of the nodes -1, 0, 1, 2 at t, in the header's
    expression order (what the kernel evaluates, in float64)."""
    tm1, tm2, tp1 = t - 1.0, t - 2.0, t + 1.0
    return [-t * tm1 * tm2 / 6.0, tp1 * tm1 * tm2 / 2.0, -tp1 * t * tm2 / 2.0,
            tp1 * t * tm1 / 6.0]


def linear_weights(t: float) -> List[float]:
    """The order-2 weights of the nodes 0, 1 at t."""
    return [1.0 - t, t]


@dataclass
class SampleResult:
    """values[p]: the field at point p (NaN where no level holds it);
    level[p]: the level it was taken from (-1: none); order[p]: 4, 2 or 1,
    the stencil that was used (0: none)."""
    values: np.ndarray
    level: np.ndarray
    order: np.ndarray


def _levels(fields) -> List[LevelData]:
    return [fields] if isinstance(fields, LevelData) else list(fields)


def sample_points(fields, points, order: int = 4) -> SampleResult:
    """The field at each of `points` (npts x 3, the puncture table's
    coordinates).  fields: a LevelData, or one per AMR level, coarsest first.
    order: 4, 2 or 1, the stencil tried first; a point too close to a domain
    face that is not periodic, to a coarse-fine boundary or to a level's edge
    takes the next lower one.  A point outside the domain in a direction that
    is not periodic, or with a non-finite coordinate, gives NaN, level -1,
    order 0.  Refusals are a ValueError before anything is launched."""
    func = "sample_points"
    levels = _levels(fields)
    if not 1 <= len(levels) <= MAX_LEVELS:
        raise SampleArgumentError(func, f"level count {len(levels)} outside 1..{MAX_LEVELS}")
    if isinstance(order, bool) or order not in ORDERS:
        raise SampleArgumentError(func, f"order {order!r} is not 1, 2 or 4")
    try:
        xyz = np.ascontiguousarray(points, dtype=np.float64)
    except (TypeError, ValueError):
        raise SampleArgumentError(func, "points must be numbers, npts x 3")
    if xyz.ndim == 1 and xyz.size == 3:
        xyz = xyz.reshape(1, 3)
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise SampleArgumentError(func, f"points must be npts x 3, not {xyz.shape}")
    npts = xyz.shape[0]
    if not 1 <= npts <= MAX_POINTS:
        raise SampleArgumentError(func, f"point count {npts} outside 1..{MAX_POINTS}")
    values = np.empty(npts, dtype=np.float64)
    level = np.empty(npts, dtype=np.int32)
    used = np.empty(npts, dtype=np.int32)
    handles = (ctypes.c_void_p * len(levels))(*[f.handle.value for f in levels])
    PD, PI = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    try:
        sample_call("mgic_sample_points", levels[0].grid.comm.handle, len(levels), handles, npts,
                    xyz.ctypes.data_as(PD), int(order), values.ctypes.data_as(PD),
                    level.ctypes.data_as(PI), used.ctypes.data_as(PI))
    except MgicError as e:
        if e.code == -1:  # MGIC_EBADARG: the package's ValueError
            raise SampleArgumentError(func, str(e)) from None
        raise
    return SampleResult(values, level, used)


@dataclass
class Lineout:
    """n points from a to b inclusive: s[p] the arc length from a, points[p],
    and the sample there (SampleResult's three arrays)."""
    s: np.ndarray
    points: np.ndarray
    values: np.ndarray
    level: np.ndarray
    order: np.ndarray

    def lines(self) -> List[str]:
        """One "lineout s value level order" line per point
        (tools/run_poisson.py --lineout)."""
        return [f"lineout {s:.16e} {v:.16e} {l} {o}"
                for s, v, l, o in zip(self.s, self.values, self.level, self.order)]


def lineout_points(a, b, n: int) -> Tuple[np.ndarray, np.ndarray]:
    """(s, points): point p is a + (b - a) * (p / (n - 1)), s[p] = |b - a| *
    (p / (n - 1)); n = 1 is a alone."""
    try:
        a = np.array([float(v) for v in a])
        b = np.array([float(v) for v in b])
    except (TypeError, ValueError):
        a = b = np.zeros(0)
    if a.shape != (3,) or b.shape != (3,):
        raise SampleArgumentError("lineout", "a and b must be three numbers each")
    if isinstance(n, bool) or int(n) != n or not 1 <= n <= MAX_POINTS:
        raise SampleArgumentError("lineout", f"point count {n!r} outside 1..{MAX_POINTS}")
    n = int(n)
    frac = np.arange(n, dtype=np.float64) / max(n - 1, 1)
    length = math.sqrt(float(np.sum((b - a) * (b - a))))
    return frac * length, a[None, :] + frac[:, None] * (b - a)[None, :]


def lineout(fields, a, b, n: int, order: int = 4) -> Lineout:
    """The field along the segment from a to b at n equally spaced points, both
    ends included."""
    s, pts = lineout_points(a, b, n)
    r = sample_points(fields, pts, order)
    return Lineout(s, pts, r.values, r.level, r.order)


def parse_lineout(value) -> Tuple[Tuple[float, ...], Tuple[float, ...], int]:
    """(a, b, n) from "x0 y0 z0 x1 y1 z1 n" (tools/run_poisson.py --lineout)."""
    items = value.replace(",", " ").split() if isinstance(value, str) else list(value)
    try:
        nums = [float(v) for v in items[:6]]
        n = int(items[6])
        ok = len(items) == 7 and float(items[6]) == n
    except (TypeError, ValueError, IndexError):
        ok = False
    if not ok:
        raise SampleArgumentError("lineout", f"a line-out is \"x0 y0 z0 x1 y1 z1 n\", not {value!r}")
    return tuple(nums[:3]), tuple(nums[3:]), n


# ---------------------------------------------------------------- puncture masses
@dataclass
class PunctureMass:
    """One puncture of the table: u is psi at its position, sampled on `level`
    with the stencil `order`; adm_mass = 2 m (u + sum_{j != i} m_j / d_ij)."""
    bare_mass: float
    position: Tuple[float, float, float]
    u: float
    level: int
    order: int
    adm_mass: float


@dataclass
class PunctureMassReport:
    """One PunctureMass per puncture of the table, in table order."""
    punctures: List[PunctureMass] = field(default_factory=list)

    @property
    def adm_masses(self) -> List[float]:
        return [p.adm_mass for p in self.punctures]

    def lines(self) -> List[str]:
        """One line per puncture (tools/run_poisson.py --puncture-masses)."""
        return [f"puncture mass {i + 1}: m = {p.bare_mass:.16e} at "
                + " ".join(f"{c:.16e}" for c in p.position)
                + f": psi = {p.u:.16e} (level {p.level}, order {p.order}) M = {p.adm_mass:.16e}"
                for i, p in enumerate(self.punctures)]


def check_distinct(punct: Sequence[Puncture], func: str = "puncture_masses") -> None:
    """ValueError for two punctures at the same position (m_j / d_ij)."""
    for i in range(len(punct)):
        for j in range(i):
            if tuple(punct[i].position) == tuple(punct[j].position):
                raise SampleArgumentError(
                    func, f"punctures {j + 1} and {i + 1} are at the same position "
                          f"{tuple(punct[i].position)}")


def adm_masses(punct: Sequence[Puncture], u: Sequence[float]) -> List[float]:
    """M_i = 2 m_i (u_i + sum_{j != i} m_j / d_ij) in float64, the other
    punctures added in table order, d_ij = sqrt((dx dx + dy dy) + dz dz)."""
    out = []
    for i, p in enumerate(punct):
        acc = float(u[i])
        for j, q in enumerate(punct):
            if j == i:
                continue
            d = [p.position[c] - q.position[c] for c in range(3)]
            acc = acc + q.mass / math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        out.append(2.0 * p.mass * acc)
    return out


def mass_report(punct: Sequence[Puncture], u, level, order) -> PunctureMassReport:
    M = adm_masses(punct, u)
    return PunctureMassReport([
        PunctureMass(p.mass, tuple(p.position), float(u[i]), int(level[i]), int(order[i]), M[i])
        for i, p in enumerate(punct)])


def puncture_masses(psi, prm, punctures=None, order: int = 4) -> PunctureMassReport:
    """The ADM mass of every puncture from psi (a LevelData, or one per AMR
    level, coarsest first) sampled at its position.

    prm: the PoissonParameters of the solve (or the bh dict of BH_KEYS).
    punctures None -- the deck's table if it has one, else its two holes, as
    adm.resolve_table resolves them; the puncture that completes an odd table
    inside the kernels is not one of them.  Two punctures at the same position
    are a ValueError before anything is launched.  A puncture outside the
    domain reports NaN on level -1."""
    punct = resolve_table(punctures, prm)
    check_distinct(punct)
    r = sample_points(psi, [p.position for p in punct], order)
    return mass_report(punct, r.values, r.level, r.order)


# ---------------------------------------------------------------- target masses
def parse_masses(value, func: str = "target_masses") -> List[float]:
    """Positive finite masses from a list of numbers or a string of them
    ("1.0 0.7", the deck's target_masses and --target-masses)."""
    items = value.replace(",", " ").split() if isinstance(value, str) else value
    try:
        items = list(items)
    except TypeError:
        items = [items]
    out = []
    for v in items:
        try:
            x = float(v)
            ok = not isinstance(v, bool) and math.isfinite(x) and x > 0.0
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise SampleArgumentError(func, f"a target mass must be a positive number, not {v!r}")
        out.append(x)
    if not out:
        raise SampleArgumentError(func, "no target masses")
    return out


def check_target_count(targets, count: int, func: str = "target_masses") -> None:
    """One target per puncture of the table."""
    if len(targets) != count:
        raise SampleArgumentError(
            func, f"{len(targets)} target masses for a table of {count} punctures")


@dataclass
class MassSolveStep:
    """One solve of the iteration: the bare masses it ran with, the ADM masses
    it gave, and max_i |M_i - T_i|."""
    bare_masses: List[float]
    adm_masses: List[float]
    error: float


@dataclass
class MassSolveResult:
    result: object              # the NLResult of the last solve
    punctures: PunctureSet      # the table of the last solve
    targets: List[float]
    history: List[MassSolveStep] = field(default_factory=list)
    converged: bool = False

    def lines(self) -> List[str]:
        out = [f"mass solve {k + 1}: m = " + " ".join(f"{m:.16e}" for m in h.bare_masses)
               + " M = " + " ".join(f"{m:.16e}" for m in h.adm_masses)
               + f" max|M - T| = {h.error:.3e}" for k, h in enumerate(self.history)]
        out.append(f"mass solve: {'converged' if self.converged else 'not converged'} after "
                   f"{len(self.history)} solves")
        return out


def check_targets(punct: Sequence[Puncture], targets, func: str = "solve_for_masses") -> List[float]:
    """The refusals of solve_for_masses that need the table alone."""
    T = parse_masses(targets, func)
    check_target_count(T, len(punct), func)
    for i, p in enumerate(punct):
        if p.mass == 0.0:
            raise SampleArgumentError(
                func, f"puncture {i + 1} has bare mass 0: no scaling reaches the target {T[i]!r}")
    check_distinct(punct, func)
    return T


def solve_for_masses(grid, prm, targets, punctures=None, rel_tol: float = 1e-8,
                     max_solves: int = 8, **solve_kwargs) -> MassSolveResult:
    """The bare masses that give the ADM masses `targets` (one per puncture of
    the table, in table order): the fixed point m_i <- m_i T_i / M_i, one full
    poisson_solve(grid, prm, **solve_kwargs) per step on the caller's grids,
    starting from the table's bare masses, until max_i |M_i - T_i| <= rel_tol
    max_i T_i.  When max_solves runs out, converged is False (nothing is
    raised).  The result carries the last NLResult, the table it was solved
    with, and the bare and ADM masses of every solve.

    A target count other than the table's, a target that is not positive, a
    puncture of bare mass 0 and two punctures at one position are a ValueError
    before the first solve."""
    from .nl import poisson_solve
    punct = resolve_table(punctures, prm)
    T = check_targets(punct, targets)
    if isinstance(max_solves, bool) or int(max_solves) != max_solves or max_solves < 1:
        raise SampleArgumentError("solve_for_masses", f"max_solves {max_solves!r} is below 1")
    solve_kwargs["puncture_masses"] = True
    masses = [p.mass for p in punct]
    out = MassSolveResult(None, punct, T)
    for k in range(int(max_solves)):
        out.punctures = PunctureSet(Puncture(m, p.position, p.momentum, p.spin)
                                    for m, p in zip(masses, punct))
        out.result = poisson_solve(grid, prm, punctures=out.punctures, **solve_kwargs)
        M = out.result.puncture_masses.adm_masses
        err = max(abs(m - t) for m, t in zip(M, T))
        out.history.append(MassSolveStep(list(masses), list(M), err))
        if err <= rel_tol * max(T):
            out.converged = True
            break
        masses = [m * t / big for m, t, big in zip(masses, T, M)]
    return out
