"""ADM mass, momentum and spin of the solved data, on cube surfaces of level 0.

The constraints (constraints.py) say whether the data are a solution; the
charges say of what.  For an asymptotically flat deck (K = 0, Dirichlet
dpsi = 0) they are surface integrals of fields the device already holds
(libmgic_adm.so, include/mgic_adm.h).  Geometric units, as the
bare masses enter psi_bh = sum m / r: no factor G.

Level 0 has N_d cells (all even), spacing dx, cell centres at
(iv + 0.5) dx - N_d dx / 2.  A surface is the cell-aligned cube of half-width
n_R cells about the domain centre: 6 sides, side = 2 d + (s > 0) for the
outward normal s e_d, each (2 n_R)^2 cell faces (b, a), a and b along the two
other directions in increasing order.  For a face with centre x_f, inner cell
`in` and outer cell `out`:

    g    = (psi[out] - psi[in]) / dx + s * d_d psi_bh(x_f)
    A_kd = A^BY_kd(x_f)  [ + 0.5 * (LW_kd[in] + LW_kd[out]) ]
    mass = -(1 / (2 pi)) * g * dx^2
    P_i  =  (1 / (8 pi)) * s * A_id * dx^2
    J_i  =  (1 / (8 pi)) * s * sum_jk eps_ijk x_f,j A_kd * dx^2

and M(R), P_i(R), J_i(R) are their sums over the surface.  In the continuum
every cube that encloses all punctures gives P = sum P_n and
J = sum (J_n + x_n x P_n) of the Bowen-York tensor exactly, and M -> 2 sum m_n
for psi = 1; the midpoint rule makes all three second order in dx.  With a
momentum solve's fields the tensor is the total one, Abar^BY_ij + LW_ij, so
P(R) and J(R) also carry what the matter current adds.

    surface_terms(psi, half_widths, punctures, lw=None)   the 7 terms of every face
    charges(psi, half_widths, punctures, lw=None)         the 7 sums per surface
    adm_charges(psi, prm, half_widths, ...)               a level or a hierarchy -> AdmReport

The holes are always a table: the deck's two go through
PunctureSet.from_params.  Only valid cells of level 0 are read.  On a
hierarchy level 0's psi under finer levels is not the solution, so a surface
whose inner or outer cells are covered by level 1 is refused.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from ._lib import MgicError, adm_call
from .core import Grid, LevelData
from .punctures import PunctureSet, resolve_punctures, table_args

MAX_SURFACES = 8  # MGIC_ADM_MAX_SURFACES (include/mgic_adm.h)
TERMS = ("mass", "P1", "P2", "P3", "J1", "J2", "J3")


class AdmArgumentError(MgicError, ValueError):
    """A charges request refused on the host before anything is launched: the
    library's bad-argument status (MGIC_EBADARG)."""

    def __init__(self, func: str, msg: str):
        MgicError.__init__(self, func, -1, msg)


def parse_half_widths(value, func: str = "adm") -> List[int]:
    """1 to MAX_SURFACES half-widths >= 1 from a list of integers or a string
    of them ("12 15", the deck's adm_half_widths and --adm)."""
    items = value.replace(",", " ").split() if isinstance(value, str) else value
    try:
        items = list(items)
    except TypeError:
        items = [items]
    out = []
    for v in items:
        try:
            i = int(v)
            ok = not isinstance(v, bool) and float(v) == i
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise AdmArgumentError(func, f"a half-width must be an integer, not {v!r}")
        out.append(i)
    if not 1 <= len(out) <= MAX_SURFACES:
        raise AdmArgumentError(func, f"surface count {len(out)} outside 1..{MAX_SURFACES}")
    for n in out:
        if n < 1:
            raise AdmArgumentError(func, f"half-width {n} is below 1")
    return out


def max_half_width(domain) -> int:
    """min_d N_d / 2 - 1: the outer cells of the cube stay inside the domain."""
    return min((domain[3 + d] - domain[d] + 1) // 2 for d in range(3)) - 1


def check_base(domain, periodic, half_widths, func: str = "adm") -> None:
    """The refusals that need level 0's domain alone (the library's own)."""
    if any(periodic):
        raise AdmArgumentError(func, "the charges are not defined on a periodic domain")
    if any(domain[d] != 0 for d in range(3)):
        raise AdmArgumentError(func, "the domain's low corner must be 0")
    for d in range(3):
        n = domain[3 + d] + 1
        if n % 2:
            raise AdmArgumentError(
                func, f"N = {n} is odd: no cell-aligned cube about the centre")
    top = max_half_width(domain)
    for n in half_widths:
        if n > top:
            raise AdmArgumentError(
                func, f"half-width {n} is above {top}: its outer cells would leave the domain")


def _shell_boxes(domain, n: int):
    """The inner and outer cells of the cube of half-width n, as 6 boxes
    (one slab of two cells' depth per side)."""
    c = [(domain[3 + d] + 1) // 2 for d in range(3)]
    out = []
    for d in range(3):
        for s in (-1, 1):
            lo = [c[e] - n for e in range(3)]
            hi = [c[e] + n - 1 for e in range(3)]
            m = c[d] + n if s > 0 else c[d] - n
            lo[d], hi[d] = m - 1, m
            out.append(tuple(lo) + tuple(hi))
    return out


def _covered(domain, n: int, fine_boxes) -> bool:
    for sb in _shell_boxes(domain, n):
        for b in fine_boxes:
            if all(max(sb[d], b[d]) <= min(sb[3 + d], b[3 + d]) for d in range(3)):
                return True
    return False


def check_hierarchy(grids: Sequence[Grid], half_widths, func: str = "adm") -> None:
    """ValueError for a surface with an inner or outer cell under level 1."""
    if len(grids) < 2:
        return
    dom = grids[0].domain
    fine = [tuple(v // 2 for v in b) for b in grids[1].boxes]  # in level-0 cells
    for n in half_widths:
        if _covered(dom, n, fine):
            clear = next((m for m in range(1, max_half_width(dom) + 1)
                          if not _covered(dom, m, fine)), None)
            hint = (f"the smallest half-width that clears level 1 is {clear}" if clear is not None
                    else "no half-width inside the domain clears level 1")
            raise AdmArgumentError(
                func, f"the surface of half-width {n} crosses cells covered by level 1, where "
                      f"level 0's psi is not the solution; {hint}")


def _ints(vals):
    return (ctypes.c_int * len(vals))(*[int(v) for v in vals])


def _lw_arg(lw):
    if lw is None:
        return None
    lw = list(lw)
    if len(lw) != 6:
        raise AdmArgumentError("adm", f"lw is the six stored LW_ij, not {len(lw)} fields")
    return (ctypes.c_void_p * 6)(*[f.handle.value for f in lw])


def surface_count(half_widths) -> int:
    """The number of doubles surface_terms writes: sum of 6 * 7 * (2 n)^2."""
    hw = parse_half_widths(half_widths)
    n = ctypes.c_longlong()
    adm_call("mgic_adm_surface_count", len(hw), _ints(hw), ctypes.byref(n))
    return n.value


def surface_terms(psi: LevelData, half_widths, punctures, lw=None,
                  out_device_ptr: Optional[int] = None) -> Optional[List[np.ndarray]]:
    """The 7 terms (TERMS) of every face: one (6, 7, 2 n, 2 n) array per
    surface, indexed (side, term, b, a); or written to device memory at
    out_device_ptr, the surfaces concatenated (returns None).  psi: the level-0
    field; punctures: a PunctureSet (or rows); lw: the six stored LW_ij of level
    0 (MomentumFields.lw(0)), None: the Bowen-York tensor alone."""
    hw = parse_half_widths(half_widths, "surface_terms")
    check_base(psi.grid.domain, psi.grid.periodic, hw, "surface_terms")
    if out_device_ptr is not None:
        ptr, flat = ctypes.c_void_p(out_device_ptr), None
    else:
        flat = np.empty(sum(6 * 7 * (2 * n) ** 2 for n in hw))
        ptr = flat.ctypes.data_as(ctypes.c_void_p)
    adm_call("mgic_adm_surface_terms", psi.grid.comm.handle, psi.handle, len(hw), _ints(hw),
             *table_args(punctures), _lw_arg(lw), ptr, int(out_device_ptr is not None))
    if flat is None:
        return None
    out, at = [], 0
    for n in hw:
        size = 6 * 7 * (2 * n) ** 2
        out.append(flat[at:at + size].reshape(6, 7, 2 * n, 2 * n))
        at += size
    return out


def charges(psi: LevelData, half_widths, punctures, lw=None) -> np.ndarray:
    """The sums of the 7 terms over each surface: (nsurf, 7), in the library's
    fixed order (repeatable bit for bit, independent of the box layout)."""
    hw = parse_half_widths(half_widths, "charges")
    check_base(psi.grid.domain, psi.grid.periodic, hw, "charges")
    out = np.empty((len(hw), 7))
    adm_call("mgic_adm_charges", psi.grid.comm.handle, psi.handle, len(hw), _ints(hw),
             *table_args(punctures), _lw_arg(lw), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    return out


Vec3 = Tuple[float, float, float]


@dataclass
class AdmSurface:
    """The charges on one surface; radius = half_width * dx."""
    half_width: int
    radius: float
    mass: float
    momentum: Vec3
    angular_momentum: Vec3


@dataclass
class AdmExpected:
    """What the table asks for, in float64 on the host: 2 sum m (the mass at
    psi = 1), sum P, sum (J + x x P)."""
    mass: float
    momentum: Vec3
    angular_momentum: Vec3


def expected_charges(punctures) -> AdmExpected:
    t = resolve_punctures(punctures).table().reshape(-1, 10)
    m = 0.0
    P = [0.0, 0.0, 0.0]
    J = [0.0, 0.0, 0.0]
    for r in t:
        x, p, j = r[1:4], r[4:7], r[7:10]
        m += float(r[0])
        xp = (x[1] * p[2] - x[2] * p[1], x[2] * p[0] - x[0] * p[2], x[0] * p[1] - x[1] * p[0])
        for i in range(3):
            P[i] += float(p[i])
            J[i] += float(j[i] + xp[i])
    return AdmExpected(2.0 * m, tuple(P), tuple(J))


@dataclass
class AdmReport:
    """surfaces: one AdmSurface per requested half-width, in the order given;
    expected: the table's own totals."""
    surfaces: List[AdmSurface] = field(default_factory=list)
    expected: Optional[AdmExpected] = None

    def lines(self) -> List[str]:
        """One line per surface, then the table's totals (tools/run_poisson.py
        --adm)."""
        def v(x):
            return " ".join(f"{c:.16e}" for c in x)
        out = [f"adm n_R = {s.half_width} (R = {s.radius:.16e}): M = {s.mass:.16e} "
               f"P = {v(s.momentum)} J = {v(s.angular_momentum)}" for s in self.surfaces]
        e = self.expected
        out.append(f"adm expected: 2 sum m = {e.mass:.16e} sum P = {v(e.momentum)} "
                   f"sum (J + x x P) = {v(e.angular_momentum)}")
        return out


def resolve_table(punctures, prm) -> PunctureSet:
    """The holes as a table: the caller's, else the deck's table, else the
    deck's two holes through PunctureSet.from_params."""
    punct = resolve_punctures(punctures, prm)
    if punct is None:
        punct = PunctureSet.from_params(prm)
        punct.table()
    return punct


def adm_charges(psi, prm, half_widths, punctures=None, momentum=None) -> AdmReport:
    """The charges of the data at psi (a LevelData, or one per AMR level,
    coarsest first) on the cubes of the given half-widths (level-0 cells).

    prm: the PoissonParameters of the solve (or the bh dict of BH_KEYS).
    punctures None -- the deck's table if it has one, else its two holes, as
    poisson_solve resolves them.  momentum: the momentum.MomentumFields of a
    solve with momentum=True (NLResult.momentum): the charges of the total
    tensor Abar^BY_ij + LW_ij; None: of the Bowen-York tensor alone.

    Refused with a ValueError before anything is launched: a periodic base, an
    odd N_d, a half-width < 1 or > min_d N_d / 2 - 1, more than MAX_SURFACES
    surfaces, and on a hierarchy a surface with an inner or outer cell covered
    by level 1 (the message names the smallest half-width that clears it)."""
    psis = [psi] if isinstance(psi, LevelData) else list(psi)
    grids = [f.grid for f in psis]
    hw = parse_half_widths(half_widths, "adm_charges")
    check_base(grids[0].domain, grids[0].periodic, hw, "adm_charges")
    check_hierarchy(grids, hw, "adm_charges")
    punct = resolve_table(punctures, prm)
    sums = charges(psis[0], hw, punct, momentum.lw(0) if momentum is not None else None)
    dx = grids[0].dx
    rep = AdmReport(expected=expected_charges(punct))
    for n, row in zip(hw, sums):
        rep.surfaces.append(AdmSurface(n, n * dx, float(row[0]), tuple(float(x) for x in row[1:4]),
                                       tuple(float(x) for x in row[4:7])))
    return rep
