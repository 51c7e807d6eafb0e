"""Apparent horizons of the solved data: the expansion at points, a surface in
spherical harmonics, and a flow that finds the surface of zero expansion.

For conformally flat data (gamma_ij = psi^4 delta_ij, K_ij = psi^-2 Abar_ij,
K = 0) the expansion of the outgoing null normals of a surface with flat unit
normal n is

    Theta = div n / psi^2 + 4 n . grad psi / psi^3 + Abar_ij n^i n^j / psi^6

with psi = psi_reg + sum m / r and Abar_ij = A^BY_ij [+ LW_ij].  The device
side is one kernel, libmgic_horizon.so (include/mgic_horizon.h):
psi, grad psi and Abar_ij n^i n^j at arbitrary points of the hierarchy, each on
the finest level that holds it, cubic (4^3 cells) or linear (2^3), whichever
is the first whose cells are all valid and not covered; the analytic parts are
taken at the point itself.  The rest is small dense numpy on the host.

    expansion_points(psi, points, normals, divn, prm, ...)   -> ExpansionResult
    SurfaceBasis(lmax, ntheta, nphi)        the surface grid and real Y_lm
    find_horizon(psi, prm, centre, r0, ...) -> HorizonResult
    horizons_of(psi, prm, spec, ...)        one HorizonResult per requested surface

A surface is r = h(theta, phi) about a centre c (star-shaped about it),
h = sum a_lm Y_lm up to lmax.  With F = r - h, everything at r = h:

    q = h_theta^2 + h_phi^2 / sin^2 theta        g = sqrt(1 + q / h^2)
    n = (rhat - (h_theta / h) thetahat - (h_phi / (h sin theta)) phihat) / g
    Lap F = 2 / h - Lap_S h / h^2                div n = (Lap F - n . grad g) / g

the flat area element is h^2 g sin theta dtheta dphi, and the horizon's area
is A = sum W psi^4 h^2 g.  Geometric units as adm.py and sample.py: a single
puncture of bare mass m has its horizon at r = m, A = 64 pi m^2, M_irr = 2 m.

The flow, from a_00 = r0 sqrt(4 pi): per iteration Theta at the surface points,
b_lm = Y^T (W rho Theta) with rho = psi^2 h^2 g, da_lm = -A / (1 + B l (l + 1))
b_lm with A = 1 / (lmax (lmax + 1)) + 0.5 and B = 0.5, and the step limiter: a
da with max |Y da| > 0.1 min h is scaled down to that (without it the flow
overshoots from a poor start radius and diverges).
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from ._lib import MgicError, horizon_call
from .adm import resolve_table
from .core import LevelData
from .punctures import table_args

MAX_LEVELS = 8         # MGIC_HORIZON_MAX_LEVELS (include/mgic_horizon.h)
MAX_POINTS = 1 << 20   # MGIC_HORIZON_MAX_POINTS
TERMS = ("theta", "psi", "dpsi_x", "dpsi_y", "dpsi_z", "A_nn")
STATUSES = ("converged", "collapsed", "left_grid", "max_iter")
FLOW_A_OFFSET, FLOW_B = 0.5, 0.5   # A = 1 / (lmax (lmax + 1)) + 0.5, B = 0.5
STEP_LIMIT = 0.1                   # max |Y da| <= 0.1 min h
COLLAPSE = 0.05                    # collapsed: min h <= 0.05 r0


class HorizonArgumentError(MgicError, ValueError):
    """A horizon request refused before anything is launched: the library's
    bad-argument status (MGIC_EBADARG)."""

    def __init__(self, func: str, msg: str):
        MgicError.__init__(self, func, -1, msg)


def cubic_weights(t: float) -> List[float]:
    """The order-4 value weights of the nodes -1, 0, 1, 2 at t (mgic_sample.h)."""
    tm1, tm2, tp1 = t - 1.0, t - 2.0, t + 1.0
    return [-t * tm1 * tm2 / 6.0, tp1 * tm1 * tm2 / 2.0, -tp1 * t * tm2 / 2.0,
            tp1 * t * tm1 / 6.0]


def cubic_derivative_weights(t: float) -> List[float]:
    """d/dt of cubic_weights: the product rule on the same factors, in the
    header's expression order (what the kernel evaluates, in float64)."""
    tm1, tm2, tp1 = t - 1.0, t - 2.0, t + 1.0
    a, b, c, d, e, f = tm1 * tm2, t * tm2, t * tm1, tp1 * tm2, tp1 * tm1, tp1 * t
    return [-((a + b) + c) / 6.0, ((a + d) + e) / 2.0, -((b + d) + f) / 2.0,
            ((c + e) + f) / 6.0]


def linear_weights(t: float) -> List[float]:
    return [1.0 - t, t]


def linear_derivative_weights(t: float) -> List[float]:
    return [-1.0, 1.0]


# ---------------------------------------------------------------- the expansion at points
@dataclass
class ExpansionResult:
    """Per point: theta, psi (the total conformal factor), dpsi (npts x 3),
    a_nn = Abar_ij n^i n^j; level: the level it was taken from (-1: none);
    order: 4 or 2, the stencil that was used (0: none, the six values NaN)."""
    theta: np.ndarray
    psi: np.ndarray
    dpsi: np.ndarray
    a_nn: np.ndarray
    level: np.ndarray
    order: np.ndarray


def _levels(fields) -> List[LevelData]:
    return [fields] if isinstance(fields, LevelData) else list(fields)


def _points(func: str, name: str, value, cols: int) -> np.ndarray:
    try:
        a = np.ascontiguousarray(value, dtype=np.float64)
    except (TypeError, ValueError):
        raise HorizonArgumentError(func, f"{name} must be numbers")
    if cols == 3 and a.ndim == 1 and a.size == 3:
        a = a.reshape(1, 3)
    if cols == 1:
        a = a.reshape(-1) if a.ndim <= 1 else a
        if a.ndim != 1:
            raise HorizonArgumentError(func, f"{name} must be npts numbers, not {a.shape}")
    elif a.ndim != 2 or a.shape[1] != 3:
        raise HorizonArgumentError(func, f"{name} must be npts x 3, not {a.shape}")
    return a


def check_not_periodic(prm, func: str) -> None:
    """Asymptotically flat decks only (as adm.py)."""
    if prm is not None and not isinstance(prm, dict) and getattr(prm, "is_periodic", 0):
        raise HorizonArgumentError(func, "horizons are not defined on a periodic domain")


def expansion_points(psi, points, normals, divn, prm, punctures=None,
                     momentum=None) -> ExpansionResult:
    """Theta, psi, grad psi and Abar_ij n^i n^j at each of `points` (npts x 3,
    the puncture table's coordinates) for the flat unit normals `normals`
    (npts x 3) with flat divergence `divn` (npts).  psi: the regular part, a
    LevelData, or one per AMR level, coarsest first.  The table and the LW
    fields are resolved as adm_charges resolves them: punctures None -- the
    deck's table, else its two holes; momentum: the MomentumFields of a solve
    with momentum=True (the total tensor), None: the Bowen-York tensor alone.
    Refusals are a ValueError before anything is launched."""
    func = "expansion_points"
    check_not_periodic(prm, func)
    levels = _levels(psi)
    if not 1 <= len(levels) <= MAX_LEVELS:
        raise HorizonArgumentError(func, f"level count {len(levels)} outside 1..{MAX_LEVELS}")
    xyz = _points(func, "points", points, 3)
    nrm = _points(func, "normals", normals, 3)
    dv = _points(func, "divn", divn, 1)
    npts = xyz.shape[0]
    if not 1 <= npts <= MAX_POINTS:
        raise HorizonArgumentError(func, f"point count {npts} outside 1..{MAX_POINTS}")
    if nrm.shape[0] != npts or dv.shape[0] != npts:
        raise HorizonArgumentError(
            func, f"{npts} points, {nrm.shape[0]} normals and {dv.shape[0]} divergences")
    punct = resolve_table(punctures, prm)
    lw = None
    if momentum is not None:
        if momentum.num_levels != len(levels):
            raise HorizonArgumentError(
                func, f"momentum has {momentum.num_levels} levels, psi {len(levels)}")
        flat = [f for l in range(len(levels)) for f in momentum.lw(l)]
        lw = (ctypes.c_void_p * len(flat))(*[f.handle.value for f in flat])
    out = np.empty((npts, len(TERMS)), dtype=np.float64)
    level = np.empty(npts, dtype=np.int32)
    used = np.empty(npts, dtype=np.int32)
    handles = (ctypes.c_void_p * len(levels))(*[f.handle.value for f in levels])
    PD, PI = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    try:
        horizon_call("mgic_horizon_expansion", levels[0].grid.comm.handle, len(levels), handles,
                     lw, *table_args(punct), npts, xyz.ctypes.data_as(PD), nrm.ctypes.data_as(PD),
                     dv.ctypes.data_as(PD), out.ctypes.data_as(PD), level.ctypes.data_as(PI),
                     used.ctypes.data_as(PI))
    except MgicError as e:
        if e.code == -1:  # MGIC_EBADARG: the package's ValueError
            raise HorizonArgumentError(func, str(e)) from None
        raise
    return ExpansionResult(out[:, 0].copy(), out[:, 1].copy(), out[:, 2:5].copy(),
                           out[:, 5].copy(), level, used)


# ---------------------------------------------------------------- the surface basis
def real_harmonics(lmax: int, x, phi):
    """The real orthonormal Y_lm, l <= lmax, at cos theta = x and phi (arrays of
    one shape, |x| < 1), with their derivatives: (Y, Y_theta, Y_phi, Y_theta_phi,
    Y_phi_phi, l, m), each harmonic array (npts, (lmax + 1)^2), columns ordered
    l = 0 .. lmax, m = -l .. l; m < 0: sin(|m| phi), m > 0: cos(m phi).  The
    associated Legendre functions come from the standard recurrences in their
    orthonormal form:

        P_mm = sqrt((2 m + 1) / (2 m)) sin theta P_(m-1)(m-1),  P_00 = sqrt(1 / (4 pi))
        P_(m+1)m = sqrt(2 m + 3) x P_mm
        P_lm = sqrt((4 l^2 - 1) / (l^2 - m^2))
               (x P_(l-1)m - sqrt(((l - 1)^2 - m^2) / (4 (l - 1)^2 - 1)) P_(l-2)m)
        sin theta dP_lm / dtheta = l x P_lm - sqrt((2 l + 1) (l^2 - m^2) / (2 l - 1)) P_(l-1)m
    """
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    phi = np.asarray(phi, dtype=np.float64).reshape(-1)
    s = np.sqrt(1.0 - x * x)
    P = {}
    for m in range(lmax + 1):
        if m == 0:
            P[(0, 0)] = np.full_like(x, math.sqrt(1.0 / (4.0 * math.pi)))
        else:
            P[(m, m)] = math.sqrt((2.0 * m + 1.0) / (2.0 * m)) * s * P[(m - 1, m - 1)]
        if m + 1 <= lmax:
            P[(m + 1, m)] = math.sqrt(2.0 * m + 3.0) * x * P[(m, m)]
        for l in range(m + 2, lmax + 1):
            c1 = math.sqrt((4.0 * l * l - 1.0) / (l * l - m * m))
            c2 = math.sqrt(((l - 1.0) ** 2 - m * m) / (4.0 * (l - 1.0) ** 2 - 1.0))
            P[(l, m)] = c1 * (x * P[(l - 1, m)] - c2 * P[(l - 2, m)])
    n = (lmax + 1) ** 2
    Y, Yt, Yp, Ytp, Ypp = (np.empty((x.size, n)) for _ in range(5))
    ls, ms = np.empty(n, dtype=int), np.empty(n, dtype=int)
    col = 0
    for l in range(lmax + 1):
        for m in range(-l, l + 1):
            k = abs(m)
            p = P[(l, k)]
            below = P[(l - 1, k)] if l - 1 >= k else 0.0
            dp = (l * x * p - math.sqrt((2.0 * l + 1.0) * (l * l - k * k) / (2.0 * l - 1.0))
                  * below) / s if l > 0 else np.zeros_like(x)
            if m == 0:
                az, daz = np.ones_like(phi), np.zeros_like(phi)
            elif m > 0:
                az, daz = math.sqrt(2.0) * np.cos(k * phi), -math.sqrt(2.0) * k * np.sin(k * phi)
            else:
                az, daz = math.sqrt(2.0) * np.sin(k * phi), math.sqrt(2.0) * k * np.cos(k * phi)
            Y[:, col] = p * az
            Yt[:, col] = dp * az
            Yp[:, col] = p * daz
            Ytp[:, col] = dp * daz
            Ypp[:, col] = -(k * k) * p * az
            ls[col], ms[col] = l, m
            col += 1
    return Y, Yt, Yp, Ytp, Ypp, ls, ms


class SurfaceBasis:
    """The surface grid and the harmonics on it.  Gauss-Legendre nodes in
    cos theta (ntheta of them), uniform phi_j = 2 pi j / nphi, point index
    i * nphi + j; W: the quadrature weights of the unit sphere (sum W = 4 pi);
    Y, Y_theta, Y_phi, Y_theta_phi, Y_phi_phi: (npts, (lmax + 1)^2);
    Y_theta_theta from Lap_S Y = -l (l + 1) Y."""

    def __init__(self, lmax: int, ntheta: Optional[int] = None, nphi: Optional[int] = None):
        if isinstance(lmax, bool) or int(lmax) != lmax or lmax < 0:
            raise HorizonArgumentError("SurfaceBasis", f"lmax {lmax!r} is not an integer >= 0")
        self.lmax = int(lmax)
        self.ntheta = int(ntheta) if ntheta is not None else self.lmax + 4
        self.nphi = int(nphi) if nphi is not None else 2 * self.ntheta
        if 2 * self.ntheta <= 2 * self.lmax or self.nphi <= 2 * self.lmax:
            raise HorizonArgumentError(
                "SurfaceBasis", f"{self.ntheta} x {self.nphi} points do not resolve lmax = {lmax}")
        nodes, wts = np.polynomial.legendre.leggauss(self.ntheta)
        x = np.repeat(nodes[::-1], self.nphi)  # theta increasing
        phi = np.tile(2.0 * math.pi * np.arange(self.nphi) / self.nphi, self.ntheta)
        self.cos_theta, self.phi = x, phi
        self.sin_theta = np.sqrt(1.0 - x * x)
        self.W = np.repeat(wts[::-1], self.nphi) * (2.0 * math.pi / self.nphi)
        (self.Y, self.Y_theta, self.Y_phi, self.Y_theta_phi, self.Y_phi_phi,
         self.l, self.m) = real_harmonics(self.lmax, x, phi)
        self.ll1 = (self.l * (self.l + 1)).astype(np.float64)
        st, ct, cp, sp = self.sin_theta, x, np.cos(phi), np.sin(phi)
        self.rhat = np.stack([st * cp, st * sp, ct], axis=1)
        self.thetahat = np.stack([ct * cp, ct * sp, -st], axis=1)
        self.phihat = np.stack([-sp, cp, np.zeros_like(sp)], axis=1)
        # Y_theta_theta = -l (l + 1) Y - cot theta Y_theta - Y_phi_phi / sin^2 theta
        self.Y_theta_theta = (-self.ll1[None, :] * self.Y - (ct / st)[:, None] * self.Y_theta
                              - self.Y_phi_phi / (st * st)[:, None])

    @property
    def npts(self) -> int:
        return self.ntheta * self.nphi

    @property
    def ncoef(self) -> int:
        return (self.lmax + 1) ** 2

    def project(self, f) -> np.ndarray:
        """Y^T (W f): the coefficients of f."""
        return self.Y.T @ (self.W * np.asarray(f))

    def geometry(self, coeffs, centre=(0.0, 0.0, 0.0)) -> "SurfaceGeometry":
        """The flat geometry of r = h(theta, phi) about `centre`."""
        a = np.asarray(coeffs, dtype=np.float64)
        st, ct = self.sin_theta, self.cos_theta
        h = self.Y @ a
        ht, hp = self.Y_theta @ a, self.Y_phi @ a
        htt, htp, hpp = self.Y_theta_theta @ a, self.Y_theta_phi @ a, self.Y_phi_phi @ a
        s2 = st * st
        q = ht * ht + hp * hp / s2
        g = np.sqrt(1.0 + q / (h * h))
        n = (self.rhat - (ht / h)[:, None] * self.thetahat
             - (hp / (h * st))[:, None] * self.phihat) / g[:, None]
        lap_s = -(self.Y @ (self.ll1 * a))
        lap_f = 2.0 / h - lap_s / (h * h)
        q_t = 2.0 * ht * htt + 2.0 * hp * htp / s2 - 2.0 * hp * hp * ct / (s2 * st)
        q_p = 2.0 * ht * htp + 2.0 * hp * hpp / s2
        # g as a field: G = sqrt(1 + q / r^2); its gradient at r = h
        g_r = -q / (g * h ** 3)
        g_t = q_t / (2.0 * g * h * h)
        g_p = q_p / (2.0 * g * h * h)
        n_dot_grad_g = (g_r - (ht / h) * g_t / h - (hp / (h * st)) * g_p / (h * st)) / g
        divn = (lap_f - n_dot_grad_g) / g
        c = np.asarray(centre, dtype=np.float64)
        return SurfaceGeometry(h, g, n, divn, c[None, :] + h[:, None] * self.rhat)


@dataclass
class SurfaceGeometry:
    """h, g = |grad F|, the flat unit normal n (npts x 3), its flat divergence
    and the surface points (npts x 3)."""
    h: np.ndarray
    g: np.ndarray
    normal: np.ndarray
    divn: np.ndarray
    points: np.ndarray


# ---------------------------------------------------------------- the finder
@dataclass
class HorizonResult:
    found: bool
    status: str
    iterations: int
    centre: Tuple[float, float, float]
    coeffs: np.ndarray
    lmax: int
    r_min: float
    r_mean: float
    r_max: float
    area: float
    irreducible_mass: float
    theta_rms: float
    theta_max: float
    degraded_points: int                 # surface points below order 4, last evaluation
    enclosed: List[int] = field(default_factory=list)
    spin: Optional[float] = None         # |J| of the table: one puncture enclosed
    christodoulou_mass: Optional[float] = None
    steps: List[float] = field(default_factory=list)  # max |Y da| of every iteration

    def summary(self) -> dict:
        """The JSON summary keys of tools/run_poisson.py (a value that is not
        finite is None)."""
        def num(v):
            return v if v is not None and math.isfinite(v) else None
        return {"status": self.status, "found": self.found, "iterations": self.iterations,
                "centre": list(self.centre), "area": num(self.area),
                "irreducible_mass": num(self.irreducible_mass), "enclosed": list(self.enclosed),
                "christodoulou_mass": num(self.christodoulou_mass)}

    def lines(self, label: str = "horizon") -> List[str]:
        """The lines tools/run_poisson.py prints for one surface."""
        c = " ".join(f"{v:.16e}" for v in self.centre)
        out = [f"{label} about {c}: {self.status} after {self.iterations} iterations"
               + ("" if self.found else " (not found)")]
        if self.found:
            out.append(f"{label}: r = {self.r_min:.16e} .. {self.r_max:.16e} (mean "
                       f"{self.r_mean:.16e}) area = {self.area:.16e} "
                       f"M_irr = {self.irreducible_mass:.16e}")
            out.append(f"{label}: theta rms = {self.theta_rms:.3e} max = {self.theta_max:.3e}, "
                       f"{self.degraded_points} points below order 4, encloses punctures "
                       + (" ".join(str(i + 1) for i in self.enclosed) or "none"))
            if self.christodoulou_mass is not None:
                out.append(f"{label}: |J| = {self.spin:.16e} "
                           f"M_chr = {self.christodoulou_mass:.16e}")
        return out


def _vec3(func: str, name: str, v) -> Tuple[float, float, float]:
    try:
        t = tuple(float(c) for c in v)
    except (TypeError, ValueError):
        t = ()
    if len(t) != 3 or not all(math.isfinite(c) for c in t):
        raise HorizonArgumentError(func, f"{name} must be three finite numbers, not {v!r}")
    return t


def check_request(centre, r0, lmax=8, tol=1e-10, max_iter=200, func: str = "find_horizon"):
    """The refusals of find_horizon that need no device: (centre, r0)."""
    c = _vec3(func, "centre", centre)
    try:
        r = float(r0)
        ok = not isinstance(r0, bool) and math.isfinite(r) and r > 0.0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise HorizonArgumentError(func, f"the start radius must be a positive number, not {r0!r}")
    if isinstance(lmax, bool) or not isinstance(lmax, (int, np.integer)) or not 0 <= lmax <= 32:
        raise HorizonArgumentError(func, f"lmax {lmax!r} is not an integer in 0..32")
    if not (isinstance(tol, (int, float)) and not isinstance(tol, bool) and tol > 0.0
            and math.isfinite(tol)):
        raise HorizonArgumentError(func, f"tol {tol!r} is not a positive number")
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
        raise HorizonArgumentError(func, f"max_iter {max_iter!r} is not an integer >= 1")
    return c, r


def _enclosed(basis_lmax: int, coeffs, centre, punct) -> List[int]:
    out = []
    for i, p in enumerate(punct):
        d = np.array(p.position) - np.array(centre)
        r = math.sqrt(float(d @ d))
        if r == 0.0:
            out.append(i)
            continue
        x = min(max(d[2] / r, -1.0 + 1e-15), 1.0 - 1e-15)
        Y = real_harmonics(basis_lmax, [x], [math.atan2(d[1], d[0])])[0]
        if r < float(Y[0] @ coeffs):
            out.append(i)
    return out


def find_horizon(psi, prm, centre, r0, lmax: int = 8, punctures=None, momentum=None,
                 tol: float = 1e-10, max_iter: int = 200,
                 evaluator: Optional[Callable] = None, basis: Optional[SurfaceBasis] = None
                 ) -> HorizonResult:
    """The surface of zero expansion about `centre`, starting from the sphere of
    radius r0 (the flow of the module's docstring).  psi, prm, punctures and
    momentum as expansion_points takes them.  evaluator: a callable with
    expansion_points' signature (default: the device).  It stops, and raises
    for none of them, as

        "converged"   max |Y da| <= tol mean h                     (found)
        "collapsed"   min h <= 0.05 r0
        "left_grid"   a point came back with order 0 or a non-finite Theta
        "max_iter"

    A periodic deck, a centre that is not three finite numbers, r0 <= 0, a bad
    lmax, tol or max_iter are a ValueError before anything is launched."""
    func = "find_horizon"
    check_not_periodic(prm, func)
    c, r0 = check_request(centre, r0, lmax, tol, max_iter, func)
    punct = resolve_table(punctures, prm)
    ev = evaluator if evaluator is not None else expansion_points
    B = basis if basis is not None else SurfaceBasis(lmax)
    if B.lmax != lmax:
        raise HorizonArgumentError(func, f"the basis has lmax {B.lmax}, not {lmax}")
    a = np.zeros(B.ncoef)
    a[0] = r0 * math.sqrt(4.0 * math.pi)
    gain = (1.0 / (lmax * (lmax + 1)) if lmax > 0 else 0.0) + FLOW_A_OFFSET
    scale = -gain / (1.0 + FLOW_B * B.ll1)
    status, it, steps = "max_iter", 0, []
    geo = B.geometry(a, c)
    last = None
    while True:
        if not np.min(geo.h) > COLLAPSE * r0:
            status = "collapsed"
            break
        res = ev(psi, geo.points, geo.normal, geo.divn, prm, punctures=punct, momentum=momentum)
        if np.any(np.asarray(res.order) == 0) or not np.all(np.isfinite(res.theta)):
            status = "left_grid"
            break
        last = (geo, res)
        if status == "converged" or it >= max_iter:
            break
        rho = res.psi * res.psi * geo.h * geo.h * geo.g
        da = scale * B.project(rho * res.theta)
        step = float(np.max(np.abs(B.Y @ da)))
        limit = STEP_LIMIT * float(np.min(geo.h))
        if step > limit:
            da *= limit / step
            step = limit
        a = a + da
        it += 1
        steps.append(step)
        if step <= tol * float(np.mean(geo.h)):
            status = "converged"  # one more evaluation: the final surface's own Theta
        geo = B.geometry(a, c)
    found = status == "converged"
    nan = float("nan")
    h = geo.h
    if last is not None and last[0] is geo:
        res = last[1]
        area = float(np.sum(B.W * res.psi ** 4 * h * h * geo.g))
        trms = math.sqrt(float(np.sum(B.W * res.theta ** 2)) / (4.0 * math.pi))
        tmax = float(np.max(np.abs(res.theta)))
        degraded = int(np.sum(np.asarray(res.order) < 4))
    else:
        area = trms = tmax = nan
        degraded = 0
    out = HorizonResult(found, status, it, c, a, lmax, float(np.min(h)), float(np.mean(h)),
                        float(np.max(h)), area,
                        math.sqrt(area / (16.0 * math.pi)) if area == area else nan, trms, tmax,
                        degraded, steps=steps)
    if found:
        out.enclosed = _enclosed(lmax, a, c, punct)
        if len(out.enclosed) == 1:
            J = punct[out.enclosed[0]].spin
            out.spin = math.sqrt((J[0] * J[0] + J[1] * J[1]) + J[2] * J[2])
            m = out.irreducible_mass
            out.christodoulou_mass = math.sqrt(m * m + out.spin * out.spin / (4.0 * m * m))
    return out


# ---------------------------------------------------------------- requests
def parse_horizon(value, func: str = "horizon") -> Tuple[Tuple[float, float, float], float]:
    """((cx, cy, cz), r0) from "cx cy cz r0" or four numbers (the deck's horizonN
    and tools/run_poisson.py --horizon)."""
    items = value.replace(",", " ").split() if isinstance(value, str) else value
    try:  # what resolve_horizons returns is taken as it is: ((cx, cy, cz), r0)
        if len(items) == 2 and len(items[0]) == 3:
            items = list(items[0]) + [items[1]]
    except TypeError:
        pass
    try:
        nums = [float(v) for v in items]
        ok = len(nums) == 4 and not any(isinstance(v, bool) for v in items)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise HorizonArgumentError(func, f"a horizon is \"cx cy cz r0\", not {value!r}")
    return check_request(nums[:3], nums[3], func=func)


def resolve_horizons(spec, punct, func: str = "horizons"):
    """A `horizons=` argument as a list of ((cx, cy, cz), r0): a list of four
    numbers each, or "punctures": one surface per puncture of the table `punct`,
    centred on it, with r0 = m_i (a puncture of bare mass <= 0 is refused)."""
    if isinstance(spec, str):
        if spec.strip() != "punctures":
            raise HorizonArgumentError(
                func, f"horizons is a list of (cx, cy, cz, r0) or \"punctures\", not {spec!r}")
        out = []
        for i, p in enumerate(punct):
            if not p.mass > 0.0:
                raise HorizonArgumentError(
                    func, f"puncture {i + 1} has bare mass {p.mass!r}: no start radius")
            out.append((tuple(p.position), float(p.mass)))
        return out
    try:
        items = list(spec)
    except TypeError:
        raise HorizonArgumentError(func, f"horizons is a list of (cx, cy, cz, r0), not {spec!r}")
    if not items:
        raise HorizonArgumentError(func, "no horizons")
    return [parse_horizon(v, func) for v in items]


def horizons_of(psi, prm, spec, punctures=None, momentum=None, evaluator=None,
                **kwargs) -> List[HorizonResult]:
    """One find_horizon per surface of `spec` (resolve_horizons)."""
    check_not_periodic(prm, "horizons")
    punct = resolve_table(punctures, prm)
    return [find_horizon(psi, prm, c, r, punctures=punct, momentum=momentum,
                         evaluator=evaluator, **kwargs)
            for c, r in resolve_horizons(spec, punct)]


def horizon_lines(horizons: Sequence[HorizonResult], masses=None) -> List[str]:
    """The lines of every surface; with a PunctureMassReport and one surface per
    puncture (horizons = punctures), M_irr next to M_i."""
    out = []
    for k, h in enumerate(horizons):
        out.extend(h.lines(f"horizon {k + 1}"))
    if masses is not None and len(masses.punctures) == len(horizons):
        for k, (h, p) in enumerate(zip(horizons, masses.punctures)):
            if h.found and h.enclosed == [k]:
                out.append(f"horizon {k + 1}: M_irr = {h.irreducible_mass:.16e} "
                           f"M_{k + 1} = {p.adm_mass:.16e}")
    return out
