"""The compiled reference -- TEST INFRASTRUCTURE ONLY.

A ctypes binding of oracle/_ref/libmgic_ref.so, which oracle/ref/Makefile
compiles from a checkout of the reference itself: the seven ChomboFortran
subroutines (translated by oracle/ref/chf2f.py, compiled by flang),
Source/SetLevelData.cpp with its headers (compiled unmodified against
oracle/ref/chombo_standin.H), and Source/VariableCoeffPoissonOperator.cpp and
Source/SetBCs.cpp with theirs (`Operator` below), and
Source/VariableCoeffPoissonOperatorFactory.cpp, Source/SetGrids.cpp and
Source/PoissonParameters.cpp (`Factory`, `tag_cells`, `domains_and_dx`,
`poisson_parameters`), all compiled unmodified against
oracle/ref/chombo_operator_standin.H.  This is what the
oracle's restatement is pinned to; nothing here restates arithmetic.

Array conventions are those of oracle/__init__.py: numpy float64 of shape
(nz, ny, nx) over an explicit box (i fastest), `Fab(arr, lo)` ties an array
to its box's low corner.  A 4-D array (ncomp, nz, ny, nx) is a FArrayBox of
ncomp components.

The library is never built on import.  `build()` compiles it when the
reference checkout is there; `available()` says whether it can be loaded.
The checkout is looked for in the directory `reference` beside the
repository, or where the environment variable MGIC_REFERENCE_DIR points.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import sys
from ctypes import POINTER, byref, c_double, c_int
from typing import Sequence

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "_ref", "libmgic_ref.so")
RECIPE = os.path.join(HERE, "ref")

# component order of the reference's two variable enums
MULTIGRID_VARS = ("psi", "A11_0", "A12_0", "A13_0", "A22_0", "A23_0", "A33_0", "phi_0")
GRCHOMBO_VARS = ("chi", "h11", "h12", "h13", "h22", "h23", "h33", "K", "A11", "A12", "A13", "A22",
                 "A23", "A33", "Theta", "Gamma1", "Gamma2", "Gamma3", "lapse", "shift1", "shift2",
                 "shift3", "B1", "B2", "B3", "phi", "Pi", "Ham", "Mom1", "Mom2", "Mom3")
C_PSI, C_PHI_0 = 0, 7


def reference_dir() -> str:
    """Where the reference checkout is expected (it need not exist)."""
    return os.environ.get("MGIC_REFERENCE_DIR") or os.path.join(
        os.path.dirname(os.path.dirname(HERE)), "reference")


def checkout_present() -> bool:
    return os.path.isfile(os.path.join(reference_dir(), "Source", "SetLevelData.cpp"))


def available() -> bool:
    return os.path.isfile(LIB)


def build() -> bool:
    """Compile the library when the checkout is present (an error if that
    fails); leave whatever oracle/_ref/ holds alone when it is not."""
    if not checkout_present():
        return available()
    subprocess.run(["make", "-s", "-C", RECIPE, "REF=" + os.path.abspath(reference_dir()),
                    "PYTHON=" + (sys.executable or "python3")], check=True)
    return True


class _CFab(ctypes.Structure):
    _fields_ = [("p", POINTER(c_double)), ("lo", c_int * 3), ("hi", c_int * 3), ("ncomp", c_int)]


class _Params(ctypes.Structure):
    _fields_ = [("L", c_double * 3)] + [(k, c_double) for k in (
        "G_Newton", "phi_amplitude", "phi_wavelength", "bh1_bare_mass", "bh2_bare_mass",
        "bh1_spin", "bh2_spin", "bh1_momentum", "bh2_momentum", "bh1_offset", "bh2_offset")]


class _PoissonParameters(ctypes.Structure):
    _fields_ = ([("nCells", c_int * 3), ("maxGridSize", c_int), ("blockFactor", c_int),
                 ("bufferSize", c_int), ("fillRatio", c_double), ("refineThresh", c_double),
                 ("coefficient_average_type", c_int), ("verbosity", c_int), ("maxLevel", c_int),
                 ("numLevels", c_int), ("n_periodic", c_int), ("periodic", c_int * 8),
                 ("n_refRatio", c_int), ("refRatio", c_int * 32), ("domain", c_int * 6),
                 ("domain_periodic", c_int * 3), ("coarsestDx", c_double),
                 ("domainLength", c_double * 3), ("probLo", c_double * 3), ("probHi", c_double * 3)] +
                [(k, c_double) for k in (
                    "alpha", "beta", "G_Newton", "phi_amplitude", "phi_wavelength", "bh1_bare_mass",
                    "bh2_bare_mass", "bh1_spin", "bh2_spin", "bh1_momentum", "bh2_momentum",
                    "bh1_offset", "bh2_offset")])


_lib = None
PD, PI, PF, PP = POINTER(c_double), POINTER(c_int), POINTER(_CFab), POINTER(_Params)
VP = ctypes.c_void_p


def lib():
    global _lib
    if _lib is None:
        if not available():
            raise FileNotFoundError(LIB + ": build it with oracle.reference.build()")
        L = ctypes.CDLL(LIB)
        for name, args, res in (
                ("mgic_ref_mayday_count", [], c_int),
                ("mgic_ref_mayday_reset", [], None),
                ("mgic_ref_set_initial_conditions", [PP, PF, PF, c_double], None),
                ("mgic_ref_set_rhs", [PP, PF, PF, c_double, c_double], None),
                ("mgic_ref_set_a_coef", [PP, PF, PF, c_double, c_double], None),
                ("mgic_ref_set_b_coef", [PP, PF, c_double], None),
                ("mgic_ref_set_constant_K_integrand", [PP, PF, PF, c_double], None),
                ("mgic_ref_set_regrid_condition", [PP, PF, PF, c_double], None),
                ("mgic_ref_set_update_psi0", [PF, PF], None),
                ("mgic_ref_set_output_data", [PP, PF, PF, c_double, c_double], None),
                ("mgic_ref_set_m_value", [PP, c_double, c_double], c_double),
                ("mgic_ref_get_Aij", [PP, c_int, c_int, c_double, c_double] + [PD] * 6, c_double),
                ("mgic_ref_set_binary_bh_Aij", [PP, PF, PI, PD], None),
                ("mgic_ref_set_binary_bh_psi", [PP, PD], c_double),
                ("mgic_ref_my_phi_function", [PD, c_double, c_double, PD], c_double),
                ("mgic_ref_num_multigrid_vars", [], c_int),
                ("mgic_ref_num_grchombo_vars", [], c_int),
                ("mgic_ref_op_create", [c_int, PI, PI, PI, c_double, c_double, c_double, PI, PI,
                                        c_double], ctypes.c_void_p),
                ("mgic_ref_op_destroy", [VP], None),
                ("mgic_ref_op_field", [VP, c_int, c_int], c_int),
                ("mgic_ref_op_field_set", [VP, c_int, c_int, PD], None),
                ("mgic_ref_op_field_get", [VP, c_int, c_int, PD], None),
                ("mgic_ref_op_lambda_get", [VP, c_int, PD], c_int),
                ("mgic_ref_op_residual", [VP, c_int, c_int, c_int, c_int], None),
                ("mgic_ref_op_apply_op", [VP, c_int, c_int, c_int], None),
                ("mgic_ref_op_apply_op_no_boundary", [VP, c_int, c_int], None),
                ("mgic_ref_op_precond", [VP, c_int, c_int], None),
                ("mgic_ref_op_relax", [VP, c_int, c_int, c_int], None),
                ("mgic_ref_op_level_gsrb", [VP, c_int, c_int], None),
                ("mgic_ref_op_level_jacobi", [VP, c_int, c_int], None),
                ("mgic_ref_op_restrict_residual", [VP, c_int, c_int, c_int], None),
                ("mgic_ref_op_set_alpha_beta", [VP, c_double, c_double], None),
                ("mgic_ref_op_set_coefs", [VP, c_int, c_int, c_double, c_double], None),
                ("mgic_ref_op_reset_lambda", [VP], None),
                ("mgic_ref_op_compute_lambda", [VP], None),
                ("mgic_ref_op_set_time", [VP, c_double], None),
                ("mgic_ref_parse_bc", [VP, c_int, c_int, c_int], None),
                ("mgic_ref_last_error", [], ctypes.c_char_p),
                ("mgic_ref_deck_clear", [], None),
                ("mgic_ref_deck_add", [ctypes.c_char_p, ctypes.c_char_p], None),
                ("mgic_ref_get_poisson_parameters", [POINTER(_PoissonParameters)], c_int),
                ("mgic_ref_set_domains_and_dx", [c_int, PI, PI, c_double, PI, PI, PI, PD], c_int),
                ("mgic_ref_set_tag_cells", [c_int, PI, PI, PI, PI, PD, PD, c_double, c_int, c_int], VP),
                ("mgic_ref_tags_count", [VP, c_int], ctypes.c_long),
                ("mgic_ref_tags_get", [VP, c_int, PI], None),
                ("mgic_ref_tags_destroy", [VP], None),
                ("mgic_ref_factory_create", [c_int, PI, PI, PI, PI, PI, c_double, c_double, c_double,
                                             PI, PI, c_double, c_int, c_int, c_int], VP),
                ("mgic_ref_factory_destroy", [VP], None),
                ("mgic_ref_factory_average_type", [VP], c_int),
                ("mgic_ref_factory_coef_set", [VP, c_int, c_int, c_int, PD], None),
                ("mgic_ref_factory_coef_get", [VP, c_int, c_int, c_int, PD], None),
                ("mgic_ref_factory_mg_new_op", [VP, c_int, c_int, PI], VP),
                ("mgic_ref_factory_amr_new_op", [VP, PI, PI], VP),
                ("mgic_ref_factory_ref_to_finer", [VP, PI, PI], c_int),
                ("mgic_ref_op_info", [VP, PD, PI, PI, PI, PI, PI], None),
                ("mgic_ref_op_box", [VP, c_int, PI], None),
                ("mgic_ref_op_coef_get", [VP, c_int, c_int, PD], None),
                ("mgic_ref_op_copier_count", [VP], c_int),
                ("mgic_ref_op_copier_get", [VP, PI], None)):
            f = getattr(L, name)
            f.argtypes, f.restype = args, res
        for name in ("gsrbhelmholtzvc3d_", "vccomputeop3d_", "vccomputeres3d_", "restrictresvc3d_",
                     "sumfaces_", "getlaplacianpsif_", "getrhogradphif_"):
            getattr(L, name).restype = None
        assert L.mgic_ref_num_multigrid_vars() == len(MULTIGRID_VARS)
        assert L.mgic_ref_num_grchombo_vars() == len(GRCHOMBO_VARS)
        _lib = L
    return _lib


def mayday_count() -> int:
    """MAYDAYERROR / CH_assert calls recorded since the last reset."""
    return lib().mgic_ref_mayday_count()


def mayday_reset() -> None:
    lib().mgic_ref_mayday_reset()


class Fab:
    """numpy array (nz, ny, nx) or (ncomp, nz, ny, nx) over the box at `lo`."""

    def __init__(self, arr: np.ndarray, lo: Sequence[int]):
        assert arr.dtype == np.float64 and arr.flags.c_contiguous and arr.ndim in (3, 4)
        self.arr = arr
        self.ncomp = arr.shape[0] if arr.ndim == 4 else 1
        self.lo = tuple(int(x) for x in lo)
        nz, ny, nx = arr.shape[-3:]
        self.hi = (self.lo[0] + nx - 1, self.lo[1] + ny - 1, self.lo[2] + nz - 1)
        self._c = _CFab(arr.ctypes.data_as(PD), (c_int * 3)(*self.lo), (c_int * 3)(*self.hi),
                        self.ncomp)

    @property
    def c(self):
        return byref(self._c)

    def fra1(self):
        """CHF_FRA1: pointer, lo0..2, hi0..2 (all by reference)."""
        return [self.arr.ctypes.data_as(PD)] + _ints(self.lo) + _ints(self.hi)

    def fra(self):
        """CHF_FRA: CHF_FRA1 then the number of components."""
        return self.fra1() + _ints([self.ncomp])


def _ints(v):
    return [byref(c_int(int(x))) for x in v]


def _real(x):
    return byref(c_double(float(x)))


# ---------------------------------------------------------------- the .ChF kernels
# `abi`: another library that exports the same symbols with the same argument
# lists (the HIP drop-ins of include/mgic_chf.h); None: the compiled reference.
def gsrb(u: Fab, rhs: Fab, rlo, rhi, dx, alpha, a: Fab, beta, b: Fab, lam: Fab, red_black: int,
         abi=None):
    (abi or lib()).gsrbhelmholtzvc3d_(*u.fra(), *rhs.fra(), *_ints(rlo), *_ints(rhi), _real(dx),
                             _real(alpha), *a.fra(), _real(beta), *b.fra(), *lam.fra(),
                             *_ints([red_black]))


def apply_op(lof: Fab, u: Fab, alpha, a: Fab, beta, b: Fab, rlo, rhi, dx, abi=None):
    (abi or lib()).vccomputeop3d_(*lof.fra(), *u.fra(), _real(alpha), *a.fra(), _real(beta), *b.fra(),
                         *_ints(rlo), *_ints(rhi), _real(dx))


def residual(res: Fab, u: Fab, rhs: Fab, alpha, a: Fab, beta, b: Fab, rlo, rhi, dx, abi=None):
    (abi or lib()).vccomputeres3d_(*res.fra(), *u.fra(), *rhs.fra(), _real(alpha), *a.fra(), _real(beta),
                          *b.fra(), *_ints(rlo), *_ints(rhi), _real(dx))


def restrict_residual(res: Fab, u: Fab, rhs: Fab, alpha, a: Fab, beta, b: Fab, rlo, rhi, dx,
                      abi=None):
    """RESTRICTRESVC3D as the Fortran has it: ACCUMULATES into res(i/2, j/2, k/2)."""
    (abi or lib()).restrictresvc3d_(*res.fra(), *u.fra(), *rhs.fra(), _real(alpha), *a.fra(), _real(beta),
                           *b.fra(), *_ints(rlo), *_ints(rhi), _real(dx))


def sumfaces(lhs: Fab, beta, b: Fab, lo, hi, direction: int, scale):
    lib().sumfaces_(*lhs.fra(), _real(beta), *b.fra(), *_ints(lo), *_ints(hi),
                    *_ints([direction]), _real(scale))


def laplacian_psi(out: Fab, psi: Fab, dx, lo, hi, abi=None):
    (abi or lib()).getlaplacianpsif_(*out.fra1(), *psi.fra1(), _real(dx), *_ints(lo), *_ints(hi))


def rho_grad_phi(out: Fab, phi: Fab, dx, lo, hi, abi=None):
    (abi or lib()).getrhogradphif_(*out.fra1(), *phi.fra1(), _real(dx), *_ints(lo), *_ints(hi))


def _shape(lo, hi, grow=0):
    return tuple(hi[d] - lo[d] + 1 + 2 * grow for d in (2, 1, 0))


def getlaplacianpsif(psi_g, lo, hi, dx):
    """GETLAPLACIANPSIF over [lo, hi]; psi_g over the box grown by one."""
    out = np.zeros(_shape(lo, hi))
    laplacian_psi(Fab(out, lo), Fab(np.ascontiguousarray(psi_g), [l - 1 for l in lo]), dx, lo, hi)
    return out


def getrhogradphif(phi_g, lo, hi, dx):
    """GETRHOGRADPHIF over [lo, hi]; phi_g over the box grown by one."""
    out = np.zeros(_shape(lo, hi))
    rho_grad_phi(Fab(out, lo), Fab(np.ascontiguousarray(phi_g), [l - 1 for l in lo]), dx, lo, hi)
    return out


# ---------------------------------------------------------------- SetLevelData.cpp
def _params(bh: dict) -> _Params:
    L = bh["domain_length"]
    L = (L, L, L) if np.isscalar(L) else tuple(L)
    return _Params((c_double * 3)(*L), *[bh[k] for k in (
        "G_Newton", "phi_amplitude", "phi_wavelength", "bh1_bare_mass", "bh2_bare_mass",
        "bh1_spin", "bh2_spin", "bh1_momentum", "bh2_momentum", "bh1_offset", "bh2_offset")])


def initial_conditions(bh: dict, lo, hi, dx):
    """set_initial_conditions over [lo, hi]: (multigrid_vars (8, nz, ny, nx)
    in MULTIGRID_VARS order, dpsi)."""
    mv = np.full((len(MULTIGRID_VARS),) + _shape(lo, hi), np.nan)
    dpsi = np.full(_shape(lo, hi), np.nan)
    p = _params(bh)
    lib().mgic_ref_set_initial_conditions(byref(p), Fab(mv, lo).c, Fab(dpsi, lo).c, float(dx))
    return mv, dpsi


def multigrid_vars(bh: dict, lo, hi, dx, psi=None, grow=1):
    """The reference's multigrid_vars over [lo, hi] grown by `grow`, as
    set_initial_conditions leaves them, with psi replaced when given."""
    glo, ghi = [l - grow for l in lo], [h + grow for h in hi]
    mv, _ = initial_conditions(bh, glo, ghi, dx)
    if psi is not None:
        assert np.shape(psi) == mv.shape[1:]
        mv[C_PSI] = psi
    return mv, glo


def _level(fn, bh, lo, hi, dx, psi, *tail, ncomp=1, grow=1):
    mv, glo = multigrid_vars(bh, lo, hi, dx, psi, grow)
    out = np.full(((ncomp,) if ncomp > 1 else ()) + _shape(lo, hi), np.nan)
    p = _params(bh)
    fn(byref(p), Fab(out, lo).c, Fab(mv, glo).c, float(dx), *tail)
    return out


def nl_coefs(bh: dict, lo, hi, dx, psi=None):
    """set_a_coef, set_rhs at psi given over [lo-1, hi+1] (None: psi = 1)."""
    K = float(bh["constant_K"])
    return (_level(lib().mgic_ref_set_a_coef, bh, lo, hi, dx, psi, K),
            _level(lib().mgic_ref_set_rhs, bh, lo, hi, dx, psi, K))


def nl_integrand(bh: dict, lo, hi, dx, psi=None):
    """set_constant_K_integrand at psi over [lo-1, hi+1]."""
    return _level(lib().mgic_ref_set_constant_K_integrand, bh, lo, hi, dx, psi)


def regrid_condition(bh: dict, lo, hi, dx, psi=None):
    """set_regrid_condition at psi over [lo-1, hi+1]."""
    return _level(lib().mgic_ref_set_regrid_condition, bh, lo, hi, dx, psi)


def output_vars(bh: dict, lo, hi, dx, psi):
    """set_output_data: the 31 GRChombo variables (31, nz, ny, nx) from psi
    over [lo, hi] (constant_K from bh)."""
    return _level(lib().mgic_ref_set_output_data, bh, lo, hi, dx, psi, float(bh["constant_K"]),
                  ncomp=len(GRCHOMBO_VARS), grow=0)


def update_psi0(mv: np.ndarray, mlo, dpsi: np.ndarray, dlo):
    lib().mgic_ref_set_update_psi0(Fab(mv, mlo).c, Fab(dpsi, dlo).c)


def m_value(bh: dict, phi_here: float, constant_K: float) -> float:
    p = _params(bh)
    return lib().mgic_ref_set_m_value(byref(p), float(phi_here), float(constant_K))


def _v3(v):
    return (c_double * 3)(*[float(x) for x in v])


def get_Aij(bh: dict, i, j, r1, r2, n1, n2, J1, J2, P1, P2) -> float:
    p = _params(bh)
    return lib().mgic_ref_get_Aij(byref(p), int(i), int(j), float(r1), float(r2), _v3(n1), _v3(n2),
                                  _v3(J1), _v3(J2), _v3(P1), _v3(P2))


def binary_bh_psi(bh: dict, loc) -> float:
    p = _params(bh)
    return lib().mgic_ref_set_binary_bh_psi(byref(p), _v3(loc))


def binary_bh_psi_on_box(bh: dict, lo, hi, dx):
    """set_binary_bh_psi at every cell centre of [lo, hi], the location
    computed as SetLevelData.cpp computes it."""
    L = bh["domain_length"]
    out = np.empty(_shape(lo, hi))
    for k in range(lo[2], hi[2] + 1):
        for j in range(lo[1], hi[1] + 1):
            for i in range(lo[0], hi[0] + 1):
                loc = [(float(v) + 0.5) * dx - L / 2.0 for v in (i, j, k)]
                out[k - lo[2], j - lo[1], i - lo[0]] = binary_bh_psi(bh, loc)
    return out


def my_phi_function(loc, amplitude, wavelength, L) -> float:
    L = (L, L, L) if np.isscalar(L) else L
    return lib().mgic_ref_my_phi_function(_v3(loc), float(amplitude), float(wavelength), _v3(L))


# ---------------------------------------------------------------- the operator class
def _iarr(v):
    v = [int(x) for x in v]
    return (c_int * len(v))(*v)


class Operator:
    """The reference's VariableCoeffPoissonOperator on one level of boxes
    (each lo0 lo1 lo2 hi0 hi1 hi2) over a domain, with ParseBC as its boundary
    function.  Fields are numbers handed out by `field()`; arrays are
    (nz, ny, nx) over a box grown by the field's ghost layers.  `aCoef` and
    `bCoef` are fields like any other: `set_coefs` hands them to the operator,
    which keeps them by reference, as the reference's factory does."""

    def __init__(self, boxes, domain, dx, alpha=1.0, beta=-1.0, periodic=(0, 0, 0),
                 bc_lo=(0, 0, 0), bc_hi=(0, 0, 0), bc_value=0.0, _made=None):
        self._ghost = {}
        self._level = {}
        self._h = None
        if _made is not None:  # an operator the reference's factory made (Factory below)
            self._h = VP(_made)
            nb = self.info()["nbox"]
            out = (c_int * 6)()
            self.boxes = []
            for n in range(nb):
                lib().mgic_ref_op_box(self._h, n, out)
                self.boxes.append(tuple(out))
            self.coarse_boxes = [tuple(v // 2 for v in b) for b in self.boxes]
            return
        self.boxes = [tuple(int(v) for v in b) for b in boxes]
        self.coarse_boxes = [tuple(v // 2 for v in b) for b in self.boxes]
        h = lib().mgic_ref_op_create(len(self.boxes), _iarr([v for b in self.boxes for v in b]),
                                     _iarr(domain), _iarr(periodic), float(dx), float(alpha),
                                     float(beta), _iarr(bc_lo), _iarr(bc_hi), float(bc_value))
        self._h = VP(h)

    def field(self, ghost=1, level=0, values=None):
        """A new zero field; `values`: one array per box over the valid cells."""
        f = lib().mgic_ref_op_field(self._h, int(level), int(ghost))
        self._ghost[f], self._level[f] = int(ghost), int(level)
        if values is not None:
            for b, v in enumerate(values):
                self.set(f, b, v)
        return f

    def shape(self, f, b, full=False):
        x = (self.coarse_boxes if self._level[f] else self.boxes)[b]
        g = self._ghost[f] if full else 0
        return tuple(x[3 + d] - x[d] + 1 + 2 * g for d in (2, 1, 0))

    def get(self, f, b, full=False):
        """Valid cells of box b (full: the whole fab, ghosts included)."""
        out = np.empty(self.shape(f, b, True))
        lib().mgic_ref_op_field_get(self._h, f, b, out.ctypes.data_as(PD))
        g = self._ghost[f]
        return out if full or g == 0 else np.ascontiguousarray(out[g:-g, g:-g, g:-g])

    def set(self, f, b, arr, full=False):
        """Valid cells of box b, the ghosts kept (full: the whole fab)."""
        arr = np.asarray(arr, dtype=np.float64)
        assert arr.shape == self.shape(f, b, full), (arr.shape, self.shape(f, b, full))
        g = self._ghost[f]
        if full or g == 0:
            whole = np.ascontiguousarray(arr)
        else:
            whole = self.get(f, b, full=True)
            whole[g:-g, g:-g, g:-g] = arr
        lib().mgic_ref_op_field_set(self._h, f, b, whole.ctypes.data_as(PD))

    def lam(self, b):
        """m_lambda over box b, or None while it is not defined."""
        x = self.boxes[b]
        out = np.empty(tuple(x[3 + d] - x[d] + 1 for d in (2, 1, 0)))
        return out if lib().mgic_ref_op_lambda_get(self._h, b, out.ctypes.data_as(PD)) else None

    def info(self):
        """dx, dxCrse, alpha, beta, refToCoarser, refToFiner, nbox, the ghost
        layers of aCoef and bCoef, the domain box and its periodic flags."""
        v, r, nb, g = (c_double * 4)(), (c_int * 2)(), c_int(), (c_int * 2)()
        dom, per = (c_int * 6)(), (c_int * 3)()
        lib().mgic_ref_op_info(self._h, v, r, byref(nb), g, dom, per)
        return dict(dx=v[0], dxCrse=v[1], alpha=v[2], beta=v[3], refToCoarser=r[0], refToFiner=r[1],
                    nbox=nb.value, coef_ghost=tuple(g), domain=tuple(dom), periodic=tuple(per))

    def coef(self, which, b, full=True):
        """m_aCoef (which 0) or m_bCoef (1) over box b, ghosts included (full)."""
        g = self.info()["coef_ghost"][which]
        x = self.boxes[b]
        out = np.empty(tuple(x[3 + d] - x[d] + 1 + 2 * g for d in (2, 1, 0)))
        lib().mgic_ref_op_coef_get(self._h, int(which), int(b), out.ctypes.data_as(PD))
        return out if full or g == 0 else np.ascontiguousarray(out[g:-g, g:-g, g:-g])

    def copier(self):
        """The exchange copier's motions: (to box, cells lo+hi, from box, shift)."""
        n = lib().mgic_ref_op_copier_count(self._h)
        out = (c_int * (11 * max(n, 1)))()
        lib().mgic_ref_op_copier_get(self._h, out)
        return sorted((out[11 * m], tuple(out[11 * m + 1:11 * m + 7]), out[11 * m + 7],
                       tuple(out[11 * m + 8:11 * m + 11])) for m in range(n))

    def residual(self, lhs, dpsi, rhs, homogeneous=False):
        lib().mgic_ref_op_residual(self._h, lhs, dpsi, rhs, int(bool(homogeneous)))

    def apply_op(self, lhs, dpsi, homogeneous=False):
        lib().mgic_ref_op_apply_op(self._h, lhs, dpsi, int(bool(homogeneous)))

    def apply_op_no_boundary(self, lhs, dpsi):
        lib().mgic_ref_op_apply_op_no_boundary(self._h, lhs, dpsi)

    def precond(self, cor, res):
        lib().mgic_ref_op_precond(self._h, cor, res)

    def relax(self, e, r, iterations):
        lib().mgic_ref_op_relax(self._h, e, r, int(iterations))

    def level_gsrb(self, dpsi, rhs):
        lib().mgic_ref_op_level_gsrb(self._h, dpsi, rhs)

    def level_jacobi(self, dpsi, rhs):
        lib().mgic_ref_op_level_jacobi(self._h, dpsi, rhs)

    def restrict_residual(self, res_coarse, dpsi, rhs):
        lib().mgic_ref_op_restrict_residual(self._h, res_coarse, dpsi, rhs)

    def set_alpha_beta(self, alpha, beta):
        lib().mgic_ref_op_set_alpha_beta(self._h, float(alpha), float(beta))

    def set_coefs(self, a, b, alpha, beta):
        lib().mgic_ref_op_set_coefs(self._h, a, b, float(alpha), float(beta))

    def reset_lambda(self):
        lib().mgic_ref_op_reset_lambda(self._h)

    def compute_lambda(self):
        lib().mgic_ref_op_compute_lambda(self._h)

    def set_time(self, t):
        lib().mgic_ref_op_set_time(self._h, float(t))

    def parse_bc(self, f, b, homogeneous=False):
        """ParseBC alone on box b's fab of field f."""
        lib().mgic_ref_parse_bc(self._h, f, b, int(bool(homogeneous)))

    def __del__(self):
        if getattr(self, "_h", None):
            lib().mgic_ref_op_destroy(self._h)
            self._h = None


# ---------------------------------------------------------------- factory, tagging, deck
class MayDay(RuntimeError):
    """The reference called MayDay::Error or MayDay::Abort; str() is its message."""


UNWRITTEN_BITS = 0x7FF800006D676963
"""What a LevelData the stand-in defines holds in every cell nobody wrote."""


def unwritten(a) -> np.ndarray:
    """Where an array still holds the stand-in's unwritten NaN."""
    return np.ascontiguousarray(a).view(np.uint64) == np.uint64(UNWRITTEN_BITS)


def _failed():
    return MayDay(lib().mgic_ref_last_error().decode())


class Factory:
    """The reference's VariableCoeffPoissonOperatorFactory over AMR levels of
    boxes: levels[l] a list of boxes, a[l][n] / b[l][n] the coefficients over
    the valid cells of box n (ghosts stay unwritten).  by_deck False: define(),
    then m_coefficient_average_type set to average_type when that is >= 0;
    by_deck True: defineOperatorFactory with a PoissonParameters whose
    coefficient_average_type is average_type."""

    def __init__(self, levels, domain0, dx0, a, b, alpha=1.0, beta=-1.0, periodic=(0, 0, 0),
                 bc_lo=(0, 0, 0), bc_hi=(0, 0, 0), bc_value=0.0, ref_ratio=None, coef_ghost=1,
                 by_deck=False, average_type=-1):
        self._h = None
        self.levels = [[tuple(int(v) for v in x) for x in lev] for lev in levels]
        nl = len(self.levels)
        self.ref_ratio = list(ref_ratio) if ref_ratio is not None else [2] * nl
        self.ghost = int(coef_ghost)
        self.domains = [tuple(int(v) for v in domain0)]
        for l in range(1, nl):
            r, d = self.ref_ratio[l - 1], self.domains[-1]
            self.domains.append(tuple(r * v for v in d[:3]) + tuple(r * (v + 1) - 1 for v in d[3:]))
        h = lib().mgic_ref_factory_create(
            nl, _iarr([len(x) for x in self.levels]), _iarr([v for lev in self.levels for x in lev for v in x]),
            _iarr(domain0), _iarr(periodic), _iarr(self.ref_ratio), float(dx0), float(alpha), float(beta),
            _iarr(bc_lo), _iarr(bc_hi), float(bc_value), self.ghost, int(bool(by_deck)), int(average_type))
        if not h:
            raise _failed()
        self._h = VP(h)
        for l in range(nl):
            for n in range(len(self.levels[l])):
                for which, src in ((0, a), (1, b)):
                    whole = self.coef(l, which, n)
                    g = self.ghost
                    whole[(slice(g, -g),) * 3 if g else ...] = src[l][n]
                    lib().mgic_ref_factory_coef_set(self._h, l, which, n, whole.ctypes.data_as(PD))

    def coef(self, level, which, n):
        """The factory's aCoef (0) or bCoef (1) of one box, ghosts included."""
        x, g = self.levels[level][n], self.ghost
        out = np.empty(tuple(x[3 + d] - x[d] + 1 + 2 * g for d in (2, 1, 0)))
        lib().mgic_ref_factory_coef_get(self._h, level, which, n, out.ctypes.data_as(PD))
        return out

    @property
    def average_type(self):
        return lib().mgic_ref_factory_average_type(self._h)

    def mg_new_op(self, level, depth):
        """MGnewOp(the domain of `level`, depth): an Operator, or None for NULL."""
        st = c_int()
        h = lib().mgic_ref_factory_mg_new_op(self._h, int(level), int(depth), byref(st))
        if st.value == 2:
            raise _failed()
        return None if st.value == 1 else Operator(None, None, 0.0, _made=h)

    def amr_new_op(self, level=None, domain=None):
        st = c_int()
        h = lib().mgic_ref_factory_amr_new_op(self._h, _iarr(domain or self.domains[level]), byref(st))
        if st.value:
            raise _failed()
        return Operator(None, None, 0.0, _made=h)

    def ref_to_finer(self, level=None, domain=None):
        r = c_int()
        if lib().mgic_ref_factory_ref_to_finer(self._h, _iarr(domain or self.domains[level]), byref(r)):
            raise _failed()
        return r.value

    def __del__(self):
        if getattr(self, "_h", None):
            lib().mgic_ref_factory_destroy(self._h)
            self._h = None


def tag_cells(levels, domains, values, dx, refine_thresh, tags_grow, periodic=(0, 0, 0), base_level=0):
    """set_tag_cells: levels[l] a list of boxes, values[l][n] over box n,
    domains[l] the level's domain box.  Returns, per level, an int array (n, 3)
    of the tagged cells (i, j, k), ordered by k, then j, then i."""
    nl = len(levels)
    flat = np.concatenate([np.ascontiguousarray(v, dtype=np.float64).ravel()
                           for lev in values for v in lev])
    for lev, vals in zip(levels, values):
        for x, v in zip(lev, vals):
            assert np.shape(v) == tuple(x[3 + d] - x[d] + 1 for d in (2, 1, 0))
    h = lib().mgic_ref_set_tag_cells(
        nl, _iarr([len(x) for x in levels]), _iarr([v for lev in levels for x in lev for v in x]),
        _iarr([v for d in domains for v in d]), _iarr(periodic), flat.ctypes.data_as(PD),
        (c_double * nl)(*[float(x) for x in dx]), float(refine_thresh), int(tags_grow), int(base_level))
    if not h:
        raise _failed()
    h = VP(h)
    out = []
    for l in range(nl):
        n = lib().mgic_ref_tags_count(h, l)
        cells = np.zeros((n, 3), dtype=np.int32)
        if n:
            lib().mgic_ref_tags_get(h, l, cells.ctypes.data_as(PI))
        out.append(cells)
    lib().mgic_ref_tags_destroy(h)
    return out


def domains_and_dx(nlevels, domain0, dx0, periodic=(0, 0, 0), ref_ratio=None):
    """set_domains_and_dx: ([domain box per level], [periodic flags per level], [dx per level])."""
    ref_ratio = list(ref_ratio) if ref_ratio is not None else [2] * nlevels
    dom, per, dx = (c_int * (6 * nlevels))(), (c_int * (3 * nlevels))(), (c_double * nlevels)()
    if lib().mgic_ref_set_domains_and_dx(nlevels, _iarr(domain0), _iarr(periodic), float(dx0),
                                         _iarr(ref_ratio), dom, per, dx):
        raise _failed()
    return ([tuple(dom[6 * l:6 * l + 6]) for l in range(nlevels)],
            [tuple(per[3 * l:3 * l + 3]) for l in range(nlevels)], list(dx))


def poisson_parameters(deck: dict) -> dict:
    """getPoissonParameters on a deck {name: [words]}: every field of the class."""
    lib().mgic_ref_deck_clear()
    for k, words in deck.items():
        for w in words:
            lib().mgic_ref_deck_add(k.encode(), str(w).encode())
    p = _PoissonParameters()
    if lib().mgic_ref_get_poisson_parameters(byref(p)):
        raise _failed()
    out = {}
    for k, _ in _PoissonParameters._fields_:
        v = getattr(p, k)
        out[k] = v if isinstance(v, (int, float)) else list(v)
    out["periodic"] = out["periodic"][:out.pop("n_periodic")]
    out["refRatio"] = out["refRatio"][:out.pop("n_refRatio")]
    return out
