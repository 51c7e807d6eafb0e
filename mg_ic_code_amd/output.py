"""HDF5 output in the reference's layouts, through
libmgic_io.so (include/mgic_io.h).

    output_final_data   WriteOutput.H:127-227 (the GRChombo checkpoint,
                        set_output_data's 31 variables, SetLevelData.cpp:343-396)
    output_solver_data  WriteOutput.H:52-123 (the per-NL-iteration file:
                        dpsi, rhs and the 8 multigrid_vars)

The per-box components are computed on the GPU (k_output_vars) and streamed
into the file in z-slabs; there is no host fallback.  The multigrid_vars
A_ij_0 are not stored fields here: set_initial_conditions sets them
analytically and nothing changes them, so the kernels evaluate them in place.
phi_0 is evaluated in place too (the Gaussian of MyPhiFunction.H) unless the
caller passes the stored field (`phi`, one LevelData per level; phi.py): then
the "phi" / "phi_0" component is copied from it.  With `punctures` (a
punctures.PunctureSet) the A_ij_0, A_ij and chi components come from the
puncture table instead of the deck's two holes.  With `matter` (matter.py)
the final data's "Pi" component (26) is the stored Pi_0, as given; the solver
data (the reference's multigrid_vars) has no Pi.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np

from ._lib import call, io_call
from .core import BH_KEYS, LevelData
from .matter import MatterArgumentError, fill_matter, table_or_null
from .punctures import table_args

GRCHOMBO_VARS = (  # GRChomboUserVariables.hpp:58-75
    "chi", "h11", "h12", "h13", "h22", "h23", "h33", "K", "A11", "A12", "A13", "A22", "A23",
    "A33", "Theta", "Gamma1", "Gamma2", "Gamma3", "lapse", "shift1", "shift2", "shift3", "B1",
    "B2", "B3", "phi", "Pi", "Ham", "Mom1", "Mom2", "Mom3")
SOLVER_VARS = ("dpsi", "rhs", "psi", "A11_0", "A12_0", "A13_0", "A22_0", "A23_0", "A33_0",
               "phi_0")  # WriteOutput.H:74-80 + MultigridUserVariables.hpp:29-33


def _bh(bh: dict):
    return (ctypes.c_double * 13)(*[float(bh[k]) for k in BH_KEYS])


def _handles(fields: Sequence[LevelData]):
    return (ctypes.c_void_p * len(fields))(*[f.handle for f in fields])


def _enc(filename: Optional[str]):
    return filename.encode() if filename is not None else None


def output_final_data(psi: Sequence[LevelData], bh: dict, max_level: int = 0,
                      ref_ratio: Optional[Sequence[int]] = None,
                      filename: Optional[str] = None,
                      phi: Optional[Sequence[LevelData]] = None, punctures=None,
                      matter=None, constraints: bool = False, momentum=None) -> None:
    """output_final_data (WriteOutput.H:127-227); constant_K = bh['constant_K'].
    filename None: "vcPoissonFinal.3d.hdf5" in the working directory.
    phi: the stored phi_0 per level (None: the analytic Gaussian).
    punctures: the puncture table (None: the deck's two holes).
    matter: a matter.Matter (None: today's calls, Pi = 0): the stored Pi_0 is
    written as given into component 26, "Pi".  GRChombo calls Pi the "(minus)
    conjugate momentum"; only Pi^2 enters the sources here, so its sign is the
    caller's convention.
    constraints: components 27-30 (Ham, Mom1..3) carry the constraints of the
    data (constraints.py; Pi enters Mom_i with the sign it is stored with)
    instead of set_output_data's zeros; nothing else in the file changes.
    momentum: the momentum.MomentumFields of a solve with momentum=True (needs
    the matter): A11..A33, and with `constraints` Ham and Mom1..3, carry the
    total tensor Abar^BY_ij + LW_ij."""
    n = len(psi)
    rr = list(ref_ratio) if ref_ratio is not None else [2] * n
    if momentum is not None:
        mat = fill_matter(matter, [f.grid for f in psi], bh, "output_final_data")
        if mat is None:
            raise MatterArgumentError("output_final_data", "momentum= needs the matter of the solve")
        io_call("mgic_io_write_final_data_ctt", _enc(filename), n, _handles(psi),
                _handles(phi) if phi is not None else None, _bh(bh), *table_or_null(punctures),
                _handles(mat.pi) if mat.pi is not None else None, mat.potential.pot(),
                _handles([f for l in range(n) for f in momentum.lw(l)]), int(bool(constraints)),
                int(max_level), (ctypes.c_int * n)(*rr))
        return
    if constraints:
        mat = None
        if matter is not None:
            mat = fill_matter(matter, [f.grid for f in psi], bh, "output_final_data")
        io_call("mgic_io_write_final_data_constraints", _enc(filename), n, _handles(psi),
                _handles(phi) if phi is not None else None, _bh(bh), *table_or_null(punctures),
                _handles(mat.pi) if mat is not None and mat.pi is not None else None,
                mat.potential.pot() if mat is not None else None, int(max_level),
                (ctypes.c_int * n)(*rr))
        return
    if matter is not None:
        mat = fill_matter(matter, [f.grid for f in psi], bh, "output_final_data")
        io_call("mgic_io_write_final_data_matter", _enc(filename), n, _handles(psi),
                _handles(phi) if phi is not None else None, _bh(bh), *table_or_null(punctures),
                _handles(mat.pi) if mat.pi is not None else None, mat.potential.pot(),
                int(max_level), (ctypes.c_int * n)(*rr))
        return
    if punctures is not None:
        io_call("mgic_io_write_final_data_punct", _enc(filename), n, _handles(psi),
                _handles(phi) if phi is not None else None, _bh(bh), *table_args(punctures),
                int(max_level), (ctypes.c_int * n)(*rr))
        return
    if phi is not None:
        io_call("mgic_io_write_final_data_phi", _enc(filename), n, _handles(psi), _handles(phi),
                _bh(bh), int(max_level), (ctypes.c_int * n)(*rr))
        return
    io_call("mgic_io_write_final_data", _enc(filename), n, _handles(psi), _bh(bh), int(max_level),
            (ctypes.c_int * n)(*rr))


def output_solver_data(dpsi: Sequence[LevelData], rhs: Sequence[LevelData],
                       psi: Sequence[LevelData], bh: dict, iteration: int,
                       ref_ratio: Optional[Sequence[int]] = None,
                       filename: Optional[str] = None,
                       phi: Optional[Sequence[LevelData]] = None, punctures=None) -> None:
    """output_solver_data (WriteOutput.H:52-123) for NL iteration `iteration`.
    filename None: "vcPoissonOut.3d_<iteration>.hdf5".
    phi: the stored phi_0 per level (None: the analytic Gaussian).
    punctures: the puncture table (None: the deck's two holes)."""
    n = len(psi)
    rr = list(ref_ratio) if ref_ratio is not None else [2] * n
    if punctures is not None:
        io_call("mgic_io_write_solver_data_punct", _enc(filename), n, _handles(dpsi),
                _handles(rhs), _handles(psi), _handles(phi) if phi is not None else None,
                _bh(bh), *table_args(punctures), (ctypes.c_int * n)(*rr), int(iteration))
        return
    if phi is not None:
        io_call("mgic_io_write_solver_data_phi", _enc(filename), n, _handles(dpsi), _handles(rhs),
                _handles(psi), _handles(phi), _bh(bh), (ctypes.c_int * n)(*rr), int(iteration))
        return
    io_call("mgic_io_write_solver_data", _enc(filename), n, _handles(dpsi), _handles(rhs),
            _handles(psi), _bh(bh), (ctypes.c_int * n)(*rr), int(iteration))


def grchombo_vars(psi: LevelData, n: int, bh: dict, k0: int = 0, nk: Optional[int] = None,
                  out_device_ptr: Optional[int] = None,
                  phi: Optional[LevelData] = None, punctures=None,
                  matter=None, constraints: bool = False, abar=None) -> Optional[np.ndarray]:
    """set_output_data for local box n, planes [k0, k0+nk): (31, nk, ny, nx) on
    the host, or written to device memory at out_device_ptr (returns None).
    phi: the stored phi_0 (None: the analytic Gaussian).
    punctures: the puncture table (None: the deck's two holes).
    matter: a matter.Matter (None: today's calls): component 26, "Pi", is its
    stored Pi_0 as given (the sign is the caller's convention).
    constraints: components 27-30 (Ham, Mom1..3) are filled by a second launch
    into the same array (constraints.py) instead of left at zero.
    abar: six stored fields (11, 12, 13, 22, 23, 33) of psi's level added to
    the Bowen-York tensor in A11..A33 and, with `constraints`, in Ham and
    Mom1..3 (needs the matter; momentum.MomentumFields.lw(level))."""
    return _vars(0, psi, None, None, n, bh, k0, nk, out_device_ptr, phi, punctures, matter,
                 constraints, abar)


def solver_vars(dpsi: LevelData, rhs: LevelData, psi: LevelData, n: int, bh: dict, k0: int = 0,
                nk: Optional[int] = None, out_device_ptr: Optional[int] = None,
                phi: Optional[LevelData] = None, punctures=None):
    """output_solver_data's 10 components for local box n: (10, nk, ny, nx)."""
    return _vars(1, psi, dpsi, rhs, n, bh, k0, nk, out_device_ptr, phi, punctures)


def _vars(kind, psi, dpsi, rhs, n, bh, k0, nk, dev, phi=None, punctures=None, matter=None,
          constraints=False, abar=None):
    lo, hi = psi.grid.local_box(n)[:3], psi.grid.local_box(n)[3:]
    nx, ny, nz = (hi[d] - lo[d] + 1 for d in range(3))
    nk = nz - k0 if nk is None else nk
    nc = 31 if kind == 0 else 10
    if dev is not None:
        ptr, out = ctypes.c_void_p(dev), None
    else:
        out = np.empty((nc, nk, ny, nx))
        ptr = out.ctypes.data_as(ctypes.c_void_p)
    hphi = phi.handle if phi is not None else None
    mat = None
    if abar is not None and matter is None:
        raise MatterArgumentError("grchombo_vars", "abar= needs the matter of the solve")
    if abar is not None:  # kind 0 only
        mat = fill_matter(matter, [psi.grid], bh, "grchombo_vars")
        call("mgic_field_grchombo_vars_ctt", psi.handle, hphi, n, k0, nk, _bh(bh),
             *table_or_null(punctures), mat.pi[0].handle if mat.pi is not None else None,
             mat.potential.pot(), _handles(abar), ptr, int(dev is not None))
    elif matter is not None:  # kind 0 only
        mat = fill_matter(matter, [psi.grid], bh, "grchombo_vars")
        call("mgic_field_grchombo_vars_matter", psi.handle, hphi, n, k0, nk, _bh(bh),
             *table_or_null(punctures), mat.pi[0].handle if mat.pi is not None else None,
             mat.potential.pot(), ptr, int(dev is not None))
    elif punctures is not None and kind == 0:
        call("mgic_field_grchombo_vars_punct", psi.handle, hphi, n, k0, nk, _bh(bh),
             *table_args(punctures), ptr, int(dev is not None))
    elif punctures is not None:
        call("mgic_field_solver_vars_punct", dpsi.handle, rhs.handle, psi.handle, hphi, n, k0, nk,
             _bh(bh), *table_args(punctures), ptr, int(dev is not None))
    elif phi is not None and kind == 0:
        call("mgic_field_grchombo_vars_phi", psi.handle, phi.handle, n, k0, nk, _bh(bh), ptr,
             int(dev is not None))
    elif phi is not None:
        call("mgic_field_solver_vars_phi", dpsi.handle, rhs.handle, psi.handle, phi.handle, n, k0,
             nk, _bh(bh), ptr, int(dev is not None))
    elif kind == 0:
        call("mgic_field_grchombo_vars", psi.handle, n, k0, nk, _bh(bh), ptr, int(dev is not None))
    else:
        call("mgic_field_solver_vars", dpsi.handle, rhs.handle, psi.handle, n, k0, nk, _bh(bh), ptr,
             int(dev is not None))
    if constraints:  # kind 0 only: Ham, Mom1..3 are the array's last four components
        slab = 8 * 27 * nk * ny * nx
        cptr = ctypes.c_void_p((dev if dev is not None else out.ctypes.data) + slab)
        if abar is not None:
            call("mgic_field_constraint_vars_ctt", psi.handle, hphi, n, k0, nk, _bh(bh),
                 *table_or_null(punctures), mat.pi[0].handle if mat.pi is not None else None,
                 mat.potential.pot(), _handles(abar), cptr, int(dev is not None))
            return out
        call("mgic_field_constraint_vars", psi.handle, hphi, n, k0, nk, _bh(bh),
             *table_or_null(punctures),
             mat.pi[0].handle if mat is not None and mat.pi is not None else None,
             mat.potential.pot() if mat is not None else None, cptr, int(dev is not None))
    return out


def write_host(filename: str, kind: int, levels, ref_ratio: Sequence[int], max_level: int = 0,
               iteration: int = 0) -> None:
    """Either layout from host arrays.  levels: [(domain lohi6, dx, [(box lohi6,
    data (ncomp, nz, ny, nx)), ...]), ...] in layout order."""
    nbox, boxes, domains, dxs, chunks = [], [], [], [], []
    nc = 31 if kind == 0 else 10
    for dom, dx, bl in levels:
        nbox.append(len(bl))
        domains += list(dom)
        dxs.append(float(dx))
        for b, data in bl:
            boxes += list(b)
            shape = (nc, b[5] - b[2] + 1, b[4] - b[1] + 1, b[3] - b[0] + 1)
            a = np.ascontiguousarray(data, dtype=np.float64)
            if kind in (0, 1) and a.shape != shape:
                raise ValueError(f"box {b}: data shape {a.shape} != {shape}")
            chunks.append(a.ravel())
    data = np.concatenate(chunks) if chunks else np.zeros(1)
    nl = len(levels)
    io_call("mgic_io_write_host", filename.encode(), int(kind), nl, (ctypes.c_int * nl)(*nbox),
            (ctypes.c_int * max(1, len(boxes)))(*boxes), (ctypes.c_int * (6 * nl))(*domains),
            (ctypes.c_double * nl)(*dxs), (ctypes.c_int * nl)(*list(ref_ratio)),
            data.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(max_level), int(iteration))
