"""ctypes binding of libmgic.so (the C ABI declared in include/mgic.h).

The library is built in-tree by ``__graft_entry__.build()`` (hipcc,
gfx950).  There is no fallback: if the shared object is missing or fails to
load, importing this module raises, so nothing can silently run on a CPU
path.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_int, c_long, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# MGIC_LIB_PATH: another build of the library (A/B measurements only)
LIB_PATH = os.environ.get("MGIC_LIB_PATH") or os.path.join(_HERE, "libmgic.so")


class MgicError(RuntimeError):
    """A libmgic call returned a negative status."""

    def __init__(self, func: str, code: int, msg: str):
        super().__init__(f"{func} failed ({code}): {msg}")
        self.code = code


class OpParams(ctypes.Structure):
    """mgic_op_params (include/mgic.h)."""

    _fields_ = [
        ("alpha", c_double),
        ("beta", c_double),
        ("bc_lo", c_int * 3),
        ("bc_hi", c_int * 3),
        ("bc_value", c_double),
        ("coefficient_average_type", c_int),
        ("prolong_type", c_int),
        ("relax_mode", c_int),
        ("fused_smoother", c_int),
        ("deep_halo", c_int),
    ]


class SolveParams(ctypes.Structure):
    """mgic_solve_params (include/mgic.h)."""

    _fields_ = [
        ("num_mg_iterations", c_int),
        ("max_iterations", c_int),
        ("tolerance", c_double),
        ("norm_type", c_int),
    ]


class MGParams(ctypes.Structure):
    """mgic_mg_params (include/mgic.h)."""

    _fields_ = [
        ("max_depth", c_int),
        ("n_pre", c_int),
        ("n_post", c_int),
        ("n_bottom", c_int),
        ("bottom_solver", c_int),
        ("cycles", c_int),
        ("agglomerate_below", c_int),
        ("bicg_imax", c_int),
        ("bicg_eps", c_double),
        ("bicg_reps", c_double),
        ("bicg_small", c_double),
        ("bicg_restarts", c_int),
        ("bicg_norm_type", c_int),
    ]


H = c_void_p  # every opaque handle
PI = POINTER(c_int)
PD = POINTER(c_double)
PH = POINTER(c_void_p)
PLL = POINTER(ctypes.c_longlong)

# name -> argtypes (all return int status unless listed in _RESTYPE)
SIGNATURES = {
    "mgic_version": [],
    "mgic_abi_version": [],
    "mgic_last_error": [],
    "mgic_set_device": [c_int],
    "mgic_get_device_count": [PI],
    "mgic_device_synchronize": [],
    "mgic_op_params_default": [POINTER(OpParams)],
    "mgic_mg_params_default": [POINTER(MGParams)],
    "mgic_comm_unique_id": [ctypes.c_char_p],
    "mgic_comm_create": [c_int, c_int, ctypes.c_char_p, c_int, PH],
    "mgic_comm_create_ipc": [c_int, c_int, c_void_p, c_void_p, ctypes.c_size_t, PH],
    "mgic_comm_transport": [H, PI],
    "mgic_comm_destroy": [H],
    "mgic_comm_set_stream": [H, c_void_p],
    "mgic_comm_get_stream": [H, PH],
    "mgic_comm_set_self_messages": [H, c_int],
    "mgic_comm_exchanges": [H, ctypes.POINTER(ctypes.c_ulonglong)],
    "mgic_comm_synchronize": [H],
    "mgic_comm_rank": [H, PI, PI, PI],
    "mgic_grid_create": [H, PI, PI, c_double, c_int, PI, PI, PH],
    "mgic_grid_destroy": [H],
    "mgic_grid_num_local": [H, PI],
    "mgic_grid_local_box": [H, c_int, PI, PI],
    "mgic_grid_coarsen": [H, c_int, PH],
    "mgic_field_nl_coefs": [H, H, H, PD],
    "mgic_field_nl_integrand": [H, H, PD],
    "mgic_field_set_val_all": [H, c_double],
    "mgic_field_regrid_condition": [H, H, PD],
    "mgic_field_norm": [H, c_int, PD],
    "mgic_field_tag_lattice": [H, c_double, c_int, c_int, PI, PI, c_void_p],
    "mgic_regrid_lattice": [c_int, c_int, PI, PI],
    "mgic_regrid_cluster": [c_void_p, PI, c_double, c_int, c_int, PI, PI],
    "mgic_regrid_levels": [c_int, PI, POINTER(c_void_p), PI, PI, c_int, c_int, c_double, c_int,
                           c_int, PI, PI, PI],
    "mgic_regrid_levels_periodic": [c_int, PI, PI, POINTER(c_void_p), PI, PI, c_int, c_int,
                                    c_double, c_int, c_int, PI, PI, PI],
    "mgic_regrid_owners": [c_int, PI, c_int, PI],
    "mgic_op_update_psi": [H, H, H],
    "mgic_plan_create": [c_int, c_int, PI, PI, c_int, PI, PI, c_int, PI, PI, c_int, c_int, PH],
    "mgic_plan_create_shell": [c_int, c_int, PI, PI, c_int, PI, PI, c_int, PH],
    "mgic_plan_check_transport": [H, c_int],
    "mgic_plan_ipc_blocks": [H, PI, PLL],
    "mgic_plan_ipc_blocks_per": [H, ctypes.c_longlong, PI, PLL],
    "mgic_plan_destroy": [H],
    "mgic_plan_sizes": [H, PI, PI, PI, PI],
    "mgic_plan_items": [H, c_int, PLL],
    "mgic_plan_peers": [H, PI, PLL, PLL, PLL, PLL],
    "mgic_plan_geom": [H, c_int, c_int, PLL],
    "mgic_field_create": [H, PH],
    "mgic_field_destroy": [H],
    "mgic_field_device_ptr": [H, c_int, PH, POINTER(c_long)],
    "mgic_field_upload": [H, c_int, PD, c_int],
    "mgic_field_download": [H, c_int, PD, c_int],
    "mgic_field_set_val": [H, c_double],
    "mgic_field_set_zero": [H],
    "mgic_field_exchange": [H],
    "mgic_field_copy_to": [H, H, c_int],
    "mgic_field_binary_bh": [H, H, PD],
    "mgic_factory_define": [H, POINTER(OpParams), H, H, PH],
    "mgic_factory_destroy": [H],
    "mgic_factory_mg_new_op": [H, c_int, PH],
    "mgic_factory_amr_new_op": [H, PH],
    "mgic_factory_ref_to_finer": [H, PI],
    "mgic_op_destroy": [H],
    "mgic_op_grid": [H, PH],
    "mgic_op_coef": [H, c_int, PH],
    "mgic_op_residual": [H, H, H, H, c_int],
    "mgic_op_apply_op": [H, H, H, c_int],
    "mgic_op_apply_op_no_boundary": [H, H, H],
    "mgic_op_precond": [H, H, H],
    "mgic_op_relax": [H, H, H, c_int],
    "mgic_op_level_gsrb": [H, H, H],
    "mgic_op_level_jacobi": [H, H, H],
    "mgic_op_restrict_residual": [H, H, H, H],
    "mgic_op_prolong_increment": [H, H, H],
    "mgic_op_set_alpha_beta": [H, c_double, c_double],
    "mgic_op_set_coefs": [H, H, H, c_double, c_double],
    "mgic_op_reset_lambda": [H],
    "mgic_op_set_time": [H, c_double],
    "mgic_op_fill_bc": [H, H, c_int],
    "mgic_op_set_to_zero": [H, H],
    "mgic_op_assign": [H, H, H],
    "mgic_op_incr": [H, H, H, c_double],
    "mgic_op_axby": [H, H, H, H, c_double, c_double],
    "mgic_op_scale": [H, H, c_double],
    "mgic_op_dot": [H, H, H, PD],
    "mgic_op_norm": [H, H, c_int, PD],
    "mgic_op_axpy2_norm": [H, H, H, H, c_double, H, H, c_double, c_int, PD],
    "mgic_op_dot2": [H, H, H, PD, PD],
    "mgic_op_bicg_p": [H, H, H, H, c_double, c_double],
    "mgic_op_bicgstab": [H, H, H, c_int, POINTER(MGParams), PI],
    "mgic_op_bicgstab_info": [PI],
    "mgic_mg_create": [H, POINTER(MGParams), PH],
    "mgic_mg_destroy": [H],
    "mgic_mg_num_depths": [H, PI],
    "mgic_mg_op": [H, c_int, PH],
    "mgic_mg_level_field": [H, c_int, c_int, PH],
    "mgic_mg_one_cycle": [H, H, H],
    "mgic_mg_iteration": [H, H, H, H, c_int, c_int, PD],
    "mgic_mg_iterations": [H, H, H, H, c_int, c_int, c_int, PD],
    "mgic_mg_init_residual": [H, H, H, H, c_int, c_int, PD],
    "mgic_mg_precondition": [H, H, H, c_int],
    "mgic_mg_bottom_timer": [H, c_int],
    "mgic_mg_bottom_ms": [H, PD, PI],
    "mgic_mg_bottom_iters": [H, PLL, PD, PD],
    "mgic_mg_bottom_replay": [H, c_int, PD, PI, PD, PI],
    "mgic_mg_bottom_info": [H, PI, PI, PD],
    "mgic_mg_fmg": [H, H, H, H, c_int, c_int, c_int, PD],
    "mgic_grid_create_patches": [H, PI, PI, c_double, c_int, PI, PI, PH],
    "mgic_amr_create": [c_int, POINTER(H), POINTER(H), POINTER(H), POINTER(OpParams),
                        POINTER(MGParams), PH],
    "mgic_amr_destroy": [H],
    "mgic_amr_num_levels": [H, PI],
    "mgic_amr_level_op": [H, c_int, PH],
    "mgic_amr_cf_interp": [H, c_int, H, H],
    "mgic_amr_average_down": [H, c_int, H, H],
    "mgic_amr_operator": [H, c_int, H, H, H, c_int],
    "mgic_amr_residual": [H, c_int, H, H, H, H, c_int],
    "mgic_amr_restrict": [H, c_int, H, H, H, H],
    "mgic_amr_prolong": [H, c_int, H, H],
    "mgic_amr_update_residual": [H, c_int, H, H, H],
    "mgic_amr_init_residual": [H, POINTER(H), POINTER(H), c_int, PD],
    "mgic_amr_iteration": [H, POINTER(H), POINTER(H), c_int, PD],
    "mgic_amr_residual_field": [H, c_int, PH],
    "mgic_amr_apply_op": [H, POINTER(H), POINTER(H), c_int],
    "mgic_amr_composite_residual": [H, POINTER(H), POINTER(H), POINTER(H), c_int],
    "mgic_amr_dot": [H, POINTER(H), POINTER(H), PD],
    "mgic_amr_norm": [H, POINTER(H), c_int, PD],
    "mgic_amr_composite_norm": [H, POINTER(H), c_int, PD],
    "mgic_amr_composite_sum": [H, POINTER(H), PD],
    "mgic_amr_precondition": [H, POINTER(H), POINTER(H), c_int],
    "mgic_amr_reflux_register": [c_void_p],
    "mgic_amr_set_reflux": [H, c_int],
    "mgic_amr_reflux": [H, c_int, H, H, H, c_int],
    "mgic_mixed_create": [H, POINTER(MGParams), PH],
    "mgic_mixed_destroy": [H],
    "mgic_mixed_num_depths": [H, PI],
    "mgic_mixed_init_residual": [H, H, H, H, c_int, PD],
    "mgic_mixed_iteration": [H, H, H, H, c_int, PD],
    "mgic_mixed_fmg": [H, H, H, H, c_int, c_int, PD],
    "mgic_solve_params_default": [POINTER(SolveParams)],
    "mgic_mg_solve": [H, H, H, POINTER(SolveParams), PI, PD],
    "mgic_amr_solve": [H, POINTER(H), POINTER(H), POINTER(SolveParams), PI, PD],
    "mgic_field_grchombo_vars": [H, c_int, c_int, c_int, PD, c_void_p, c_int],
    "mgic_field_solver_vars": [H, H, H, c_int, c_int, c_int, PD, c_void_p, c_int],
    "mgic_field_fill_phi": [H, c_int, PD],
    "mgic_field_nl_coefs_phi": [H, H, H, H, PD],
    "mgic_field_nl_integrand_phi": [H, H, H, PD],
    "mgic_field_regrid_condition_phi": [H, H, H, PD],
    "mgic_field_grchombo_vars_phi": [H, H, c_int, c_int, c_int, PD, c_void_p, c_int],
    "mgic_field_solver_vars_phi": [H, H, H, H, c_int, c_int, c_int, PD, c_void_p, c_int],
    "mgic_field_nl_coefs_punct": [H, H, H, H, PD, c_int, PD],
    "mgic_field_nl_integrand_punct": [H, H, H, PD, c_int, PD],
    "mgic_field_regrid_condition_punct": [H, H, H, PD, c_int, PD],
    "mgic_field_grchombo_vars_punct": [H, H, c_int, c_int, c_int, PD, c_int, PD, c_void_p, c_int],
    "mgic_field_solver_vars_punct": [H, H, H, H, c_int, c_int, c_int, PD, c_int, PD, c_void_p,
                                     c_int],
    "mgic_field_nl_coefs_matter": [H, H, H, H, PD, c_int, PD, H, PD],
    "mgic_field_nl_integrand_matter": [H, H, H, PD, c_int, PD, H, PD],
    "mgic_field_regrid_condition_matter": [H, H, H, PD, c_int, PD, H, PD],
    "mgic_field_grchombo_vars_matter": [H, H, c_int, c_int, c_int, PD, c_int, PD, H, PD, c_void_p,
                                        c_int],
    "mgic_field_constraints": [H, H, H, H, H, H, H, PD, c_int, PD, H, PD],
    "mgic_field_constraint_vars": [H, H, c_int, c_int, c_int, PD, c_int, PD, H, PD, c_void_p,
                                   c_int],
    "mgic_field_momentum_source": [H, H, H, H, H, PD, c_int, PD, H, PD],
    "mgic_field_nl_coefs_ctt": [H, H, H, H, PD, c_int, PD, H, PD, PH],
    "mgic_field_nl_integrand_ctt": [H, H, H, PD, c_int, PD, H, PD, PH],
    "mgic_field_grchombo_vars_ctt": [H, H, c_int, c_int, c_int, PD, c_int, PD, H, PD, PH, c_void_p,
                                     c_int],
    "mgic_field_constraints_ctt": [H, H, H, H, H, H, H, PD, c_int, PD, H, PD, PH],
    "mgic_field_constraint_vars_ctt": [H, H, c_int, c_int, c_int, PD, c_int, PD, H, PD, PH,
                                       c_void_p, c_int],
    "mgic_field_layout": [H, PI, PI, PD, PI, PI, PI],
    "mgic_field_box": [H, c_int, PI, PI, PI],
    "mgic_field_barrier": [H],
    "mgic_host_alloc": [c_size_t, PH],
    "mgic_host_free": [c_void_p],
    "mgic_prof_smoother": [c_int, c_long],
    "mgic_prof_smoother_read": [PI, POINTER(c_long), PD],
    "mgic_launch_ledger_dump": [c_char_p],
    "mgic_launch_ledger_reset": [],
    # ChomboFortran drop-ins (include/mgic_chf.h); argtypes left open
    "gsrbhelmholtzvc3d_": None,
    "vccomputeop3d_": None,
    "vccomputeres3d_": None,
    "restrictresvc3d_": None,
    "getlaplacianpsif_": None,
    "getrhogradphif_": None,
}

_RESTYPE = {
    "mgic_version": c_char_p,
    "mgic_last_error": c_char_p,
    "mgic_op_params_default": None,
    "mgic_mg_params_default": None,
    "mgic_solve_params_default": None,
    "gsrbhelmholtzvc3d_": None,
    "vccomputeop3d_": None,
    "vccomputeres3d_": None,
    "restrictresvc3d_": None,
    "getlaplacianpsif_": None,
    "getrhogradphif_": None,
}


def hip_runtime_images() -> list:
    """The distinct HIP runtime files (libamdhip64*) mapped into this process,
    from /proc/self/maps ([] where that file does not exist)."""
    paths = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                parts = line.split(None, 5)
                if len(parts) == 6:
                    p = parts[5].strip()
                    if os.path.basename(p).startswith("libamdhip64"):
                        paths.add(os.path.realpath(p))
    except OSError:
        return []
    return sorted(paths)


def check_single_hip_runtime() -> None:
    """Fail loudly when this process maps more than one HIP runtime: torch
    bundles its own libamdhip64 under another path, and a process that loads
    libmgic.so (which binds /opt/rocm's by soname) before torch holds both --
    they corrupt each other's heap at exit ("double free or corruption",
    status -6).  Checked at load, and again wherever a Comm or a device is
    set up (torch may be imported after this package)."""
    imgs = hip_runtime_images()
    if len(imgs) > 1:
        raise RuntimeError(
            "two HIP runtimes in one process (" + ", ".join(imgs) + "): import torch before "
            "mg_ic_code_amd (the default preload does this unless MGIC_NO_TORCH_PRELOAD is set)")


def _preload_torch() -> None:
    """Import torch (when installed) before the library, so that libmgic.so
    binds to torch's HIP runtime by soname instead of loading a second one
    (check_single_hip_runtime).  MGIC_NO_TORCH_PRELOAD=1 skips it (a process
    that never imports torch); a torch that is present but broken is not this
    library's failure: any exception is swallowed, and the runtime check
    still guards the process."""
    if os.environ.get("MGIC_NO_TORCH_PRELOAD", "0") not in ("", "0"):
        return
    try:
        import torch  # noqa: F401
    except Exception:  # noqa: BLE001 -- see the docstring
        pass


def _load() -> ctypes.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
        )
    _preload_torch()
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    check_single_hip_runtime()
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError = missing export: fail loudly
        if argtypes is not None:
            fn.argtypes = argtypes
        fn.restype = _RESTYPE.get(name, c_int)
    return lib


lib = _load()


# ---- libmgic_io.so (include/mgic_io.h): the HDF5 writers, loaded on first
# use (it links libhdf5); missing or unloadable = an ImportError, no fallback
IO_LIB_PATH = os.path.join(_HERE, "libmgic_io.so")
IO_SIGNATURES = {
    "mgic_io_last_error": [],
    "mgic_io_write_final_data": [c_char_p, c_int, PH, PD, c_int, PI],
    "mgic_io_write_solver_data": [c_char_p, c_int, PH, PH, PH, PD, PI, c_int],
    "mgic_io_write_final_data_phi": [c_char_p, c_int, PH, PH, PD, c_int, PI],
    "mgic_io_write_solver_data_phi": [c_char_p, c_int, PH, PH, PH, PH, PD, PI, c_int],
    "mgic_io_write_final_data_punct": [c_char_p, c_int, PH, PH, PD, c_int, PD, c_int, PI],
    "mgic_io_write_solver_data_punct": [c_char_p, c_int, PH, PH, PH, PH, PD, c_int, PD, PI, c_int],
    "mgic_io_write_final_data_matter": [c_char_p, c_int, PH, PH, PD, c_int, PD, PH, PD, c_int, PI],
    "mgic_io_write_final_data_constraints": [c_char_p, c_int, PH, PH, PD, c_int, PD, PH, PD, c_int,
                                             PI],
    "mgic_io_write_final_data_ctt": [c_char_p, c_int, PH, PH, PD, c_int, PD, PH, PD, PH, c_int,
                                     c_int, PI],
    "mgic_io_write_final_data_cttk": [c_char_p, c_int, PH, PH, PD, c_int, PD, PH, PD, PH, PH, PH,
                                      c_int, PI],
    "mgic_io_write_host": [c_char_p, c_int, c_int, PI, PI, PI, PD, PI, PD, c_int, c_int],
}
_io = None


def io_lib() -> ctypes.CDLL:
    global _io
    if _io is None:
        if not os.path.exists(IO_LIB_PATH):
            raise ImportError(f"{IO_LIB_PATH} not found: build it with __graft_entry__.build()")
        L = ctypes.CDLL(IO_LIB_PATH)
        for name, argtypes in IO_SIGNATURES.items():
            fn = getattr(L, name)
            fn.argtypes = argtypes
            fn.restype = c_char_p if name == "mgic_io_last_error" else c_int
        _io = L
    return _io


def io_call(name: str, *args) -> int:
    L = io_lib()
    st = getattr(L, name)(*args)
    if st < 0:
        msg = L.mgic_io_last_error()
        raise MgicError(name, st, msg.decode() if msg else "")
    return st


# ---- libmgic_ctt.so (include/mgic_ctt.h): the conformal transverse-traceless
# kernels of the momentum solve, loaded on first use (momentum.py); missing or
# unloadable = an ImportError, no fallback
CTT_LIB_PATH = os.path.join(_HERE, "libmgic_ctt.so")
CTT_SIGNATURES = {
    "mgic_ctt_last_error": [],
    "mgic_ctt_div_rhs": [H, PH, H],
    "mgic_ctt_w": [H, PH, H, PH],
    "mgic_ctt_lw": [H, PH, PH],
    "mgic_ctt_extrap": [H, H],
    "mgic_ctt_launch_ledger_dump": [c_char_p],
    "mgic_ctt_launch_ledger_reset": [],
}
_ctt = None


def ctt_lib() -> ctypes.CDLL:
    global _ctt
    if _ctt is None:
        if not os.path.exists(CTT_LIB_PATH):
            raise ImportError(f"{CTT_LIB_PATH} not found: build it with __graft_entry__.build()")
        L = ctypes.CDLL(CTT_LIB_PATH)
        for name, argtypes in CTT_SIGNATURES.items():
            fn = getattr(L, name)
            fn.argtypes = argtypes
            fn.restype = c_char_p if name == "mgic_ctt_last_error" else c_int
        _ctt = L
    return _ctt


def ctt_loaded() -> bool:
    """Whether libmgic_ctt.so has been loaded by this process."""
    return _ctt is not None


def ctt_call(name: str, *args) -> int:
    L = ctt_lib()
    st = getattr(L, name)(*args)
    if st < 0:
        msg = L.mgic_ctt_last_error()
        raise MgicError(name, st, msg.decode() if msg else "")
    return st


# ---- libmgic_zm.so (include/mgic_zm.h): the zero-mode kernel of a periodic
# level, loaded on first use (momentum.py, zero_mode="project"); missing or
# unloadable = an ImportError, no fallback
ZM_LIB_PATH = os.path.join(_HERE, "libmgic_zm.so")
ZM_SIGNATURES = {
    "mgic_zm_last_error": [],
    "mgic_zm_shift": [H, c_int, PH, PD],
    "mgic_zm_launch_ledger_dump": [c_char_p],
    "mgic_zm_launch_ledger_reset": [],
}
_zm = None


def zm_lib() -> ctypes.CDLL:
    global _zm
    if _zm is None:
        if not os.path.exists(ZM_LIB_PATH):
            raise ImportError(f"{ZM_LIB_PATH} not found: build it with __graft_entry__.build()")
        L = ctypes.CDLL(ZM_LIB_PATH)
        for name, argtypes in ZM_SIGNATURES.items():
            fn = getattr(L, name)
            fn.argtypes = argtypes
            fn.restype = c_char_p if name == "mgic_zm_last_error" else c_int
        _zm = L
    return _zm


def zm_loaded() -> bool:
    """Whether libmgic_zm.so has been loaded by this process."""
    return _zm is not None


def zm_call(name: str, *args) -> int:
    L = zm_lib()
    st = getattr(L, name)(*args)
    if st < 0:
        msg = L.mgic_zm_last_error()
        raise MgicError(name, st, msg.decode() if msg else "")
    return st


# ---- libmgic_reflux.so (include/mgic_reflux.h): the reflux kernel of the
# coarse-fine faces, loaded on first use (AMRSolver(..., reflux=True) with more
# than one level, AMRSolver.reflux) and registered with libmgic then; missing
# or unloadable = an ImportError, no fallback
REFLUX_LIB_PATH = os.path.join(_HERE, "libmgic_reflux.so")
REFLUX_SIGNATURES = {
    "mgic_reflux_last_error": [],
    "mgic_reflux_register": [],
    "mgic_reflux_launch_ledger_dump": [c_char_p],
    "mgic_reflux_launch_ledger_reset": [],
}
_reflux = None


def reflux_lib() -> ctypes.CDLL:
    global _reflux
    if _reflux is None:
        if not os.path.exists(REFLUX_LIB_PATH):
            raise ImportError(
                f"{REFLUX_LIB_PATH} not found: build it with __graft_entry__.build()")
        L = ctypes.CDLL(REFLUX_LIB_PATH)
        for name, argtypes in REFLUX_SIGNATURES.items():
            fn = getattr(L, name)
            fn.argtypes = argtypes
            fn.restype = c_char_p if name == "mgic_reflux_last_error" else c_int
        st = L.mgic_reflux_register()
        if st < 0:
            msg = L.mgic_reflux_last_error()
            raise MgicError("mgic_reflux_register", st, msg.decode() if msg else "")
        _reflux = L
    return _reflux


def reflux_loaded() -> bool:
    """Whether libmgic_reflux.so has been loaded by this process."""
    return _reflux is not None


def reflux_call(name: str, *args) -> int:
    L = reflux_lib()
    st = getattr(L, name)(*args)
    if st < 0:
        msg = L.mgic_reflux_last_error()
        raise MgicError(name, st, msg.decode() if msg else "")
    return st


# ---- libmgic_ptag.so (include/mgic_ptag.h): the periodic tagging kernel of
# set_grids, loaded on first use (grids.py, periodic_regrid on a base with a
# periodic direction); missing or unloadable = an ImportError, no fallback
PTAG_LIB_PATH = os.path.join(_HERE, "libmgic_ptag.so")
PTAG_SIGNATURES = {
    "mgic_ptag_last_error": [],
    "mgic_ptag_lattice": [H, H, c_double, c_int, c_int, PI, PI, c_void_p],
    "mgic_ptag_launch_ledger_dump": [c_char_p],
    "mgic_ptag_launch_ledger_reset": [],
}
_ptag = None


def ptag_lib() -> ctypes.CDLL:
    global _ptag
    if _ptag is None:
        if not os.path.exists(PTAG_LIB_PATH):
            raise ImportError(f"{PTAG_LIB_PATH} not found: build it with __graft_entry__.build()")
        L = ctypes.CDLL(PTAG_LIB_PATH)
        for name, argtypes in PTAG_SIGNATURES.items():
            fn = getattr(L, name)
            fn.argtypes = argtypes
            fn.restype = c_char_p if name == "mgic_ptag_last_error" else c_int
        _ptag = L
    return _ptag


def ptag_loaded() -> bool:
    """Whether libmgic_ptag.so has been loaded by this process."""
    return _ptag is not None


def ptag_call(name: str, *args) -> int:
    L = ptag_lib()
    st = getattr(L, name)(*args)
    if st < 0:
        msg = L.mgic_ptag_last_error()
        raise MgicError(name, st, msg.decode() if msg else "")
    return st


# ---- libmgic_adm.so (include/mgic_adm.h): the surface-charge kernels (ADM
# mass, momentum and spin on cubes of level 0), loaded on first use (adm.py);
# missing or unloadable = an ImportError, no fallback
ADM_LIB_PATH = os.path.join(_HERE, "libmgic_adm.so")
ADM_SIGNATURES = {
    "mgic_adm_last_error": [],
    "mgic_adm_surface_count": [c_int, PI, PLL],
    "mgic_adm_surface_terms": [H, H, c_int, PI, c_int, PD, PH, c_void_p, c_int],
    "mgic_adm_charges": [H, H, c_int, PI, c_int, PD, PH, PD],
    "mgic_adm_launch_ledger_dump": [c_char_p],
    "mgic_adm_launch_ledger_reset": [],
}
_adm = None


def adm_lib() -> ctypes.CDLL:
    global _adm
    if _adm is None:
        if not os.path.exists(ADM_LIB_PATH):
            raise ImportError(f"{ADM_LIB_PATH} not found: build it with __graft_entry__.build()")
        L = ctypes.CDLL(ADM_LIB_PATH)
        for name, argtypes in ADM_SIGNATURES.items():
            fn = getattr(L, name)
            fn.argtypes = argtypes
            fn.restype = c_char_p if name == "mgic_adm_last_error" else c_int
        _adm = L
    return _adm


def adm_loaded() -> bool:
    """Whether libmgic_adm.so has been loaded by this process."""
    return _adm is not None


def adm_call(name: str, *args) -> int:
    L = adm_lib()
    st = getattr(L, name)(*args)
    if st < 0:
        msg = L.mgic_adm_last_error()
        raise MgicError(name, st, msg.decode() if msg else "")
    return st


# ---- libmgic_sample.so (include/mgic_sample.h): the point-sampling kernel (a
# field of the hierarchy interpolated at points), loaded on first use
# (sample.py); missing or unloadable = an ImportError, no fallback
SAMPLE_LIB_PATH = os.path.join(_HERE, "libmgic_sample.so")
SAMPLE_SIGNATURES = {
    "mgic_sample_last_error": [],
    "mgic_sample_points": [H, c_int, PH, c_int, PD, c_int, PD, PI, PI],
    "mgic_sample_launch_ledger_dump": [c_char_p],
    "mgic_sample_launch_ledger_reset": [],
}
_sample = None


def sample_lib() -> ctypes.CDLL:
    global _sample
    if _sample is None:
        if not os.path.exists(SAMPLE_LIB_PATH):
            raise ImportError(
                f"{SAMPLE_LIB_PATH} not found: build it with __graft_entry__.build()")
        L = ctypes.CDLL(SAMPLE_LIB_PATH)
        for name, argtypes in SAMPLE_SIGNATURES.items():
            fn = getattr(L, name)
            fn.argtypes = argtypes
            fn.restype = c_char_p if name == "mgic_sample_last_error" else c_int
        _sample = L
    return _sample


def sample_loaded() -> bool:
    """Whether libmgic_sample.so has been loaded by this process."""
    return _sample is not None


def sample_call(name: str, *args) -> int:
    L = sample_lib()
    st = getattr(L, name)(*args)
    if st < 0:
        msg = L.mgic_sample_last_error()
        raise MgicError(name, st, msg.decode() if msg else "")
    return st


# ---- libmgic_horizon.so (include/mgic_horizon.h): the expansion kernel (psi,
# its gradient and Abar_ij n^i n^j at the points of a surface), loaded on first
# use (horizon.py); missing or unloadable = an ImportError, no fallback
HORIZON_LIB_PATH = os.path.join(_HERE, "libmgic_horizon.so")
HORIZON_SIGNATURES = {
    "mgic_horizon_last_error": [],
    "mgic_horizon_expansion": [H, c_int, PH, PH, c_int, PD, c_int, PD, PD, PD, PD, PI, PI],
    "mgic_horizon_launch_ledger_dump": [c_char_p],
    "mgic_horizon_launch_ledger_reset": [],
}
_horizon = None


def horizon_lib() -> ctypes.CDLL:
    global _horizon
    if _horizon is None:
        if not os.path.exists(HORIZON_LIB_PATH):
            raise ImportError(
                f"{HORIZON_LIB_PATH} not found: build it with __graft_entry__.build()")
        L = ctypes.CDLL(HORIZON_LIB_PATH)
        for name, argtypes in HORIZON_SIGNATURES.items():
            fn = getattr(L, name)
            fn.argtypes = argtypes
            fn.restype = c_char_p if name == "mgic_horizon_last_error" else c_int
        _horizon = L
    return _horizon


def horizon_loaded() -> bool:
    """Whether libmgic_horizon.so has been loaded by this process."""
    return _horizon is not None


def horizon_call(name: str, *args) -> int:
    L = horizon_lib()
    st = getattr(L, name)(*args)
    if st < 0:
        msg = L.mgic_horizon_last_error()
        raise MgicError(name, st, msg.decode() if msg else "")
    return st


# ---- libmgic_cttk.so (include/mgic_cttk.h): the K(x) kernels of the CTTK
# method, loaded on first use (cttk.py); missing or unloadable = an
# ImportError, no fallback
CTTK_LIB_PATH = os.path.join(_HERE, "libmgic_cttk.so")
CTTK_SIGNATURES = {
    "mgic_cttk_last_error": [],
    "mgic_cttk_K": [H, H, H, PLL],
    "mgic_cttk_source": [H, H, H, PH],
    "mgic_cttk_constraints": [H, H, H, PH, H],
    "mgic_cttk_launch_ledger_dump": [c_char_p],
    "mgic_cttk_launch_ledger_reset": [],
}
_cttk = None


def cttk_lib() -> ctypes.CDLL:
    global _cttk
    if _cttk is None:
        if not os.path.exists(CTTK_LIB_PATH):
            raise ImportError(f"{CTTK_LIB_PATH} not found: build it with __graft_entry__.build()")
        L = ctypes.CDLL(CTTK_LIB_PATH)
        for name, argtypes in CTTK_SIGNATURES.items():
            fn = getattr(L, name)
            fn.argtypes = argtypes
            fn.restype = c_char_p if name == "mgic_cttk_last_error" else c_int
        _cttk = L
    return _cttk


def cttk_loaded() -> bool:
    """Whether libmgic_cttk.so has been loaded by this process."""
    return _cttk is not None


def cttk_call(name: str, *args) -> int:
    L = cttk_lib()
    st = getattr(L, name)(*args)
    if st < 0:
        msg = L.mgic_cttk_last_error()
        raise MgicError(name, st, msg.decode() if msg else "")
    return st


# ---- libmgic_khyb.so (include/mgic_khyb.h): K(x) from the matter's energy,
# the hybrid CTTK choice, loaded on first use (khyb.py); missing or
# unloadable = an ImportError, no fallback
KHYB_LIB_PATH = os.path.join(_HERE, "libmgic_khyb.so")
KHYB_SIGNATURES = {
    "mgic_khyb_last_error": [],
    "mgic_khyb_K": [H, H, H, PD, c_double, H, PLL],
    "mgic_khyb_launch_ledger_dump": [c_char_p],
    "mgic_khyb_launch_ledger_reset": [],
}
_khyb = None


def khyb_lib() -> ctypes.CDLL:
    global _khyb
    if _khyb is None:
        if not os.path.exists(KHYB_LIB_PATH):
            raise ImportError(f"{KHYB_LIB_PATH} not found: build it with __graft_entry__.build()")
        L = ctypes.CDLL(KHYB_LIB_PATH)
        for name, argtypes in KHYB_SIGNATURES.items():
            fn = getattr(L, name)
            fn.argtypes = argtypes
            fn.restype = c_char_p if name == "mgic_khyb_last_error" else c_int
        _khyb = L
    return _khyb


def khyb_loaded() -> bool:
    """Whether libmgic_khyb.so has been loaded by this process."""
    return _khyb is not None


def khyb_call(name: str, *args) -> int:
    L = khyb_lib()
    st = getattr(L, name)(*args)
    if st < 0:
        msg = L.mgic_khyb_last_error()
        raise MgicError(name, st, msg.decode() if msg else "")
    return st


def last_error() -> str:
    msg = lib.mgic_last_error()
    return msg.decode() if msg else ""


def check(func: str, status: int) -> int:
    """Raise MgicError on a negative status; pass through 0 / 1."""
    if status < 0:
        raise MgicError(func, status, last_error())
    return status


def call(name: str, *args) -> int:
    return check(name, getattr(lib, name)(*args))
