"""mg_ic_code_amd -- MI355X-native multigrid V-cycle for the
VariableCoeffPoissonOperator hot path of eugenealim/MG_IC_code.

The compute lives in libmgic.so (hand-written HIP kernels for gfx950 behind
the C ABI in include/mgic.h); this package is the host-side mirror of the
reference's operator / factory / solver interface (see core.py).
"""
from .core import (  # noqa: F401
    AMRMultiGrid,
    AMRSolver,
    BiCGStabSolver,
    Comm,
    Grid,
    LevelData,
    MgicError,
    MixedMultiGrid,
    MultilevelLinearOp,
    OperatorParams,
    SolverParams,
    VariableCoeffPoissonOperator,
    VariableCoeffPoissonOperatorFactory,
    bicgstab,
    bicgstab_on_device,
    defineOperatorFactory,
    device_synchronize,
    launch_ledger,
    launch_ledger_reset,
    prof_smoother,
    prof_smoother_read,
    set_binary_bh_coefs,
    set_nl_coefs,
    set_device,
)
from .adm import AdmReport, adm_charges, surface_terms  # noqa: F401
from .constraints import (  # noqa: F401
    ConstraintFields,
    ConstraintReport,
    constraint_vars,
    constraints,
    set_constraints,
)
from .cttk import CTTKError, CTTKResult, cttk_solve  # noqa: F401
from .grids import set_grids  # noqa: F401
from .khyb import HybridKError, set_K_from_matter  # noqa: F401
from .horizon import (  # noqa: F401
    ExpansionResult,
    HorizonResult,
    SurfaceBasis,
    expansion_points,
    find_horizon,
    horizons_of,
)
from ._lib import CTT_LIB_PATH, IO_LIB_PATH, LIB_PATH, lib  # noqa: F401
from .matter import Matter, PiProfile, ScalarPotential  # noqa: F401
from .momentum import (  # noqa: F401
    MomentumFields,
    fill_ghosts,
    momentum_source,
    set_longitudinal,
    solve_vector_potential,
)
from .output import output_final_data, output_solver_data  # noqa: F401
from .phi import PhiProfile  # noqa: F401
from .punctures import Puncture, PunctureSet  # noqa: F401
from .sample import (  # noqa: F401
    MassSolveResult,
    PunctureMassReport,
    SampleResult,
    lineout,
    puncture_masses,
    sample_points,
    solve_for_masses,
)

__version__ = "0.1.0"
