"""params.txt reader: the ParmParse keys the reference reads for this path.

Mirrors getPoissonParameters (Source/PoissonParameters.cpp:26-131) and the
solver knobs of Main_PoissonSolver.cpp:107-126, with the same defaults and
the same derived values (coarsestDx = L / N[0], domainLength = coarsestDx *
N, refRatio forced to 2, one periodicity flag for all directions).
"""
from __future__ import annotations

import math
import shlex
from dataclasses import dataclass, field
from typing import Dict, List, Optional


def parse_parmparse(text: str) -> Dict[str, List[str]]:
    """Parse ``key = v1 v2 ...`` lines; '#' starts a comment (ParmParse)."""
    out: Dict[str, List[str]] = {}
    for raw in text.splitlines():
        line = raw.split("#", 1)[0].strip()
        if not line or "=" not in line:
            continue
        key, val = line.split("=", 1)
        out[key.strip()] = shlex.split(val.strip())
    return out


# the values of momentum_zero_mode (poisson_solve's zero_mode)
ZERO_MODES = ("refuse", "project")


@dataclass
class PoissonParameters:
    alpha: float = 1.0
    beta: float = -1.0
    N: List[int] = field(default_factory=lambda: [64, 64, 64])
    L: float = 100.0
    max_level: int = 0
    coarsestDx: float = 100.0 / 64
    domainLength: List[float] = field(default_factory=lambda: [100.0] * 3)
    is_periodic: int = 0
    bc_lo: List[int] = field(default_factory=lambda: [0, 0, 0])
    bc_hi: List[int] = field(default_factory=lambda: [0, 0, 0])
    bc_value: float = 0.0
    coefficient_average_type: int = -1  # -1: factory default (arithmetic)
    numMGsmooth: int = 4
    numMGIterations: int = 1
    preCondSolverDepth: int = -1
    tolerance: float = 1.0e-7
    max_iterations: int = 10
    max_NL_iterations: int = 4
    max_grid_size: int = 16
    block_factor: int = 8
    refine_threshold: float = 0.1
    fill_ratio: float = 0.5
    buffer_size: int = 3  # read and unused, as in the reference
    verbosity: int = 3
    G_Newton: float = 1.0
    phi_amplitude: float = 0.0
    phi_wavelength: float = 1.0
    bh1_bare_mass: float = 0.0
    bh2_bare_mass: float = 0.0
    bh1_spin: float = 0.0
    bh2_spin: float = 0.0
    bh1_offset: float = 0.0
    bh2_offset: float = 0.0
    bh1_momentum: float = 0.0
    bh2_momentum: float = 0.0
    # the optional puncture table (num_punctures, puncture1 .. punctureN): rows
    # of m x y z Px Py Pz Jx Jy Jz (punctures.py); None: the two holes above
    punctures: Optional[list] = None
    # the optional matter keys (scalar_V0, scalar_mass, scalar_self_coupling,
    # pi_amplitude: a constant Pi; matter.py): the keys the deck gives, by
    # name; None: no matter
    matter: Optional[dict] = None
    # solve_momentum = 0|1 (not a key of the reference): 1 solves the momentum
    # constraint for the matter's Pi d_i phi source (momentum.py); absent: 0
    solve_momentum: int = 0
    # momentum_zero_mode = refuse|project (not a key of the reference): what the
    # momentum solve does on a periodic base, where its operator is singular;
    # project removes the mean of every right-hand side and solution
    # (momentum.py); absent: refuse.  It has no effect on a base that is not
    # periodic
    momentum_zero_mode: str = "refuse"
    # reflux = 0|1 (not a key of the reference): 1 adds the reflux term at the
    # coarse-fine faces to every multi-level operator of the solve (DESIGN.md
    # 3l), which makes the composite operator conservative; absent: 0.  It has
    # no effect on one level
    reflux: int = 0
    # regrid_periodic = 0|1 (not a key of the reference): 1 takes set_grids'
    # tags and proper nesting through the wrap of a periodic base (DESIGN.md
    # 3m); absent: 0.  It has no effect on a base that is not periodic
    regrid_periodic: int = 0
    # adm_half_widths = n1 n2 ... (not a key of the reference): the half-widths,
    # in level-0 cells, of the cubes on which the ADM mass, momentum and spin of
    # the solved data are reported (adm.py); 1 to 8 integers;
    # absent: None, nothing of it is loaded or launched
    adm_half_widths: Optional[List[int]] = None
    # puncture_masses = 0|1 (not a key of the reference): 1 reports psi at every
    # puncture and the ADM mass it gives (sample.py); absent: 0,
    # nothing of it is loaded or launched
    puncture_masses: int = 0
    # target_masses = T1 T2 ... (not a key of the reference): the ADM masses the
    # punctures are to have, one positive number per puncture in table order;
    # tools/run_poisson.py then iterates the bare masses (sample.solve_for_masses);
    # absent: None
    target_masses: Optional[List[float]] = None
    # num_horizons = n with horizon1 .. horizonN = cx cy cz r0, or horizons =
    # punctures (not keys of the reference): the apparent horizon about each
    # centre, from the sphere of radius r0, or about every puncture of the table
    # from r0 = m_i, is looked for in the solved data (horizon.py, DESIGN.md
    # 3p); a list of [cx, cy, cz, r0], or "punctures"; absent: None, nothing of
    # it is loaded or launched
    horizons: Optional[object] = None
    # cttk = 0|1 (not a key of the reference): 1 closes the constraints of a
    # periodic one-level deck by the CTTK method (cttk.py): psi is
    # chosen, K varies in space and the momentum constraint is solved with its
    # gradient as a source; tools/run_poisson.py then runs cttk_solve in place
    # of poisson_solve; absent: 0, nothing of it is loaded or launched.
    # cttk_tolerance: the loop stops at max|K - K_prev| <= tolerance * max|K|
    # (positive; absent: 1e-10); cttk_max_iterations: the momentum passes it
    # may take (at least 1; absent: 50)
    cttk: int = 0
    cttk_tolerance: float = 1.0e-10
    cttk_max_iterations: int = 50
    # hybrid_K = 0|1 (not a key of the reference): 1 solves a deck that is not
    # periodic by the hybrid CTTK method (khyb.py): K varies in
    # space so that the matter's energy drops out of the Hamiltonian
    # constraint, and the momentum constraint is solved with its gradient as a
    # source; absent: 0, nothing of it is loaded or launched
    hybrid_K: int = 0

    # what getPoissonParameters derives besides (PoissonParameters.cpp:68, :78-79,
    # :111-128): one more level than max_level, ratio 2 on every level, the
    # domain from the origin, one periodicity flag for every direction
    @property
    def numLevels(self) -> int:
        return self.max_level + 1

    @property
    def refRatio(self) -> List[int]:
        return [2] * self.numLevels

    @property
    def probLo(self) -> List[float]:
        return [0.0, 0.0, 0.0]

    @property
    def probHi(self) -> List[float]:
        return [0.0 + v for v in self.domainLength]

    @property
    def coarsestDomain(self) -> tuple:
        return (0, 0, 0) + tuple(n - 1 for n in self.N)

    @property
    def periodic(self) -> List[int]:
        return [self.is_periodic] * 3

    def bh(self, constant_K: float = 0.0) -> dict:
        """Inputs of set_a_coef / set_rhs (domain length of direction 0)."""
        return dict(domain_length=self.domainLength[0], G_Newton=self.G_Newton,
                    phi_amplitude=self.phi_amplitude, phi_wavelength=self.phi_wavelength,
                    bh1_bare_mass=self.bh1_bare_mass, bh2_bare_mass=self.bh2_bare_mass,
                    bh1_spin=self.bh1_spin, bh2_spin=self.bh2_spin, bh1_offset=self.bh1_offset,
                    bh2_offset=self.bh2_offset, bh1_momentum=self.bh1_momentum,
                    bh2_momentum=self.bh2_momentum, constant_K=constant_K)


def read_params(text: str, overrides: Optional[Dict[str, str]] = None) -> PoissonParameters:
    kv = parse_parmparse(text)
    for k, v in (overrides or {}).items():  # CLI overrides (Main_PoissonSolver.cpp:272)
        kv[k] = shlex.split(str(v))
    p = PoissonParameters()

    def get(key, conv, required=True):
        if key not in kv:
            if required:
                raise KeyError(f"ParmParse::get: key '{key}' not found")
            return None
        return conv(kv[key][0])

    p.alpha = get("alpha", float)
    p.beta = get("beta", float)
    for k in ("G_Newton", "phi_amplitude", "phi_wavelength", "bh1_bare_mass", "bh2_bare_mass",
              "bh1_spin", "bh2_spin", "bh1_offset", "bh2_offset", "bh1_momentum",
              "bh2_momentum"):
        setattr(p, k, get(k, float))
    v = get("verbosity", int, required=False)
    if v is not None:
        p.verbosity = v
    p.max_level = get("max_level", int)
    p.N = [int(x) for x in kv["N"][:3]]
    p.L = get("L", float)
    p.coarsestDx = p.L / p.N[0]                               # PoissonParameters.cpp:82
    p.domainLength = [p.coarsestDx * n for n in p.N]          # :83-85
    p.refine_threshold = get("refine_threshold", float)      # :88-92
    p.block_factor = get("block_factor", int)
    p.max_grid_size = get("max_grid_size", int)
    p.fill_ratio = get("fill_ratio", float)
    p.buffer_size = get("buffer_size", int)
    if "coefficient_average_type" in kv:                      # :97-108
        s = kv["coefficient_average_type"][0]
        if s == "arithmetic":
            p.coefficient_average_type = 0
        elif s == "harmonic":
            p.coefficient_average_type = 1
        else:
            raise ValueError("bad coefficient_average_type in input")
    p.is_periodic = get("is_periodic", int)                   # :119-128
    if "bc_lo" in kv:
        p.bc_lo = [int(x) for x in kv["bc_lo"][:3]]
    if "bc_hi" in kv:
        p.bc_hi = [int(x) for x in kv["bc_hi"][:3]]
    bv = get("bc_value", float, required=False)
    if bv is not None:
        p.bc_value = bv
    # solver knobs, Main_PoissonSolver.cpp:107-126 (query with defaults)
    for k, conv in (("numMGIterations", int), ("numMGsmooth", int), ("preCondSolverDepth", int),
                    ("tolerance", float), ("max_iterations", int), ("max_NL_iterations", int)):
        val = get(k, conv, required=False)
        if val is not None:
            setattr(p, k, val)
    # the puncture table (not a key of the reference): absent = nothing changes
    npunct = get("num_punctures", int, required=False)
    if npunct is not None:
        rows = []
        for i in range(1, npunct + 1):
            key = f"puncture{i}"
            if key not in kv:
                raise KeyError(f"ParmParse::get: key '{key}' not found")
            if len(kv[key]) != 10:
                raise ValueError(f"{key} needs ten numbers (m x y z Px Py Pz Jx Jy Jz), "
                                 f"got {len(kv[key])}")
            rows.append([float(x) for x in kv[key]])
        p.punctures = rows
    # the matter keys (not keys of the reference): absent = nothing changes
    matter = {k: get(k, float, required=False)
              for k in ("scalar_V0", "scalar_mass", "scalar_self_coupling", "pi_amplitude")}
    matter = {k: v for k, v in matter.items() if v is not None}
    if matter:
        p.matter = matter
    sm = get("solve_momentum", int, required=False)
    if sm is not None:
        if sm not in (0, 1):
            raise ValueError(f"solve_momentum must be 0 or 1, got {sm}")
        p.solve_momentum = sm
    zm = get("momentum_zero_mode", str, required=False)
    if zm is not None:
        if zm not in ZERO_MODES:
            raise ValueError(f"momentum_zero_mode must be refuse or project, got {zm!r}")
        p.momentum_zero_mode = zm
    rf = get("reflux", int, required=False)
    if rf is not None:
        if rf not in (0, 1):
            raise ValueError(f"reflux must be 0 or 1, got {rf}")
        p.reflux = rf
    rp = get("regrid_periodic", int, required=False)
    if rp is not None:
        if rp not in (0, 1):
            raise ValueError(f"regrid_periodic must be 0 or 1, got {rp}")
        p.regrid_periodic = rp
    if "adm_half_widths" in kv:
        try:
            hw = [int(x) for x in kv["adm_half_widths"]]
        except ValueError:
            raise ValueError(f"adm_half_widths must be integers, got {kv['adm_half_widths']}")
        if not 1 <= len(hw) <= 8 or min(hw) < 1:
            raise ValueError(f"adm_half_widths must be 1 to 8 integers >= 1, got {hw}")
        p.adm_half_widths = hw
    pm = get("puncture_masses", int, required=False)
    if pm is not None:
        if pm not in (0, 1):
            raise ValueError(f"puncture_masses must be 0 or 1, got {pm}")
        p.puncture_masses = pm
    if "target_masses" in kv:
        from .sample import check_target_count, parse_masses
        tm = parse_masses(kv["target_masses"], "target_masses")  # a ValueError of its own
        check_target_count(tm, len(p.punctures) if p.punctures is not None else 2, "target_masses")
        p.target_masses = tm
    nh = get("num_horizons", int, required=False)
    if "horizons" in kv:
        if kv["horizons"] != ["punctures"]:
            raise ValueError(f"horizons must be punctures, got {' '.join(kv['horizons'])!r}")
        if nh is not None:
            raise ValueError("horizons = punctures and num_horizons exclude each other")
        p.horizons = "punctures"
    elif nh is not None:
        from .horizon import parse_horizon
        if nh < 1:
            raise ValueError(f"num_horizons must be at least 1, got {nh}")
        rows = []
        for i in range(1, nh + 1):
            key = f"horizon{i}"
            if key not in kv:
                raise KeyError(f"ParmParse::get: key '{key}' not found")
            c, r0 = parse_horizon(kv[key], key)  # a ValueError of its own
            rows.append([c[0], c[1], c[2], r0])
        p.horizons = rows
    if p.horizons is not None and p.is_periodic:
        raise ValueError("horizons are not defined on a periodic domain (is_periodic = 1)")
    ck = get("cttk", int, required=False)
    if ck is not None:
        if ck not in (0, 1):
            raise ValueError(f"cttk must be 0 or 1, got {ck}")
        p.cttk = ck
    ct = get("cttk_tolerance", float, required=False)
    if ct is not None:
        if not (ct > 0.0 and math.isfinite(ct)):
            raise ValueError(f"cttk_tolerance must be a positive number, got {ct}")
        p.cttk_tolerance = ct
    cm = get("cttk_max_iterations", int, required=False)
    if cm is not None:
        if cm < 1:
            raise ValueError(f"cttk_max_iterations must be at least 1, got {cm}")
        p.cttk_max_iterations = cm
    hk = get("hybrid_K", int, required=False)
    if hk is not None:
        if hk not in (0, 1):
            raise ValueError(f"hybrid_K must be 0 or 1, got {hk}")
        p.hybrid_K = hk
    return p


def read_params_file(path: str, overrides: Optional[Dict[str, str]] = None) -> PoissonParameters:
    with open(path) as f:
        return read_params(f.read(), overrides)
