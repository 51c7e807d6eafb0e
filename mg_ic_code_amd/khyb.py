"""Hybrid CTTK: K(x) from the matter's energy, for decks with holes.

`matter=` puts rho = Pi^2/2 + V(phi_0) into m = (2/3) K^2 - 16 pi G rho.  On an
asymptotically flat deck K = 0, so aCoef gains +10 pi G rho psi_0^4, the wrong
sign for the operator Lap + aCoef, and the NL loop diverges for all but tiny
potentials (matter.py).  The hybrid CTTK method (Aurrekoetxea,
Clough & Lim) chooses K cell by cell so that m vanishes,

    (2/3) K(x)^2 = 16 pi G rho(x),   K = -sqrt(24 pi G (Pi_0^2 / 2 + V(phi_0)))

The psi equation then keeps only A2 and the gradient energy -- the equation
the deck solves without matter -- and the momentum constraint gains
(2/3) psi^6 D_i K, which cttk.py's k_cttk_source adds to the momentum solve's
source and its k_cttk_constraints to the report.  K does not depend on psi, so
it is evaluated once, before the NL loop:

    1. K_l on the valid cells of every level              (k_khyb_K)
    2. its ghost layer 1: momentum.fill_ghosts            (cf_interp, exchange,
                                                           linear extrapolation)
    3. every NL iteration: the momentum step with the extra source, then the
       coefficients with a zero potential, no Pi_0 and constant_K = 0

A cell with rho < 0 (a negative potential outweighing Pi^2/2) has no real K:
HybridKError names the count and the level.

The coupling psi^6 D_i K -> LW -> A2 -> psi is a fixed point, not Newton: it
converges at a linear rate that worsens with the amplitude and diverges for
large ones (DESIGN.md 3r has the figures).

The kernel is libmgic_khyb.so's (include/mgic_khyb.h), loaded on first use;
`poisson_solve` without `hybrid_K` never loads it.

    set_K_from_matter(phi, pi, potential, G, K) -> bad    the kernel, one level
    HybridK                                               K over a hierarchy
    khyb_launch_ledger()                                  the library's ledger
"""
from __future__ import annotations

import ctypes
import os
from typing import List, Optional, Sequence

from ._lib import khyb_call
from .core import Grid, LevelData
from .matter import FilledMatter, ScalarPotential, _pot


class HybridKError(RuntimeError):
    """rho = Pi^2/2 + V(phi_0) is negative (or NaN) somewhere: no real K
    cancels it in the Hamiltonian constraint."""

    def __init__(self, bad_cells: int, level: int):
        super().__init__(f"hybrid_K: rho < 0 in {bad_cells} cells of level {level}: a negative "
                         "potential outweighs Pi^2/2 there, and no real K cancels it")
        self.bad_cells = bad_cells
        self.level = level


def set_K_from_matter(phi: LevelData, pi: Optional[LevelData], potential: ScalarPotential,
                      G: float, K: LevelData) -> int:
    """K = -sqrt(24 pi G (Pi^2/2 + V(phi))) on the valid cells (k_khyb_K); pi
    None: Pi = 0.  A cell whose radicand is negative or NaN gets K = 0 and is
    counted.  Returns the count."""
    bad = ctypes.c_longlong(0)
    khyb_call("mgic_khyb_K", phi.grid.comm.handle, phi.handle,
              pi.handle if pi is not None else None, _pot(potential).pot(), float(G), K.handle,
              ctypes.byref(bad))
    return int(bad.value)


def khyb_launch_ledger() -> dict:
    """{kernel: launches so far in this process} of libmgic_khyb.so."""
    import tempfile

    from .core import read_launch_ledger
    fd, path = tempfile.mkstemp(prefix="mgic_khyb_ledger_")
    os.close(fd)
    try:
        khyb_call("mgic_khyb_launch_ledger_dump", path.encode())
        return read_launch_ledger(path)
    finally:
        os.unlink(path)


def resolve_hybrid_K(hybrid_K, prm) -> bool:
    """poisson_solve's hybrid_K: None -- the deck's hybrid_K (absent: 0); True /
    False / 1 / 0; anything else is a ValueError."""
    if hybrid_K is None:
        hybrid_K = getattr(prm, "hybrid_K", 0)
    if isinstance(hybrid_K, bool) or (isinstance(hybrid_K, int) and hybrid_K in (0, 1)):
        return bool(hybrid_K)
    raise ValueError(f"hybrid_K must be 0 or 1 (False or True), got {hybrid_K!r}")


def check_hybrid_request(prm, mat, momentum, adm, horizons, func: str = "poisson_solve") -> None:
    """The refusals of hybrid_K, raised before anything is stored, loaded or
    launched.  mat: the resolved matter; momentum, adm, horizons: the caller's
    arguments after the deck's defaults (momentum None: not given)."""
    from .momentum import check_momentum_request
    if prm.is_periodic:
        raise ValueError("hybrid_K on a periodic deck is not supported: cttk_solve is the "
                         "periodic path (K from the whole Hamiltonian constraint at a chosen psi)")
    check_momentum_request(mat, False, func)
    if momentum is not None and not momentum:
        raise ValueError("hybrid_K needs the momentum solve: (2/3) psi^6 D_i K is a source of "
                         "the momentum constraint, and momentum=False leaves it unsolved")
    if adm is not None:
        raise ValueError("hybrid_K with adm is not supported: the surface integrals assume K = 0")
    if horizons is not None:
        raise ValueError("hybrid_K with horizons is not supported: the expansion assumes K = 0")


class HybridK:
    """K of the hybrid method on a hierarchy (one level: a list of one Grid):
    evaluated from the stored phi_0 and the filled matter on construction
    (HybridKError on a cell without a real K), ghost layer 1 filled with `amr`
    (the momentum solver's AMRSolver; None on one level)."""

    def __init__(self, grids: Sequence[Grid], mat: FilledMatter, phis: Sequence[LevelData],
                 G: float, amr=None):
        from .momentum import fill_ghosts
        self.K: List[LevelData] = [LevelData(g) for g in grids]
        for l, K in enumerate(self.K):
            K.set_zero()
            bad = set_K_from_matter(phis[l], mat.level(l), mat.potential, G, K)
            if bad > 0:
                raise HybridKError(bad, l)
        fill_ghosts(self.K, amr)
        # what the coefficients read in place of the matter: m is then the
        # literal zero, not a cancellation
        self.no_matter = FilledMatter(ScalarPotential(), None)

    def source(self, psi: Sequence[LevelData]):
        """solve_vector_potential's add_source: S_i += (2/3) psi^6 D_i K."""
        from .cttk import add_source

        def add(level: int, S) -> None:
            add_source(psi[level], self.K[level], S)
        return add

    def correct(self, level: int, fields) -> None:
        """constraints()'s correct: the terms of K on top of the fields at
        constant_K = 0."""
        from .cttk import correct_constraints
        correct_constraints(self.K[level], fields)


def write_final_data(filename: str, psi: Sequence[LevelData], K: Sequence[LevelData], bh: dict,
                     mat: FilledMatter, momentum, phi: Sequence[LevelData], punctures=None,
                     constraint_fields=None, max_level: int = 0,
                     ref_ratio: Optional[Sequence[int]] = None) -> None:
    """The final data of every level with K from the field
    (mgic_io_write_final_data_cttk): what output_final_data(momentum=) writes
    at constant_K = 0, component "K" from K[l] and, with constraint_fields (the
    corrected ConstraintFields per level), components 27-30 from them."""
    from ._lib import io_call
    from .matter import table_or_null
    from .momentum import handles
    from .output import _bh
    n = len(psi)
    rr = list(ref_ratio) if ref_ratio is not None else [2] * n
    cons = None
    if constraint_fields is not None:
        cons = handles([f for lev in constraint_fields for f in lev.fields()])
    io_call("mgic_io_write_final_data_cttk", filename.encode(), n, handles(psi), handles(phi),
            _bh(bh), *table_or_null(punctures),
            handles(mat.pi) if mat.pi is not None else None, mat.potential.pot(),
            handles([f for l in range(n) for f in momentum.lw(l)]), handles(K), cons,
            int(max_level), (ctypes.c_int * n)(*rr))
