"""set_grids (Source/SetGrids.cpp:31-149): the AMR hierarchy from tagging.

The loop of SetGrids.cpp:61-138, on device where the work is O(cells):

    topLevel = 0
    repeat:
        per existing level:                                :80-106
            cond = set_regrid_condition at psi = 1         k_regrid_condition
        per existing level:                                set_tag_cells, :172-207
            tagVal = norm(cond, 0) * refine_threshold      the level's exact max norm
            tags   = |cond| >= tagVal, grown by 2, & domain
                                                           k_tag_lattice, onto the
                                                           clustering lattice
        new boxes = meshrefine.regrid(tags)                :113-114, regrid.cpp (host)
        topLevel += 1 if a finer level appeared            :116-118
        levels 1..topLevel rebuilt, LoadBalance            :123-132
    until topLevel == max_level or topLevel did not grow   :135-136

With periodic_regrid (the keyword, or the deck's regrid_periodic = 1) on a
base with a periodic direction the tags and the proper nesting go through the
wrap: the tag kernel is libmgic_ptag.so's k_ptag_lattice (one
launch per level) and the nesting mgic_regrid_levels_periodic's.  This departs
from the reference's local_tags &= domainBox (:201-202) on purpose.

Chombo's BRMeshRefine is not part of the reference tree; the clustering is
the Berger-Rigoutsos algorithm DESIGN.md 3f writes out, restated and not
pinned against Chombo's box lists.  The base level stays the caller's grid
(the reference's domainSplit of level 0 is out of scope).
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import call
from .core import BH_KEYS, Box6, Grid, LevelData, _ints, gloo_allgather
from .matter import (FilledMatter, MatterArgumentError, PiProfile, resolve_matter,
                     set_regrid_condition_matter)
from .params import PoissonParameters
from .phi import PhiArgumentError, PhiProfile, set_regrid_condition_phi
from .punctures import resolve_punctures, set_regrid_condition_punct

TAGS_GROW = 2        # SetGrids.cpp:109
NESTING_RADIUS = 2   # SetGrids.cpp:64


def set_regrid_condition(psi: Optional[LevelData], out: LevelData, bh: dict) -> None:
    """set_regrid_condition (SetLevelData.cpp:190-240) on device; psi None: psi = 1."""
    vals = (ctypes.c_double * 13)(*[float(bh[k]) for k in BH_KEYS])
    call("mgic_field_regrid_condition", psi.handle if psi is not None else None, out.handle, vals)


def regrid_lattice(block_factor: int, max_grid_size: int) -> Tuple[int, int]:
    """(c, maxlen): the lattice spacing in level cells and the longest box side
    in lattice cells."""
    c, m = ctypes.c_int(), ctypes.c_int()
    call("mgic_regrid_lattice", int(block_factor), int(max_grid_size), ctypes.byref(c),
         ctypes.byref(m))
    return c.value, m.value


def tag_lattice(cond: LevelData, tag_val: float, grow: int, c: int):
    """set_tag_cells of one level onto the clustering lattice: (lat_lo, mask),
    mask a uint8 array (nz, ny, nx) over lattice cells from lat_lo (x, y, z),
    set where this rank's tagged cells, grown and clipped to the domain, reach."""
    lo, n = (ctypes.c_int * 3)(), (ctypes.c_int * 3)()
    call("mgic_field_tag_lattice", cond.handle, ctypes.c_double(tag_val), int(grow), int(c), lo, n,
         None)
    mask = np.zeros((n[2], n[1], n[0]), dtype=np.uint8)
    call("mgic_field_tag_lattice", cond.handle, ctypes.c_double(tag_val), int(grow), int(c), lo, n,
         mask.ctypes.data_as(ctypes.c_void_p))
    return tuple(lo), mask


def tag_lattice_periodic(cond: LevelData, tag_val: float, grow: int, c: int):
    """tag_lattice through the wrap of the periodic directions of cond's grid
    (libmgic_ptag.so, one launch for every local box): in such a direction the
    lattice spans the domain and a tag's grown range is wrapped round it, not
    clipped.  Returns (lat_lo, mask) as tag_lattice does."""
    lo, n = (ctypes.c_int * 3)(), (ctypes.c_int * 3)()
    comm = cond.grid.comm.handle
    _lib.ptag_call("mgic_ptag_lattice", comm, cond.handle, ctypes.c_double(tag_val), int(grow),
                   int(c), lo, n, None)
    mask = np.zeros((n[2], n[1], n[0]), dtype=np.uint8)
    _lib.ptag_call("mgic_ptag_lattice", comm, cond.handle, ctypes.c_double(tag_val), int(grow),
                   int(c), lo, n, mask.ctypes.data_as(ctypes.c_void_p))
    return tuple(lo), mask


def ptag_launch_ledger() -> dict:
    """{kernel: launches so far in this process} of libmgic_ptag.so."""
    import os
    import tempfile

    from .core import read_launch_ledger
    fd, path = tempfile.mkstemp(prefix="mgic_ptag_ledger_")
    os.close(fd)
    try:
        _lib.ptag_call("mgic_ptag_launch_ledger_dump", path.encode())
        return read_launch_ledger(path)
    finally:
        os.unlink(path)


def resolve_periodic_regrid(periodic_regrid, prm) -> bool:
    """set_grids' periodic_regrid: None -- the deck's regrid_periodic (absent:
    0); True / False / 1 / 0; anything else is a ValueError."""
    if periodic_regrid is None:
        periodic_regrid = getattr(prm, "regrid_periodic", 0)
    if isinstance(periodic_regrid, bool) or (isinstance(periodic_regrid, int) and
                                             periodic_regrid in (0, 1)):
        return bool(periodic_regrid)
    raise ValueError(f"regrid_periodic must be 0 or 1 (False or True), got {periodic_regrid!r}")


def _boxes_out(flat, n: int) -> List[Box6]:
    return [tuple(int(v) for v in flat[6 * i:6 * i + 6]) for i in range(n)]


def regrid_cluster(mask: np.ndarray, fill_ratio: float, maxlen: int) -> List[Box6]:
    """Berger-Rigoutsos clustering of a (nz, ny, nx) mask into boxes in mask
    indices (x first), sorted by (lo_z, lo_y, lo_x)."""
    m = np.ascontiguousarray(mask, dtype=np.uint8)
    if m.ndim != 3:
        raise ValueError("mask must be (nz, ny, nx)")
    n = _ints(m.shape[::-1])
    buf = m.ctypes.data_as(ctypes.c_void_p) if m.size else ctypes.c_char_p(b"\0")
    nb = ctypes.c_int()
    call("mgic_regrid_cluster", buf, n, ctypes.c_double(fill_ratio), int(maxlen), 0,
         ctypes.byref(nb), None)
    out = (ctypes.c_int * (6 * max(nb.value, 1)))()
    call("mgic_regrid_cluster", buf, n, ctypes.c_double(fill_ratio), int(maxlen), nb.value,
         ctypes.byref(nb), out)
    return _boxes_out(out, nb.value)


def regrid_levels(domain0: Box6, tags: Sequence[Tuple[Sequence[int], np.ndarray]],
                  block_factor: int, max_grid_size: int, fill_ratio: float,
                  nesting_radius: int = NESTING_RADIUS,
                  periodic: Optional[Sequence[int]] = None) -> Tuple[List[List[Box6]], int]:
    """BRMeshRefine::regrid stand-in: tags[l] = (lat_lo, mask) of levels
    0..top -> ([boxes of level 1, ..., boxes of level top + 1], new_finest).
    periodic: None -- nesting regions are clipped to the domain
    (mgic_regrid_levels); else three flags, and in a flagged direction they are
    wrapped round it (mgic_regrid_levels_periodic)."""
    nlev = len(tags)
    masks = [np.ascontiguousarray(m, dtype=np.uint8) for _, m in tags]
    ptrs = (ctypes.c_void_p * nlev)(*[m.ctypes.data if m.size else None for m in masks])
    lo = _ints([v for l, _ in tags for v in l])
    n = _ints([v for m in masks for v in m.shape[::-1]])
    nb = (ctypes.c_int * nlev)()
    fin = ctypes.c_int()
    tail = (ptrs, lo, n, int(block_factor), int(max_grid_size), ctypes.c_double(fill_ratio),
            int(nesting_radius))
    if periodic is None:
        name, args = "mgic_regrid_levels", (nlev, _ints(domain0)) + tail
    else:
        if len(periodic) != 3:
            raise ValueError("periodic must be three flags")
        name = "mgic_regrid_levels_periodic"
        args = (nlev, _ints(domain0), _ints([1 if v else 0 for v in periodic])) + tail
    call(name, *args, 0, nb, None, ctypes.byref(fin))
    total = sum(nb)
    out = (ctypes.c_int * (6 * max(total, 1)))()
    call(name, *args, total, nb, out, ctypes.byref(fin))
    boxes, at = [], 0
    for l in range(nlev):
        boxes.append(_boxes_out(out[6 * at:6 * (at + nb[l])], nb[l]))
        at += nb[l]
    return boxes, fin.value


def regrid_owners(boxes: Sequence[Box6], size: int) -> List[int]:
    """LoadBalance stand-in over a sorted box list."""
    nb = len(boxes)
    if nb == 0:
        return []
    own = (ctypes.c_int * nb)()
    call("mgic_regrid_owners", nb, _ints([v for b in boxes for v in b]), int(size), own)
    return list(own)


def _level_max_norm(cond: LevelData) -> float:
    """norm(levelRhs, interval, 0) (SetGrids.cpp:184): the level's max norm over
    every rank, by the operators' exact level reduction."""
    out = ctypes.c_double()
    call("mgic_field_norm", cond.handle, 0, ctypes.byref(out))
    return out.value


def set_grids(comm, prm: PoissonParameters, base_grid: Grid, max_level: Optional[int] = None,
              allgather=None, phi0: Optional[PhiProfile] = None, punctures=None,
              matter=None, periodic_regrid=None) -> List[Grid]:
    """The hierarchy set_grids generates over `base_grid` (level 0, covering
    the domain): [base_grid, Grid(patches=True) of level 1, ...], at most
    max_level (default prm.max_level) levels above the base.  comm.size > 1:
    the ranks' tag masks are OR-ed through `allgather(bytes) -> [bytes per
    rank]` (default gloo_allgather()); every rank returns the same hierarchy.
    phi0: None -- the analytic Gaussian; else a PhiProfile, stored on every
    level of every pass (new levels appear, so pre-filled fields cannot be
    taken) and read by the stored-field regrid condition.
    punctures: None -- the deck's table (prm.punctures) if it has one, else the
    deck's two holes; else a punctures.PunctureSet, read by the table form of
    the regrid condition.
    matter: None -- the deck's (prm.matter) if it has one, else no matter; else
    a matter.Matter whose pi is None or a PiProfile (levels appear and must be
    filled, so pre-filled fields cannot be taken): rho enters the regrid
    condition through 1.5 |m|.
    periodic_regrid: True -- on a base with a periodic direction the tags and
    the proper nesting go through the wrap, so the hierarchy is
    one AMRSolver accepts on that base; on a base with no periodic direction it
    changes nothing and loads nothing.  None: the deck's regrid_periodic (0
    when absent); anything but True / False / 1 / 0 is a ValueError.  With
    more than one rank the lattice is the same on every rank (a periodic
    direction spans the domain), so the OR over the ranks is unchanged; that
    path is untested."""
    wrap = resolve_periodic_regrid(periodic_regrid, prm) and any(base_grid.periodic)
    if phi0 is not None and not isinstance(phi0, PhiProfile):
        raise PhiArgumentError("set_grids", "phi0 must be a PhiProfile (levels appear and must "
                               f"be filled), not {type(phi0).__name__}")
    punct = resolve_punctures(punctures, prm)
    mat = resolve_matter(matter, prm, "set_grids")
    if mat is not None and (isinstance(mat, FilledMatter) or
                            not (mat.pi is None or isinstance(mat.pi, PiProfile))):
        raise MatterArgumentError("set_grids", "matter.pi must be None or a PiProfile (levels "
                                  "appear and must be filled), not pre-filled fields")
    max_level = prm.max_level if max_level is None else int(max_level)
    c, _ = regrid_lattice(prm.block_factor, prm.max_grid_size)
    if comm.size > 1 and allgather is None:
        allgather = gloo_allgather()
    bh = prm.bh(constant_K=0.0)
    grids: List[Grid] = [base_grid]
    top = 0
    more = max_level > 0
    while more:
        more = False
        old_top = top
        tags = []
        for g in grids:
            cond = LevelData(g)
            if mat is not None:
                set_regrid_condition_matter(
                    None, cond, bh, mat.potential,
                    mat.pi.fill(g, bh) if mat.pi is not None else None, punct,
                    phi0.fill(g, bh) if phi0 is not None else None)
            elif punct is not None:
                set_regrid_condition_punct(None, cond, bh, punct,
                                           phi=phi0.fill(g, bh) if phi0 is not None else None)
            elif phi0 is None:
                set_regrid_condition(None, cond, bh)
            else:
                set_regrid_condition_phi(None, phi0.fill(g, bh), cond, bh)
            tag_val = _level_max_norm(cond) * prm.refine_threshold
            if wrap:
                lat_lo, mask = tag_lattice_periodic(cond, tag_val, TAGS_GROW, c)
            else:
                lat_lo, mask = tag_lattice(cond, tag_val, TAGS_GROW, c)
            if comm.size > 1:
                parts = allgather(mask.tobytes())
                for p in parts:
                    mask |= np.frombuffer(p, dtype=np.uint8).reshape(mask.shape)
            tags.append((lat_lo, mask))
        boxes, new_finest = regrid_levels(base_grid.domain, tags, prm.block_factor,
                                          prm.max_grid_size, prm.fill_ratio,
                                          periodic=base_grid.periodic if wrap else None)
        if new_finest > top:
            top += 1
        elif new_finest < top:
            # not in the reference, whose topLevel never falls (:116-118): there a
            # level that lost all its tags becomes an empty layout; a Grid here
            # needs a box, so the hierarchy ends below it (and the loop stops)
            top = new_finest
        new = [base_grid]
        dom, dx = base_grid.domain, base_grid.dx
        for lev in range(1, top + 1):
            dom = tuple(2 * v for v in dom[:3]) + tuple(2 * v + 1 for v in dom[3:])
            dx = dx / 2
            bl = boxes[lev - 1]
            new.append(Grid(comm, dom, bl, dx, periodic=base_grid.periodic,
                            owners=regrid_owners(bl, comm.size), patches=True))
        grids = new
        if top < max_level and top > old_top:
            more = True
    return grids
