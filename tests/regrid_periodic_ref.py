"""Python restatement of the periodic-aware pieces of set_grids (DESIGN.md
3m), for the tests: tagging and proper nesting through the wrap.

Written from the rules of DESIGN.md 3m on top of tests/regrid_ref.py's
`cluster` -- not from csrc/ptag.hip or csrc/regrid.cpp.  Boxes are
(lo_x, lo_y, lo_z, hi_x, hi_y, hi_z), inclusive; arrays are indexed [z, y, x].

In a periodic direction d of a level whose domain has n_d cells
  * the clustering lattice spans the domain: lat_lo = dom_lo / c, lat_n = n_d / c;
  * a tagged cell's grown range [i - grow, i + grow] is not clipped: every
    index of it is taken modulo n_d into the domain;
  * the nesting region coarsen(box of level l + 2, 2) +- nesting_radius is not
    clipped: every index of it is taken modulo the level-(l + 1) domain before
    it is coarsened onto level l's lattice.
A non-periodic direction is regrid_ref's: clipped to the domain.
"""
from __future__ import annotations

import numpy as np

from tests import regrid_ref as R


def _wrap(v, lo, n):
    return lo + (v - lo) % n


def lattice_bbox_wrap(boxes, domain, periodic, grow, c):
    """(lat_lo, lat_n): regrid_ref.lattice_bbox in a non-periodic direction,
    the whole domain in a periodic one."""
    lo, n = R.lattice_bbox(boxes, domain, grow, c)
    lo, n = list(lo), list(n)
    for d in range(3):
        if periodic[d]:
            nd = domain[3 + d] - domain[d] + 1
            if domain[d] % c or nd % c:
                raise ValueError("domain is not a multiple of the lattice spacing")
            lo[d], n[d] = domain[d] // c, nd // c
    return tuple(lo), tuple(n)


def _reach(i, d, domain, periodic, grow, c, lat_lo):
    """Lattice indices (relative to lat_lo) that cell index i of direction d,
    grown by `grow`, sets."""
    if periodic[d]:
        nd = domain[3 + d] - domain[d] + 1
        return sorted({_wrap(v, domain[d], nd) // c - lat_lo[d]
                       for v in range(i - grow, i + grow + 1)})
    g0 = max(i - grow, domain[d])
    g1 = min(i + grow, domain[3 + d])
    return list(range(g0 // c - lat_lo[d], g1 // c - lat_lo[d] + 1))


def tag_lattice_wrap(conds, boxes, domain, periodic, tag_val, grow, c, all_boxes=None):
    """set_tag_cells onto the lattice with the wrap: conds[i] over boxes[i];
    the bounding box is taken over all_boxes (default boxes).  Returns
    (lat_lo, mask[z, y, x])."""
    lat_lo, lat_n = lattice_bbox_wrap(all_boxes or boxes, domain, periodic, grow, c)
    mask = np.zeros(lat_n[::-1], dtype=np.uint8)
    for a, b in zip(conds, boxes):
        with np.errstate(invalid="ignore"):
            kk, jj, ii = np.nonzero(np.abs(a) >= tag_val)  # NaN >= x is false
        for k, j, i in zip(kk + b[2], jj + b[1], ii + b[0]):
            r = [_reach(int(v), d, domain, periodic, grow, c, lat_lo)
                 for d, v in enumerate((i, j, k))]
            mask[np.ix_(r[2], r[1], r[0])] = 1
    return lat_lo, mask


def regrid_wrap(domain0, periodic, tags, block_factor, max_grid_size, fill_ratio,
                nesting_radius=2):
    """regrid_ref.regrid with the nesting region wrapped in the periodic
    directions: tags[l] = (lat_lo, mask) for l = 0..top ->
    ([boxes of level 1..top+1], new_finest)."""
    c, maxlen = R.lattice_params(block_factor, max_grid_size)
    nlev = len(tags)
    doms = [tuple(domain0)]
    for _ in range(nlev):
        p = doms[-1]
        doms.append(tuple(2 * v for v in p[:3]) + tuple(2 * v + 1 for v in p[3:]))
    for l in range(nlev):
        for d in range(3):
            if doms[l][d] % c or (doms[l][3 + d] + 1) % c:
                raise ValueError("domain is not a multiple of the lattice spacing")
    boxes = [[] for _ in range(nlev)]  # boxes[l]: level l + 1
    for l in range(nlev - 1, -1, -1):
        cells = set()  # set lattice cells of level l, global lattice indices
        lat_lo, mask = tags[l]
        for k, j, i in zip(*np.nonzero(np.asarray(mask))):
            cells.add((int(i) + lat_lo[0], int(j) + lat_lo[1], int(k) + lat_lo[2]))
        if l + 1 < nlev:
            dom = doms[l + 1]
            for f in boxes[l + 1]:  # level l + 2
                r = []
                for d in range(3):
                    a, z = f[d] // 2 - nesting_radius, f[3 + d] // 2 + nesting_radius
                    if periodic[d]:
                        nd = dom[3 + d] - dom[d] + 1
                        r.append(sorted({(_wrap(v, dom[d], nd) // 2) // c
                                         for v in range(a, z + 1)}))
                    else:
                        a, z = max(a, dom[d]), min(z, dom[3 + d])
                        r.append(list(range((a // 2) // c, (z // 2) // c + 1)) if z >= a else [])
                cells.update((i, j, k) for k in r[2] for j in r[1] for i in r[0])
        if not cells:
            continue
        w = [min(p[d] for p in cells) for d in range(3)]
        n = [max(p[d] for p in cells) - w[d] + 1 for d in range(3)]
        m = np.zeros(n[::-1], dtype=np.uint8)
        for i, j, k in cells:
            m[k - w[2], j - w[1], i - w[0]] = 1
        lat, _ = R.cluster(m, fill_ratio, maxlen)
        boxes[l] = [tuple((b[d] + w[d]) * c * 2 for d in range(3)) +
                    tuple((b[3 + d] + w[d] + 1) * c * 2 - 1 for d in range(3)) for b in lat]
    new_finest = max([l + 1 for l in range(nlev) if boxes[l]], default=0)
    return boxes, new_finest


def set_grids_wrap(prm, n0, periodic, max_level=2, grow=2):
    """The restatement's set_grids on an n0^3 base with the wrap: per pass the
    level conditions (psi = 1), tagVal margins and boxes.  Returns
    dict(levels, margins), margins keyed by (pass, level)."""
    bh = prm.bh()
    c, _ = R.lattice_params(prm.block_factor, prm.max_grid_size)
    dom0 = (0, 0, 0, n0 - 1, n0 - 1, n0 - 1)
    levels = [[dom0]]
    top, margins, npass = 0, {}, 0
    more = max_level > 0
    while more:
        more = False
        old_top = top
        tags = []
        dom, dx = dom0, prm.L / n0
        for l, boxes in enumerate(levels):
            conds = [R.regrid_condition(bh, b[:3], b[3:], dx) for b in boxes]
            tag_val = max(np.abs(a).max() for a in conds) * prm.refine_threshold
            margins[(npass, l)] = min(np.abs(np.abs(a) / tag_val - 1.0).min() for a in conds)
            tags.append(tag_lattice_wrap(conds, boxes, dom, periodic, tag_val, grow, c))
            dom = tuple(2 * v for v in dom[:3]) + tuple(2 * v + 1 for v in dom[3:])
            dx /= 2
        new, fin = regrid_wrap(dom0, periodic, tags, prm.block_factor, prm.max_grid_size,
                               prm.fill_ratio)
        if fin > top:
            top += 1
        elif fin < top:
            top = fin
        levels = [[dom0]] + new[:top]
        npass += 1
        if top < max_level and top > old_top:
            more = True
    return dict(levels=levels, margins=margins)
