"""Python restatement of set_grids' pieces, for the tests.

Written from the reference's formulas (set_regrid_condition,
SetLevelData.cpp:190-240; set_tag_cells, SetGrids.cpp:172-207) and from the
clustering algorithm as DESIGN.md 3f states it -- not from csrc/regrid.cpp.
Boxes are (lo_x, lo_y, lo_z, hi_x, hi_y, hi_z), inclusive; arrays are indexed
[z, y, x].
"""
from __future__ import annotations

import math

import numpy as np


# ------------------------------------------------------------------ condition
def _eps(a, b, c):
    return {(0, 1, 2): 1.0, (1, 2, 0): 1.0, (2, 0, 1): 1.0,
            (0, 2, 1): -1.0, (2, 1, 0): -1.0, (1, 0, 2): -1.0}.get((a, b, c), 0.0)


def regrid_condition(bh, lo, hi, dx, psi=None):
    """set_regrid_condition on the box [lo, hi] at spacing dx, in the
    reference's expression order; psi None: psi = 1, else an array over the box."""
    L = bh["domain_length"]
    G = bh["G_Newton"]
    iz, iy, ix = np.meshgrid(np.arange(lo[2], hi[2] + 1), np.arange(lo[1], hi[1] + 1),
                             np.arange(lo[0], hi[0] + 1), indexing="ij")
    iv = [ix.astype(np.float64), iy.astype(np.float64), iz.astype(np.float64)]

    def loc(d, shift=0.0):
        return (iv[d] + shift + 0.5) * dx - L / 2.0

    def phi(x, y, z):
        r2 = x * x + y * y + z * z
        return bh["phi_amplitude"] * np.exp(-r2 / bh["phi_wavelength"])

    rho_grad = np.zeros_like(iv[0])
    for d0 in range(3):
        lp = [loc(d, 1.0 if d == d0 else 0.0) for d in range(3)]
        lm = [loc(d, -1.0 if d == d0 else 0.0) for d in range(3)]
        dphidx = 0.5 / dx * (phi(*lp) - phi(*lm))
        rho_grad = rho_grad + 0.5 * dphidx * dphidx
    x = [loc(0), loc(1), loc(2)]
    l1 = [x[0] - bh["bh1_offset"], x[1], x[2]]
    l2 = [x[0] - bh["bh2_offset"], x[1], x[2]]
    r1 = np.sqrt(l1[0] * l1[0] + l1[1] * l1[1] + l1[2] * l1[2])
    r2 = np.sqrt(l2[0] * l2[0] + l2[1] * l2[1] + l2[2] * l2[2])
    n1 = [c / r1 for c in l1]
    n2 = [c / r2 for c in l2]
    J1, J2 = [0.0, 0.0, bh["bh1_spin"]], [0.0, 0.0, bh["bh2_spin"]]
    P1, P2 = [0.0, bh["bh1_momentum"], 0.0], [0.0, bh["bh2_momentum"], 0.0]

    def A(i, j):  # SetBinaryBH.H:24-53
        kd = 1.0 if i == j else 0.0
        a = (1.5 / r1 / r1 * (n1[i] * P1[j] + n1[j] * P1[i]) +
             1.5 / r2 / r2 * (n2[i] * P2[j] + n2[j] * P2[i]))
        for k in range(3):
            a = a + (1.5 / r1 / r1 * (n1[i] * n1[j] - kd) * P1[k] * n1[k] +
                     1.5 / r2 / r2 * (n2[i] * n2[j] - kd) * P2[k] * n2[k])
            for l in range(3):
                a = a + (-3.0 / r1 / r1 / r1 * (_eps(i, l, k) * n1[j] + _eps(j, l, k) * n1[i]) *
                         n1[l] * J1[k] -
                         3.0 / r2 / r2 / r2 * (_eps(i, l, k) * n2[j] + _eps(j, l, k) * n2[i]) *
                         n2[l] * J2[k])
        return a

    A2 = (np.power(A(0, 0), 2.0) + np.power(A(1, 1), 2.0) + np.power(A(2, 2), 2.0) +
          2 * np.power(A(0, 1), 2.0) + 2 * np.power(A(0, 2), 2.0) + 2 * np.power(A(1, 2), 2.0))
    rho = 0.0
    m = (2.0 / 3.0) * (0.0 * 0.0) - 16.0 * math.pi * G * rho  # set_m_value(.., K = 0)
    psi_bh = bh["bh1_bare_mass"] / r1 + bh["bh2_bare_mass"] / r2
    psi_0 = (1.0 if psi is None else psi) + psi_bh
    return (1.5 * abs(m) + 1.5 * A2 * np.power(psi_0, -7.0) +
            24.0 * math.pi * G * np.abs(rho_grad) * np.power(psi_0, 1.0) + np.log(psi_0))


# ------------------------------------------------------------------ tagging
def lattice_bbox(boxes, domain, grow, c):
    """(lat_lo, lat_n) in lattice cells: the union of `boxes` grown by `grow`,
    clipped to the domain, rounded out to whole lattice cells of c level cells."""
    lo, n = [], []
    for d in range(3):
        a = max(min(b[d] for b in boxes) - grow, domain[d])
        z = min(max(b[3 + d] for b in boxes) + grow, domain[3 + d])
        lo.append(a // c)
        n.append(z // c - a // c + 1)
    return tuple(lo), tuple(n)


def tag_lattice(conds, boxes, domain, tag_val, grow, c, all_boxes=None):
    """set_tag_cells onto the lattice: conds[i] over boxes[i]; the bounding box
    is taken over all_boxes (default boxes).  Returns (lat_lo, mask[z, y, x])."""
    lat_lo, lat_n = lattice_bbox(all_boxes or boxes, domain, grow, c)
    mask = np.zeros(lat_n[::-1], dtype=np.uint8)
    for a, b in zip(conds, boxes):
        kk, jj, ii = np.nonzero(np.abs(a) >= tag_val)
        for k, j, i in zip(kk + b[2], jj + b[1], ii + b[0]):
            cell = (i, j, k)
            r = []
            for d in range(3):
                g0 = max(cell[d] - grow, domain[d])
                g1 = min(cell[d] + grow, domain[3 + d])
                r.append((g0 // c - lat_lo[d], g1 // c - lat_lo[d]))
            mask[r[2][0]:r[2][1] + 1, r[1][0]:r[1][1] + 1, r[0][0]:r[0][1] + 1] = 1
    return lat_lo, mask


# ------------------------------------------------------------------ clustering
def lattice_params(block_factor, max_grid_size):
    if block_factor < 1 or block_factor & (block_factor - 1):
        raise ValueError("block_factor must be a power of two")
    return max(block_factor // 2, 1), max(max_grid_size // block_factor, 1)


def split_max(q, maxlen):
    cuts = []
    for d in range(3):
        ln = q[3 + d] - q[d] + 1
        p = -(-ln // maxlen)
        sizes = [ln // p + (1 if i < ln % p else 0) for i in range(p)]
        at, cd = q[d], []
        for s in sizes:
            cd.append((at, at + s - 1))
            at += s
        cuts.append(cd)
    return [(x[0], y[0], z[0], x[1], y[1], z[1]) for z in cuts[2] for y in cuts[1] for x in cuts[0]]


def _cluster(m, q, fill_ratio, maxlen, out, pre, trace):
    sub = m[q[2]:q[5] + 1, q[1]:q[4] + 1, q[0]:q[3] + 1]
    if not sub.any():
        return
    zz, yy, xx = np.nonzero(sub)
    q = (q[0] + int(xx.min()), q[1] + int(yy.min()), q[2] + int(zz.min()),
         q[0] + int(xx.max()), q[1] + int(yy.max()), q[2] + int(zz.max()))
    sub = m[q[2]:q[5] + 1, q[1]:q[4] + 1, q[0]:q[3] + 1]
    n = int(np.count_nonzero(sub))
    ln = [q[3 + d] - q[d] + 1 for d in range(3)]
    vol = ln[0] * ln[1] * ln[2]
    if float(n) >= fill_ratio * float(vol) or vol == 1:
        pre.append(q)
        out.extend(split_max(q, maxlen))
        return
    s = (sub != 0).astype(np.int64)
    S = [s.sum(axis=(0, 1)), s.sum(axis=(0, 2)), s.sum(axis=(1, 2))]  # per x, y, z plane
    cut = None  # (direction, last index of the left piece, first index of the right piece)
    # (a) hole
    best = None
    for d in range(3):
        for i in range(1, ln[d] - 1):
            if S[d][i] == 0:
                key = (abs(2 * i + 1 - ln[d]), -ln[d], d, i)
                if best is None or key < best:
                    best = key
    if best is not None:
        d, i = best[2], best[3]
        cut = (d, i - 1, i + 1)
        trace.append("hole")
    else:
        # (b) inflection
        for d in range(3):
            if ln[d] < 4:
                continue
            lap = {i: int(S[d][i - 1]) - 2 * int(S[d][i]) + int(S[d][i + 1])
                   for i in range(1, ln[d] - 1)}
            for i in range(1, ln[d] - 2):
                if lap[i] * lap[i + 1] < 0:
                    key = (-abs(lap[i] - lap[i + 1]), abs(2 * (i + 1) - ln[d]), d, i)
                    if best is None or key < best:
                        best = key
        if best is not None:
            d, i = best[2], best[3]
            cut = (d, i, i + 1)
            trace.append("inflection")
        else:
            # (c) bisect
            d = max(range(3), key=lambda e: (ln[e], -e))
            cut = (d, ln[d] // 2 - 1, ln[d] // 2)
            trace.append("bisect")
    d, a, b = cut
    left, right = list(q), list(q)
    left[3 + d] = q[d] + a
    right[d] = q[d] + b
    _cluster(m, tuple(left), fill_ratio, maxlen, out, pre, trace)
    _cluster(m, tuple(right), fill_ratio, maxlen, out, pre, trace)


def cluster(mask, fill_ratio, maxlen, trace=None):
    """(boxes sorted by (lo_z, lo_y, lo_x), the accepted boxes before split_max);
    trace (a list) receives the kind of every cut taken, in order."""
    m = np.asarray(mask)
    out, pre = [], []
    if m.size:
        _cluster(m, (0, 0, 0, m.shape[2] - 1, m.shape[1] - 1, m.shape[0] - 1), fill_ratio, maxlen,
                 out, pre, [] if trace is None else trace)
    out.sort(key=lambda b: (b[2], b[1], b[0]))
    return out, pre


def regrid(domain0, tags, block_factor, max_grid_size, fill_ratio, nesting_radius=2):
    """tags[l] = (lat_lo, mask) for l = 0..top -> ([boxes of level 1..top+1], new_finest)."""
    c, maxlen = lattice_params(block_factor, max_grid_size)
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
            for f in boxes[l + 1]:  # level l + 2
                r = []
                for d in range(3):
                    a = max(f[d] // 2 - nesting_radius, doms[l + 1][d])
                    z = min(f[3 + d] // 2 + nesting_radius, doms[l + 1][3 + d])
                    r.append(range((a // 2) // c, (z // 2) // c + 1) if z >= a else range(0))
                cells.update((i, j, k) for k in r[2] for j in r[1] for i in r[0])
        if not cells:
            continue
        w = [min(p[d] for p in cells) for d in range(3)]
        n = [max(p[d] for p in cells) - w[d] + 1 for d in range(3)]
        m = np.zeros(n[::-1], dtype=np.uint8)
        for i, j, k in cells:
            m[k - w[2], j - w[1], i - w[0]] = 1
        lat, _ = cluster(m, fill_ratio, maxlen)
        boxes[l] = [tuple((b[d] + w[d]) * c * 2 for d in range(3)) +
                    tuple((b[3 + d] + w[d] + 1) * c * 2 - 1 for d in range(3)) for b in lat]
    new_finest = max([l + 1 for l in range(nlev) if boxes[l]], default=0)
    return boxes, new_finest


def owners(boxes, size):
    cells = [(b[3] - b[0] + 1) * (b[4] - b[1] + 1) * (b[5] - b[2] + 1) for b in boxes]
    total = sum(cells)
    out, prefix = [], 0
    for n in cells:
        out.append(size * (2 * prefix + n) // (2 * total))
        prefix += n
    return out


# ------------------------------------------------------------------ invariants
def box_cells(b):
    return (b[3] - b[0] + 1) * (b[4] - b[1] + 1) * (b[5] - b[2] + 1)


def disjoint(boxes):
    for i, a in enumerate(boxes):
        for b in boxes[i + 1:]:
            if all(a[d] <= b[3 + d] and b[d] <= a[3 + d] for d in range(3)):
                return False
    return True


def paint(boxes, shape):
    """Cover count per cell of a [z, y, x] array of `shape`."""
    m = np.zeros(shape, dtype=np.int32)
    for b in boxes:
        m[b[2]:b[5] + 1, b[1]:b[4] + 1, b[0]:b[3] + 1] += 1
    return m
