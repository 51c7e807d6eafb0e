"""numpy restatement of the point-sampling rule of include/mgic_sample.h
(libmgic_sample.so), for tests/test_sample.py.  Test
infrastructure only.

Written as the rule reads, not as the kernel walks it: per point the level is
found, then every candidate stencil's cells are listed, all of them are checked
for availability, and only then the weighted sum is formed.  Python floats are
IEEE doubles and nothing is contracted, so following the header's expression
order gives the device's bits.
"""
import math

import numpy as np


class Hierarchy:
    """levels[l]: the boxes of level l as (lo, hi, array) with array[z, y, x]
    over the box's valid cells; n0: level 0's cells per direction (x, y, z);
    dx[l]: level l's spacing; periodic: per direction."""

    def __init__(self, n0, dx0, levels, periodic=(0, 0, 0), dx=None):
        self.n0 = tuple(int(v) for v in n0)
        self.levels = [[(tuple(lo), tuple(hi), np.asarray(arr)) for lo, hi, arr in boxes]
                       for boxes in levels]
        self.dx = [float(v) for v in dx] if dx is not None else \
            [float(dx0) / 2 ** l for l in range(len(levels))]
        self.periodic = tuple(int(p) for p in periodic)
        self.half = [self.n0[d] * self.dx[0] / 2.0 for d in range(3)]
        self.len = [self.n0[d] * self.dx[0] for d in range(3)]

    def cells(self, l):
        return tuple(n << l for n in self.n0)

    def box_of(self, l, c):
        """The box of level l that holds cell c (no wrap), or None."""
        for lo, hi, arr in self.levels[l]:
            if all(lo[d] <= c[d] <= hi[d] for d in range(3)):
                return lo, hi, arr
        return None

    def covered(self, l, c):
        """Whether cell c of level l lies in a box of level l + 1 coarsened by 2."""
        if l + 1 >= len(self.levels):
            return False
        for lo, hi, _ in self.levels[l + 1]:
            if all((lo[d] >> 1) <= c[d] <= (hi[d] >> 1) for d in range(3)):
                return True
        return False

    def wrapped(self, l, c):
        n = self.cells(l)
        return tuple(c[d] % n[d] if self.periodic[d] else c[d] for d in range(3))

    def available(self, l, c):
        c = self.wrapped(l, c)
        return self.box_of(l, c) is not None and not self.covered(l, c)

    def value(self, l, c):
        c = self.wrapped(l, c)
        lo, _, arr = self.box_of(l, c)
        return float(arr[c[2] - lo[2], c[1] - lo[1], c[0] - lo[0]])


def single_box(full, dx0, periodic=(0, 0, 0)):
    """One level, one box over the whole (nz, ny, nx) array."""
    nz, ny, nx = full.shape
    return Hierarchy((nx, ny, nz), dx0, [[((0, 0, 0), (nx - 1, ny - 1, nz - 1), full)]], periodic)


def weights4(t):
    tm1, tm2, tp1 = t - 1.0, t - 2.0, t + 1.0
    return [-t * tm1 * tm2 / 6.0, tp1 * tm1 * tm2 / 2.0, -tp1 * t * tm2 / 2.0, tp1 * t * tm1 / 6.0]


def weights2(t):
    return [1.0 - t, t]


def relative(h, x):
    """r_d of step 1, or None: the point is outside the domain."""
    if not all(math.isfinite(v) for v in x):
        return None
    r = []
    for d in range(3):
        v = x[d] + h.half[d]
        if h.periodic[d]:
            v = v - math.floor(v / h.len[d]) * h.len[d]
            if not (0.0 <= v < h.len[d]):
                v = 0.0
        elif not (0.0 <= v < h.len[d]):
            return None
        r.append(v)
    return r


def sample_one(h, x, order=4):
    """(value, level, order_used) of one point."""
    x = [float(v) for v in x]
    r = relative(h, x)
    if r is None:
        return float("nan"), -1, 0
    for l in reversed(range(len(h.levels))):
        q = [r[d] / h.dx[l] for d in range(3)]
        c = tuple(min(int(math.floor(q[d])), h.cells(l)[d] - 1) for d in range(3))
        if h.box_of(l, c) is None or h.covered(l, c):
            continue
        s = [v - 0.5 for v in q]
        i = [int(math.floor(v)) for v in s]
        t = [s[d] - math.floor(s[d]) for d in range(3)]
        candidates = []
        if order >= 4:
            candidates.append((4, [v - 1 for v in i], [weights4(v) for v in t]))
        if order >= 2:
            candidates.append((2, list(i), [weights2(v) for v in t]))
        for width, low, w in candidates:
            cells = [(low[0] + a, low[1] + b, low[2] + k)
                     for k in range(width) for b in range(width) for a in range(width)]
            if not all(h.available(l, cell) for cell in cells):
                continue
            value = None
            for k in range(width):
                plane = None
                for b in range(width):
                    row = None
                    for a in range(width):
                        p = w[0][a] * h.value(l, (low[0] + a, low[1] + b, low[2] + k))
                        row = p if row is None else row + p
                    p = w[1][b] * row
                    plane = p if plane is None else plane + p
                p = w[2][k] * plane
                value = p if value is None else value + p
            return value, l, width
        return h.value(l, c), l, 1
    return float("nan"), -1, 0


def sample(h, points, order=4):
    """(values, level, order_used) arrays for points (npts x 3)."""
    out = [sample_one(h, p, order) for p in np.asarray(points, dtype=np.float64).reshape(-1, 3)]
    return (np.array([o[0] for o in out], dtype=np.float64),
            np.array([o[1] for o in out], dtype=np.int32),
            np.array([o[2] for o in out], dtype=np.int32))


def abs_sum(h, x, order=4):
    """The sum of the absolute contributions |wz wy wx u| of the stencil the
    point takes (the scale its rounding error is measured against)."""
    x = [float(v) for v in x]
    _, l, used = sample_one(h, x, order)
    if used < 2:
        return 0.0
    r = relative(h, x)
    s = [r[d] / h.dx[l] - 0.5 for d in range(3)]
    i = [int(math.floor(v)) for v in s]
    t = [s[d] - math.floor(s[d]) for d in range(3)]
    low = [v - 1 for v in i] if used == 4 else i
    w = [(weights4 if used == 4 else weights2)(v) for v in t]
    return math.fsum(abs(w[0][a] * w[1][b] * w[2][k] * h.value(l, (low[0] + a, low[1] + b, low[2] + k)))
                     for k in range(used) for b in range(used) for a in range(used))


def same_bits(a, b):
    """Equal bit for bit, a NaN equal to a NaN (its payload is not part of the
    rule)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.int64), b[ok].view(np.int64))
