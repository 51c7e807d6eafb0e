"""Reference side of the surface-charge tests (tests/test_adm.py): the
definitions of mg_ic_code_amd/adm.py restated in numpy, with get_Aij
(SetBinaryBH.H:24-53) written as its loops -- not from csrc/adm.hip, which
uses the vector form.  Test infrastructure only.

Level 0 has N = (Nx, Ny, Nz) cells (even), spacing dx, cell centres at
(iv + 0.5) dx - N_d dx / 2.  The surface of half-width n is the cube of cells
[N_d/2 - n, N_d/2 + n): 6 sides, side = 2 d + (s > 0), each (2n)^2 faces
(b, a), a and b along the two directions other than d in increasing order.
Fields are (nz, ny, nx) arrays over the whole domain.

`terms` works in the dtype it is given (float64 or longdouble), and also
returns each term's sum of absolute contributions, the scale the rounding
bars are relative to.  `tree_sum` is the library's reduction order: 64 faces
by a butterfly (32, 16, .. 1), 4 waves in order, blocks of 256 in order, the
tail padded with +0.0.
"""
import math

import numpy as np

IJ = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))  # 11 12 13 22 23 33
BLOCK, WAVE = 256, 64

# the issue's table: m, x, y, z, Px, Py, Pz, Jx, Jy, Jz
TWO_HOLES = ((0.5, 2.0, 0.3, -0.4, 0.05, 0.02, -0.03, 0.01, -0.02, 0.1),
             (0.4, -1.5, -0.2, 0.6, -0.01, 0.04, 0.02, 0.03, 0.0, -0.05))
THREE_HOLES = TWO_HOLES + ((0.3, 0.4, 1.1, 0.7, 0.02, -0.03, 0.01, -0.02, 0.04, 0.03),)


def completed(table):
    t = np.asarray(table, dtype=np.float64).reshape(-1, 10)
    if len(t) % 2:
        pad = np.zeros(10)
        pad[1:4] = t[-1, 1:4]
        t = np.vstack([t, pad])
    return t


def expected(table):
    """(2 sum m, sum P, sum (J + x x P)) in float64."""
    t = np.asarray(table, dtype=np.float64).reshape(-1, 10)
    return (2.0 * t[:, 0].sum(), t[:, 4:7].sum(axis=0),
            (t[:, 7:10] + np.cross(t[:, 1:4], t[:, 4:7])).sum(axis=0))


_EPS = np.zeros((3, 3, 3))
_EPS[0, 1, 2] = _EPS[1, 2, 0] = _EPS[2, 0, 1] = 1.0
_EPS[0, 2, 1] = _EPS[2, 1, 0] = _EPS[1, 0, 2] = -1.0


def _hole_Aij(i, j, r, n, J, P, mag):
    """One hole's part of get_Aij, the loops as written; mag: |.| of every
    additive contribution instead."""
    f = np.abs if mag else (lambda v: v)
    A = f(1.5 / r / r * (n[i] * P[j])) + f(1.5 / r / r * (n[j] * P[i]))
    for k in range(3):
        A = A + f(1.5 / r / r * (n[i] * n[j]) * P[k] * n[k])
        if i == j:
            A = A + f(-1.5 / r / r * P[k] * n[k])
        for l in range(3):
            if _EPS[i, l, k] != 0.0:
                A = A + f(-3.0 / r / r / r * _EPS[i, l, k] * n[j] * n[l] * J[k])
            if _EPS[j, l, k] != 0.0:
                A = A + f(-3.0 / r / r / r * _EPS[j, l, k] * n[i] * n[l] * J[k])
    return A


def side_geometry(N, n, dx, side, dtype=np.float64):
    """(d, s, in, out, x_f): the index arrays (iz, iy, ix) of the inner and
    outer cells and the face centres (x, y, z), all of shape (2n, 2n) = (b, a)."""
    d, s = side // 2, (1 if side % 2 else -1)
    c = [N[e] // 2 for e in range(3)]
    w = 2 * n
    da, db = [e for e in range(3) if e != d]
    fa = np.arange(w)[None, :] + np.zeros((w, 1), dtype=int)
    fb = np.arange(w)[:, None] + np.zeros((1, w), dtype=int)
    m = c[d] + n if s > 0 else c[d] - n
    cell = [None] * 3
    cell[d] = np.full((w, w), m - 1 if s > 0 else m)
    cell[da] = c[da] - n + fa
    cell[db] = c[db] - n + fb
    out = [v.copy() for v in cell]
    out[d] = out[d] + s
    dxx = dtype(dx)
    x = []
    for e in range(3):
        domlen = dtype(N[e]) * dxx
        idx = np.full((w, w), m).astype(dtype) if e == d else cell[e].astype(dtype) + dtype(0.5)
        x.append(idx * dxx - domlen / dtype(2.0))
    return d, s, tuple(cell[::-1]), tuple(out[::-1]), x


def bowen_york(table, x, d, dtype=np.float64, mag=False):
    """(A_0d, A_1d, A_2d, sum_n m l_d / r^3) at the points x, summed over the
    pairs in pair order; mag: the sums of absolute contributions."""
    t = completed(table).astype(dtype)
    A, dps = None, None
    for q in range(len(t) // 2):
        e = [0, 0, 0]
        ed = 0
        for row in (t[2 * q], t[2 * q + 1]):
            l = [x[0] - row[1], x[1] - row[2], x[2] - row[3]]
            r = np.sqrt(l[0] * l[0] + l[1] * l[1] + l[2] * l[2])
            nv = [v / r for v in l]
            P, J = row[4:7], row[7:10]
            for k in range(3):
                e[k] = e[k] + _hole_Aij(k, d, r, nv, J, P, mag)
            h = row[0] * l[d] / (r * r * r)
            ed = ed + (np.abs(h) if mag else h)
        A = e if A is None else [A[k] + e[k] for k in range(3)]
        dps = ed if dps is None else dps + ed
    return A[0], A[1], A[2], dps


def terms(psi, table, N, dx, n, lw=None, dtype=np.float64):
    """(T, S): the 7 terms of every face of the surface of half-width n,
    (6, 7, 2n, 2n) indexed (side, term, b, a), and each term's sum of absolute
    contributions.  psi: (nz, ny, nx) or None (psi = 1); lw: six arrays (IJ
    order) or None."""
    w = 2 * n
    T = np.zeros((6, 7, w, w), dtype=dtype)
    S = np.zeros((6, 7, w, w), dtype=dtype)
    dxx = dtype(dx)
    dx2 = dxx * dxx
    c2pi = dtype(-1.0 / (2.0 * math.pi))
    c8pi = dtype(1.0 / (8.0 * math.pi))
    for side in range(6):
        d, s, cin, cout, x = side_geometry(N, n, dx, side, dtype)
        sd = dtype(s)
        A0, A1, A2, dps = bowen_york(table, x, d, dtype)
        M0, M1, M2, mps = bowen_york(table, x, d, dtype, mag=True)
        A, M = [A0, A1, A2], [M0, M1, M2]
        if lw is not None:
            for k in range(3):
                comp = lw[IJ.index((min(k, d), max(k, d)))].astype(dtype)
                A[k] = A[k] + dtype(0.5) * (comp[cin] + comp[cout])
                M[k] = M[k] + dtype(0.5) * (np.abs(comp[cin]) + np.abs(comp[cout]))
        if psi is None:
            po = pi_ = np.ones((w, w), dtype=dtype)
        else:
            po, pi_ = psi[cout].astype(dtype), psi[cin].astype(dtype)
        g = (po - pi_) / dxx + sd * (-dps)
        T[side, 0] = c2pi * g * dx2
        S[side, 0] = np.abs(c2pi) * ((np.abs(po) + np.abs(pi_)) / dxx + mps) * dx2
        for k in range(3):
            T[side, 1 + k] = c8pi * sd * A[k] * dx2
            S[side, 1 + k] = c8pi * M[k] * dx2
        for i in range(3):
            j, k = (i + 1) % 3, (i + 2) % 3
            T[side, 4 + i] = c8pi * sd * (x[j] * A[k] - x[k] * A[j]) * dx2
            S[side, 4 + i] = c8pi * (np.abs(x[j]) * M[k] + np.abs(x[k]) * M[j]) * dx2
    return T, S


def tree_sum(values):
    """The library's order over a 1-D float64 sequence of per-face values."""
    v = np.asarray(values, dtype=np.float64).ravel()
    nb = (v.size + BLOCK - 1) // BLOCK
    p = np.zeros(nb * BLOCK)
    p[:v.size] = v
    p = p.reshape(nb, BLOCK // WAVE, WAVE)
    width = WAVE
    while width > 1:
        width //= 2
        p = p[..., :width] + p[..., width:2 * width]
    p = p[..., 0]
    blocks = p[:, 0]
    for k in range(1, BLOCK // WAVE):
        blocks = blocks + p[:, k]
    acc = blocks[0]
    for b in range(1, nb):
        acc = acc + blocks[b]
    return float(acc)


def tree_depth(count):
    """The largest number of additions a value goes through in tree_sum."""
    nb = (count + BLOCK - 1) // BLOCK
    return 6 + (BLOCK // WAVE - 1) + (nb - 1)


def sums(T):
    """The 7 sums of one surface's terms (6, 7, w, w) in the library's order:
    faces in (side, b, a) order."""
    return np.array([tree_sum(T[:, c].ravel()) for c in range(7)])


def charges(psi, table, N, dx, n, lw=None):
    """(M, P[3], J[3]) of the surface in the library's order."""
    r = sums(terms(psi, table, N, dx, n, lw)[0])
    return r[0], r[1:4], r[4:7]
