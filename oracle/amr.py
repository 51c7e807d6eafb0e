"""numpy restatement of the AMR multi-level operators -- TEST INFRASTRUCTURE ONLY.

The checker for mg_ic_code_amd/csrc/amr.cpp: AMROracle
with one box per level, MultiBoxAMROracle with a list of disjoint boxes per
level (unions that are not boxes, sibling exchange, periodic directions).
fp64, every expression in the GPU kernels' order, so results are
bit-identical:

* coarse-fine interpolation ([Chombo] QuadCFInterp, restated; the
  reference calls homogeneousCFInterp at
  Source/VariableCoeffPoissonOperator.cpp:156,296): ghost of a non-domain
  face = ((8/15) phi* + (2/3) f1) + (-0.2) f2, phi* the coarse value
  tangentially interpolated (centred / one-sided / none by usable
  neighbours, plus the mixed term), 0 when homogeneous;
* GSRB colour passes (GSRBHELMHOLTZVC3D, .ChF:91-136), residual
  (VCCOMPUTERES3D, .ChF:283-339) with the physical BC folded in;
* CoarseAverage (sum of 8 children * 1/8), piecewise-constant prolongation;
* the AMR V-cycle of amr.cpp: l_base = 0 solved by the C oracle's
  MultiGrid one_cycle, finer levels smoothed with homogeneous CF ghosts,
  AMRRestrict / AMRProlong / AMRUpdateResidual, reflux a no-op
  (.cpp:264-271).
Parity unpinned against Chombo (its AMR code is not in the reference tree).
"""
from __future__ import annotations

import math

import numpy as np

import oracle

W0, W1, W2 = 8.0 / 15.0, 2.0 / 3.0, -0.2


class Level:
    def __init__(self, box, dx, a, b, domain, bc_lo, bc_hi, bc_value, alpha, beta,
                 periodic=(0, 0, 0)):
        self.box = tuple(box)  # lo0 lo1 lo2 hi0 hi1 hi2
        self.periodic = tuple(periodic)
        self.dx = dx
        self.a, self.b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        self.domain = tuple(domain)
        self.bc_lo, self.bc_hi, self.bc_value = tuple(bc_lo), tuple(bc_hi), bc_value
        self.alpha, self.beta = alpha, beta
        self.dxinv = 1.0 / (dx * dx)
        self.lamshift = 2.0 * 3 * beta / (dx * dx)

    @property
    def shape(self):
        b = self.box
        return (b[5] - b[2] + 1, b[4] - b[1] + 1, b[3] - b[0] + 1)

    def full(self, v=None):
        out = np.zeros(tuple(s + 2 for s in self.shape))
        if v is not None:
            out[1:-1, 1:-1, 1:-1] = v
        return out

    def domain_face(self, dir, side):
        if self.periodic[dir]:  # a face on a periodic boundary is an exchanged face
            return False
        b, d = self.box, self.domain
        return b[3 + dir] == d[3 + dir] if side else b[dir] == d[dir]

    # -------------------------------------------------------------- ghosts
    def fill_bc(self, u, hom):
        """physical BC images on domain faces (DiriBC: c - near with c =
        2 value; NeumBC: near (+ isign dx value)); faces only"""
        for dir in range(3):
            ax = 2 - dir
            for side in (0, 1):
                if not self.domain_face(dir, side):
                    continue
                flag = self.bc_hi[dir] if side else self.bc_lo[dir]
                g, n = [slice(1, -1)] * 3, [slice(1, -1)] * 3
                g[ax], n[ax] = (-1, -2) if side else (0, 1)
                near = u[tuple(n)]
                if flag == 0:  # Dirichlet
                    c = 0.0 if hom else 2.0 * self.bc_value
                    u[tuple(g)] = c - near
                elif hom:
                    u[tuple(g)] = near
                else:
                    c = (1.0 if side else -1.0) * self.dx * self.bc_value
                    u[tuple(g)] = near + c

    def cf_interp(self, u, coarse=None, cov=(), cdomain=None, phistar=None):
        """ghosts of the non-domain faces from the coarse level (lv, full
        array) or zero; cov: coarsened fine boxes (covered test).  phistar
        (loc, dir, d0, d1) -> phi*: the coarse level given some other way
        (MultiBoxAMROracle: several coarse boxes, periodic wrap)"""
        b = self.box
        for dir in range(3):
            ax = 2 - dir
            for side in (0, 1):
                if self.domain_face(dir, side):
                    continue
                d0, d1 = (1, 2) if dir == 0 else ((0, 2) if dir == 1 else (0, 1))
                n = [b[3 + d] - b[d] + 1 for d in range(3)]
                A0, A1 = np.meshgrid(np.arange(n[d0]), np.arange(n[d1]), indexing="ij")
                loc = [None] * 3
                loc[dir] = np.full(A0.shape, n[dir] if side else -1)
                loc[d0], loc[d1] = A0, A1
                gi = tuple(loc[2 - a] + 1 for a in range(3))  # (z, y, x) in the full array
                step = -1 if side else 1
                i1 = list(gi)
                i1[ax] = i1[ax] + step
                i2 = list(gi)
                i2[ax] = i2[ax] + 2 * step
                f1, f2 = u[tuple(i1)], u[tuple(i2)]
                if phistar is not None:
                    ps = phistar(loc, dir, d0, d1)
                elif coarse is None:
                    ps = np.zeros(A0.shape)
                else:
                    ps = self._phistar(loc, dir, d0, d1, coarse, cov, cdomain)
                u[gi] = (W0 * ps + W1 * f1) + W2 * f2

    def _phistar(self, loc, dir, d0, d1, cl, cov, cdom):
        b = self.box
        gf = [loc[d] + b[d] for d in range(3)]
        gc = [np.floor_divide(g, 2) for g in gf]
        cb = cl.box
        cu = cl.u_full  # coarse full array (ghost 1)

        def at(p):
            return cu[p[2] - cb[2] + 1, p[1] - cb[1] + 1, p[0] - cb[0] + 1]

        def usable(p):
            ok = np.ones(p[0].shape, bool)
            for d in range(3):
                ok &= (p[d] >= cdom[d]) & (p[d] <= cdom[3 + d])
            for c in cov:
                inside = np.ones(p[0].shape, bool)
                for d in range(3):
                    inside &= (p[d] >= c[d]) & (p[d] <= c[3 + d])
                ok &= ~inside
            return ok

        def at_clipped(p):  # (an unusable neighbour may lie outside the array)
            return at([np.clip(p[k], cb[k] - 1, cb[3 + k] + 1) for k in range(3)])

        return self._phistar_core(gf, gc, d0, d1, at_clipped, usable)

    @staticmethod
    def _phistar_core(gf, gc, d0, d1, at, usable):
        """phi* from the coarse values at(p) and the usable(p) test (p: three
        index arrays, coarse index space), in k_cf_interp's order"""
        c0 = at(gc)
        d1v, d2v, xt = [], [], []
        for d in (d0, d1):
            xt.append(np.where(gf[d] - 2 * gc[d] != 0, 0.25, -0.25))
            pp = list(gc)
            pp[d] = gc[d] + 1
            pm = list(gc)
            pm[d] = gc[d] - 1
            okp, okm = usable(pp), usable(pm)
            vp = np.where(okp, at(pp), 0.0)
            vm = np.where(okm, at(pm), 0.0)
            both = okp & okm
            g1 = np.where(both, (vp - vm) * 0.5, np.where(okp, vp - c0, np.where(okm, c0 - vm, 0.0)))
            g2 = np.where(both, (vp - 2.0 * c0) + vm, 0.0)
            d1v.append(g1)
            d2v.append(g2)
        v, allok = [], np.ones(c0.shape, bool)
        for s1 in (-1, 1):
            for s0 in (-1, 1):
                p = list(gc)
                p[d0] = gc[d0] + s0
                p[d1] = gc[d1] + s1
                ok = usable(p)
                allok &= ok
                v.append(np.where(ok, at(p), 0.0))
        d12 = np.where(allok, (((v[3] - v[2]) - v[1]) + v[0]) * 0.25, 0.0)
        ps = c0
        for t in range(2):
            ps = ps + (xt[t] * d1v[t] + 0.5 * (xt[t] * xt[t]) * d2v[t])
        return ps + (xt[0] * xt[1]) * d12

    # -------------------------------------------------------------- kernels
    def _colour(self, shape):
        b = self.box
        k, j, i = np.meshgrid(np.arange(shape[0]) + b[2], np.arange(shape[1]) + b[1],
                              np.arange(shape[2]) + b[0], indexing="ij")
        return (i + j + k) % 2

    def _lap(self, u):
        c = u[1:-1, 1:-1, 1:-1]
        tx = (u[1:-1, 1:-1, 2:] + u[1:-1, 1:-1, :-2]) - 2.0 * c
        ty = (u[1:-1, 2:, 1:-1] + u[1:-1, :-2, 1:-1]) - 2.0 * c
        tz = (u[2:, 1:-1, 1:-1] + u[:-2, 1:-1, 1:-1]) - 2.0 * c
        return (tx + ty) + tz

    def gsrb_pass(self, u, rhs, colour):
        c = u[1:-1, 1:-1, 1:-1]
        lof = self.alpha * self.a * c
        ldpsi = self._lap(u) * self.dxinv * self.b
        lof = lof - self.beta * ldpsi
        lam = 1.0 / (self.a * self.alpha + self.lamshift)
        new = c - lam * (lof - rhs)
        m = self._colour(c.shape) == colour
        c[m] = new[m]

    def residual(self, u, rhs):
        c = u[1:-1, 1:-1, 1:-1]
        res = rhs - self.alpha * self.a * c
        ldpsi = self._lap(u) * self.dxinv * self.beta * self.b
        return res + ldpsi


def average_down(fine: np.ndarray) -> np.ndarray:
    s = np.zeros(tuple(v // 2 for v in fine.shape))
    for kk in range(2):
        for jj in range(2):
            for ii in range(2):
                s = s + fine[kk::2, jj::2, ii::2]
    return s * (1.0 / 8)


class AMROracle:
    """levels: list of dict(box, a, b) from coarsest; level 0's box is the
    domain.  base: the C oracle's MultiGrid parameters for level 0."""

    def __init__(self, levels, dx0, domain0, alpha=1.0, beta=-1.0, bc_lo=(0, 0, 0),
                 bc_hi=(0, 0, 0), bc_value=0.0, n_pre=4, n_post=4, base=None):
        self.L = []
        dom = tuple(domain0)
        dx = dx0
        for lv in levels:
            self.L.append(Level(lv["box"], dx, lv["a"], lv["b"], dom, bc_lo, bc_hi, bc_value,
                                alpha, beta))
            dom = tuple(2 * v if i < 3 else 2 * v + 1 for i, v in enumerate(dom))
            dx = dx / 2
        self.n_pre, self.n_post = n_pre, n_post
        base = dict(base or {})
        self.o = oracle.OracleMG([self.L[0].box], self.L[0].box, dx0, alpha=alpha, beta=beta,
                                 bc_lo=bc_lo, bc_hi=bc_hi, bc_value=bc_value, **base)
        self.o.set(0, oracle.ACOEF, 0, self.L[0].a)
        self.o.set(0, oracle.BCOEF, 0, self.L[0].b)
        self.o.setup()

    def cov(self, l):
        b = self.L[l].box
        return [tuple([v // 2 for v in b[:3]] + [(v + 1) // 2 - 1 for v in b[3:]])]

    def fill(self, l, u, coarse_full, hom_phys):
        """CF ghosts (coarse_full None: homogeneous), then the physical BC"""
        lv = self.L[l]
        if l > 0:
            cl = None
            if coarse_full is not None:
                cl = self.L[l - 1]
                cl.u_full = coarse_full
            lv.cf_interp(u, cl, self.cov(l), self.L[l - 1].domain)
        lv.fill_bc(u, hom_phys)

    def relax(self, l, e, r, n):
        lv = self.L[l]
        for _ in range(n):
            for colour in (0, 1):
                self.fill(l, e, None, True)
                lv.gsrb_pass(e, r, colour)

    def amr_residual(self, l, phi, phi_coarse, rhs, hom=False):
        self.fill(l, phi, phi_coarse, hom)
        return self.L[l].residual(phi, rhs)

    def put_covered(self, l, coarse_valid, fine_valid_avg):
        """write the averaged fine data onto the covered coarse cells"""
        cb, fb = self.L[l - 1].box, self.L[l].box
        lo = [fb[d] // 2 - cb[d] for d in range(3)]
        n = fine_valid_avg.shape
        coarse_valid[lo[2]:lo[2] + n[0], lo[1]:lo[1] + n[1], lo[0]:lo[0] + n[2]] = fine_valid_avg

    def prolong_const(self, l, e_full, ec_full):
        cb, fb = self.L[l - 1].box, self.L[l].box
        lo = [fb[d] // 2 - cb[d] + 1 for d in range(3)]
        n = [s // 2 for s in self.L[l].shape]
        c = ec_full[lo[2]:lo[2] + n[0], lo[1]:lo[1] + n[1], lo[0]:lo[0] + n[2]]
        f = e_full[1:-1, 1:-1, 1:-1]
        for kk in range(2):
            for jj in range(2):
                for ii in range(2):
                    f[kk::2, jj::2, ii::2] = f[kk::2, jj::2, ii::2] + c

    # ---------------------------------------------------------------- driver
    def init_residual(self, phis, rhss):
        """phis: full arrays per level (modified: ghosts); returns residuals"""
        self.phis, self.rhss = phis, rhss
        res = []
        for l in range(len(self.L)):
            res.append(self.amr_residual(l, phis[l], phis[l - 1] if l else None, rhss[l]))
        for l in range(1, len(self.L)):
            self.put_covered(l, res[l - 1], np.zeros(tuple(s // 2 for s in self.L[l].shape)))
        self.res = res
        return res

    def cycle(self, l):
        if l == 0:
            o = self.o
            o.set(0, oracle.RESID, 0, self.res[0])
            o.set(0, oracle.CORR, 0, self.L[0].full(), full=True)
            o.one_cycle(0)
            self.corr[0] = self.L[0].full(o.get(0, oracle.CORR, 0))
            return
        lv = self.L[l]
        e = lv.full()
        self.relax(l, e, self.res[l], self.n_pre)
        self.corr[l] = e
        # AMRRestrict: residual of e (homogeneous CF, homogeneous physical BC)
        r = self.amr_residual(l, e, None, self.res[l], True)
        self.put_covered(l, self.res[l - 1], average_down(r))
        self.cycle(l - 1)
        e = self.corr[l]
        self.prolong_const(l, e, self.corr[l - 1])
        # AMRUpdateResidual: CF ghosts of e from e_c
        self.res[l] = self.amr_residual(l, e, self.corr[l - 1], self.res[l], True)
        de = lv.full()
        self.relax(l, de, self.res[l], self.n_post)
        e[1:-1, 1:-1, 1:-1] = e[1:-1, 1:-1, 1:-1] + de[1:-1, 1:-1, 1:-1]

    def iteration(self):
        n = len(self.L)
        self.corr = [None] * n
        self.cycle(n - 1)
        for l in range(n):
            self.phis[l][1:-1, 1:-1, 1:-1] = (self.phis[l][1:-1, 1:-1, 1:-1]
                                              + self.corr[l][1:-1, 1:-1, 1:-1])
        for l in range(n - 1, 0, -1):
            cv = self.phis[l - 1][1:-1, 1:-1, 1:-1]
            self.put_covered(l, cv, average_down(self.phis[l][1:-1, 1:-1, 1:-1]))
        return self.init_residual(self.phis, self.rhss)

    # ------------------------------------------- MultilevelLinearOp + BiCGStab
    # (csrc/amr.cpp AMRSolver::applyOp / precondition / solve restated; every
    # vector is a list of full arrays, one per level, ghost layer included)
    def weight(self, l):
        return self.L[l].dx ** 3

    def zeros_ml(self):
        return [lv.full() for lv in self.L]

    def zero_covered(self, xs):
        for l in range(1, len(self.L)):
            self.put_covered(l, xs[l - 1][1:-1, 1:-1, 1:-1],
                             np.zeros(tuple(s // 2 for s in self.L[l].shape)))

    def apply_op(self, xs, hom=True):
        """lhs = AMROperator on every level (L(u) = -(0 - L(u)), exact), the
        covered coarse cells zeroed"""
        out = []
        for l, lv in enumerate(self.L):
            self.fill(l, xs[l], xs[l - 1] if l else None, hom)
            out.append(lv.full(-lv.residual(xs[l], np.zeros(lv.shape))))
        self.zero_covered(out)
        return out

    def residual_ml(self, phis, rhss, hom=False):
        out = [lv.full(self.amr_residual(l, phis[l], phis[l - 1] if l else None,
                                         rhss[l][1:-1, 1:-1, 1:-1], hom))
               for l, lv in enumerate(self.L)]
        self.zero_covered(out)
        return out

    def dot(self, xs, ys):
        return sum(self.weight(l) * float(np.sum(x[1:-1, 1:-1, 1:-1] * y[1:-1, 1:-1, 1:-1]))
                   for l, (x, y) in enumerate(zip(xs, ys)))

    def norm(self, xs, ord=0):
        if ord == 0:
            return max(float(np.abs(x[1:-1, 1:-1, 1:-1]).max()) for x in xs)
        if ord == 1:
            return sum(self.weight(l) * float(np.abs(x[1:-1, 1:-1, 1:-1]).sum())
                       for l, x in enumerate(xs))
        return float(np.sqrt(sum(self.weight(l) * float(np.sum(x[1:-1, 1:-1, 1:-1] ** 2))
                                 for l, x in enumerate(xs))))

    def masked(self, xs):
        out = [x.copy() for x in xs]
        self.zero_covered(out)
        return out

    def precondition(self, rs, iters):
        """e = 0, then `iters` AMR iterations on (e, r), homogeneous physical BCs"""
        n = len(self.L)
        es = self.zeros_ml()
        for i in range(iters):
            if i == 0:
                self.res = [r[1:-1, 1:-1, 1:-1].copy() for r in rs]
            else:
                self.res = [self.amr_residual(l, es[l], es[l - 1] if l else None,
                                              rs[l][1:-1, 1:-1, 1:-1], True) for l in range(n)]
                for l in range(1, n):
                    self.put_covered(l, self.res[l - 1],
                                     np.zeros(tuple(s // 2 for s in self.L[l].shape)))
            self.corr = [None] * n
            self.cycle(n - 1)
            for l in range(n):
                es[l][1:-1, 1:-1, 1:-1] = es[l][1:-1, 1:-1, 1:-1] + self.corr[l][1:-1, 1:-1, 1:-1]
            for l in range(n - 1, 0, -1):
                self.put_covered(l, es[l - 1][1:-1, 1:-1, 1:-1],
                                 average_down(es[l][1:-1, 1:-1, 1:-1]))
        return es

    def solve(self, phis, rhss, num_mg_iterations=1, imax=10, eps=1e-7, norm_type=0,
              reps=1e-12, small=1e-30, num_restarts=5):
        """BiCGStabSolver::solve over the multi-level operator (the control
        flow of csrc/op.cpp BiCGStabSolver::solve); phis modified in place;
        returns (iterations, final norm)"""
        n = len(self.L)
        it_mg = max(1, num_mg_iterations)

        def ax(a, x, b, y):  # a*x + b*y per level on the valid cells
            out = []
            for xl, yl in zip(x, y):
                z = np.zeros_like(xl)
                z[1:-1, 1:-1, 1:-1] = a * xl[1:-1, 1:-1, 1:-1] + b * yl[1:-1, 1:-1, 1:-1]
                out.append(z)
            return out

        def incr(x, y, s):
            for xl, yl in zip(x, y):
                xl[1:-1, 1:-1, 1:-1] = xl[1:-1, 1:-1, 1:-1] + s * yl[1:-1, 1:-1, 1:-1]

        R = self.residual_ml(phis, rhss, False)
        RT = [r.copy() for r in R]
        E, P, V = self.zeros_ml(), self.zeros_ml(), self.zeros_ml()
        rho1 = rho2 = alpha = beta = omega = 0.0
        init_norm = self.norm(R, norm_type)
        nrm = init_norm
        it = restarts = 0
        init = True
        while it < imax and nrm > eps * init_norm and nrm > reps:
            it += 1
            rho2 = rho1
            rho1 = self.dot(RT, R)
            if rho1 == 0.0:
                break
            if init:
                P = [r.copy() for r in R]
                init = False
            else:
                beta = (rho1 / rho2) * (alpha / omega)
                c = -beta * omega
                for pl, vl, rl in zip(P, V, R):
                    pl[1:-1, 1:-1, 1:-1] = ((pl[1:-1, 1:-1, 1:-1] * beta + c * vl[1:-1, 1:-1, 1:-1])
                                            + rl[1:-1, 1:-1, 1:-1])
            PT = self.precondition(P, it_mg)
            V = self.apply_op(PT, True)
            m = self.dot(RT, V)
            if abs(m) > small * abs(rho1):
                alpha = rho1 / m
                S = ax(1.0, R, -alpha, V)
                incr(E, PT, alpha)
                nrm = self.norm(S, norm_type)
                if nrm <= eps * init_norm or nrm <= reps:
                    break
                ST = self.precondition(S, it_mg)
                T = self.apply_op(ST, True)
                ts, tt = self.dot(T, S), self.dot(T, T)
                if tt == 0.0:
                    break
                omega = ts / tt
                R = ax(1.0, S, -omega, T)
                incr(E, ST, omega)
                nrm = self.norm(R, norm_type)
                if omega == 0.0:
                    break
            else:
                if restarts >= num_restarts:
                    break
                restarts += 1
                incr(phis, E, 1.0)
                R = self.residual_ml(phis, rhss, False)
                RT = [r.copy() for r in R]
                E = self.zeros_ml()
                nrm = self.norm(R, norm_type)
                init = True
        incr(phis, E, 1.0)
        R = self.residual_ml(phis, rhss, False)
        return it, self.norm(R, norm_type)


# ---------------------------------------------------------------- multi-box
def _isect(a, b):
    lo = [max(a[d], b[d]) for d in range(3)]
    hi = [min(a[3 + d], b[3 + d]) for d in range(3)]
    return None if any(l > h for l, h in zip(lo, hi)) else tuple(lo + hi)


def _sl(region, box, ghost):
    """slices of a region (global indices) in the (z, y, x) array of a box
    with `ghost` ghost layers"""
    return tuple(slice(region[d] - box[d] + ghost, region[3 + d] - box[d] + ghost + 1)
                 for d in (2, 1, 0))


def coarsen_box(b):
    return tuple([v // 2 for v in b[:3]] + [(v + 1) // 2 - 1 for v in b[3:]])


def _valid(x):
    return x[1:-1, 1:-1, 1:-1]


class MultiBoxAMROracle(AMROracle):
    """AMROracle with a list of disjoint boxes per level (amr.cpp on any
    properly nested hierarchy: unions that are not boxes, faces that are part
    fine-fine and part coarse-fine, covered tangential neighbours, periodic
    directions).

    levels: list of dict(boxes=[box, ...], a=[array per box], b=[array per
    box]) from coarsest; level 0 is one box, the domain.  A multi-level
    vector is a FLAT list of per-box arrays, level by level, boxes in the
    order given (self.ix[l]: the flat indices of level l; split() regroups);
    with one box per level that is AMROracle's list, and its methods keep
    their conventions (full arrays with ghost 1, except where AMROracle takes
    valid ones).  Every box has its own ghosts: a cell outside the level can
    be the ghost of two boxes with two different values.

    Ghost fill of a level, in the order of amr.cpp / op.cpp: the coarse-fine
    interpolation on every non-domain face of every box (whole faces), the
    sibling exchange valid -> 1-deep face ghosts (through periodic images),
    the physical BC.  dot_fsum: dot products and 1-/2-norms summed with
    math.fsum over all cells of a level (default: per box, then over boxes)
    -- the two bracket what any summation order can give."""

    def __init__(self, levels, dx0, domain0, alpha=1.0, beta=-1.0, bc_lo=(0, 0, 0),
                 bc_hi=(0, 0, 0), bc_value=0.0, n_pre=4, n_post=4, base=None,
                 periodic=(0, 0, 0), dot_fsum=False):
        self.periodic = tuple(int(p) for p in periodic)
        self.dot_fsum = dot_fsum
        self.B, self.dom, self.ix = [], [], []
        dom, dx, n = tuple(domain0), dx0, 0
        for lv in levels:
            boxes = [tuple(b) for b in lv["boxes"]]
            self.B.append([Level(bx, dx, a, b, dom, bc_lo, bc_hi, bc_value, alpha, beta,
                                 self.periodic) for bx, a, b in zip(boxes, lv["a"], lv["b"])])
            self.dom.append(dom)
            self.ix.append(list(range(n, n + len(boxes))))
            n += len(boxes)
            dom = tuple(2 * v if i < 3 else 2 * v + 1 for i, v in enumerate(dom))
            dx = dx / 2
        assert len(self.B[0]) == 1 and self.B[0][0].box == tuple(domain0), "level 0: the domain"
        self.L = [bs[0] for bs in self.B]  # (dx per level; level 0's box)
        self.n_pre, self.n_post = n_pre, n_post
        base = dict(base or {})
        self.o = oracle.OracleMG([self.L[0].box], self.L[0].box, dx0, alpha=alpha, beta=beta,
                                 periodic=self.periodic, bc_lo=bc_lo, bc_hi=bc_hi,
                                 bc_value=bc_value, **base)
        self.o.set(0, oracle.ACOEF, 0, self.L[0].a)
        self.o.set(0, oracle.BCOEF, 0, self.L[0].b)
        self.o.setup()
        self._plans()

    def _plans(self):
        self.xplan, self.dplan, self.cmask = [], [None], [None]
        for l, bs in enumerate(self.B):
            dom = self.dom[l]
            ln = [dom[3 + d] - dom[d] + 1 for d in range(3)]
            sh = [(-1, 0, 1) if self.periodic[d] else (0,) for d in range(3)]
            plan = []
            for i, bi in enumerate(bs):
                for dir in range(3):
                    for side in (0, 1):
                        r = list(bi.box)  # the cells adjacent to the face
                        r[dir] = r[3 + dir] = bi.box[3 + dir] + 1 if side else bi.box[dir] - 1
                        for j, bj in enumerate(bs):
                            for sz in sh[2]:
                                for sy in sh[1]:
                                    for sx in sh[0]:
                                        s = (sx * ln[0], sy * ln[1], sz * ln[2])
                                        x = _isect(r, tuple(v + s[k % 3]
                                                            for k, v in enumerate(bj.box)))
                                        if x is None:
                                            continue
                                        src = tuple(v - s[k % 3] for k, v in enumerate(x))
                                        plan.append((i, _sl(x, bi.box, 1), j, _sl(src, bj.box, 1)))
            self.xplan.append(plan)
            if l == 0:
                continue
            cdom = self.dom[l - 1]
            mask = np.zeros(tuple(cdom[3 + d] - cdom[d] + 1 for d in (2, 1, 0)), bool)
            down = []
            for i, bi in enumerate(bs):
                c = coarsen_box(bi.box)
                assert all(v % 2 == 0 for v in bi.box[:3]) and all(v % 2 for v in bi.box[3:]), \
                    "fine boxes must be coarsenable by 2"
                mask[_sl(c, cdom, 0)] = True
                for j, bj in enumerate(self.B[l - 1]):
                    x = _isect(c, bj.box)
                    if x is not None:
                        down.append((i, _sl(x, c, 0), j, _sl(x, bj.box, 0)))
            self.cmask.append(mask)
            self.dplan.append(down)

    # ------------------------------------------------------------ vectors
    def split(self, xs):
        return [[xs[i] for i in ix] for ix in self.ix]

    def lv(self, xs, l):
        return [xs[i] for i in self.ix[l]]

    def cov(self, l):
        return [coarsen_box(b.box) for b in self.B[l]]

    def zeros_ml(self):
        return [b.full() for bs in self.B for b in bs]

    def full_ml(self, arrs):
        return [b.full(a) for b, a in zip([b for bs in self.B for b in bs], arrs)]

    def glob(self, l, us):
        """the level's valid data in one array over its domain (NaN where
        the level has no cell)"""
        dom = self.dom[l]
        g = np.full(tuple(dom[3 + d] - dom[d] + 1 for d in (2, 1, 0)), np.nan)
        for b, u in zip(self.B[l], us):
            g[_sl(b.box, dom, 0)] = _valid(u)
        return g

    # -------------------------------------------------------------- ghosts
    def _phistar(self, l, b, cg, loc, dir, d0, d1):
        cdom, mask, per = self.dom[l - 1], self.cmask[l], self.periodic
        gf = [loc[d] + b.box[d] for d in range(3)]
        gc = [np.floor_divide(g, 2) for g in gf]

        def wrap(p):  # cf_usable's test and wrap; indices into the domain arrays
            ok, q = np.ones(p[0].shape, bool), []
            for d in range(3):
                n = cdom[3 + d] - cdom[d] + 1
                if per[d]:
                    q.append(np.mod(p[d] - cdom[d], n))
                else:
                    ok &= (p[d] >= cdom[d]) & (p[d] <= cdom[3 + d])
                    q.append(np.clip(p[d] - cdom[d], 0, n - 1))
            return ok, (q[2], q[1], q[0])

        def at(p):
            return cg[wrap(p)[1]]

        def usable(p):
            ok, q = wrap(p)
            return ok & ~mask[q]

        return Level._phistar_core(gf, gc, d0, d1, at, usable)

    def cf_interp(self, l, us, coarse_us=None):
        """CF ghosts of every non-domain face of every box of level l (whole
        faces: the part a sibling box covers is the exchange's to replace)"""
        if coarse_us is None:
            for b, u in zip(self.B[l], us):
                for dir in range(3):
                    for side in (0, 1):
                        if b.domain_face(dir, side):
                            continue
                        g, n1, n2 = ([slice(1, -1)] * 3 for _ in range(3))
                        g[2 - dir], n1[2 - dir], n2[2 - dir] = (-1, -2, -3) if side else (0, 1, 2)
                        u[tuple(g)] = (W0 * 0.0 + W1 * u[tuple(n1)]) + W2 * u[tuple(n2)]
            return
        cg = self.glob(l - 1, coarse_us)
        for b, u in zip(self.B[l], us):
            b.cf_interp(u, phistar=lambda loc, dir, d0, d1, b=b: self._phistar(l, b, cg, loc, dir,
                                                                               d0, d1))

    def exchange(self, l, us):
        for i, di, j, sj in self.xplan[l]:
            us[i][di] = us[j][sj]

    def fill(self, l, us, coarse_us, hom_phys):
        """CF ghosts (coarse_us None: homogeneous), exchange, physical BC"""
        if l > 0:
            self.cf_interp(l, us, coarse_us)
        self.exchange(l, us)
        for b, u in zip(self.B[l], us):
            b.fill_bc(u, hom_phys)

    def relax(self, l, es, rs, n):
        for _ in range(n):
            for colour in (0, 1):
                self.fill(l, es, None, True)
                for b, e, r in zip(self.B[l], es, rs):
                    b.gsrb_pass(e, r, colour)

    def amr_residual(self, l, phis, phis_coarse, rhss, hom=False):
        self.fill(l, phis, phis_coarse, hom)
        return [b.residual(p, r) for b, p, r in zip(self.B[l], phis, rhss)]

    def put_covered(self, l, coarse_valid, fine_avg=None):
        """the averaged fine data (None: zero) onto the covered cells of the
        coarse level's valid arrays"""
        for i, si, j, sj in self.dplan[l]:
            coarse_valid[j][sj] = 0.0 if fine_avg is None else fine_avg[i][si]

    def prolong_const(self, l, es, ecs):
        cg, cdom = self.glob(l - 1, ecs), self.dom[l - 1]
        for b, e in zip(self.B[l], es):
            c = cg[_sl(coarsen_box(b.box), cdom, 0)]
            f = _valid(e)
            for kk in range(2):
                for jj in range(2):
                    for ii in range(2):
                        f[kk::2, jj::2, ii::2] = f[kk::2, jj::2, ii::2] + c

    # ---------------------------------------------------------------- driver
    def init_residual(self, phis, rhss):
        """phis: full arrays (modified: ghosts), rhss: valid arrays; returns
        the residuals (valid arrays)"""
        self.phis, self.rhss = phis, rhss
        res = []
        for l in range(len(self.B)):
            res += self.amr_residual(l, self.lv(phis, l), self.lv(phis, l - 1) if l else None,
                                     self.lv(rhss, l))
        for l in range(1, len(self.B)):
            self.put_covered(l, self.lv(res, l - 1))
        self.res = res
        return res

    def cycle(self, l):
        if l == 0:
            AMROracle.cycle(self, 0)
            return
        I, Ic = self.ix[l], self.ix[l - 1]
        es = [b.full() for b in self.B[l]]
        rs = self.lv(self.res, l)
        self.relax(l, es, rs, self.n_pre)
        for i, e in zip(I, es):
            self.corr[i] = e
        r = self.amr_residual(l, es, None, rs, True)  # AMRRestrict
        self.put_covered(l, self.lv(self.res, l - 1), [average_down(x) for x in r])
        self.cycle(l - 1)
        ecs = [self.corr[i] for i in Ic]
        self.prolong_const(l, es, ecs)
        for i, x in zip(I, self.amr_residual(l, es, ecs, rs, True)):  # AMRUpdateResidual
            self.res[i] = x
        des = [b.full() for b in self.B[l]]
        self.relax(l, des, self.lv(self.res, l), self.n_post)
        for e, de in zip(es, des):
            _valid(e)[...] = _valid(e) + _valid(de)

    def _accumulate(self, xs):
        """xs += corr, then the covered cells from the finer level's average"""
        for x, c in zip(xs, self.corr):
            _valid(x)[...] = _valid(x) + _valid(c)
        for l in range(len(self.B) - 1, 0, -1):
            self.put_covered(l, [_valid(x) for x in self.lv(xs, l - 1)],
                             [average_down(_valid(x)) for x in self.lv(xs, l)])

    def iteration(self):
        self.corr = [None] * len(self.phis)
        self.cycle(len(self.B) - 1)
        self._accumulate(self.phis)
        return self.init_residual(self.phis, self.rhss)

    # ------------------------------------------- MultilevelLinearOp + BiCGStab
    def zero_covered(self, xs):
        for l in range(1, len(self.B)):
            self.put_covered(l, [_valid(x) for x in self.lv(xs, l - 1)])

    def apply_op(self, xs, hom=True):
        out = []
        for l, bs in enumerate(self.B):
            us = self.lv(xs, l)
            self.fill(l, us, self.lv(xs, l - 1) if l else None, hom)
            out += [b.full(-b.residual(u, np.zeros(b.shape))) for b, u in zip(bs, us)]
        self.zero_covered(out)
        return out

    def residual_ml(self, phis, rhss, hom=False):
        out = []
        for l, bs in enumerate(self.B):
            r = self.amr_residual(l, self.lv(phis, l), self.lv(phis, l - 1) if l else None,
                                  [_valid(x) for x in self.lv(rhss, l)], hom)
            out += [b.full(x) for b, x in zip(bs, r)]
        self.zero_covered(out)
        return out

    def _sum(self, l, arrs):
        if self.dot_fsum:
            return math.fsum(v for a in arrs for v in a.ravel())
        s = 0.0
        for a in arrs:
            s += float(np.sum(a))
        return s

    def dot(self, xs, ys):
        return sum(self.weight(l) * self._sum(l, [_valid(x) * _valid(y) for x, y in
                                                  zip(self.lv(xs, l), self.lv(ys, l))])
                   for l in range(len(self.B)))

    def norm(self, xs, ord=0):
        if ord == 0:
            return max(float(np.abs(_valid(x)).max()) for x in xs)
        f = np.abs if ord == 1 else np.square
        s = sum(self.weight(l) * self._sum(l, [f(_valid(x)) for x in self.lv(xs, l)])
                for l in range(len(self.B)))
        return s if ord == 1 else float(np.sqrt(s))

    def precondition(self, rs, iters):
        n = len(self.B)
        es = self.zeros_ml()
        for i in range(iters):
            if i == 0:
                self.res = [_valid(r).copy() for r in rs]
            else:
                self.res = []
                for l in range(n):
                    self.res += self.amr_residual(l, self.lv(es, l),
                                                  self.lv(es, l - 1) if l else None,
                                                  [_valid(x) for x in self.lv(rs, l)], True)
                for l in range(1, n):
                    self.put_covered(l, self.lv(self.res, l - 1))
            self.corr = [None] * len(es)
            self.cycle(n - 1)
            self._accumulate(es)
        return es
