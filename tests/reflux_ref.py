"""numpy restatement of the reflux term at coarse-fine faces
-- TEST INFRASTRUCTURE ONLY.

RefluxOracle is oracle/amr.py's MultiBoxAMROracle with csrc/amr.cpp's reflux
switch on: the checker of AMRSolver(..., reflux=True), every expression in the
order of k_reflux (csrc/reflux.hip), so the device matches it bit for bit.

On level l with a finer level l + 1, for an uncovered coarse cell i whose
neighbour n = i -/+ e_d is covered (through the wrap in a periodic direction,
never across a non-periodic domain face):

    G_c   = (phi_c[n] - phi_c[i]) / dx_c           (0.0 with no coarse field)
    g_ab  = (phi_f[in-cell] - phi_f[ghost]) / dx_f  the four fine cells behind
            the face; a: offset in the higher tangential direction, b: lower
    <G_f> = 0.25 * ((g00 + g01) + (g10 + g11))
    term  = (<G_f> - G_c) / dx_c
    v     = ((-beta) * b_i) * (the terms of i's faces summed in the order
            x-lo, x-hi, y-lo, y-hi, z-lo, z-hi; the first one starts the sum)
    target_i = target_i + v   (sign > 0)   or   target_i - v   (sign < 0)

phi_c[n] is read from the ghost layer of i's own box where n lies in another
box or across the wrap (the exchange of the level's operator has put it
there); phi_f's ghost is the one of the fine box that holds the in-cell
(QuadCFInterp, kept by the exchange: no sibling lies across that face).
Cells with no such face are not touched.
"""
from __future__ import annotations

import numpy as np

from oracle.amr import MultiBoxAMROracle, _sl, _valid, average_down, coarsen_box


class RefluxOracle(MultiBoxAMROracle):
    def __init__(self, *a, reflux=True, reflux_cycle=True, **kw):
        super().__init__(*a, **kw)
        self.reflux_on = bool(reflux)
        # the term in the V-cycle's downsweep too (amr.cpp does; off: the
        # issue's "operator and residual only" variant, CPU comparison only)
        self.reflux_cycle = bool(reflux_cycle)
        self.beta = self.L[0].beta

    # ------------------------------------------------------------ the term
    def _fine_gradients(self, l, phi_f):
        """<G_f> of every non-domain face of every box of level l + 1, put at
        the covered coarse cell behind the face: six arrays over level l's
        domain, indexed by the face of the UNCOVERED cell (0 x-lo ... 5 z-hi;
        the fine box's hi face is its neighbour's lo face)"""
        cdom = self.dom[l]
        shape = tuple(cdom[3 + d] - cdom[d] + 1 for d in (2, 1, 0))
        GF = [np.full(shape, np.nan) for _ in range(6)]
        dxf = self.B[l + 1][0].dx
        for bx, u in zip(self.B[l + 1], phi_f):
            c = coarsen_box(bx.box)
            for dir in range(3):
                ax = 2 - dir
                for side in (0, 1):
                    if bx.domain_face(dir, side):
                        continue
                    i_in, i_gh = [slice(1, -1)] * 3, [slice(1, -1)] * 3
                    i_in[ax], i_gh[ax] = (-2, -1) if side else (1, 0)
                    g = (u[tuple(i_in)] - u[tuple(i_gh)]) / dxf  # (higher, lower) tangential
                    gf = 0.25 * ((g[0::2, 0::2] + g[0::2, 1::2]) + (g[1::2, 0::2] + g[1::2, 1::2]))
                    r = list(c)
                    r[dir] = r[3 + dir] = c[3 + dir] if side else c[dir]
                    GF[2 * dir + (0 if side else 1)][_sl(tuple(r), cdom, 0)] = np.expand_dims(gf, ax)
        return GF

    def interface_mask(self, l):
        """per face (0 x-lo ... 5 z-hi) over level l's domain: the cell is not
        covered by level l + 1 and its neighbour across that face is"""
        cov, per = self.cmask[l + 1], self.periodic
        out = []
        for dir in range(3):
            ax = 2 - dir
            for side in (0, 1):
                nb = np.roll(cov, 1 if side == 0 else -1, axis=ax)  # nb[i] = cov[i -/+ e_d]
                if not per[dir]:
                    edge = [slice(None)] * 3
                    edge[ax] = 0 if side == 0 else -1
                    nb[tuple(edge)] = False
                out.append(~cov & nb)
        return out

    def reflux(self, l, target, phi_c, phi_f, sign):
        """target: valid arrays of level l's boxes (modified in place); phi_c:
        full arrays of level l (None: a zero coarse field); phi_f: full arrays
        of level l + 1, ghosts filled"""
        cdom = self.dom[l]
        GF = self._fine_gradients(l, phi_f)
        masks = self.interface_mask(l)
        dxc = self.B[l][0].dx
        for j, bx in enumerate(self.B[l]):
            s = np.zeros(bx.shape)
            have = np.zeros(bx.shape, bool)
            here = _sl(bx.box, cdom, 0)
            for dir in range(3):
                ax = 2 - dir
                for side in (0, 1):
                    f = 2 * dir + side
                    m = masks[f][here]
                    if not m.any():
                        continue
                    sh = 1 if side == 0 else -1
                    gf = np.roll(GF[f], sh, axis=ax)[here]  # <G_f> at the neighbour
                    if phi_c is None:
                        gc = 0.0
                    else:
                        nbr = [slice(1, -1)] * 3
                        nbr[ax] = slice(0, -2) if side == 0 else slice(2, None)
                        gc = (phi_c[j][tuple(nbr)] - _valid(phi_c[j])) / dxc
                    with np.errstate(invalid="ignore"):
                        term = (gf - gc) / dxc
                        s = np.where(m, np.where(have, s + term, term), s)
                    have |= m
            with np.errstate(invalid="ignore"):
                v = ((-self.beta) * bx.b) * s
                new = target[j] + v if sign > 0 else target[j] - v
            target[j][have] = new[have]

    def average_covered(self, xs):
        """covered cells <- the finer level's average, finest pair first (what
        amr.cpp's applyOp / residual / initResidual do to their input first
        with the switch on: the operator then reads uncovered data alone)"""
        if not self.reflux_on:
            return
        for l in range(len(self.B) - 1, 0, -1):
            self.put_covered(l, [_valid(x) for x in self.lv(xs, l - 1)],
                             [average_down(_valid(x)) for x in self.lv(xs, l)])

    def reflux_all(self, out_valid, phis, sign):
        if not self.reflux_on:
            return
        for l in range(len(self.B) - 1):
            self.reflux(l, self.lv(out_valid, l), self.lv(phis, l), self.lv(phis, l + 1), sign)

    # ------------------------------------------------------------ overrides
    def apply_op(self, xs, hom=True):
        out = []
        self.average_covered(xs)
        for l, bs in enumerate(self.B):
            us = self.lv(xs, l)
            self.fill(l, us, self.lv(xs, l - 1) if l else None, hom)
            out += [b.full(-b.residual(u, np.zeros(b.shape))) for b, u in zip(bs, us)]
        self.reflux_all([_valid(x) for x in out], xs, +1)
        self.zero_covered(out)
        return out

    def residual_ml(self, phis, rhss, hom=False):
        out = []
        self.average_covered(phis)
        for l, bs in enumerate(self.B):
            r = self.amr_residual(l, self.lv(phis, l), self.lv(phis, l - 1) if l else None,
                                  [_valid(x) for x in self.lv(rhss, l)], hom)
            out += [b.full(x) for b, x in zip(bs, r)]
        self.reflux_all([_valid(x) for x in out], phis, -1)
        self.zero_covered(out)
        return out

    def init_residual(self, phis, rhss):
        self.phis, self.rhss = phis, rhss
        res = []
        self.average_covered(phis)
        for l in range(len(self.B)):
            res += self.amr_residual(l, self.lv(phis, l), self.lv(phis, l - 1) if l else None,
                                     self.lv(rhss, l))
        self.reflux_all(res, phis, -1)
        for l in range(1, len(self.B)):
            self.put_covered(l, self.lv(res, l - 1))
        self.res = res
        return res

    def cycle(self, l):
        if l == 0:
            MultiBoxAMROracle.cycle(self, 0)
            return
        I, Ic = self.ix[l], self.ix[l - 1]
        es = [b.full() for b in self.B[l]]
        rs = self.lv(self.res, l)
        self.relax(l, es, rs, self.n_pre)
        for i, e in zip(I, es):
            self.corr[i] = e
        r = self.amr_residual(l, es, None, rs, True)  # AMRRestrict
        self.put_covered(l, self.lv(self.res, l - 1), [average_down(x) for x in r])
        if self.reflux_on and self.reflux_cycle:
            # the coarse residual of the correction: its fine flux against a
            # zero coarse correction (es' ghosts: homogeneous CF, exchanged)
            self.reflux(l - 1, self.lv(self.res, l - 1), None, es, -1)
        self.cycle(l - 1)
        ecs = [self.corr[i] for i in Ic]
        self.prolong_const(l, es, ecs)
        for i, x in zip(I, self.amr_residual(l, es, ecs, rs, True)):  # AMRUpdateResidual
            self.res[i] = x
        des = [b.full() for b in self.B[l]]
        self.relax(l, des, self.lv(self.res, l), self.n_post)
        for e, de in zip(es, des):
            _valid(e)[...] = _valid(e) + _valid(de)

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
                self.reflux_all(self.res, es, -1)
                for l in range(1, n):
                    self.put_covered(l, self.lv(self.res, l - 1))
            self.corr = [None] * len(es)
            self.cycle(n - 1)
            self._accumulate(es)
        return es

    # ---------------------------------------------------------- diagnostics
    def composite_sum(self, xs, absolute=False):
        """sum over the uncovered cells of every level, dx_l^3 weights"""
        m = self.masked(xs)
        f = np.abs if absolute else (lambda a: a)
        return sum(self.weight(l) * self._sum(l, [f(_valid(x)) for x in self.lv(m, l)])
                   for l in range(len(self.B)))

    def num_uncovered(self):
        n = 0
        for l, bs in enumerate(self.B):
            n += sum(int(np.prod(b.shape)) for b in bs)
            if l + 1 < len(self.B):
                n -= int(self.cmask[l + 1].sum())
        return n


# ---- the coupled NL loop on a periodic hierarchy (mg_ic_code_amd/nl.py,
# _poisson_solve_amr with momentum=True, zero_mode="project", reflux=True):
# tests/nl_ref.py's multi-box loop with the projected momentum step of
# tests/momentum_periodic_ref.py in front of every K integrand, every solve
# the multilevel BiCGStab of RefluxOracle, every mean the composite one
def coupled_solve_amr(prm, boxes, n0, max_depth, profile, pot, pi_f, momentum_on=True,
                      reflux=True):
    """boxes[l]: the boxes of level l (level 0: the 0..n0-1 domain).  Returns
    dict(norms, iters, ks, nets, mom_iters, mom, mom_net): the composite
    max|Mom_i| of the final psi with the final total tensor, as it is and with
    the offset m_i psi_0^-6 of the last step's removed means added."""
    from tests import constraints_ref as C
    from tests import matter_ref as M
    from tests import momentum_ref as R
    from tests import phi_ref
    from tests import puncture_ref as P
    boxes = [[tuple(b) for b in bs] for bs in boxes]
    dom0 = (0, 0, 0, n0 - 1, n0 - 1, n0 - 1)
    L = prm.domainLength[0]
    dx0 = L / n0
    avg = prm.coefficient_average_type if prm.coefficient_average_type >= 0 else 0
    flat = [(b, dx0 / 2 ** l) for l, bs in enumerate(boxes) for b in bs]
    shapes = [(b[5] - b[2] + 1, b[4] - b[1] + 1, b[3] - b[0] + 1) for b, _ in flat]
    bh = prm.bh(constant_K=0.0)
    phi_g = [phi_ref.phi_on_box(profile, bh, b[:3], b[3:], dx) for b, dx in flat]
    pi = [M.pi_on_box(pi_f, L, b[:3], b[3:], dx) for b, dx in flat]

    def oracle_for(a):
        lv, n = [], 0
        for bs in boxes:
            lv.append(dict(boxes=bs, a=a[n:n + len(bs)], b=[np.ones(s) for s in shapes[n:n + len(bs)]]))
            n += len(bs)
        return RefluxOracle(lv, dx0, dom0, alpha=prm.alpha, beta=prm.beta, bc_lo=prm.bc_lo,
                            bc_hi=prm.bc_hi, bc_value=prm.bc_value, n_pre=prm.numMGsmooth,
                            n_post=prm.numMGsmooth, periodic=(1, 1, 1), reflux=reflux,
                            base=dict(nlevels=max_depth + 1, avg_type=avg, prolong_type=1,
                                      bottom_solver=1, n_pre=prm.numMGsmooth,
                                      n_post=prm.numMGsmooth, n_bottom=prm.numMGsmooth))

    kw = dict(num_mg_iterations=prm.numMGIterations, imax=prm.max_iterations, eps=prm.tolerance,
              norm_type=0)
    om = oracle_for([np.zeros(s) for s in shapes])  # -beta Lap: the momentum solves'
    nlev = len(boxes)

    def full(vs):
        return [np.pad(v, 1) for v in vs]

    volume_c = om.composite_sum(full([np.ones(s) for s in shapes]))

    def project(xs):
        m = om.composite_sum(xs) / volume_c
        for x in xs:
            _valid(x)[...] = _valid(x) - m
        return m

    def fill(xs):
        for l in range(nlev):
            om.fill(l, om.lv(xs, l), om.lv(xs, l - 1) if l else None, True)

    def solve(x, rhs):
        """the projected solve of momentum.MomentumSolver: (iterations, mean removed)"""
        m = project(rhs)
        if om.norm(om.masked(rhs), 0) == 0.0:
            for v in x:
                v[...] = 0.0
            it = 0
        else:
            for r in rhs:
                r *= -prm.beta
            it, _ = om.solve(x, rhs, **kw)
        project(x)
        fill(x)
        return it, m

    V = [[np.zeros(tuple(n + 2 for n in s)) for s in shapes] for _ in range(3)]
    U = [np.zeros(tuple(n + 2 for n in s)) for s in shapes]
    LW_g = None
    psi = [np.ones(tuple(n + 2 for n in s)) for s in shapes]
    dpsi = [np.zeros(tuple(n + 2 for n in s)) for s in shapes]
    zeros6 = [[np.zeros(s) for _ in range(6)] for s in shapes]
    out = dict(norms=[], iters=[], ks=[], nets=[], mom_iters=[])
    vol = L ** 3
    for _ in range(prm.max_NL_iterations):
        if momentum_on:
            S = [R.source(bh, b[:3], b[3:], dx, _valid(p), g, pot, q)[0]
                 for (b, dx), p, g, q in zip(flat, psi, phi_g, pi)]
            its, net = [], []
            for i in range(3):
                it, m = solve(V[i], full([s[i] for s in S]))
                its.append(it)
                net.append(m)
            rhs_u = [R.div_rhs([V[0][k], V[1][k], V[2][k]], dx) for k, (_, dx) in enumerate(flat)]
            its.append(solve(U, full(rhs_u))[0])
            W = [full([R.w([_valid(V[i][k]) for i in range(3)], U[k], dx)[c]
                       for k, (_, dx) in enumerate(flat)]) for c in range(3)]
            for w in W:
                fill(w)
            LW = [full([R.lw([W[i][k] for i in range(3)], dx)[c] for k, (_, dx) in enumerate(flat)])
                  for c in range(6)]
            for x in LW:
                fill(x)
            LW_g = [[LW[c][k] for c in range(6)] for k in range(len(flat))]
            out["mom_iters"].append(its)
            out["nets"].append(net)
        abar = [[_valid(a) for a in g] for g in LW_g] if momentum_on else zeros6
        bh["constant_K"] = 0.0
        integ = full([R.nl_integrand(bh, b[:3], b[3:], dx, p, g, pot, q, ab)
                      for (b, dx), p, g, q, ab in zip(flat, psi, phi_g, pi, abar)])
        bh["constant_K"] = -float(np.sqrt(abs(om.composite_sum(integ)) / vol))
        out["ks"].append(bh["constant_K"])
        ar = [R.nl_coefs(bh, b[:3], b[3:], dx, p, g, pot, q, ab)
              for (b, dx), p, g, q, ab in zip(flat, psi, phi_g, pi, abar)]
        oh = oracle_for([a for a, _ in ar])
        it, _ = oh.solve(dpsi, full([r for _, r in ar]), **kw)
        out["iters"].append(it)
        for l in range(nlev):  # QuadCFInterp, then set_update_psi0
            oh.fill(l, oh.lv(dpsi, l), oh.lv(dpsi, l - 1) if l else None, False)
        for p, d in zip(psi, dpsi):
            p += d
        nrm = oh.norm(oh.masked(dpsi), 2)
        out["norms"].append(nrm)
        if nrm < prm.tolerance or nrm > 1e5:
            break
    net = out["nets"][-1] if out["nets"] else [0.0, 0.0, 0.0]
    mom, mom_net = [[], [], []], [[], [], []]
    for k, ((b, dx), p, g, q) in enumerate(zip(flat, psi, phi_g, pi)):
        m3 = R.momentum(bh, b[:3], b[3:], dx, _valid(p), g, pot, q,
                        LW_g[k] if momentum_on else None)[0]
        _, psi_bh = P.bowen_york(C._table(bh, None), L, b[:3], b[3:], dx)
        w = (_valid(p) + psi_bh) ** -6.0
        for i in range(3):
            mom[i].append(m3[i])
            mom_net[i].append(m3[i] + net[i] * w)
    out["mom"] = [om.norm(om.masked(full(x)), 0) for x in mom]
    out["mom_net"] = [om.norm(om.masked(full(x)), 0) for x in mom_net]
    return out
