"""fp32 restatement of the mixed-precision V-cycle -- TEST INFRASTRUCTURE ONLY.

The checker for mg_ic_code_amd's MixedMultiGrid (fp32 smoother / fp64
residual, BASELINE config C5) on one box.  numpy float32 arithmetic is IEEE
single with every operation rounded, so evaluating the kernels' expressions
in the same order gives the GPU's bits:

* GSRB pass (GSRBHELMHOLTZVC3D, Source/VariableCoeffPoissonOperatorF.ChF:91-136;
  lambda = 1/(alpha a + 6 beta/dx^2), VariableCoeffPoissonOperator.cpp:234-243)
  in float with the constants alpha, beta, 1/dx^2, 6 beta/dx^2 rounded from
  their fp64 values once;
* restrictResidual (RESTRICTRESVC3D, .ChF:401-434) in float, children summed
  in k, j, i order from 0;
* linear prolongIncrement in float (slopes as oracle/mgic_oracle.c
  orc_prolong);
* the fine residual rhs - L(phi) from the fp64 oracle (VCCOMPUTERES3D,
  .ChF:283-339), rounded to float once; phi += e in fp64;
* the MultiGrid::cycle schedule (pre-relax from zero, restrict, recurse,
  prolong, post-relax; relax(n_bottom) at the bottom) and the FMG schedule of
  mg_ic_code_amd/csrc/mixed.hpp.

Coefficients per depth: the fp64 oracle hierarchy (averaged in fp64) rounded
to float.  Homogeneous BC for the correction equation.  Parity unpinned
against the reference, which has no fp32 path; this pins the GPU kernels to
their stated float semantics.
"""
from __future__ import annotations

import numpy as np

import oracle

F = np.float32


class MixedOracle:
    def __init__(self, o: "oracle.OracleMG", alpha, beta, bc_lo=(0, 0, 0), bc_hi=(0, 0, 0),
                 n_pre=4, n_post=4, n_bottom=4, prolong_type=1):
        assert o.nbox == 1, "single box"
        assert prolong_type in (0, 1)
        self.prolong_type = prolong_type  # 0: piecewise constant, 1: linear (the oracle's own)
        self.o = o
        self.D = o.nlevels
        self.n_pre, self.n_post, self.n_bottom = n_pre, n_post, n_bottom
        self.bc_lo, self.bc_hi = tuple(bc_lo), tuple(bc_hi)
        self.alpha, self.beta = F(alpha), F(beta)
        self.lev = []
        for d in range(self.D):
            dx = o.dx(d)
            box = o.box(d, 0)
            lv = dict(box=box, a=o.get(d, oracle.ACOEF, 0).astype(F),
                      b=o.get(d, oracle.BCOEF, 0).astype(F),
                      dxinv=F(1.0 / (dx * dx)), lamshift=F(2.0 * 3 * beta / (dx * dx)))
            shape = o.shape(d, 0, 1)
            lv["e"] = np.zeros(shape, F)
            lv["r"] = np.zeros(o.shape(d, 0), F)
            self.lev.append(lv)
        self.phi = None

    # ---------------------------------------------------------------- kernels
    def _fill_bc(self, u):
        """homogeneous BC images into the ghost faces (DiriBC: 0 - near,
        NeumBC: near); edges/corners untouched"""
        z = F(0)
        for d, (lo, hi) in enumerate(zip(self.bc_lo, self.bc_hi)):
            ax = 2 - d  # (z, y, x) array axes
            sl = [slice(1, -1)] * 3
            g0, n0, g1, n1 = list(sl), list(sl), list(sl), list(sl)
            g0[ax], n0[ax], g1[ax], n1[ax] = 0, 1, -1, -2
            u[tuple(g0)] = (z - u[tuple(n0)]) if lo == 0 else u[tuple(n0)]
            u[tuple(g1)] = (z - u[tuple(n1)]) if hi == 0 else u[tuple(n1)]

    def _colour(self, lv, shape):
        b = lv["box"]
        k, j, i = np.meshgrid(np.arange(shape[0]) + b[2], np.arange(shape[1]) + b[1],
                              np.arange(shape[2]) + b[0], indexing="ij")
        return (i + j + k) % 2

    def _gsrb_pass(self, d, u, rhs, colour):
        lv = self.lev[d]
        self._fill_bc(u)
        c = u[1:-1, 1:-1, 1:-1]
        xm, xp = u[1:-1, 1:-1, :-2], u[1:-1, 1:-1, 2:]
        ym, yp = u[1:-1, :-2, 1:-1], u[1:-1, 2:, 1:-1]
        zm, zp = u[:-2, 1:-1, 1:-1], u[2:, 1:-1, 1:-1]
        two = F(2)
        tx = (xp + xm) - two * c
        ty = (yp + ym) - two * c
        tz = (zp + zm) - two * c
        lap = (tx + ty) + tz
        a, b = lv["a"], lv["b"]
        lof = self.alpha * a * c
        ldpsi = lap * lv["dxinv"] * b
        lof = lof - self.beta * ldpsi
        lam = F(1) / (a * self.alpha + lv["lamshift"])
        new = c - lam * (lof - rhs)
        m = self._colour(lv, c.shape) == colour
        c[m] = new[m]

    def relax(self, d, e, r, n):
        for _ in range(n):
            self._gsrb_pass(d, e, r, 0)
            self._gsrb_pass(d, e, r, 1)

    def restrict(self, d, e, r):
        """rc = R(r - L e) in float (RESTRICTRESVC3D)"""
        lv = self.lev[d]
        self._fill_bc(e)
        c = e[1:-1, 1:-1, 1:-1]
        two = F(2)
        tx = (e[1:-1, 1:-1, 2:] + e[1:-1, 1:-1, :-2]) - two * c
        ty = (e[1:-1, 2:, 1:-1] + e[1:-1, :-2, 1:-1]) - two * c
        tz = (e[2:, 1:-1, 1:-1] + e[:-2, 1:-1, 1:-1]) - two * c
        ldpsi = (tx + ty) + tz
        lof = self.alpha * lv["a"] * c
        ldpsi = ldpsi * lv["dxinv"] * self.beta * lv["b"]
        lof = lof - ldpsi
        t = (r - lof) / F(8)
        s = np.zeros(tuple(v // 2 for v in c.shape), F)
        for kk in range(2):
            for jj in range(2):
                for ii in range(2):
                    s = s + t[kk::2, jj::2, ii::2]
        return s

    def prolong(self, d, e, ec):
        """e += P ec (linear, one-sided at the domain faces, or piecewise
        constant: every child takes its parent's value; single box)"""
        c = ec[1:-1, 1:-1, 1:-1]
        if self.prolong_type == 0:
            f = e[1:-1, 1:-1, 1:-1]
            for kk in range(2):
                for jj in range(2):
                    for ii in range(2):
                        f[kk::2, jj::2, ii::2] = f[kk::2, jj::2, ii::2] + c
            return
        nzc, nyc, nxc = c.shape
        out = [None] * 3
        for dd in range(3):  # x, y, z
            ax = 2 - dd
            n = c.shape[ax]
            idx = np.arange(n)
            lo = np.take(ec, idx, axis=ax)[tuple(slice(1, -1) if a != ax else slice(None) for a in range(3))]
            hi = np.take(ec, idx + 2, axis=ax)[tuple(slice(1, -1) if a != ax else slice(None) for a in range(3))]
            shp = [1, 1, 1]
            shp[ax] = n
            has_lo = (idx > 0).reshape(shp)
            has_hi = (idx < n - 1).reshape(shp)
            sl_hi = hi - c
            sl_lo = c - lo
            dhi = np.where(has_hi, sl_hi, sl_lo) * F(0.25)
            dlo = np.where(~has_lo, sl_hi, sl_lo) * F(-0.25)
            ok = np.broadcast_to(has_lo | has_hi, c.shape)
            out[dd] = (dlo, dhi, ok)
        f = e[1:-1, 1:-1, 1:-1]
        for kk in range(2):
            for jj in range(2):
                for ii in range(2):
                    v = c.copy()
                    for dd, sel in ((0, ii), (1, jj), (2, kk)):
                        dlo, dhi, ok = out[dd]
                        t = dhi if sel else dlo
                        v = np.where(ok, v + t, v)
                    f[kk::2, jj::2, ii::2] = f[kk::2, jj::2, ii::2] + v

    # ---------------------------------------------------------------- drivers
    def init_residual(self, phi64):
        o = self.o
        self.phi = np.array(phi64, dtype=np.float64)
        o.set(0, oracle.PHI, 0, self.phi)
        o.residual(0, oracle.RESID, oracle.PHI, oracle.RHS, 0)
        r64 = o.get(0, oracle.RESID, 0)
        self.lev[0]["r"] = r64.astype(F)
        return r64

    def cycle(self, d, e_zero, acc):
        lv = self.lev[d]
        if e_zero:
            lv["e"][...] = 0
        if d == self.D - 1:
            self.relax(d, lv["e"], lv["r"], self.n_bottom)
        else:
            self.relax(d, lv["e"], lv["r"], self.n_pre)
            self.lev[d + 1]["r"] = self.restrict(d, lv["e"], lv["r"])
            self.cycle(d + 1, True, False)
            self.prolong(d, lv["e"], self.lev[d + 1]["e"])
            self.relax(d, lv["e"], lv["r"], self.n_post)
        if acc:
            self.phi = self.phi + lv["e"][1:-1, 1:-1, 1:-1].astype(np.float64)

    def iteration(self):
        self.cycle(0, True, True)
        return self.init_residual(self.phi)

    def fmg(self, ncycles=1):
        D = self.D
        if D == 1:
            self.cycle(0, True, True)
            return self.init_residual(self.phi)
        for d in range(D - 1):
            self.lev[d]["e"][...] = 0
            self.lev[d + 1]["r"] = self.restrict(d, self.lev[d]["e"], self.lev[d]["r"])
        B = self.lev[D - 1]
        B["e"][...] = 0
        self.relax(D - 1, B["e"], B["r"], self.n_bottom)
        for d in range(D - 2, -1, -1):
            lv = self.lev[d]
            lv["e"][...] = 0
            self.prolong(d, lv["e"], self.lev[d + 1]["e"])
            for c in range(ncycles):
                self.cycle(d, False, d == 0 and c == ncycles - 1)
        return self.init_residual(self.phi)
