// horizon.hip -- the expansion of a surface at points of an AMR hierarchy
// (gfx950, fp64).  include/mgic_horizon.h states the rule and the
// order of every expression; this file follows it line by line.
//
// One thread per point, one launch per call.  The thread finds its level as
// sample.hip does (the finest whose boxes hold the point's cell, uncovered),
// then tries the 4^3 stencil and the 2^3 stencil.  A stencil is walked plane by
// plane, row by row: each cell is looked up in the box table (the box of the
// point's own cell first), checked against the next finer level's boxes
// coarsened by 2, and read; the first cell that is not available ends the
// stencil, so a covered cell, a ghost cell or a cell outside every box is never
// read.  One walk forms psi's value and its three derivatives (two row sums,
// three plane sums, four totals) and, with LW, the values of the six LW_ij on
// the same cells.  The analytic parts (sum m / r, its gradient, the Bowen-York
// tensor) are taken at the real-valued point, the table's pairs in pair order.
// Every direction is not periodic (the host refuses the others), so an index is
// never wrapped: one outside the domain is in no box.  No atomics, no LDS;
// nothing depends on timing.  Built with -ffp-contract=off.
//
// Launches go through ledger::launch; with -fvisibility=hidden the ledger's
// registry is this library's own (mgic_horizon_launch_ledger_dump).
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "horizon.hpp"
#include "launch_ledger.hpp"

namespace mgic {
namespace horizon {

namespace {

void check_launch() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    throw std::runtime_error(std::string("kernel launch: ") + hipGetErrorString(e));
}

// what a thread needs of its level: its boxes and the next finer level's
// (f0 == f1: there is none)
struct Level {
  int b0, b1, f0, f1;
};

// the weights of one direction (W = 2 uses the first two); at<W>(k) selects
// without an array indexed at run time, which would go to LDS or scratch
struct Weights {
  double w0, w1, w2, w3;
  template <int W>
  __device__ __forceinline__ double at(int k) const {
    if constexpr (W == 2) return k == 0 ? w0 : w1;
    return k == 0 ? w0 : (k == 1 ? w1 : (k == 2 ? w2 : w3));
  }
};

// what one stencil gives: psi's value and gradient (per cell, not yet divided
// by dx) and the six LW_ij
struct Sums {
  double v, gx, gy, gz;
  double lw[6];
};

// the box of b0 .. b1 - 1 that holds cell (x, y, z), or -1; `hint` is tried first
__device__ __forceinline__ int find_box(const Box *__restrict__ boxes, int b0, int b1, int hint,
                                        int x, int y, int z) {
  auto holds = [&](int i) {
    const Box &b = boxes[i];
    return x >= b.lo[0] && x <= b.hi[0] && y >= b.lo[1] && y <= b.hi[1] && z >= b.lo[2] &&
           z <= b.hi[2];
  };
  if (hint >= 0 && holds(hint)) return hint;
  for (int i = b0; i < b1; ++i)
    if (holds(i)) return i;
  return -1;
}

// whether cell (x, y, z) lies in a box of f0 .. f1 - 1 coarsened by 2
__device__ __forceinline__ bool covered(const Box *__restrict__ boxes, int f0, int f1, int x,
                                        int y, int z) {
  for (int i = f0; i < f1; ++i) {
    const Box &b = boxes[i];
    if (x >= (b.lo[0] >> 1) && x <= (b.hi[0] >> 1) && y >= (b.lo[1] >> 1) &&
        y <= (b.hi[1] >> 1) && z >= (b.lo[2] >> 1) && z <= (b.hi[2] >> 1))
      return true;
  }
  return false;
}

__device__ __forceinline__ long cell_offset(const Box &b, int x, int y, int z) {
  return (long)(x - b.lo[0]) + (long)(y - b.lo[1]) * b.sy + (long)(z - b.lo[2]) * b.sz;
}

// the sums of the W^3 stencil whose lowest cell is (x0, y0, z0), or false: one
// of its cells is not available.  Nothing is looked up or read after the first
// such cell (what was read until then was available).  The loops have one exit
// each: `ok` ends them, there is no return from inside.
template <int W, bool LW>
__device__ __forceinline__ bool stencil(const Args &a, const Level &L, int hint, int x0, int y0,
                                        int z0, const Weights &wx, const Weights &dwx,
                                        const Weights &wy, const Weights &dwy, const Weights &wz,
                                        const Weights &dwz, Sums &out) {
  bool ok = true;
  double v = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
  double lv[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
  for (int k = 0; k < W && ok; ++k) {
    const int z = z0 + k;
    double pv = 0.0, px = 0.0, py = 0.0;
    double lp[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (int j = 0; j < W && ok; ++j) {
      const int y = y0 + j;
      double rv = 0.0, rd = 0.0;
      double lr[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int i = 0; i < W; ++i) {
        if (ok) {
          const int x = x0 + i;
          const int b = find_box(a.boxes, L.b0, L.b1, hint, x, y, z);
          if (b < 0 || covered(a.boxes, L.f0, L.f1, x, y, z)) {
            ok = false;
          } else {
            const Box &B = a.boxes[b];
            const long o = cell_offset(B, x, y, z);
            const double u = B.psi[o];
            const double w = wx.template at<W>(i), dw = dwx.template at<W>(i);
            const double p = w * u, q = dw * u;
            rv = i == 0 ? p : rv + p;
            rd = i == 0 ? q : rd + q;
            if constexpr (LW) {
#pragma unroll
              for (int c = 0; c < 6; ++c) {
                const double s = w * B.lw[c][o];
                lr[c] = i == 0 ? s : lr[c] + s;
              }
            }
          }
        }
      }
      const double w = wy.template at<W>(j), dw = dwy.template at<W>(j);
      const double p = w * rv, q = w * rd, r = dw * rv;
      pv = j == 0 ? p : pv + p;
      px = j == 0 ? q : px + q;
      py = j == 0 ? r : py + r;
      if constexpr (LW) {
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          const double s = w * lr[c];
          lp[c] = j == 0 ? s : lp[c] + s;
        }
      }
    }
    const double w = wz.template at<W>(k), dw = dwz.template at<W>(k);
    const double p = w * pv, q = w * px, r = w * py, s = dw * pv;
    v = k == 0 ? p : v + p;
    gx = k == 0 ? q : gx + q;
    gy = k == 0 ? r : gy + r;
    gz = k == 0 ? s : gz + s;
    if constexpr (LW) {
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        const double t = w * lp[c];
        lv[c] = k == 0 ? t : lv[c] + t;
      }
    }
  }
  if (ok) {
    out.v = v, out.gx = gx, out.gy = gy, out.gz = gz;
#pragma unroll
    for (int c = 0; c < 6; ++c) out.lw[c] = lv[c];
  }
  return ok;
}

__device__ __forceinline__ Weights cubic(double t) {
  const double tm1 = t - 1.0, tm2 = t - 2.0, tp1 = t + 1.0;
  Weights w;
  w.w0 = -t * tm1 * tm2 / 6.0;
  w.w1 = tp1 * tm1 * tm2 / 2.0;
  w.w2 = -tp1 * t * tm2 / 2.0;
  w.w3 = tp1 * t * tm1 / 6.0;
  return w;
}

// d/dt of cubic(t): the product rule on the same factors
__device__ __forceinline__ Weights dcubic(double t) {
  const double tm1 = t - 1.0, tm2 = t - 2.0, tp1 = t + 1.0;
  const double a = tm1 * tm2, b = t * tm2, c = t * tm1, d = tp1 * tm2, e = tp1 * tm1, f = tp1 * t;
  Weights w;
  w.w0 = -((a + b) + c) / 6.0;
  w.w1 = ((a + d) + e) / 2.0;
  w.w2 = -((b + d) + f) / 2.0;
  w.w3 = ((c + e) + f) / 6.0;
  return w;
}

__device__ __forceinline__ Weights linear(double t) {
  return Weights{1.0 - t, t, t, t};
}

__device__ __forceinline__ Weights dlinear() {
  return Weights{-1.0, 1.0, 1.0, 1.0};
}

// one puncture at the point (px, py, pz): m / r, m l_d / r^3 and the six
// A_ij (11, 12, 13, 22, 23, 33) of adm.hip's vector form
struct HoleTerms {
  double psi, d0, d1, d2;
  double A[6];
};
__device__ __forceinline__ HoleTerms hole(const double *__restrict__ row, double px, double py,
                                          double pz) {
  const double l0 = px - row[1], l1 = py - row[2], l2 = pz - row[3];
  const double r = sqrt(l0 * l0 + l1 * l1 + l2 * l2);
  const double n0 = l0 / r, n1 = l1 / r, n2 = l2 / r;
  const double P0 = row[4], P1 = row[5], P2 = row[6];
  const double J0 = row[7], J1 = row[8], J2 = row[9];
  const double nP = n0 * P0 + n1 * P1 + n2 * P2;
  const double c0 = n1 * J2 - n2 * J1, c1 = n2 * J0 - n0 * J2, c2 = n0 * J1 - n1 * J0;  // n x J
  const double fP = 1.5 / r / r, fJ = 3.0 / r / r / r;
  const double r3 = r * r * r;
  HoleTerms h;
  h.psi = row[0] / r;
  h.d0 = row[0] * l0 / r3;
  h.d1 = row[0] * l1 / r3;
  h.d2 = row[0] * l2 / r3;
  h.A[0] = fP * (n0 * P0 + n0 * P0 + (n0 * n0 - 1.0) * nP) - fJ * (c0 * n0 + c0 * n0);
  h.A[1] = fP * (n0 * P1 + n1 * P0 + (n0 * n1 - 0.0) * nP) - fJ * (c0 * n1 + c1 * n0);
  h.A[2] = fP * (n0 * P2 + n2 * P0 + (n0 * n2 - 0.0) * nP) - fJ * (c0 * n2 + c2 * n0);
  h.A[3] = fP * (n1 * P1 + n1 * P1 + (n1 * n1 - 1.0) * nP) - fJ * (c1 * n1 + c1 * n1);
  h.A[4] = fP * (n1 * P2 + n2 * P1 + (n1 * n2 - 0.0) * nP) - fJ * (c1 * n2 + c2 * n1);
  h.A[5] = fP * (n2 * P2 + n2 * P2 + (n2 * n2 - 1.0) * nP) - fJ * (c2 * n2 + c2 * n2);
  return h;
}

template <bool LW>
__global__ __launch_bounds__(kBlock) void k_horizon_expansion(const Args a, const PunctureTable t) {
  const int p = (int)blockIdx.x * kBlock + (int)threadIdx.x;
  if (p >= a.npts) return;
  const double x0 = a.xyz[3 * (long)p], x1 = a.xyz[3 * (long)p + 1], x2 = a.xyz[3 * (long)p + 2];
  const double nan = __builtin_nan("");
  double theta = nan, psi = nan, dp0 = nan, dp1 = nan, dp2 = nan, Ann = nan;
  int level = -1, order = 0;
  const double r0 = x0 + a.half[0], r1 = x1 + a.half[1], r2 = x2 + a.half[2];
  bool inside = __builtin_isfinite(x0) && __builtin_isfinite(x1) && __builtin_isfinite(x2);
  inside = inside && r0 >= 0.0 && r0 < a.len[0] && r1 >= 0.0 && r1 < a.len[1] && r2 >= 0.0 &&
           r2 < a.len[2];
  if (inside) {
    for (int l = a.nlev - 1; l >= 0; --l) {
      const double dx = a.dx[l];
      const double q0 = r0 / dx, q1 = r1 / dx, q2 = r2 / dx;
      // (r just below len can give q = N 2^l after rounding: the last cell)
      const int n0 = a.n0[0] << l, n1 = a.n0[1] << l, n2 = a.n0[2] << l;
      const int c0 = min((int)floor(q0), n0 - 1), c1 = min((int)floor(q1), n1 - 1),
                c2 = min((int)floor(q2), n2 - 1);
      Level L;
      L.b0 = a.box0[l];
      L.b1 = a.box0[l + 1];
      L.f0 = L.b1;
      L.f1 = l + 1 < a.nlev ? a.box0[l + 2] : L.b1;
      const int own = find_box(a.boxes, L.b0, L.b1, -1, c0, c1, c2);
      if (own < 0 || covered(a.boxes, L.f0, L.f1, c0, c1, c2)) continue;
      level = l;
      const double s0 = q0 - 0.5, s1 = q1 - 0.5, s2 = q2 - 0.5;
      const double f0 = floor(s0), f1 = floor(s1), f2 = floor(s2);
      const int i0 = (int)f0, i1 = (int)f1, i2 = (int)f2;
      const double t0 = s0 - f0, t1 = s1 - f1, t2 = s2 - f2;
      Sums S;
      if (stencil<4, LW>(a, L, own, i0 - 1, i1 - 1, i2 - 1, cubic(t0), dcubic(t0), cubic(t1),
                         dcubic(t1), cubic(t2), dcubic(t2), S))
        order = 4;
      if (order == 0 && stencil<2, LW>(a, L, own, i0, i1, i2, linear(t0), dlinear(), linear(t1),
                                       dlinear(), linear(t2), dlinear(), S))
        order = 2;
      if (order != 0) {
        const double g0 = S.gx / dx, g1 = S.gy / dx, g2 = S.gz / dx;
        // the analytic parts: the pairs in pair order, the first pair's value first
        const int npairs = (t.n + 1) / 2;
        double pb = 0.0, d0 = 0.0, d1 = 0.0, d2 = 0.0;
        double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
        for (int q = 0; q < npairs; ++q) {
          const HoleTerms h1 = hole(t.v[2 * q], x0, x1, x2);
          const HoleTerms h2 = hole(t.v[2 * q + 1], x0, x1, x2);
          const double ep = h1.psi + h2.psi, e0 = h1.d0 + h2.d0, e1 = h1.d1 + h2.d1,
                       e2 = h1.d2 + h2.d2;
          pb = q == 0 ? ep : pb + ep;
          d0 = q == 0 ? e0 : d0 + e0;
          d1 = q == 0 ? e1 : d1 + e1;
          d2 = q == 0 ? e2 : d2 + e2;
#pragma unroll
          for (int c = 0; c < 6; ++c) {
            const double e = h1.A[c] + h2.A[c];
            A[c] = q == 0 ? e : A[c] + e;
          }
        }
        if constexpr (LW) {
#pragma unroll
          for (int c = 0; c < 6; ++c) A[c] = A[c] + S.lw[c];
        }
        psi = S.v + pb;
        dp0 = g0 - d0;
        dp1 = g1 - d1;
        dp2 = g2 - d2;
        const double m0 = a.normal[3 * (long)p], m1 = a.normal[3 * (long)p + 1],
                     m2 = a.normal[3 * (long)p + 2];
        Ann = ((m0 * m0 * A[0] + m1 * m1 * A[3]) + m2 * m2 * A[5]) +
              2.0 * ((m0 * m1 * A[1] + m0 * m2 * A[2]) + m1 * m2 * A[4]);
        const double p2 = psi * psi, p3 = p2 * psi, p6 = p3 * p3;
        const double dn = (m0 * dp0 + m1 * dp1) + m2 * dp2;
        theta = (a.divn[p] / p2 + 4.0 * dn / p3) + Ann / p6;
      }
      break;
    }
  }
  double *o = a.out + (long)p * kTerms;
  o[0] = theta;
  o[1] = psi;
  o[2] = dp0;
  o[3] = dp1;
  o[4] = dp2;
  o[5] = Ann;
  a.level[p] = level;
  a.order[p] = order;
}

}  // namespace

void expansion(const Args &a, const PunctureTable &t, bool lw, hipStream_t st) {
  const dim3 grid((a.npts + kBlock - 1) / kBlock), block(kBlock);
  if (lw)
    ledger::launch<k_horizon_expansion<true>>(grid, block, 0, st, a, t);
  else
    ledger::launch<k_horizon_expansion<false>>(grid, block, 0, st, a, t);
  check_launch();
}

}  // namespace horizon
}  // namespace mgic
