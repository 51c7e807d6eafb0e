// sample.hip -- a field of an AMR hierarchy interpolated at points (gfx950,
// fp64).  include/mgic_sample.h states the rule and the order of
// every expression; this file follows it line by line.
//
// One thread per point, one launch per call.  The thread finds its level (the
// finest whose boxes hold the point's cell, uncovered), then tries the 4^3
// stencil, the 2^3 stencil and the cell itself, from the requested order down.
// A stencil is walked plane by plane, row by row: each cell is looked up in the
// box table (the box of the point's own cell first), checked against the next
// finer level's boxes coarsened by 2, and read; the first cell that is not
// available ends the stencil, so a covered cell, a ghost cell or a cell
// outside every box is never read.  At most a row sum, a plane sum and the
// value are live: nothing is held per cell.  No atomics, no LDS; nothing
// depends on timing.  Built with -ffp-contract=off.
//
// Launches go through ledger::launch; with -fvisibility=hidden the ledger's
// registry is this library's own (mgic_sample_launch_ledger_dump).
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "launch_ledger.hpp"
#include "sample.hpp"

namespace mgic {
namespace sample {

namespace {

void check_launch() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    throw std::runtime_error(std::string("kernel launch: ") + hipGetErrorString(e));
}

// what a thread needs of its level: its boxes, the next finer level's boxes
// (f0 == f1: there is none) and the period of a cell index per direction: the
// level's cells in a periodic direction, kNoWrap in one that is not
struct Level {
  int b0, b1, f0, f1;
  int w0, w1, w2;
};

// beyond every index the host accepts (N_d 2^l < 2^27): wrap(i, kNoWrap) keeps
// an index inside the domain as it is and sends a negative one past every box,
// so a direction that is not periodic needs no branch of its own
constexpr int kNoWrap = 1 << 30;

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

__device__ __forceinline__ int wrap(int i, int n) {
  while (i < 0) i += n;
  while (i >= n) i -= n;
  return i;
}

__device__ __forceinline__ long cell_offset(const Box &b, int x, int y, int z) {
  return (long)(x - b.lo[0]) + (long)(y - b.lo[1]) * b.sy + (long)(z - b.lo[2]) * b.sz;
}

// the value of the W^3 stencil whose lowest cell is (x0, y0, z0), or false:
// one of its cells is not available.  Nothing is looked up or read after the
// first such cell (what was read until then was available).  The loops have one
// exit each: `ok` ends them, there is no return from inside.
template <int W>
__device__ __forceinline__ bool stencil(const Args &a, const Level &L, int hint, int x0, int y0,
                                        int z0, const Weights &wx, const Weights &wy,
                                        const Weights &wz, double &value) {
  bool ok = true;
  double vz = 0.0;
#pragma unroll 1
  for (int k = 0; k < W && ok; ++k) {
    const int z = wrap(z0 + k, L.w2);
    double vy = 0.0;
#pragma unroll 1
    for (int j = 0; j < W && ok; ++j) {
      const int y = wrap(y0 + j, L.w1);
      double vx = 0.0;
#pragma unroll
      for (int i = 0; i < W; ++i) {
        if (ok) {
          const int x = wrap(x0 + i, L.w0);
          const int b = find_box(a.boxes, L.b0, L.b1, hint, x, y, z);
          if (b < 0 || covered(a.boxes, L.f0, L.f1, x, y, z)) {
            ok = false;
          } else {
            const Box &B = a.boxes[b];
            const double p = wx.template at<W>(i) * B.u[cell_offset(B, x, y, z)];
            vx = i == 0 ? p : vx + p;
          }
        }
      }
      const double p = wy.template at<W>(j) * vx;
      vy = j == 0 ? p : vy + p;
    }
    const double p = wz.template at<W>(k) * vy;
    vz = k == 0 ? p : vz + p;
  }
  if (ok) value = vz;
  return ok;
}

// r = x + half inside [0, len), wrapped first in a periodic direction; false:
// the point is outside the domain
__device__ __forceinline__ bool relative(double x, double half, double len, int periodic,
                                         double &r) {
  r = x + half;
  if (periodic) {
    r = r - floor(r / len) * len;
    if (!(r >= 0.0 && r < len)) r = 0.0;
    return true;
  }
  return r >= 0.0 && r < len;
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

__device__ __forceinline__ Weights linear(double t) {
  return Weights{1.0 - t, t, t, t};
}

// ORDER: the order the candidates start from (1, 2 or 4)
template <int ORDER>
__global__ __launch_bounds__(kBlock) void k_sample_points(const Args a) {
  const int p = (int)blockIdx.x * kBlock + (int)threadIdx.x;
  if (p >= a.npts) return;
  const double x0 = a.xyz[3 * (long)p], x1 = a.xyz[3 * (long)p + 1], x2 = a.xyz[3 * (long)p + 2];
  double value = __builtin_nan("");
  int level = -1, order = 0;
  double r0 = 0.0, r1 = 0.0, r2 = 0.0;
  bool inside = __builtin_isfinite(x0) && __builtin_isfinite(x1) && __builtin_isfinite(x2);
  inside = inside && relative(x0, a.half[0], a.len[0], a.periodic[0], r0);
  inside = inside && relative(x1, a.half[1], a.len[1], a.periodic[1], r1);
  inside = inside && relative(x2, a.half[2], a.len[2], a.periodic[2], r2);
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
      L.w0 = a.periodic[0] ? n0 : kNoWrap;
      L.w1 = a.periodic[1] ? n1 : kNoWrap;
      L.w2 = a.periodic[2] ? n2 : kNoWrap;
      const int own = find_box(a.boxes, L.b0, L.b1, -1, c0, c1, c2);
      if (own < 0 || covered(a.boxes, L.f0, L.f1, c0, c1, c2)) continue;
      level = l;
      const double s0 = q0 - 0.5, s1 = q1 - 0.5, s2 = q2 - 0.5;
      const double f0 = floor(s0), f1 = floor(s1), f2 = floor(s2);
      const int i0 = (int)f0, i1 = (int)f1, i2 = (int)f2;
      const double t0 = s0 - f0, t1 = s1 - f1, t2 = s2 - f2;
      if constexpr (ORDER >= 4) {
        if (stencil<4>(a, L, own, i0 - 1, i1 - 1, i2 - 1, cubic(t0), cubic(t1), cubic(t2), value))
          order = 4;
      }
      if constexpr (ORDER >= 2) {
        if (order == 0 && stencil<2>(a, L, own, i0, i1, i2, linear(t0), linear(t1), linear(t2), value))
          order = 2;
      }
      if (order == 0) {
        const Box &B = a.boxes[own];
        value = B.u[cell_offset(B, c0, c1, c2)];
        order = 1;
      }
      break;
    }
  }
  a.values[p] = value;
  a.level[p] = level;
  a.order[p] = order;
}

}  // namespace

void points(const Args &a, int order, hipStream_t st) {
  const dim3 grid((a.npts + kBlock - 1) / kBlock), block(kBlock);
  if (order == 4)
    ledger::launch<k_sample_points<4>>(grid, block, 0, st, a);
  else if (order == 2)
    ledger::launch<k_sample_points<2>>(grid, block, 0, st, a);
  else
    ledger::launch<k_sample_points<1>>(grid, block, 0, st, a);
  check_launch();
}

}  // namespace sample
}  // namespace mgic
