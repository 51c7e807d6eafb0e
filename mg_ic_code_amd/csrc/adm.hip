// adm.hip -- ADM mass, momentum and spin of the data as surface integrals over
// cell-aligned cubes of level 0 (gfx950, fp64).
//
// One thread per cell face.  For a face with centre x_f, outward normal
// s e_d, inner cell `in` and outer cell `out`:
//
//   g    = (psi[out] - psi[in]) / dx + s * d_d psi_bh(x_f)
//   A_kd = A^BY_kd(x_f) [ + 0.5 * (LW_kd[in] + LW_kd[out]) ]
//   mass = -(1 / (2 pi)) * g * dx^2
//   P_i  =  (1 / (8 pi)) * s * A_id * dx^2
//   J_i  =  (1 / (8 pi)) * s * (x_f x A_.d)_i * dx^2
//
// A^BY is get_Aij's expression (SetBinaryBH.H:24-53) in vector form, at the
// real-valued face centre: with n = l / r, l = x_f - x_n,
//
//   A_ij = 1.5 / r^2 * (n_i P_j + n_j P_i + (n_i n_j - delta_ij) (n . P))
//          - 3 / r^3 * ((n x J)_i n_j + (n x J)_j n_i)
//
// summed over the table's pairs in pair order, as the generators sum it.
// Only valid cells are read: each thread finds the boxes that own `in` and
// `out` in the box table.  The 7 terms are reduced in a fixed order (no
// floating-point atomics): xor-butterfly over the wave (32, 16, .. 1), the
// block's 4 waves in order through LDS, one partial of 7 per block; k_adm_finish
// adds a surface's partials in block order.  Faces are indexed per surface, not
// per box, so the sums do not depend on the box layout.  Built with
// -ffp-contract=off.
//
// Launches go through ledger::launch; with -fvisibility=hidden the ledger's
// registry is this library's own (mgic_adm_launch_ledger_dump).
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "adm.hpp"
#include "launch_ledger.hpp"

namespace mgic {
namespace adm {

namespace {

void check_launch() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    throw std::runtime_error(std::string("kernel launch: ") + hipGetErrorString(e));
}

// v[d] of three values without a register array indexed at run time
__device__ __forceinline__ double sel(int d, double v0, double v1, double v2) {
  return d == 0 ? v0 : (d == 1 ? v1 : v2);
}
__device__ __forceinline__ int seli(int d, int v0, int v1, int v2) {
  return d == 0 ? v0 : (d == 1 ? v1 : v2);
}

// the box of the table that holds cell (x, y, z), or -1; `hint` is tried first
__device__ __forceinline__ int find_box(const Box *__restrict__ boxes, int nbox, int hint, int x,
                                        int y, int z) {
  auto holds = [&](int i) {
    const Box &b = boxes[i];
    return x >= b.lo[0] && x <= b.hi[0] && y >= b.lo[1] && y <= b.hi[1] && z >= b.lo[2] &&
           z <= b.hi[2];
  };
  if (hint >= 0 && holds(hint)) return hint;
  for (int i = 0; i < nbox; ++i)
    if (holds(i)) return i;
  return -1;
}

__device__ __forceinline__ long cell_offset(const Box &b, int x, int y, int z) {
  return (long)(x - b.lo[0]) + (long)(y - b.lo[1]) * b.sy + (long)(z - b.lo[2]) * b.sz;
}

// one puncture's A_kd (k = 0, 1, 2) and m l_d / r^3 at the point (px, py, pz)
struct HoleTerms {
  double A0, A1, A2, dpsi;
};
__device__ __forceinline__ HoleTerms hole(const double *__restrict__ row, double px, double py,
                                          double pz, int d) {
  const double l0 = px - row[1], l1 = py - row[2], l2 = pz - row[3];
  const double r = sqrt(l0 * l0 + l1 * l1 + l2 * l2);
  const double n0 = l0 / r, n1 = l1 / r, n2 = l2 / r;
  const double P0 = row[4], P1 = row[5], P2 = row[6];
  const double J0 = row[7], J1 = row[8], J2 = row[9];
  const double nP = n0 * P0 + n1 * P1 + n2 * P2;
  const double c0 = n1 * J2 - n2 * J1, c1 = n2 * J0 - n0 * J2, c2 = n0 * J1 - n1 * J0;  // n x J
  const double nd = sel(d, n0, n1, n2), Pd = sel(d, P0, P1, P2), cd = sel(d, c0, c1, c2);
  const double fP = 1.5 / r / r, fJ = 3.0 / r / r / r;
  HoleTerms h;
  h.A0 = fP * (n0 * Pd + nd * P0 + (n0 * nd - (d == 0 ? 1.0 : 0.0)) * nP) - fJ * (c0 * nd + cd * n0);
  h.A1 = fP * (n1 * Pd + nd * P1 + (n1 * nd - (d == 1 ? 1.0 : 0.0)) * nP) - fJ * (c1 * nd + cd * n1);
  h.A2 = fP * (n2 * Pd + nd * P2 + (n2 * nd - (d == 2 ? 1.0 : 0.0)) * nP) - fJ * (c2 * nd + cd * n2);
  h.dpsi = row[0] * sel(d, l0, l1, l2) / (r * r * r);
  return h;
}

// The block's surface comes from its index (block-uniform), so a block never
// straddles two surfaces; lanes past the surface's last face carry +0.0.
template <bool LW>
__global__ __launch_bounds__(kBlock) void k_adm_surface(const Args a, const PunctureTable t) {
  __shared__ double red[kWaves][kTerms];
  int s = 0;
  while (s + 1 < a.nsurf && (int)blockIdx.x >= a.block0[s + 1]) ++s;
  const int n = a.half[s], w = 2 * n;
  const long ww = (long)w * w;
  const long f = (long)((int)blockIdx.x - a.block0[s]) * kBlock + threadIdx.x;
  double v[kTerms] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (f < 6 * ww) {
    const int q = (int)(f / ww);
    const long rem = f - q * ww;
    const int fb = (int)(rem / w), fa = (int)(rem - (long)fb * w);
    const int d = q >> 1, sg = (q & 1) ? 1 : -1;
    // the inner cell: normal index next to the face, tangential (a, b)
    const int cd = seli(d, a.centre[0], a.centre[1], a.centre[2]);
    const int m = sg > 0 ? cd + n : cd - n;  // the face's index along d
    const int nin = sg > 0 ? m - 1 : m;
    const int ta = (d == 0 ? a.centre[1] : a.centre[0]) - n + fa;
    const int tb = (d == 2 ? a.centre[1] : a.centre[2]) - n + fb;
    const int ix = d == 0 ? nin : ta;
    const int iy = d == 0 ? ta : (d == 1 ? nin : tb);
    const int iz = d == 2 ? nin : tb;
    const int ox = ix + (d == 0 ? sg : 0), oy = iy + (d == 1 ? sg : 0), oz = iz + (d == 2 ? sg : 0);
    // the face centre: bh_loc's coordinates, the normal one at the face
    const double px = (d == 0 ? (double)m : (double)ix + 0.5) * a.dx - a.domlen[0] / 2.0;
    const double py = (d == 1 ? (double)m : (double)iy + 0.5) * a.dx - a.domlen[1] / 2.0;
    const double pz = (d == 2 ? (double)m : (double)iz + 0.5) * a.dx - a.domlen[2] / 2.0;
    const double sd = (double)sg;
    const double dx2 = a.dx * a.dx;
    const int bi = find_box(a.boxes, a.nbox, -1, ix, iy, iz);
    const int bo = find_box(a.boxes, a.nbox, bi, ox, oy, oz);
    if (bi < 0 || bo < 0) {
      // no box owns the cell (the host refuses such a layout): nothing is read
      const double nan = __builtin_nan("");
      for (int c = 0; c < kTerms; ++c) v[c] = nan;
    } else {
      const Box &Bi = a.boxes[bi], &Bo = a.boxes[bo];
      const long oi = cell_offset(Bi, ix, iy, iz), oo = cell_offset(Bo, ox, oy, oz);
      // Bowen-York: the pairs in pair order, the first pair's value first
      const int npairs = (t.n + 1) / 2;
      double A0 = 0.0, A1 = 0.0, A2 = 0.0, dpsi = 0.0;
      for (int p = 0; p < npairs; ++p) {
        const HoleTerms h1 = hole(t.v[2 * p], px, py, pz, d);
        const HoleTerms h2 = hole(t.v[2 * p + 1], px, py, pz, d);
        const double e0 = h1.A0 + h2.A0, e1 = h1.A1 + h2.A1, e2 = h1.A2 + h2.A2;
        const double ed = h1.dpsi + h2.dpsi;
        if (p == 0) {
          A0 = e0, A1 = e1, A2 = e2, dpsi = ed;
        } else {
          A0 += e0, A1 += e1, A2 += e2, dpsi += ed;
        }
      }
      if constexpr (LW) {
        // LW_kd: the symmetric components 11, 12, 13, 22, 23, 33
        const int c0 = d, c1 = d == 0 ? 1 : (d == 1 ? 3 : 4), c2 = d == 0 ? 2 : (d == 1 ? 4 : 5);
        A0 = A0 + 0.5 * (Bi.lw[c0][oi] + Bo.lw[c0][oo]);
        A1 = A1 + 0.5 * (Bi.lw[c1][oi] + Bo.lw[c1][oo]);
        A2 = A2 + 0.5 * (Bi.lw[c2][oi] + Bo.lw[c2][oo]);
      }
      const double g = (Bo.psi[oo] - Bi.psi[oi]) / a.dx + sd * (-dpsi);
      const double c2pi = -1.0 / (2.0 * M_PI), c8pi = 1.0 / (8.0 * M_PI);
      v[0] = c2pi * g * dx2;
      v[1] = c8pi * sd * A0 * dx2;
      v[2] = c8pi * sd * A1 * dx2;
      v[3] = c8pi * sd * A2 * dx2;
      v[4] = c8pi * sd * (py * A2 - pz * A1) * dx2;
      v[5] = c8pi * sd * (pz * A0 - px * A2) * dx2;
      v[6] = c8pi * sd * (px * A1 - py * A0) * dx2;
    }
    if (a.terms) {
      double *o = a.terms + a.face0[s] * kTerms + (long)q * kTerms * ww + rem;
#pragma unroll
      for (int c = 0; c < kTerms; ++c) o[c * ww] = v[c];
    }
  }
  // in-wave: xor butterfly, every lane ends with the wave's sum
#pragma unroll
  for (int c = 0; c < kTerms; ++c) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v[c] = v[c] + __shfl_xor(v[c], off, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < kTerms; ++c) red[wave][c] = v[c];
  }
  __syncthreads();
  if (threadIdx.x < kTerms) {
    double acc = red[0][threadIdx.x];
    for (int k = 1; k < kWaves; ++k) acc = acc + red[k][threadIdx.x];
    a.partials[(long)blockIdx.x * kTerms + threadIdx.x] = acc;
  }
}

// one block per surface, thread c < 7 adds component c's partials in block order
__global__ __launch_bounds__(64) void k_adm_finish(const Args a) {
  const int s = blockIdx.x, c = threadIdx.x;
  if (s >= a.nsurf || c >= kTerms) return;
  const int b0 = a.block0[s], b1 = a.block0[s + 1];
  double acc = a.partials[(long)b0 * kTerms + c];
  for (int b = b0 + 1; b < b1; ++b) acc = acc + a.partials[(long)b * kTerms + c];
  a.sums[s * kTerms + c] = acc;
}

}  // namespace

void surface(const Args &a, const PunctureTable &t, bool lw, hipStream_t st) {
  const dim3 grid(a.block0[a.nsurf]), block(kBlock);
  if (lw)
    ledger::launch<k_adm_surface<true>>(grid, block, 0, st, a, t);
  else
    ledger::launch<k_adm_surface<false>>(grid, block, 0, st, a, t);
  check_launch();
}

void finish(const Args &a, hipStream_t st) {
  ledger::launch<k_adm_finish>(dim3(a.nsurf), dim3(64), 0, st, a);
  check_launch();
}

}  // namespace adm
}  // namespace mgic
