// ctt.hip -- the conformal transverse-traceless step's kernels (gfx950, fp64).
//
// The longitudinal piece LW_ij of the total tensor Abar_ij = Abar^BY_ij +
// LW_ij comes from a vector W_i = V_i + D_i U.  The Poisson
// solves for V_i and U are the library's own; what is here are the four
// streaming stencils between them.  One thread per cell of a TX x TY tile per
// z plane, as the generator kernels of kernels.hip; built with
// -ffp-contract=off, each expression is evaluated left to right as written, so
// a numpy restatement in the same association gives the same bits.
//
// Launches go through ledger::launch; with -fvisibility=hidden the ledger's
// registry is this library's own (mgic_ctt_launch_ledger_dump).
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "ctt.hpp"
#include "launch_ledger.hpp"

namespace mgic {
namespace ctt {

namespace {

constexpr int TX = 64;  // one wavefront along x
constexpr int TY = 4;   // 4 waves per block
const dim3 kBlock(TX, TY, 1);

dim3 grid_cells(int nx, int ny, int nz) { return dim3((nx + TX - 1) / TX, (ny + TY - 1) / TY, nz); }

void check_launch() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    throw std::runtime_error(std::string("kernel launch: ") + hipGetErrorString(e));
}

// the project's centred difference along the direction of stride st
__device__ __forceinline__ double cdiff(const double *__restrict__ f, long idx, long st, double h) {
  return h * (f[idx + st] - f[idx - st]);
}

struct Vec3In {
  const double *p[3];
};
struct Vec3Out {
  double *p[3];
};
struct Sym6Out {
  double *p[6];
};

// 3 x 2 neighbour loads + 1 store per cell: 8 B compulsory read per operand
// cell (each value is a neighbour of two cells along its own direction only)
__global__ __launch_bounds__(256) void k_ctt_div_rhs(double *__restrict__ out, const Vec3In v,
                                                     const BoxGeom g, double dx) {
  const int i = blockIdx.x * TX + threadIdx.x;
  const int j = blockIdx.y * TY + threadIdx.y;
  const int k = blockIdx.z;
  if (i >= g.nx || j >= g.ny) return;
  const long idx = (long)i + (long)j * g.sy + (long)k * g.sz;
  const double h = 0.5 / dx;
  const double dxx = cdiff(v.p[0], idx, 1, h);
  const double dyy = cdiff(v.p[1], idx, g.sy, h);
  const double dzz = cdiff(v.p[2], idx, g.sz, h);
  out[idx] = -0.25 * (dxx + dyy + dzz);
}

// U's six neighbours are read once per cell; three outputs in one pass
__global__ __launch_bounds__(256) void k_ctt_w(const Vec3Out w, const Vec3In v,
                                               const double *__restrict__ u, const BoxGeom g,
                                               double dx) {
  const int i = blockIdx.x * TX + threadIdx.x;
  const int j = blockIdx.y * TY + threadIdx.y;
  const int k = blockIdx.z;
  if (i >= g.nx || j >= g.ny) return;
  const long idx = (long)i + (long)j * g.sy + (long)k * g.sz;
  const double h = 0.5 / dx;
  w.p[0][idx] = v.p[0][idx] + cdiff(u, idx, 1, h);
  w.p[1][idx] = v.p[1][idx] + cdiff(u, idx, g.sy, h);
  w.p[2][idx] = v.p[2][idx] + cdiff(u, idx, g.sz, h);
}

// d[a][b] = D_a W_b: the 18 neighbour values of the three W, nine
// differences, the divergence formed once
__global__ __launch_bounds__(256) void k_ctt_lw(const Sym6Out o, const Vec3In w, const BoxGeom g,
                                                double dx) {
  const int i = blockIdx.x * TX + threadIdx.x;
  const int j = blockIdx.y * TY + threadIdx.y;
  const int k = blockIdx.z;
  if (i >= g.nx || j >= g.ny) return;
  const long idx = (long)i + (long)j * g.sy + (long)k * g.sz;
  const double h = 0.5 / dx;
  const long st[3] = {1, g.sy, g.sz};
  double d[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) d[a][b] = cdiff(w.p[b], idx, st[a], h);
  const double div = d[0][0] + d[1][1] + d[2][2];
  const double third = (2.0 / 3.0) * div;
  o.p[0][idx] = 2.0 * d[0][0] - third;
  o.p[1][idx] = d[0][1] + d[1][0];
  o.p[2][idx] = d[0][2] + d[2][0];
  o.p[3][idx] = 2.0 * d[1][1] - third;
  o.p[4][idx] = d[1][2] + d[2][1];
  o.p[5][idx] = 2.0 * d[2][2] - third;
}

// one thread per cell of the face: (na, nb) cells spanned by strides (sa, sb);
// near = offset of the face's first cell, step = one cell inwards
__global__ __launch_bounds__(256) void k_ctt_extrap(double *__restrict__ f, int na, int nb, long sa,
                                                    long sb, long near, long step) {
  const int a = blockIdx.x * TX + threadIdx.x;
  const int b = blockIdx.y * TY + threadIdx.y;
  if (a >= na || b >= nb) return;
  const long c = near + (long)a * sa + (long)b * sb;
  f[c - step] = 2.0 * f[c] - f[c + step];
}

}  // namespace

void div_rhs(double *out, const double *const v[3], const BoxGeom &g, double dx, hipStream_t st) {
  if (g.nx <= 0 || g.ny <= 0 || g.nz <= 0) return;
  const Vec3In vi{{v[0], v[1], v[2]}};
  ledger::launch<k_ctt_div_rhs>(grid_cells(g.nx, g.ny, g.nz), kBlock, 0, st, out, vi, g, dx);
  check_launch();
}

void w(double *const wout[3], const double *const v[3], const double *u, const BoxGeom &g,
       double dx, hipStream_t st) {
  if (g.nx <= 0 || g.ny <= 0 || g.nz <= 0) return;
  const Vec3Out wo{{wout[0], wout[1], wout[2]}};
  const Vec3In vi{{v[0], v[1], v[2]}};
  ledger::launch<k_ctt_w>(grid_cells(g.nx, g.ny, g.nz), kBlock, 0, st, wo, vi, u, g, dx);
  check_launch();
}

void lw(double *const out[6], const double *const wv[3], const BoxGeom &g, double dx,
        hipStream_t st) {
  if (g.nx <= 0 || g.ny <= 0 || g.nz <= 0) return;
  const Sym6Out o{{out[0], out[1], out[2], out[3], out[4], out[5]}};
  const Vec3In wi{{wv[0], wv[1], wv[2]}};
  ledger::launch<k_ctt_lw>(grid_cells(g.nx, g.ny, g.nz), kBlock, 0, st, o, wi, g, dx);
  check_launch();
}

void extrap(double *f, const BoxGeom &g, int face, hipStream_t st) {
  if (g.nx <= 0 || g.ny <= 0 || g.nz <= 0) return;
  if (face < 0 || face > 5) throw std::invalid_argument("face outside 0..5");
  const int dir = face >> 1, side = face & 1;
  const int n[3] = {g.nx, g.ny, g.nz};
  const long s[3] = {1, g.sy, g.sz};
  if (n[dir] < 2) throw std::invalid_argument("extrapolation needs two cells along the face normal");
  // the two directions of the face, the faster one first (coalesced for y and z faces)
  const int da = dir == 0 ? 1 : 0, db = dir == 2 ? 1 : 2;
  const long near = side ? (long)(n[dir] - 1) * s[dir] : 0;
  const long step = side ? -s[dir] : s[dir];
  ledger::launch<k_ctt_extrap>(grid_cells(n[da], n[db], 1), kBlock, 0, st, f, n[da], n[db], s[da],
                               s[db], near, step);
  check_launch();
}

}  // namespace ctt
}  // namespace mgic
