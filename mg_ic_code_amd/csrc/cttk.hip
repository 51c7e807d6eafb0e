// cttk.hip -- the K(x) kernels of the CTTK method (gfx950, fp64; DESIGN.md
// 3q, include/mgic_cttk.h).
//
// Three streaming kernels, one thread per cell of a TX x TY tile per z plane
// as the generator kernels of kernels.hip and k_zm_shift.  One launch covers
// every local box: a block finds its box in the table (a scan of at most
// `nrow` rows, uniform over the block), then its tile and plane.  Nothing is
// shared between threads: no LDS.  k_cttk_K counts refused cells with an
// integer atomic, whose result does not depend on the order; there is no
// floating-point reduction.  Bytes per cell: K 16, source 8 + 56 (K's six
// neighbours come from cache lines the x-neighbours and the next planes'
// blocks share), constraints 88 + the same neighbours: all three are bound by
// memory, nothing to reuse beyond what the caches give.
// Built with -ffp-contract=off: every operation is the one the header spells
// out, in its order, so tests/cttk_ref.py matches bit for bit.
//
// Launches go through ledger::launch; with -fvisibility=hidden the ledger's
// registry is this library's own (mgic_cttk_launch_ledger_dump).
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "cttk.hpp"
#include "launch_ledger.hpp"

namespace mgic {
namespace cttk {

namespace {

constexpr int TX = 64;  // one wavefront along x
constexpr int TY = 4;   // 4 waves per block
const dim3 kBlock(TX, TY, 1);

void check_launch() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    throw std::runtime_error(std::string("kernel launch: ") + hipGetErrorString(e));
}

// the cell of this thread: false when it has none (past the box's edge)
__device__ __forceinline__ bool locate(const Row *rows, int nrow, const Row *&r, long &idx) {
  const long long b = blockIdx.x;
  int n = 0;
  while (n + 1 < nrow && rows[n + 1].first <= b) ++n;
  r = rows + n;
  const long long q = b - r->first;  // < bx * by * nz: the host sized the grid
  const int tiles = r->bx * r->by;
  const int k = (int)(q / tiles);
  const int t = (int)(q - (long long)k * tiles);
  const int tj = t / r->bx;
  const int i = (t - tj * r->bx) * TX + threadIdx.x;
  const int j = tj * TY + threadIdx.y;
  if (i >= r->nx || j >= r->ny || k >= r->nz) return false;
  idx = (long)i + (long)j * r->sy + (long)k * r->sz;
  return true;
}

__global__ __launch_bounds__(256) void k_cttk_K(const Row *rows, int nrow, int *bad) {
  const Row *r;
  long idx;
  if (!locate(rows, nrow, r, idx)) return;
  const double v = r->p[0][idx];
  if (v >= 0.0) {
    r->p[1][idx] = -sqrt(v);
  } else {
    r->p[1][idx] = 0.0;
    atomicAdd(bad, 1);
  }
}

__global__ __launch_bounds__(256) void k_cttk_source(const Row *rows, int nrow, double h) {
  const Row *r;
  long idx;
  if (!locate(rows, nrow, r, idx)) return;
  const double p = r->p[0][idx];
  const double p2 = p * p;
  const double p6 = (p2 * p2) * p2;
  const double c = (2.0 / 3.0) * p6;
  const double *K = r->p[1] + idx;
  const long st[3] = {1, r->sy, r->sz};
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double D = h * (K[st[d]] - K[-st[d]]);
    double *S = r->p[2 + d] + idx;
    *S = *S + c * D;
  }
}

__global__ __launch_bounds__(256) void k_cttk_constraints(const Row *rows, int nrow, double h) {
  const Row *r;
  long idx;
  if (!locate(rows, nrow, r, idx)) return;
  const double *K = r->p[0] + idx;
  const double t = (2.0 / 3.0) * (K[0] * K[0]);
  r->p[1][idx] = r->p[1][idx] + t;
  r->p[5][idx] = r->p[5][idx] + fabs(t);
  const long st[3] = {1, r->sy, r->sz};
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double D = h * (K[st[d]] - K[-st[d]]);
    double *M = r->p[2 + d] + idx;
    *M = *M - (2.0 / 3.0) * D;
  }
}

dim3 grid_of(long long nblocks) {
  if (nblocks > 0x7fffffffLL) throw std::invalid_argument("cttk: too many blocks for one launch");
  return dim3((unsigned)nblocks);
}

void check(const Row *rows, int nrow) {
  if (!rows || nrow <= 0) throw std::invalid_argument("cttk: null box table");
}

}  // namespace

long long blocks_of(Row &r) {
  r.bx = (r.nx + TX - 1) / TX;
  r.by = (r.ny + TY - 1) / TY;
  return (long long)r.bx * r.by * r.nz;
}

void set_K(const Row *rows, int nrow, long long nblocks, int *bad, hipStream_t st) {
  if (nblocks <= 0) return;
  check(rows, nrow);
  if (!bad) throw std::invalid_argument("cttk: null counter");
  ledger::launch<k_cttk_K>(grid_of(nblocks), kBlock, 0, st, rows, nrow, bad);
  check_launch();
}

void add_source(const Row *rows, int nrow, long long nblocks, double h, hipStream_t st) {
  if (nblocks <= 0) return;
  check(rows, nrow);
  ledger::launch<k_cttk_source>(grid_of(nblocks), kBlock, 0, st, rows, nrow, h);
  check_launch();
}

void correct_constraints(const Row *rows, int nrow, long long nblocks, double h, hipStream_t st) {
  if (nblocks <= 0) return;
  check(rows, nrow);
  ledger::launch<k_cttk_constraints>(grid_of(nblocks), kBlock, 0, st, rows, nrow, h);
  check_launch();
}

}  // namespace cttk
}  // namespace mgic
