// khyb.hip -- K(x) from the matter's energy, the hybrid CTTK choice (gfx950,
// fp64; DESIGN.md 3r, include/mgic_khyb.h).
//
// One streaming kernel, one thread per cell of a TX x TY tile per z plane as
// the kernels of cttk.hip.  One launch covers every local box: a block finds
// its box in the table (a scan of at most `nrow` rows, uniform over the
// block), then its tile and plane.  Nothing is shared between threads: no
// LDS.  Refused cells are counted with an integer atomic, whose result does
// not depend on the order; there is no floating-point reduction.  Bytes per
// cell: 8 or 16 read, 8 written, against nine multiplications, two additions
// and a square root: bound by memory, nothing to reuse.
// Built with -ffp-contract=off: every operation is the one the header spells
// out, in its order, so tests/khyb_ref.py matches bit for bit.
//
// The launch goes through ledger::launch; with -fvisibility=hidden the
// ledger's registry is this library's own (mgic_khyb_launch_ledger_dump).
#include <hip/hip_runtime.h>

#include <cmath>
#include <stdexcept>
#include <string>

#include "khyb.hpp"
#include "launch_ledger.hpp"

namespace mgic {
namespace khyb {

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

__global__ __launch_bounds__(256) void k_khyb_K(const Row *rows, int nrow, Params prm, int *bad) {
  const Row *r;
  long idx;
  if (!locate(rows, nrow, r, idx)) return;
  const double p = r->phi[idx];
  const double q = r->pi ? r->pi[idx] : 0.0;
  const double V = prm.V0 + 0.5 * prm.mass * prm.mass * p * p + 0.25 * prm.lambda * p * p * p * p;
  const double rho = 0.5 * q * q + V;
  const double m16 = 16.0 * M_PI * prm.G * rho;
  const double v = 1.5 * m16;
  if (v >= 0.0) {
    r->K[idx] = -sqrt(v);
  } else {
    r->K[idx] = 0.0;
    atomicAdd(bad, 1);
  }
}

}  // namespace

long long blocks_of(Row &r) {
  r.bx = (r.nx + TX - 1) / TX;
  r.by = (r.ny + TY - 1) / TY;
  return (long long)r.bx * r.by * r.nz;
}

void set_K(const Row *rows, int nrow, long long nblocks, Params prm, int *bad, hipStream_t st) {
  if (nblocks <= 0) return;
  if (!rows || nrow <= 0) throw std::invalid_argument("khyb: null box table");
  if (!bad) throw std::invalid_argument("khyb: null counter");
  if (nblocks > 0x7fffffffLL) throw std::invalid_argument("khyb: too many blocks for one launch");
  ledger::launch<k_khyb_K>(dim3((unsigned)nblocks), kBlock, 0, st, rows, nrow, prm, bad);
  check_launch();
}

}  // namespace khyb
}  // namespace mgic
