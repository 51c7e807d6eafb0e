// ptag.hip -- set_tag_cells onto the clustering lattice through the wrap of a
// periodic domain (gfx950).
//
// A cell is tagged iff |cond| >= tag_val (a NaN is not).  The tag grown by
// `grow` cells sets every lattice cell (c^3 level cells, lattice index =
// floor(cell / c)) it reaches in the byte mask over lattice cells
// [lat_lo, lat_lo + lat_n):
//   * a non-periodic direction is k_tag_lattice's of libmgic: the grown range
//     is clipped to the domain;
//   * in a periodic direction the lattice spans the domain (lat_lo = dom_lo /
//     c, lat_n = n / c, the caller sees to it) and the grown range is not
//     clipped: its lattice indices are taken modulo lat_n, which is the cell
//     index modulo n because n is a multiple of c.
// One launch covers every local box of the level: a block looks up its tile
// (ptag.hpp) and takes one z plane of it.  A wave is one row of 64 cells in x;
// a lane leaves a lattice column to the lane before it when that lane is
// tagged and reaches the column too (ballot), on the UNWRAPPED lattice
// indices, so a run of tagged cells stores each byte about once per row
// instead of c times; the wrap is applied to what is left.  Every store
// writes the same value 1: plain byte stores, in any order.
//
// Launches go through ledger::launch; with -fvisibility=hidden the ledger's
// registry is this library's own (mgic_ptag_launch_ledger_dump).
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "launch_ledger.hpp"
#include "ptag.hpp"

namespace mgic {
namespace ptag {

namespace {

const dim3 kBlock(kTileX, kTileY, 1);

void check_launch() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    throw std::runtime_error(std::string("kernel launch: ") + hipGetErrorString(e));
}

__device__ inline int fdiv(int a, int c) { return a >= 0 ? a / c : -((-a + c - 1) / c); }
__device__ inline int fmod_n(int a, int n) {
  const int r = a % n;
  return r < 0 ? r + n : r;
}

// the lattice range [*ua, *ub] (relative to lat_lo) that cell index v of
// direction d, grown, reaches: inside [0, lat_n) when the direction is not
// periodic (empty never: v lies in the domain), unwrapped when it is
__device__ inline void reach(const Args &t, int d, int v, int *ua, int *ub) {
  if (t.periodic[d]) {
    *ua = fdiv(v - t.grow - t.dom_lo[d], t.c);
    *ub = fdiv(v + t.grow - t.dom_lo[d], t.c);
  } else {
    const int lo = max(v - t.grow, t.dom_lo[d]), hi = min(v + t.grow, t.dom_hi[d]);
    *ua = max(fdiv(lo, t.c) - t.lat_lo[d], 0);
    *ub = min(fdiv(hi, t.c) - t.lat_lo[d], t.lat_n[d] - 1);
  }
}

__global__ __launch_bounds__(256) void k_ptag_lattice(unsigned char *__restrict__ mask,
                                                      const Tile *__restrict__ tiles,
                                                      double tag_val, const Args t) {
  const Tile T = tiles[blockIdx.x];
  const int k = blockIdx.y;
  if (k >= T.n[2]) return;  // (the whole block: the grid has the deepest box's planes)
  const int i = T.i0 + threadIdx.x;
  const int j = T.j0 + threadIdx.y;
  const bool in = i < T.n[0] && j < T.n[1];
  bool tagged = false;
  if (in) tagged = fabs(T.p[(long)i + (long)j * T.sy + (long)k * T.sz]) >= tag_val;
  const unsigned long long wave = __ballot(tagged);  // a wave is one row of 64 cells in x
  if (!tagged) return;
  const int iv[3] = {T.glo[0] + i, T.glo[1] + j, T.glo[2] + k};
  int ua[3], ub[3];
  for (int d = 0; d < 3; ++d) reach(t, d, iv[d], &ua[d], &ub[d]);
  // columns the previous lane (cell i - 1 of the same row) already stores
  const int lane = threadIdx.x;
  if (lane > 0 && ((wave >> (lane - 1)) & 1ull)) {
    int pa, pb;
    reach(t, 0, iv[0] - 1, &pa, &pb);
    ua[0] = max(ua[0], pb + 1);  // (its low end is never above this lane's)
  }
  // a range of lat_n or more columns is all of them once
  for (int d = 0; d < 3; ++d)
    if (ub[d] - ua[d] + 1 > t.lat_n[d]) ub[d] = ua[d] + t.lat_n[d] - 1;
  for (int z = ua[2]; z <= ub[2]; ++z) {
    const int mz = t.periodic[2] ? fmod_n(z, t.lat_n[2]) : z;
    for (int y = ua[1]; y <= ub[1]; ++y) {
      const int my = t.periodic[1] ? fmod_n(y, t.lat_n[1]) : y;
      unsigned char *row = mask + ((long)mz * t.lat_n[1] + my) * t.lat_n[0];
      for (int x = ua[0]; x <= ub[0]; ++x) row[t.periodic[0] ? fmod_n(x, t.lat_n[0]) : x] = 1;
    }
  }
}

}  // namespace

void tag_lattice(unsigned char *mask, const Tile *tiles, int ntiles, int nz_max, double tag_val,
                 const Args &a, hipStream_t st) {
  if (ntiles <= 0 || nz_max <= 0) return;
  if (ntiles > (1 << 24) || nz_max > 65535)
    throw std::invalid_argument("ptag: too many tiles or planes for one launch");
  for (int d = 0; d < 3; ++d)
    if (a.lat_n[d] < 1 || a.c < 1 || a.grow < 0)
      throw std::invalid_argument("ptag: bad lattice");
  ledger::launch<k_ptag_lattice>(dim3(ntiles, nz_max, 1), kBlock, 0, st, mask, tiles, tag_val, a);
  check_launch();
}

}  // namespace ptag
}  // namespace mgic
