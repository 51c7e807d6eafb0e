// adm.hpp -- host-side launcher of the surface-charge kernels in adm.hip
// (libmgic_adm.so; include/mgic_adm.h is the C ABI).
//
// A surface is the cell-aligned cube of half-width n level-0 cells about the
// domain centre: 6 sides (side = 2 d + (s > 0), d the normal direction, s the
// sign of the outward normal), each (2 n)^2 cell faces (b, a), a fastest; a and
// b run along the two directions other than d, in increasing order.  A face's
// index within its surface is ((side * 2n) + b) * 2n + a.
#pragma once

#include <hip/hip_runtime.h>

namespace mgic {
namespace adm {

constexpr int kMaxSurfaces = 8;  // MGIC_ADM_MAX_SURFACES
constexpr int kTerms = 7;        // mass, P1, P2, P3, J1, J2, J3
constexpr int kBlock = 256;      // 4 waves; one thread per face
constexpr int kWaves = kBlock / 64;
constexpr int kMaxPunctures = 8, kPunctureDoubles = 10;

// The puncture table as kernels.hpp's: rows m, x, y, z, Px, Py, Pz, Jx, Jy, Jz,
// an odd count completed by the host with a row of m = P = J = 0 at the last
// puncture's position.  Passed to the kernel by value.
struct PunctureTable {
  int n;
  double v[kMaxPunctures][kPunctureDoubles];
};

// one level-0 box of the device-resident box table: its valid cells, the
// strides of its allocation (sx = 1) and the valid-lo pointers of psi and of
// the six LW_ij (11, 12, 13, 22, 23, 33; unused without them)
struct Box {
  int lo[3], hi[3];
  long sy, sz;
  const double *psi;
  const double *lw[6];
};

struct Args {
  int nsurf, nbox;
  int half[kMaxSurfaces];        // half-width n of each surface
  long face0[kMaxSurfaces + 1];  // faces of the surfaces before this one
  int block0[kMaxSurfaces + 1];  // blocks of the surfaces before this one
  int centre[3];                 // N_d / 2: the cube is [centre - n, centre + n)
  double domlen[3];              // N_d * dx
  double dx;
  const Box *boxes;  // device
  double *terms;     // device, (surface, side, 7, b, a) or nullptr: not written
  double *partials;  // device, 7 per block
  double *sums;      // device, 7 per surface
};

// the per-face terms (a.terms, when set) and the block partials: one launch
void surface(const Args &a, const PunctureTable &t, bool lw, hipStream_t st);
// a.sums[s][c] = the partials of surface s added in block order: one launch
void finish(const Args &a, hipStream_t st);

}  // namespace adm
}  // namespace mgic
