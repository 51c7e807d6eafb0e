// horizon.hpp -- host-side launcher of the expansion kernel in horizon.hip
// (libmgic_horizon.so; include/mgic_horizon.h is the C ABI and states the rule,
// DESIGN.md 3p).
#pragma once

#include <hip/hip_runtime.h>

namespace mgic {
namespace horizon {

constexpr int kMaxLevels = 8;        // MGIC_HORIZON_MAX_LEVELS
constexpr int kMaxPoints = 1 << 20;  // MGIC_HORIZON_MAX_POINTS
constexpr int kTerms = 6;            // theta, psi, dpsi_x, dpsi_y, dpsi_z, A_nn
constexpr int kBlock = 256;          // one thread per point
constexpr int kMaxPunctures = 8, kPunctureDoubles = 10;

// The puncture table as adm.hpp's: rows m, x, y, z, Px, Py, Pz, Jx, Jy, Jz, an
// odd count completed by the host with a row of m = P = J = 0 at the last
// puncture's position.  Passed to the kernel by value.
struct PunctureTable {
  int n;
  double v[kMaxPunctures][kPunctureDoubles];
};

// one box of the device-resident box table (the boxes of all levels, coarsest
// level first): its valid cells in its level's index space, the strides of its
// allocation (sx = 1) and the valid-lo pointers of psi and of the six LW_ij
// (11, 12, 13, 22, 23, 33; unused without them), which share psi's layout
struct Box {
  int lo[3], hi[3];
  long sy, sz;
  const double *psi;
  const double *lw[6];
};

struct Args {
  int nlev, npts;
  int box0[kMaxLevels + 1];  // level l's boxes are box0[l] .. box0[l + 1] - 1
  double dx[kMaxLevels];     // level l's spacing
  int n0[3];                 // level 0's cells per direction
  double half[3];            // N_d * dx_0 / 2.0
  double len[3];             // N_d * dx_0
  const Box *boxes;          // device
  const double *xyz;         // device, npts x 3
  const double *normal;      // device, npts x 3
  const double *divn;        // device, npts
  double *out;               // device, npts x kTerms
  int *level;                // device, npts
  int *order;                // device, npts
};

// one launch: lw = whether the boxes carry the six LW_ij
void expansion(const Args &a, const PunctureTable &t, bool lw, hipStream_t st);

}  // namespace horizon
}  // namespace mgic
