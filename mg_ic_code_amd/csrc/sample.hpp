// sample.hpp -- host-side launcher of the point-sampling kernel in sample.hip
// (libmgic_sample.so; include/mgic_sample.h is the C ABI and states the rule,
// DESIGN.md 3o).
#pragma once

#include <hip/hip_runtime.h>

namespace mgic {
namespace sample {

constexpr int kMaxLevels = 8;       // MGIC_SAMPLE_MAX_LEVELS
constexpr int kMaxPoints = 1 << 20; // MGIC_SAMPLE_MAX_POINTS
constexpr int kBlock = 256;         // one thread per point

// one box of the device-resident box table (the boxes of all levels, coarsest
// level first): its valid cells in its level's index space, the strides of its
// allocation (sx = 1) and the valid-lo pointer of the field
struct Box {
  int lo[3], hi[3];
  long sy, sz;
  const double *u;
};

struct Args {
  int nlev, npts;
  int box0[kMaxLevels + 1];  // level l's boxes are box0[l] .. box0[l + 1] - 1
  double dx[kMaxLevels];     // level l's spacing
  int n0[3];                 // level 0's cells per direction
  int periodic[3];
  double half[3];            // N_d * dx_0 / 2.0
  double len[3];             // N_d * dx_0
  const Box *boxes;          // device
  const double *xyz;         // device, npts x 3
  double *values;            // device, npts
  int *level;                // device, npts
  int *order;                // device, npts
};

// one launch: order = 1, 2 or 4, the order the candidates start from
void points(const Args &a, int order, hipStream_t st);

}  // namespace sample
}  // namespace mgic
