// khyb.hpp -- host-side launcher of the kernel in khyb.hip (libmgic_khyb.so;
// include/mgic_khyb.h is the C ABI and states every expression with its
// order).
//
// The launcher works on ALL local boxes of a level in one launch: `rows` is a
// table in device memory, one Row per box.  All fields of the call share the
// box's strides (sy, sz in doubles, sx = 1) and every pointer points at the
// valid-lo cell, as mgic_field_device_ptr gives them.
#pragma once

#include <hip/hip_runtime.h>

namespace mgic {
namespace khyb {

struct Row {
  int nx, ny, nz;     // valid cells
  int bx, by;         // tiles along x and y: the box takes bx * by * nz blocks
  int pad;
  long sy, sz;        // strides in doubles
  long long first;    // the box's first block in the launch
  const double *phi;
  const double *pi;   // null: Pi = 0 (in every row or in none)
  double *K;
};

struct Params {
  double V0, mass, lambda, G;
};

// blocks a box of nx x ny x nz cells takes (fills bx, by)
long long blocks_of(Row &r);

// K from phi and pi; *bad (device) += the cells with !(1.5 * 16 pi G rho >= 0)
void set_K(const Row *rows, int nrow, long long nblocks, Params prm, int *bad, hipStream_t st);

}  // namespace khyb
}  // namespace mgic
