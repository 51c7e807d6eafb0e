// cttk.hpp -- host-side launchers of the three kernels in cttk.hip
// (libmgic_cttk.so; include/mgic_cttk.h is the C ABI and states every
// expression with its order).
//
// A launcher works on ALL local boxes of a level in one launch: `rows` is a
// table in device memory, one Row per box.  All fields of a call share the
// box's strides (sy, sz in doubles, sx = 1) and every pointer points at the
// valid-lo cell, as mgic_field_device_ptr gives them.
#pragma once

#include <hip/hip_runtime.h>

namespace mgic {
namespace cttk {

constexpr int kMaxFields = 6;

struct Row {
  int nx, ny, nz;     // valid cells
  int bx, by;         // tiles along x and y: the box takes bx * by * nz blocks
  int pad;
  long sy, sz;        // strides in doubles
  long long first;    // the box's first block in the launch
  double *p[kMaxFields];
};

// blocks a box of nx x ny x nz cells takes (fills bx, by)
long long blocks_of(Row &r);

// p[0] = integrand, p[1] = K; *bad (device) += the cells with !(I >= 0)
void set_K(const Row *rows, int nrow, long long nblocks, int *bad, hipStream_t st);
// p[0] = psi, p[1] = K, p[2..4] = S_i; h = 0.5 / dx
void add_source(const Row *rows, int nrow, long long nblocks, double h, hipStream_t st);
// p[0] = K, p[1] = ham, p[2..4] = mom_i, p[5] = ham_abs
void correct_constraints(const Row *rows, int nrow, long long nblocks, double h, hipStream_t st);

}  // namespace cttk
}  // namespace mgic
