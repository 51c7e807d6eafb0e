// zm.hpp -- host-side launcher of the zero-mode kernel in zm.hip
// (libmgic_zm.so; include/mgic_zm.h is the C ABI).
//
// The launcher works on ONE box.  All fields of a level share the box's
// strides (sy, sz in doubles, sx = 1) and every pointer points at the
// valid-lo cell, as mgic_field_device_ptr gives them.
#pragma once

#include <hip/hip_runtime.h>

namespace mgic {
namespace zm {

struct BoxGeom {
  int nx, ny, nz;
  long sy, sz;
};

// f[i][cell] = f[i][cell] - c[i] over the valid cells, i < n; n is 1 or 3
void shift(int n, double *const f[], const double c[], const BoxGeom &g, hipStream_t st);

}  // namespace zm
}  // namespace mgic
