// reflux.hpp -- host-side launcher of the reflux kernel in reflux.hip
// (libmgic_reflux.so; include/mgic_reflux.h is the C ABI, include/mgic.h has
// the table rows).
//
// Every pointer is a device pointer: the two tables (csrc/amr.cpp,
// FluxRegister) and the fields' tables of valid-lo pointers per local box
// (LevelData::d_tab).
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/mgic.h"

namespace mgic {
namespace reflux {

struct Args {
  const mgic_reflux_cell *cells;
  const mgic_reflux_face *faces;
  long long ncell;
  double *const *target;  // coarse level
  double *const *phi_c;   // coarse level, or null: a zero coarse field
  double *const *phi_f;   // fine level, ghosts filled
  double *const *b;       // coarse level's bCoef
  double coef;            // -beta
  double dx_c, dx_f;
  int sign;               // > 0: target += v; else target -= v
};

void apply(const Args &a, hipStream_t st);

}  // namespace reflux
}  // namespace mgic
