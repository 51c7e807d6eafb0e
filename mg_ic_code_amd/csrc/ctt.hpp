// ctt.hpp -- host-side launchers of the conformal transverse-traceless
// kernels in ctt.hip (libmgic_ctt.so; include/mgic_ctt.h is the C ABI).
//
// Every launcher works on ONE box.  All fields of a level share the box's
// strides (sy, sz in doubles, sx = 1) and every pointer points at the
// valid-lo cell, as mgic_field_device_ptr gives them; ghost layer 1 of an
// operand is read as stored.
#pragma once

#include <hip/hip_runtime.h>

namespace mgic {
namespace ctt {

struct BoxGeom {
  int nx, ny, nz;
  long sy, sz;
};

// out = -0.25 * (D_x V_x + D_y V_y + D_z V_z) over the valid cells,
// D_d f = 0.5 / dx * (f(+e_d) - f(-e_d))
void div_rhs(double *out, const double *const v[3], const BoxGeom &g, double dx, hipStream_t st);
// W_i = V_i + D_i U over the valid cells, i = x, y, z
void w(double *const wout[3], const double *const v[3], const double *u, const BoxGeom &g,
       double dx, hipStream_t st);
// LW_ij = D_i W_j + D_j W_i - (2/3) delta_ij D_k W_k over the valid cells, in
// the order 11, 12, 13, 22, 23, 33
void lw(double *const out[6], const double *const wv[3], const BoxGeom &g, double dx,
        hipStream_t st);
// ghost layer 1 across face `face` (dir * 2 + side) of the box, faces only:
// g = 2 * f(face cell) - f(next cell in).  The box needs two cells along dir.
void extrap(double *f, const BoxGeom &g, int face, hipStream_t st);

}  // namespace ctt
}  // namespace mgic
