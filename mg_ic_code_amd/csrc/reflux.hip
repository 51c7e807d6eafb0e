// reflux.hip -- the reflux term at coarse-fine faces (gfx950, fp64;
// DESIGN.md 3l, include/mgic_reflux.h).
//
// One thread per interface cell of the coarse level: a cell that level l + 1
// does not cover with a face neighbour that it does.  The thread walks the
// cell's faces in the order x-lo ... z-hi; for each it reads the four fine
// cells behind the face and their ghosts across it (the fine box's own,
// QuadCFInterp's), averages the four gradients, subtracts the coarse
// stencil's gradient and accumulates.  A surface kernel: 8 fine loads, 2
// coarse loads and 1 table row per face, one load-modify-store of the target
// per cell; nothing is shared between threads, so no LDS and no atomics.
// Built with -ffp-contract=off: every operation is the one tests/reflux_ref.py
// spells out, in its order.
//
// Launches go through ledger::launch; with -fvisibility=hidden the ledger's
// registry is this library's own (mgic_reflux_launch_ledger_dump).
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "launch_ledger.hpp"
#include "reflux.hpp"

namespace mgic {
namespace reflux {

namespace {

constexpr int kThreads = 256;  // 4 waves

static_assert(sizeof(mgic_reflux_cell) == 24 && sizeof(mgic_reflux_face) == 48,
              "the rows libmgic builds (include/mgic.h, csrc/amr.cpp)");

void check_launch() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    throw std::runtime_error(std::string("kernel launch: ") + hipGetErrorString(e));
}

// HASC: a coarse field (false: zero, G_c = 0)
template <bool HASC>
__global__ __launch_bounds__(kThreads) void k_reflux(const Args a) {
  const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (t >= a.ncell) return;
  const mgic_reflux_cell c = a.cells[t];
  const double *pc = HASC ? a.phi_c[c.box] + c.off : nullptr;
  double sum = 0.0;
  bool any = false;
  int q = c.first;
  for (int f = 0; f < 6; ++f) {
    if (!((c.mask >> f) & 1)) continue;
    const mgic_reflux_face fc = a.faces[q++];
    const double *pf = a.phi_f[fc.fbox] + fc.foff;
    const double g00 = (pf[0] - pf[fc.fstep]) / a.dx_f;
    const double g01 = (pf[fc.ft0] - pf[fc.ft0 + fc.fstep]) / a.dx_f;
    const double g10 = (pf[fc.ft1] - pf[fc.ft1 + fc.fstep]) / a.dx_f;
    const double g11 = (pf[fc.ft1 + fc.ft0] - pf[fc.ft1 + fc.ft0 + fc.fstep]) / a.dx_f;
    const double gf = 0.25 * ((g00 + g01) + (g10 + g11));
    const double gc = HASC ? (pc[fc.cstep] - pc[0]) / a.dx_c : 0.0;
    const double term = (gf - gc) / a.dx_c;
    sum = any ? sum + term : term;
    any = true;
  }
  if (!any) return;  // (no such row: the table lists interface cells only)
  const double v = (a.coef * a.b[c.box][c.off]) * sum;
  double *p = a.target[c.box] + c.off;
  *p = a.sign > 0 ? *p + v : *p - v;
}

}  // namespace

void apply(const Args &a, hipStream_t st) {
  if (a.ncell <= 0) return;
  if (!a.cells || !a.faces || !a.target || !a.phi_f || !a.b)
    throw std::invalid_argument("reflux: null table");
  if (a.ncell > 0x7fffffffLL * kThreads) throw std::invalid_argument("reflux: too many cells");
  const dim3 grid((unsigned)((a.ncell + kThreads - 1) / kThreads));
  if (a.phi_c)
    ledger::launch<k_reflux<true>>(grid, dim3(kThreads), 0, st, a);
  else
    ledger::launch<k_reflux<false>>(grid, dim3(kThreads), 0, st, a);
  check_launch();
}

}  // namespace reflux
}  // namespace mgic
