// zm.hip -- the zero-mode kernel of a periodic level (gfx950, fp64).
//
// On a periodic domain the momentum solve's operator -beta Lap is singular
// (DESIGN.md 3k): the mean of each right-hand side is removed before the
// solve and the mean of each solution after it.  The sums are the level's own
// dotProduct(f, ones); what is here is the subtraction.  One thread per cell
// of a TX x TY tile per z plane, as the generator kernels of kernels.hip;
// built with -ffp-contract=off, and the one operation is a subtraction, so
// numpy's f - c gives the same bits.
//
// Launches go through ledger::launch; with -fvisibility=hidden the ledger's
// registry is this library's own (mgic_zm_launch_ledger_dump).
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "launch_ledger.hpp"
#include "zm.hpp"

namespace mgic {
namespace zm {

namespace {

constexpr int TX = 64;  // one wavefront along x
constexpr int TY = 4;   // 4 waves per block
const dim3 kBlock(TX, TY, 1);

dim3 grid_cells(int nx, int ny, int nz) { return dim3((nx + TX - 1) / TX, (ny + TY - 1) / TY, nz); }

void check_launch() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    throw std::runtime_error(std::string("kernel launch: ") + hipGetErrorString(e));
}

template <int N>
struct Shift {
  double *p[N];
  double c[N];
};

// 1 load + 1 store per cell and field: 16 B per cell, nothing to reuse
template <int N>
__global__ __launch_bounds__(256) void k_zm_shift(const Shift<N> s, const BoxGeom g) {
  const int i = blockIdx.x * TX + threadIdx.x;
  const int j = blockIdx.y * TY + threadIdx.y;
  const int k = blockIdx.z;
  if (i >= g.nx || j >= g.ny || k >= g.nz) return;
  const long idx = (long)i + (long)j * g.sy + (long)k * g.sz;
#pragma unroll
  for (int n = 0; n < N; ++n) s.p[n][idx] = s.p[n][idx] - s.c[n];
}

template <int N>
void shift_n(double *const f[], const double c[], const BoxGeom &g, hipStream_t st) {
  Shift<N> s;
  for (int n = 0; n < N; ++n) {
    s.p[n] = f[n];
    s.c[n] = c[n];
  }
  ledger::launch<k_zm_shift<N>>(grid_cells(g.nx, g.ny, g.nz), kBlock, 0, st, s, g);
  check_launch();
}

}  // namespace

void shift(int n, double *const f[], const double c[], const BoxGeom &g, hipStream_t st) {
  if (n != 1 && n != 3) throw std::invalid_argument("the number of fields is 1 or 3");
  if (g.nx <= 0 || g.ny <= 0 || g.nz <= 0) return;
  if (n == 1)
    shift_n<1>(f, c, g, st);
  else
    shift_n<3>(f, c, g, st);
}

}  // namespace zm
}  // namespace mgic
