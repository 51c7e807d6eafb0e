// rcp_div1_probe.hip -- where does the two-sweep smoother's short reciprocal
// (smoother_tb.hip: rcp_div1, restated here) leave the bits of the fp64
// division 1.0 / d?  Prints both for denominators at the ends of the range:
// the ones the host's lambda-range guard (resetLambda: rcp_fast) keeps away
// from it.  Recorded in profiles/r07_rcp_div1_probe.txt.
//   hipcc -O3 -ffp-contract=off --offload-arch=gfx950 tools/rcp_div1_probe.hip -o rcp_div1_probe
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

__device__ double rcp_div1(double d) {
  double r = __builtin_amdgcn_rcp(d);
  double e = __builtin_fma(-d, r, 1.0);
  r = __builtin_fma(r, e, r);
  e = __builtin_fma(-d, r, 1.0);
  r = __builtin_fma(r, e, r);
  e = __builtin_fma(-d, r, 1.0);
  return __builtin_fma(e, r, r);
}

__global__ void k_probe(const double *d, double *out, int n) {
  const int i = threadIdx.x;
  if (i < n) {
    out[2 * i] = rcp_div1(d[i]);
    out[2 * i + 1] = 1.0 / d[i];
  }
}

int main() {
  constexpr int n = 9;
  const double h[n] = {-1.0e308 - 12.24, -1.0e308, 1.0e308, -3.3e307, -1.7,
                       0x1p600,          0.0,      -0.0,    0x1p-1023};
  double *d, *o, ho[2 * n];
  if (hipMalloc(&d, sizeof h) != hipSuccess || hipMalloc(&o, sizeof ho) != hipSuccess) return 2;
  if (hipMemcpy(d, h, sizeof h, hipMemcpyHostToDevice) != hipSuccess) return 2;
  k_probe<<<1, 64>>>(d, o, n);
  if (hipMemcpy(ho, o, sizeof ho, hipMemcpyDeviceToHost) != hipSuccess) return 3;
  for (int i = 0; i < n; ++i) {
    unsigned long long a, b;
    memcpy(&a, &ho[2 * i], 8);
    memcpy(&b, &ho[2 * i + 1], 8);
    printf("d=%.17g rcp_div1=%.17g (%016llx) div=%.17g (%016llx) %s\n", h[i], ho[2 * i], a,
           ho[2 * i + 1], b, a == b ? "same" : "DIFFER");
  }
  return 0;
}
