// lanes.hip -- device side of the lane-local pins (TEST INFRASTRUCTURE ONLY; tests/lane_lib.py builds it twice: with the product flags
// and with the IEEE flags of dial_mpc_amd/_lib.py).  One lane runs one case; 64-thread workgroups = one wavefront each.
#include <hip/hip_runtime.h>
#include "rollout_body.h"   // (-I dial_mpc_amd/csrc: tests/lane_lib.py)
using namespace dial;
#include "lane_cases.h"

// fill: what the polygon slices hold before use (0: zeros, 1: NaNs).  Every lane owns DIAL_BOX_POLY_WORDS words at LANE_POLY_STRIDE.
__global__ __launch_bounds__(64) void lane_geom_kernel(const float* in, unsigned* out, int n, int fill) {
  __shared__ float poly[63 * LANE_POLY_STRIDE + DIAL_BOX_POLY_WORDS];
  float* mine = poly + threadIdx.x * LANE_POLY_STRIDE;
  const float v = __builtin_bit_cast(float, fill ? 0x7fc00000 : 0);
  for (int k = 0; k < DIAL_BOX_POLY_WORDS; k++) mine[k] = v;
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i < (size_t)n) lane::geom_case(in + i * lane::G_IN, out + i * lane::G_OUT, mine);
}

__global__ __launch_bounds__(64) void lane_seg_kernel(const float* in, unsigned* out, int n) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i < (size_t)n) lane::seg_case(in + i * lane::S_IN, out + i * lane::S_OUT);
}

__global__ __launch_bounds__(64) void lane_key_kernel(const int* in, unsigned* out, int n, int op, int par) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i < (size_t)n) lane::key_case(in + i * lane::K_IN, out + i * lane::K_OUT, op, par);
}

template <bool MINMAX>
__global__ __launch_bounds__(64) void lane_key_uniform_kernel(const int* in, unsigned* out, int rule) {
  Wave w;
  w.lane = w.lane_r = threadIdx.x;
  lane::key_uniform_case<MINMAX>(w, in + (size_t)blockIdx.x * lane::U_IN, out + (size_t)blockIdx.x * lane::U_OUT, rule, threadIdx.x == 0);
}

__global__ __launch_bounds__(64) void lane_trig_kernel(const float* in, unsigned* out, int n) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i < (size_t)n) lane::trig_case(in + i * lane::T_IN, out + i * lane::T_OUT);
}

extern "C" {

int lane_sizes(int* v) {
  const int s[12] = {lane::G_IN, lane::G_OUT, lane::S_IN, lane::S_OUT, lane::K_IN, lane::K_OUT, lane::U_IN, lane::U_OUT, lane::T_IN, lane::T_OUT,
                     DIAL_BOX_POLY_WORDS, LANE_POLY_STRIDE};
  for (int k = 0; k < 12; k++) v[k] = s[k];
  return 0;
}

// every call: n cases, rows as in lane_cases.h; returns the HIP error code, -1 for a bad argument
int lane_geom(const float* in, unsigned* out, int n, int fill, void* stream) {
  if (n <= 0) return -1;
  lane_geom_kernel<<<(n + 63) / 64, 64, 0, (hipStream_t)stream>>>(in, out, n, fill);
  return (int)hipGetLastError();
}

int lane_seg(const float* in, unsigned* out, int n, void* stream) {
  if (n <= 0) return -1;
  lane_seg_kernel<<<(n + 63) / 64, 64, 0, (hipStream_t)stream>>>(in, out, n);
  return (int)hipGetLastError();
}

int lane_key(const int* in, unsigned* out, int n, int op, int par, void* stream) {
  if (n <= 0 || op < 0 || op >= lane::K_COUNT) return -1;
  lane_key_kernel<<<(n + 63) / 64, 64, 0, (hipStream_t)stream>>>(in, out, n, op, par);
  return (int)hipGetLastError();
}

int lane_key_uniform(const int* in, unsigned* out, int n, int rule, int minmax, void* stream) {
  if (n <= 0) return -1;
  if (minmax) lane_key_uniform_kernel<true><<<n, 64, 0, (hipStream_t)stream>>>(in, out, rule);
  else lane_key_uniform_kernel<false><<<n, 64, 0, (hipStream_t)stream>>>(in, out, rule);
  return (int)hipGetLastError();
}

int lane_trig(const float* in, unsigned* out, int n, void* stream) {
  if (n <= 0) return -1;
  lane_trig_kernel<<<(n + 63) / 64, 64, 0, (hipStream_t)stream>>>(in, out, n);
  return (int)hipGetLastError();
}

}  // extern "C"
