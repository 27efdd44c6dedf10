// plan_ens_aggregate.hip -- the aggregation step of robust planning over a model ensemble (plan_ens_kernel.h states the contract): the
// raw rewards [R][MB] of one ensemble rollout launch -> one reward per candidate, out [MB], on which the planner's softmax then runs.
// A translation unit of its own in libdialplanens.so: no other library gains a kernel.
// One thread per candidate; its R values are read with stride MB, k passes for the CVaR tail (each pass picks the next (value, index)
// in lexicographic order, so no per-thread array and no scratch; the re-reads hit L2).  The arithmetic is spelled out so that a NumPy
// fp64 restatement reproduces it bit for bit (tests/ensemble_ref.py): sums in fp64 in a fixed order, one division, one rounding.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/dial_mpc.h"

extern "C" __global__ void __launch_bounds__(256)
plan_ens_aggregate_kernel(const float* __restrict__ raw, float* __restrict__ out, int R, int MB, int mode, int k) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= MB) return;
  const float* x = raw + c;
  if (mode == DIAL_ENSEMBLE_MEAN) {
    double acc = 0.0;
    for (int r = 0; r < R; r++) acc += (double)x[(size_t)r * MB];
    out[c] = (float)(acc / (double)R);
  } else {
    // the k smallest in ascending (value, index) order: pass j picks the smallest pair above the pair of pass j - 1.  MIN is the
    // tail of one -- the first of the smallest values; (float)((double)x / 1.0) is x -- so that CVaR with k = 1 IS the minimum.
    if (mode == DIAL_ENSEMBLE_MIN) k = 1;
    double acc = 0.0;
    float pv = 0.f;
    int pi = -1;   // (no pair picked yet)
    for (int j = 0; j < k; j++) {
      float bv = 0.f;
      int bi = -1;
      for (int r = 0; r < R; r++) {
        const float v = x[(size_t)r * MB];
        const bool above = pi < 0 || v > pv || (v == pv && r > pi);
        if (above && (bi < 0 || v < bv)) { bv = v; bi = r; }   // (strict <: among equal values the lower r stays)
      }
      acc += (double)bv;
      pv = bv; pi = bi;
    }
    out[c] = (float)(acc / (double)k);
  }
}

extern "C" __attribute__((visibility("hidden"))) hipError_t dial_plan_ens_aggregate(hipStream_t st, const float* raw, float* out, int R, int MB,
                                                                                     int mode, int k) {
  hipLaunchKernelGGL(plan_ens_aggregate_kernel, dim3((MB + 255) / 256), dim3(256), 0, st, raw, out, R, MB, mode, k);
  return hipGetLastError();
}
