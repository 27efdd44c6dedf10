// reward_defer_kernel.h -- the Go2's plain-grid rollout kernel with the step rewards evaluated ONCE PER ROLLOUT (wave.h: WaveD;
// rollout_body.h: reward_view, env_step<.., EPI>; rollout_driver.h).  One wavefront per workgroup, one rollout -- or one relay piece of
// the mean trajectory -- per wavefront: rollout_kernel<DimsGo2, 1, 3> with WaveD for Wave and T x DIAL_REWARD_STASH_W words of dynamic
// LDS behind the workspace (and the profiling counters) for the stash -- LDS of THIS launch, not a field of the workspace, which the
// eight-wavefront and the pair kernels would pay for too.
// A kernel of its own in a library of its own (libdialdefer.so, reward_defer.hip): chosen at run time inside rollout_kernel the two
// reward paths cost that kernel 57 spilled SGPRs (45 without) and 12 B of scratch; apart, rollout_kernel and every other shipped code
// object stay exactly what they were (tests/golden/shipped_kernel_resources.txt) and this kernel has 30 spilled SGPRs and no scratch.
// libdialhip.so loads the library from its own directory when a context that can use it is created (dial_hip.hip); without the file
// such a context runs rollout_kernel's per-step reward lane, and dial_debug_last_launch says so.
#pragma once
#include "rollout_kernel.h"

#define DIAL_REWARD_DEFER_ABI_VERSION 1
#define DIAL_REWARD_DEFER_SYMBOL "dial_reward_defer_ops_v1"
// blocks: the grid (rollouts + relay pieces); lds: constants + workspace (+ profiling counters) + the stash
typedef hipError_t (*dial_reward_defer_launch_fn)(int blocks, size_t lds, hipStream_t st, const void* dcm, const dial_task* dtask,
                                                  const dial_cfg* dcfg, const dial::RolloutIO* io, int B, int ws_words);
typedef hipError_t (*dial_reward_defer_occupancy_fn)(int* blocks_per_cu, size_t lds);
struct dial_reward_defer_ops {
  int abi_version;                                   // DIAL_REWARD_DEFER_ABI_VERSION
  size_t sizeof_task, sizeof_cfg, sizeof_io;         // (ABI check)
  size_t cmodel_bytes;                               // sizeof(CModel<DimsGo2>) (ABI check)
  dial_reward_defer_launch_fn launch;
  dial_reward_defer_occupancy_fn occupancy;
};
typedef const dial_reward_defer_ops* (*dial_reward_defer_entry)(void);

template <class D>
__global__ void __launch_bounds__(64, 3)
rollout_defer_kernel(const CModel<D>* __restrict__ gm, const dial_task* __restrict__ tg, const dial_cfg* __restrict__ cfg, dial::RolloutIO io,
                     int B, int ws_words) {
  static_assert(D::is_static && D::pre_ctrl && dial::kQuadDims<D> && !D::user, "the Go2's own instantiation");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  Ws s;
  const CModel<D>* m = stage_model<D, 1>(gm, smem, s, io.Hn1, ws_words, io.con_cap, io.T);
  int n = (int)blockIdx.x + io.n_first;
  int relay = -1;   // (the mean trajectory's pieces: rollout_kernel.h)
  if (io.relay_flag && (int)blockIdx.x >= io.relay_base) { relay = (int)blockIdx.x - io.relay_base; n = B - 1; }
  if (n >= B) return;
  WaveD w;
  w.lane = threadIdx.x & 63;
  w.lane_r = w.lane;
  w.launder = DIAL_LAUNDER_STATIC;
  constexpr int CMW = (int)((sizeof(CModel<D>) + 15) / 16) * 4;
#ifdef DIAL_PROFILE
  w.acc = reinterpret_cast<unsigned long long*>(smem + (ws_words + CMW + 2) / 2 * 2);
  if (w.lane < 32) w.acc[w.lane] = 0;
  __syncthreads();
  w.stash = smem + CMW + ws_words + (16 + 32 * (int)sizeof(unsigned long long)) / 4;
  unsigned long long t_start = wall_clock64();
#else
  w.stash = smem + CMW + ws_words;   // (16-byte aligned: the host checks the sizes)
#endif
  w.zbase = w.stash + 16 * io.T;
  dial::rollout_sample<false>(w, m, tg, cfg, s, io, n, relay, -1, /*init_ws=*/true);
#ifdef DIAL_PROFILE
  if (io.prof && w.lane == 0) {
    unsigned long long* p = io.prof + 32 + 6 * (size_t)n;
    p[0] = t_start; p[1] = wall_clock64(); p[2] = w.acc[27]; p[3] = w.acc[28]; p[4] = w.acc[30]; p[5] = w.acc[31];
  }
#endif
}

template <class D>
hipError_t reward_defer_launch(int blocks, size_t lds, hipStream_t st, const void* dcm, const dial_task* dtask, const dial_cfg* dcfg,
                               const dial::RolloutIO* io, int B, int ws_words) {
  hipLaunchKernelGGL(rollout_defer_kernel<D>, dim3(blocks), dim3(64), lds, st, (const CModel<D>*)dcm, dtask, dcfg, *io, B, ws_words);
  return hipGetLastError();
}
template <class D>
hipError_t reward_defer_occupancy(int* blocks_per_cu, size_t lds) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, rollout_defer_kernel<D>, 64, lds);
}
