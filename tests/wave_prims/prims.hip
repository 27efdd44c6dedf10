// prims.hip -- device side of the wave.h / register L D L^T pins (TEST INFRASTRUCTURE ONLY; tests/prim_lib.py builds it twice: with
// the product flags and with the IEEE flags of dial_mpc_amd/_lib.py).  One 64-thread workgroup = one wavefront per input set.
#include <hip/hip_runtime.h>
#include "rollout_body.h"   // (-I dial_mpc_amd/csrc: tests/prim_lib.py)
using namespace dial;
#include "prim_cases.h"
#include "chol_cases.h"

using prim::IO;

__global__ __launch_bounds__(64) void prim_wave_kernel(const float* in, unsigned* out, int id, int par) {
  Wave w;
  w.lane = w.lane_r = threadIdx.x;
  const IO io{in + (size_t)blockIdx.x * prim::NIN * 64, out + (size_t)blockIdx.x * prim::NOUT * 64, 0, par};
  prim::run_case(w, io, id);
}

// mode 0: both halves run case id0 (convergent).  1 / 2: only half 0 / half 1 runs it.  3: half 0 runs id0 in the `if`, half 1 runs id1
// in the `else`.
__global__ __launch_bounds__(64) void prim_half_kernel(const float* in, unsigned* out, int id0, int par0, int id1, int par1, int mode) {
  WaveH w;
  w.init(threadIdx.x);
  const float* pin = in + (size_t)blockIdx.x * prim::NIN * 64;
  unsigned* pout = out + (size_t)blockIdx.x * prim::NOUT * 64;
  const IO io0{pin, pout, 32 * w.half, par0}, io1{pin, pout, 32 * w.half, par1};
  if (mode == 0) {
    prim::run_case(w, io0, id0);
  } else if (mode == 1) {
    if (w.half == 0) prim::run_case(w, io0, id0);
  } else if (mode == 2) {
    if (w.half == 1) prim::run_case(w, io0, id0);
  } else {
    if (w.half == 0) prim::run_case(w, io0, id0);
    else prim::run_case(w, io1, id1);
  }
}

template <class D, class TopoT, int FORM>
__global__ __launch_bounds__(64) void chol_wave_kernel(const float* A, const float* b, const float* scr0, unsigned* out, int alias) {
  constexpr int N = D::NV, S = kCholStride<N>;
  __shared__ __attribute__((aligned(16))) float A_lds[N * S];
  __shared__ __attribute__((aligned(16))) float scr_lds[N * S];
  Wave w;
  w.lane = w.lane_r = threadIdx.x;
  const size_t k = blockIdx.x;
  prim::chol_case<D, TopoT, FORM>(w, A + k * prim::CH_A, b + k * 64, scr0 + k * prim::CH_A, out + k * prim::CH_OUT, 0, alias, A_lds, scr_lds);
}

// two systems per wavefront: system 2 * block + half in each half
template <class D, class TopoT>
__global__ __launch_bounds__(64) void chol_half_kernel(const float* A, const float* b, const float* scr0, unsigned* out, int alias) {
  constexpr int N = D::NV, S = kCholStride<N>;
  __shared__ __attribute__((aligned(16))) float A_lds[2][N * S];
  __shared__ __attribute__((aligned(16))) float scr_lds[2][N * S];
  WaveH w;
  w.init(threadIdx.x);
  const size_t k = 2 * (size_t)blockIdx.x + w.half;
  prim::chol_case<D, TopoT, 1>(w, A + k * prim::CH_A, b + k * 64, scr0 + k * prim::CH_A, out + k * prim::CH_OUT, 32 * w.half, alias,
                               A_lds[w.half], scr_lds[w.half]);
}

template <class D, class TopoT>
static int chol_launch(int form, const float* A, const float* b, const float* scr0, unsigned* out, int nsys, int alias, hipStream_t st) {
  if (form == 0) chol_wave_kernel<D, TopoT, 0><<<nsys, 64, 0, st>>>(A, b, scr0, out, alias);
  else if (form == 1) chol_wave_kernel<D, TopoT, 1><<<nsys, 64, 0, st>>>(A, b, scr0, out, alias);
  else return -1;
  return (int)hipGetLastError();
}

extern "C" {

int prim_sizes(int* nin, int* nout, int* ncase, int* ch_a, int* ch_out) {
  *nin = prim::NIN; *nout = prim::NOUT; *ncase = prim::C_COUNT; *ch_a = prim::CH_A; *ch_out = prim::CH_OUT;
  return 0;
}

int prim_run_wave(const float* in, unsigned* out, int nset, int id, int par, void* stream) {
  prim_wave_kernel<<<nset, 64, 0, (hipStream_t)stream>>>(in, out, id, par);
  return (int)hipGetLastError();
}

int prim_run_half(const float* in, unsigned* out, int nset, int id0, int par0, int id1, int par1, int mode, void* stream) {
  prim_half_kernel<<<nset, 64, 0, (hipStream_t)stream>>>(in, out, id0, par0, id1, par1, mode);
  return (int)hipGetLastError();
}

// inst: 0 Go2, 1 H1, 2 H1 loco, 3 Allegro on its dof tree, 4 Allegro dense (the cone solver's H); the generic path's DimsPadV (rollout_body.h:
// solve_spd_reg / solve_sq_reg): 5 crate climb (18, the Go2's tree: M and H), 6 push crate M (26, the H1's tree + the crate's own root),
// 7 push crate H (26, dense), 8 the capacity dimension (DIAL_MAX_V, dense).  form: 0 reg_chol_solve_v, 1
// reg_chol_solve2, 2 reg_chol_solve2 on WaveH (Go2 only; nsys must be even).  Returns the HIP error code, -1 for a bad argument.
int chol_run(int inst, int form, const float* A, const float* b, const float* scr0, unsigned* out, int nsys, int alias, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (form == 2) {
    if (inst != 0 || (nsys & 1)) return -1;
    chol_half_kernel<DimsGo2, TopoGo2><<<nsys / 2, 64, 0, st>>>(A, b, scr0, out, alias);
    return (int)hipGetLastError();
  }
  switch (inst) {
    case 0: return chol_launch<DimsGo2, TopoGo2>(form, A, b, scr0, out, nsys, alias, st);
    case 1: return chol_launch<DimsH1, TopoH1>(form, A, b, scr0, out, nsys, alias, st);
    case 2: return chol_launch<DimsH1Loco, TopoH1Loco>(form, A, b, scr0, out, nsys, alias, st);
    case 3: return chol_launch<DimsAllegro, TopoAllegro>(form, A, b, scr0, out, nsys, alias, st);
    case 4: return chol_launch<DimsAllegro, TopoDense>(form, A, b, scr0, out, nsys, alias, st);
    case 5: return chol_launch<DimsPadV<18>, TopoGo2>(form, A, b, scr0, out, nsys, alias, st);
    case 6: return chol_launch<DimsPadV<26>, TopoH1PushCrate>(form, A, b, scr0, out, nsys, alias, st);
    case 7: return chol_launch<DimsPadV<26>, TopoDense>(form, A, b, scr0, out, nsys, alias, st);
    case 8: return chol_launch<DimsPadV<DIAL_MAX_V>, TopoDense>(form, A, b, scr0, out, nsys, alias, st);
  }
  return -1;
}

}  // extern "C"
