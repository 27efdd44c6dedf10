// prims_emu.cpp -- host side of the wave.h / register L D L^T pins (TEST INFRASTRUCTURE ONLY): the cases of prim_cases.h and
// chol_cases.h on the emulator (-DDIAL_EMU, -ffp-contract=off), with the same C interface as prims.hip minus the stream.  Wave runs
// with tree_sums (the GPU's association); the emulator's WaveH is ONE half, so prim_run_half takes which half's data to run on.
#define DIAL_EMU 1
#include "rollout_body.h"   // (-I dial_mpc_amd/csrc: tests/prim_lib.py)
using namespace dial;
#include "prim_cases.h"
#include "chol_cases.h"

#include <vector>

using prim::IO;

template <class W, class D, class TopoT, int FORM>
static void chol_one(const float* A, const float* b, const float* scr0, unsigned* out, int off, int alias) {
  constexpr int N = D::NV, S = kCholStride<N>;
  W w;
  w.tree_sums = true;
  std::vector<float> A_lds(N * S), scr_lds(N * S);
  prim::chol_case<D, TopoT, FORM>(w, A, b, scr0, out, off, alias, A_lds.data(), scr_lds.data());
}

template <class D, class TopoT>
static int chol_all(int form, const float* A, const float* b, const float* scr0, unsigned* out, int nsys, int alias) {
  for (int k = 0; k < nsys; k++) {
    const float *Ak = A + (size_t)k * prim::CH_A, *bk = b + (size_t)k * 64, *sk = scr0 + (size_t)k * prim::CH_A;
    unsigned* ok = out + (size_t)k * prim::CH_OUT;
    if (form == 0) chol_one<Wave, D, TopoT, 0>(Ak, bk, sk, ok, 0, alias);
    else if (form == 1) chol_one<Wave, D, TopoT, 1>(Ak, bk, sk, ok, 0, alias);
    else if (form == 2) chol_one<WaveH, D, TopoT, 1>(Ak, bk, sk, ok, 32 * (k & 1), alias);
    else return -1;
  }
  return 0;
}

extern "C" {

int prim_sizes(int* nin, int* nout, int* ncase, int* ch_a, int* ch_out) {
  *nin = prim::NIN; *nout = prim::NOUT; *ncase = prim::C_COUNT; *ch_a = prim::CH_A; *ch_out = prim::CH_OUT;
  return 0;
}

int prim_run_wave(const float* in, unsigned* out, int nset, int id, int par) {
  for (int k = 0; k < nset; k++) {
    Wave w;
    w.tree_sums = true;
    const IO io{in + (size_t)k * prim::NIN * 64, out + (size_t)k * prim::NOUT * 64, 0, par};
    prim::run_case(w, io, id);
  }
  return 0;
}

int prim_run_half(const float* in, unsigned* out, int nset, int id, int par, int half) {
  for (int k = 0; k < nset; k++) {
    WaveH w;
    const IO io{in + (size_t)k * prim::NIN * 64, out + (size_t)k * prim::NOUT * 64, 32 * half, par};
    prim::run_case(w, io, id);
  }
  return 0;
}

int chol_run(int inst, int form, const float* A, const float* b, const float* scr0, unsigned* out, int nsys, int alias) {
  if (form == 2 && inst != 0) return -1;
  switch (inst) {
    case 0: return chol_all<DimsGo2, TopoGo2>(form, A, b, scr0, out, nsys, alias);
    case 1: return chol_all<DimsH1, TopoH1>(form, A, b, scr0, out, nsys, alias);
    case 2: return chol_all<DimsH1Loco, TopoH1Loco>(form, A, b, scr0, out, nsys, alias);
    case 3: return chol_all<DimsAllegro, TopoAllegro>(form, A, b, scr0, out, nsys, alias);
    case 4: return chol_all<DimsAllegro, TopoDense>(form, A, b, scr0, out, nsys, alias);
    case 5: return chol_all<DimsPadV<18>, TopoGo2>(form, A, b, scr0, out, nsys, alias);
    case 6: return chol_all<DimsPadV<26>, TopoH1PushCrate>(form, A, b, scr0, out, nsys, alias);
    case 7: return chol_all<DimsPadV<26>, TopoDense>(form, A, b, scr0, out, nsys, alias);
    case 8: return chol_all<DimsPadV<DIAL_MAX_V>, TopoDense>(form, A, b, scr0, out, nsys, alias);
  }
  return -1;
}

// the device's documented associations (wave.h), for the host side of the sum checks
float prim_row_tree(const float* v16) { return emu_row_tree(v16); }
float prim_tree64(const float* v64) { return emu_tree64(v64); }
float prim_tree32(const float* v32) { return emu_tree32(v32); }

// out[i] = fma(a[i], b[i], c[i]) with ONE rounding (what v_fmac_f32 computes), and the separately rounded a[i] * b[i]
void prim_fmaf(int n, const float* a, const float* b, const float* c, float* out) {
  for (int i = 0; i < n; i++) out[i] = std::fmaf(a[i], b[i], c[i]);
}
void prim_mulf(int n, const float* a, const float* b, float* out) {
  for (int i = 0; i < n; i++) out[i] = a[i] * b[i];
}

}  // extern "C"
