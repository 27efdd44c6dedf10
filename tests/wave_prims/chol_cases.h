// chol_cases.h -- the register L D L^T of solver_reg.h on ONE system per wave / half (TEST INFRASTRUCTURE ONLY): a fresh solve, what
// it leaves in `scratch` and in the pivot reciprocals, and a REUSE solve of the same right-hand side on that factor.  Compiled for
// gfx950 (prims.hip) and for the host emulator (prims_emu.cpp); see prim_cases.h.
//
// Per system:  A    [CH_A]   the N x kCholStride<N> square (row-major), exact zeros off the pattern and in the pad columns
//              b    [64]     right-hand side per physical lane (the caller puts NaN in lanes >= N)
//              scr0 [CH_A]   what `scratch` holds before the fresh solve
//              out  [CH_OUT] x (64) | pivot reciprocals, lane = REVERSED dof (64) | x of the REUSE solve (64) | scratch after (CH_A)
// FORM 0: reg_chol_solve_v, 1: reg_chol_solve2.  alias != 0: scratch IS the storage of A (as the Newton solver passes s.H, s.H).
#pragma once

namespace prim {

constexpr int CH_A = 1024, CH_OUT = 3 * 64 + CH_A;

template <class D, class TopoT, int FORM, bool REUSE, class W>
DIAL_DEV vfloat chol_call(W& w, const float* A, vfloat b, float* scratch, vfloat* dinv) {
  const int* m = nullptr;
  if constexpr (FORM == 0) return dial::reg_chol_solve_v<D, TopoT, REUSE>(w, m, A, b, scratch, dinv);
  else return dial::reg_chol_solve2<D, TopoT, REUSE>(w, m, A, b, scratch, dinv);
}

// A_lds / scr_lds: N * kCholStride<N> floats each, 16-byte aligned, private to this wave / half.  off: first physical lane.
template <class D, class TopoT, int FORM, class W>
DIAL_DEV void chol_case(W& w, const float* A, const float* b, const float* scr0, unsigned* out, int off, int alias, float* A_lds,
                        float* scr_lds) {
  constexpr int N = D::NV, S = dial::kCholStride<N>;
  static_assert(N * S <= CH_A, "CH_A");
  float* scratch = alias ? A_lds : scr_lds;
  w.items(N * S, [&](int e) { scr_lds[e] = scr0[e]; });
  w.items(N * S, [&](int e) { A_lds[e] = A[e]; });
  const vfloat bv = w.per_lane([&](int l) { return b[off + l]; });
  const IO io{nullptr, out, off, 0};
  vfloat dinv = vsplat(0.f);
  const vfloat x = chol_call<D, TopoT, FORM, false>(w, A_lds, bv, scratch, &dinv);
  st(w, io, 0, x);
  st(w, io, 1, dinv);
  w.fence();
  w.items(N * S, [&](int e) { out[3 * 64 + e] = __builtin_bit_cast(unsigned, scratch[e]); });
  const vfloat x2 = chol_call<D, TopoT, FORM, true>(w, A_lds, bv, scratch, &dinv);
  st(w, io, 2, x2);
}

}  // namespace prim
