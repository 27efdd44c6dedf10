// prim_cases.h -- one test case per family of wave.h primitives (TEST INFRASTRUCTURE ONLY), written ONCE against the wave.h
// interface and compiled twice: by hipcc for gfx950 (prims.hip: one 64-thread workgroup per input set) and by g++ with -DDIAL_EMU
// (prims_emu.cpp: the host emulator).  tests/test_gpu_wave_prims.py compares the two bit for bit, tests/test_wave_prims_emu.py
// compares the emulator side with NumPy statements of wave.h's comments.
//
// A case reads up to NIN per-lane inputs and writes up to NOUT per-lane results of ONE input set:
//   in  [k * 64 + lane]   input k  (k < NIN)          out [k * 64 + lane]   result slot k  (k < NOUT), as raw bits
// For WaveH the physical lane is 32 * half + logical lane (`off` = 32 * half): the two halves of a launch read different data.
// The emulator's WaveH runs ONE half, so the host calls it once per half with that half's `off`.  A slot a case does not write
// keeps whatever the caller put there (a sentinel).
#pragma once

namespace prim {

constexpr int NIN = 4, NOUT = 66;

struct IO {
  const float* in;
  unsigned* out;
  int off;    // first physical lane of this wave / half
  int par;    // the case's run-time argument (a count, or the near / far variant of the fused-DPP cases)
};

enum Case {
  C_ROW = 0,    // quad_xor, row_shr/shl(_lo)<1..4>, row_bcast<0..15>, grp8_bcast3
  C_PICK,       // dup_rows, pick<0..31>
  C_BCAST,      // bc<K>, rowbc<0..15>, dup_halves
  C_PERM,       // lane_reverse, gather64 / gather
  C_MASK,       // mask, lane_gt / eq / lt
  C_COMPACT,    // compact (Wave)
  C_VSUMS,      // vsum, vsumN<3>, row16_sum, row16_sum3, row16_sumN<2>, seg8_sumN<2>
  C_FSUMS,      // sum, sum3, maxv over `par` items
  C_CONTRACT,   // a product formed in the case body, summed
  C_FMA,        // fma_pick<0..31>
  C_FNMA,       // fnma_pick<0..31>
  C_MUL,        // mul_pick<0..31>
  C_RCP,        // rcp_pick<0..31> and fast_rcp of the same lane
  C_COUNT
};

template <class W>
DIAL_DEV vfloat ld(W& w, const IO& io, int k) {
  return w.per_lane([&](int l) { return io.in[k * 64 + io.off + l]; });
}
#ifdef DIAL_EMU
template <class W>
inline void st(W&, const IO& io, int k, const vfloat& v) {
  for (int l = 0; l < (W::half2 ? 32 : 64); l++) io.out[k * 64 + io.off + l] = __builtin_bit_cast(unsigned, lane_val(v, l));
}
template <class W>
inline void st(W&, const IO& io, int k, float v) {   // a wave- (half-) uniform scalar: the same bits in every lane
  for (int l = 0; l < (W::half2 ? 32 : 64); l++) io.out[k * 64 + io.off + l] = __builtin_bit_cast(unsigned, v);
}
template <class W>
inline void stu(W&, const IO& io, int k, unsigned v) {
  for (int l = 0; l < (W::half2 ? 32 : 64); l++) io.out[k * 64 + io.off + l] = v;
}
#else
template <class W>
DIAL_DEV void st(W& w, const IO& io, int k, float v) { io.out[k * 64 + io.off + w.lane] = __builtin_bit_cast(unsigned, v); }
template <class W>
DIAL_DEV void stu(W& w, const IO& io, int k, unsigned v) { io.out[k * 64 + io.off + w.lane] = v; }
#endif

// shifts: every N the kernels use (smooth_quad*.h: 1, 2; smooth_rows.h: row_shr<1..4>, row_shr_lo / row_shl_lo<1, 2, 4>) and 3
template <class W>
DIAL_DEV void case_row(W& w, const IO& io) {
  const vfloat v = ld(w, io, 0);
  st(w, io, 0, w.quad_xor1(v));
  st(w, io, 1, w.quad_xor2(v));
  static_for<1, 5>([&](auto NN) {
    constexpr int n = NN;
    st(w, io, 2 + (n - 1), w.template row_shr<n>(v));
    st(w, io, 6 + (n - 1), w.template row_shl<n>(v));
    st(w, io, 10 + (n - 1), w.template row_shr_lo<n>(v));
    st(w, io, 14 + (n - 1), w.template row_shl_lo<n>(v));
  });
  static_for<0, 16>([&](auto KK) { constexpr int k = KK; st(w, io, 18 + k, w.template row_bcast<k>(v)); });
  if constexpr (W::half2) st(w, io, 34, w.grp8_bcast3(v));
}

template <class W>
DIAL_DEV void case_pick(W& w, const IO& io) {
  const vfloat v = ld(w, io, 0);
  vfloat X, Y;
  w.dup_rows(v, X, Y);
  st(w, io, 0, X);
  st(w, io, 1, Y);
  static_for<0, 32>([&](auto KK) { constexpr int k = KK; st(w, io, 2 + k, w.template pick<k>(X, Y)); });
}

// rowbc is defined for values every row holds a copy of: input 1 is read row-replicated (lane l takes word l & 15)
template <class W>
DIAL_DEV void case_bcast(W& w, const IO& io) {
  const vfloat v = ld(w, io, 0);
  if constexpr (W::half2) {
    static_for<0, 32>([&](auto KK) { constexpr int k = KK; st(w, io, k, w.template bc<k>(v)); });
  } else {
    st(w, io, 0, w.template bc<0>(v));
    st(w, io, 1, w.template bc<15>(v));
    st(w, io, 2, w.template bc<16>(v));
    st(w, io, 3, w.template bc<31>(v));
    st(w, io, 4, w.template bc<32>(v));
    st(w, io, 5, w.template bc<63>(v));
    vfloat LO, HI;
    w.dup_halves(v, LO, HI);
    st(w, io, 6, LO);
    st(w, io, 7, HI);
  }
  const vfloat r = w.per_lane([&](int l) { return io.in[64 + io.off + (l & 15)]; });
  static_for<0, 16>([&](auto KK) { constexpr int k = KK; st(w, io, 32 + k, w.template rowbc<k>(r)); });
}

// input 1: the source lane of every lane, as a float
template <class W>
DIAL_DEV void case_perm(W& w, const IO& io) {
  const vfloat v = ld(w, io, 0);
  const auto src = [&](int l) { return (int)io.in[64 + io.off + l]; };
  if constexpr (W::half2) st(w, io, 0, w.gather(v, src));
  else st(w, io, 0, w.gather64(v, src));
  st(w, io, 1, w.lane_reverse(v, 1));
  st(w, io, 2, w.lane_reverse(v, 18));
  st(w, io, 3, w.lane_reverse(v, 22));
  st(w, io, 4, w.lane_reverse(v, 26));
  st(w, io, 5, w.lane_reverse(v, 32));
  if constexpr (!W::half2) st(w, io, 6, w.lane_reverse(v, 64));
}

// the predicate is "input 0 is negative"
template <class W>
DIAL_DEV void case_mask(W& w, const IO& io) {
  const vfloat v = ld(w, io, 0);
  const unsigned long long b = w.mask(vlt0(v));
  stu(w, io, 0, (unsigned)b);
  stu(w, io, 1, (unsigned)(b >> 32));
  const vfloat one = vsplat(1.f), zero = vsplat(0.f);
  const int ks[4] = {0, 17, 31, W::half2 ? 30 : 63};
  for (int q = 0; q < 4; q++) {
    st(w, io, 2 + 3 * q, vsel(w.lane_gt(ks[q]), one, zero));
    st(w, io, 3 + 3 * q, vsel(w.lane_eq(ks[q]), one, zero));
    st(w, io, 4 + 3 * q, vsel(w.lane_lt(ks[q]), one, zero));
  }
}

// list = result slot 1 (words past the returned count keep the caller's sentinel); one-sample layouts only
template <class W>
DIAL_DEV void case_compact(W& w, const IO& io) {
  if constexpr (!W::half2) {
    const int n = w.compact(io.par, [&](int l) { return io.in[io.off + l] < 0.f; }, reinterpret_cast<float*>(io.out + 64));
    stu(w, io, 0, (unsigned)n);
  }
}

template <class W>
DIAL_DEV void case_vsums(W& w, const IO& io) {
  const vfloat a = ld(w, io, 0), b = ld(w, io, 1), c = ld(w, io, 2);
  st(w, io, 0, w.vsum(a));
  {
    vfloat t[3] = {a, b, c};
    float r[3];
    w.template vsumN<3>(t, r);
    st(w, io, 1, r[0]); st(w, io, 2, r[1]); st(w, io, 3, r[2]);
  }
  st(w, io, 4, w.row16_sum(a));
  {
    vfloat x = a, y = b, z = c;
    w.row16_sum3(x, y, z);
    st(w, io, 5, x); st(w, io, 6, y); st(w, io, 7, z);
  }
  {
    vfloat t[2] = {b, c};
    w.template row16_sumN<2>(t);
    st(w, io, 8, t[0]); st(w, io, 9, t[1]);
  }
  {
    vfloat t[2] = {a, c};
    w.template seg8_sumN<2>(t);
    st(w, io, 10, t[0]); st(w, io, 11, t[1]);
  }
}

// item i is word i % LW of input i / LW (LW = lanes of the wave / half): a loaded value, no arithmetic next to the strided add
template <class W>
DIAL_DEV void case_fsums(W& w, const IO& io) {
  constexpr int LW = W::half2 ? 32 : 64;
  const int count = io.par;
  const auto item = [&](int i) { return io.in[(i / LW) * 64 + io.off + (i % LW)]; };
  st(w, io, 0, w.sum(count, item));
  float a, b, c;
  w.sum3(count, [&](int i, float& x, float& y, float& z) { x += item(i); y += item(count - 1 - i); z += -item(i); }, a, b, c);
  st(w, io, 1, a); st(w, io, 2, b); st(w, io, 3, c);
  if constexpr (!W::half2) st(w, io, 4, w.maxv(count, item));
}

// The summand is a PRODUCT formed here and fed straight into the reductions: hipcc's contraction may fuse the multiply into the
// first butterfly add unless the reduction takes an opaque copy (wave.h: WaveH::opaque)
template <class W>
DIAL_DEV void case_contract(W& w, const IO& io) {
  constexpr int LW = W::half2 ? 32 : 64;
  const vfloat a = ld(w, io, 0), b = ld(w, io, 1);
  st(w, io, 0, w.vsum(a * b));
  st(w, io, 1, w.row16_sum(a * b));
  st(w, io, 2, w.sum(LW, [&](int i) { return io.in[io.off + i] * io.in[64 + io.off + i]; }));
}

// fused DPP arithmetic on the X | Y of dup_rows.  par = 0: in source order the first consumer comes immediately after dup_rows (what the
// s_nop in dup_rows is for); par = 1: three dependent VALU results (exact: x 2, x 2, x 0.25) that the consumer needs -- through `other`, or
// for rcp_pick, which has no operand but X | Y, results computed FROM X and kept live in a slot of their own -- are written after
// dup_rows.  Source order does not bind the scheduler: the two variants are two instruction streams around the same hand-written DPP
// instructions, not a guarantee of how many VALU instructions sit in between.
template <int WHICH, class W>
DIAL_DEV void case_fused(W& w, const IO& io) {
  const vfloat v = ld(w, io, 0);
  vfloat other = ld(w, io, 1);
  const vfloat acc = ld(w, io, 2);
  vfloat X, Y;
  w.dup_rows(v, X, Y);
  if (io.par) {
    other = other * 2.f;
    other = other * 2.f;
    other = other * 0.25f;
  }
  static_for<0, 32>([&](auto KK) {
    constexpr int k = KK;
    if constexpr (WHICH == 0) st(w, io, k, w.template fma_pick<k>(acc, X, Y, other));
    else if constexpr (WHICH == 1) st(w, io, k, w.template fnma_pick<k>(acc, X, Y, other));
    else st(w, io, k, w.template mul_pick<k>(X, Y, other));
  });
}

template <class W>
DIAL_DEV void case_rcp(W& w, const IO& io) {
  const vfloat v = ld(w, io, 0);
  vfloat X, Y;
  w.dup_rows(v, X, Y);
  if (io.par) {
    vfloat t = X * 2.f;
    t = t * 2.f;
    t = t * 0.25f;
    st(w, io, 64, t);   // (== X for normal numbers)
  }
  static_for<0, 32>([&](auto KK) { constexpr int k = KK; st(w, io, k, w.template rcp_pick<k>(X, Y)); });
  static_for<0, 32>([&](auto KK) {
    constexpr int k = KK;
    if constexpr (W::half2) st(w, io, 32 + k, vsplat(fast_rcp(w.template bc<k>(v))));
    else st(w, io, 32 + k, vrcp(w.template pick<k>(X, Y)));
  });
}

template <class W>
DIAL_DEV void run_case(W& w, const IO& io, int id) {
  switch (id) {
    case C_ROW: case_row(w, io); break;
    case C_PICK: case_pick(w, io); break;
    case C_BCAST: case_bcast(w, io); break;
    case C_PERM: case_perm(w, io); break;
    case C_MASK: case_mask(w, io); break;
    case C_COMPACT: case_compact(w, io); break;
    case C_VSUMS: case_vsums(w, io); break;
    case C_FSUMS: case_fsums(w, io); break;
    case C_CONTRACT: case_contract(w, io); break;
    case C_FMA: case_fused<0>(w, io); break;
    case C_FNMA: case_fused<1>(w, io); break;
    case C_MUL: case_fused<2>(w, io); break;
    case C_RCP: case_rcp(w, io); break;
    default: break;
  }
}

}  // namespace prim
