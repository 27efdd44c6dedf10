// lane_cases.h -- the lane-local code of the kernels, one case per lane (TEST INFRASTRUCTURE ONLY): the box narrow phases of
// box_collide.h, the MJX segment helpers and make_frame of rollout_body.h, the integer-key bracket bookkeeping of ls_bracket.h and
// dm::fast_sincos / axis_angle_to_quat.  Included by lanes.hip (gfx950: product flags and IEEE flags) and by lanes_emu.cpp (host,
// -DDIAL_EMU -ffp-contract=off); tests/lane_lib.py builds the three libraries.  Inputs are plain float / int rows, results are raw
// 32-bit words, so that two builds can be compared bit for bit.
#pragma once

namespace lane {

constexpr int G_IN = 22, G_OUT = 13;   // geom: (kind, sub, g1[10], g2[10]) -> (dist, pos[3], frame[9]); g = (pos[3], quat[4], size[3])
constexpr int S_IN = 13, S_OUT = 9;    // seg:  (op, 12 floats) -> up to 9 words
constexpr int K_IN = 8, K_OUT = 10;    // key:  8 ints -> up to 10 words
constexpr int U_IN = 5, U_OUT = 9;     // key, wave-uniform: (lo.d0, hi.d0, k_lo_next, k_hi_next, k_mid) -> (lo[4], hi[4], any)
constexpr int T_IN = 4, T_OUT = 6;     // trig: (axis[3], angle) -> (sin, cos of the angle; the quaternion of axis_angle_to_quat)
#ifndef LANE_POLY_STRIDE
#define LANE_POLY_STRIDE DIAL_BOX_POLY_WORDS   // words between the polygon slices of neighbouring lanes
#endif

enum { S_POINT = 0, S_SEGSEG = 1, S_FRAME = 2 };
enum { K_FKEY = 0, K_PACK, K_OPEN, K_UPDATE, K_LAZY, K_GATE, K_RESULT, K_COUNT };

DIAL_DEV unsigned ubits(float x) { return __builtin_bit_cast(unsigned, x); }

// exactly the call shapes of collide_contact (rollout_body.h) / emu_box_contact (tests/wave_emu/emu.cpp); geom2 is the box
DIAL_DEV void geom_case(const float* in, unsigned* out, float* poly) {
  const int kind = (int)in[0], sub = (int)in[1];
  const float *g1 = in + 2, *g2 = in + 12;
  BoxG b1, b2;
  for (int k = 0; k < 3; k++) { b1.c[k] = g1[k]; b1.h[k] = g1[7 + k]; b2.c[k] = g2[k]; b2.h[k] = g2[7 + k]; }
  for (int k = 0; k < 4; k++) { b1.q[k] = g1[3 + k]; b2.q[k] = g2[3 + k]; }
  float mat[9];
  dm::quat_to_mat(mat, b1.q);
  const float ax1[3] = {mat[2], mat[5], mat[8]};
  const float p1[3] = {g1[0], g1[1], g1[2]};
  float dist = 0.f, pos[3] = {0.f, 0.f, 0.f}, fr[9];
  if (kind == DIAL_CON_PLANE_BOX) plane_box(ax1, p1, b2, sub, dist, pos, fr);
  else if (kind == DIAL_CON_SPHERE_BOX) sphere_box(p1, g1[7], b2, dist, pos, fr);
  else if (kind == DIAL_CON_CAPSULE_BOX) capsule_box(p1, ax1, g1[8], g1[7], b2, sub, dist, pos, fr);
  else box_box(b1, b2, sub, dist, pos, fr, poly);
  out[0] = ubits(dist);
  for (int k = 0; k < 3; k++) out[1 + k] = ubits(pos[k]);
  for (int k = 0; k < 9; k++) out[4 + k] = ubits(fr[k]);
}

DIAL_DEV void seg_case(const float* in, unsigned* out) {
  const int op = (int)in[0];
  const float* x = in + 1;
  if (op == S_POINT) {
    float o[3];
    closest_segment_point(o, x, x + 3, x + 6);
    for (int k = 0; k < 3; k++) out[k] = ubits(o[k]);
  } else if (op == S_SEGSEG) {
    float a[3], b[3];
    closest_segment_to_segment(a, b, x, x + 3, x + 6, x + 9);
    for (int k = 0; k < 3; k++) { out[k] = ubits(a[k]); out[3 + k] = ubits(b[k]); }
  } else {
    float fr[9];
    make_frame(fr, x);
    for (int k = 0; k < 9; k++) out[k] = ubits(fr[k]);
  }
}

// the words a bracket point carries besides its slope key: 0x100 * id + word (id 1 lo, 2 hi, 3 lo_next, 4 hi_next, 5 mid)
DIAL_DEV LsPt key_point(int id, int d0) { return LsPt{0x100 * id, 0x100 * id + 1, 0x100 * id + 2, d0}; }
DIAL_DEV void key_put(unsigned* out, const LsPt& p) { out[0] = p.alpha; out[1] = p.nalpha; out[2] = p.cost; out[3] = p.d0; }

// par: K_UPDATE the rule (1 = `swap`); K_LAZY 0 / 1 = ls_update_lazy<true> with that rule, 2 = ls_update_lazy<false> (`_in_bracket` as booleans)
DIAL_DEV void key_case(const int* in, unsigned* out, int op, int par) {
  if (op == K_FKEY) {
    const float x = bitsf(in[0]);
    out[0] = fkey(x);
    out[1] = ubits(fkeyf(x));
  } else if (op == K_PACK) {
    float o[4];
    ls_pack(bitsf(in[0]), bitsf(in[1]), bitsf(in[2]), bitsf(in[3]), o[0], o[1], o[2], o[3]);
    for (int k = 0; k < 4; k++) out[k] = ubits(o[k]);
  } else if (op == K_OPEN) {
    const LsPt p0{in[0], in[1], in[2], in[3]}, p1{in[4], in[5], in[6], in[7]};
    LsPt lo, hi;
    ls_open(p0, p1, lo, hi);
    key_put(out, lo);
    key_put(out + 4, hi);
  } else if (op == K_UPDATE) {
    LsPt lo = key_point(1, in[0]), hi = key_point(2, in[1]);
    const bool any = ls_update(par != 0, lo, hi, key_point(3, in[2]), key_point(4, in[3]), key_point(5, in[4]));
    key_put(out, lo);
    key_put(out + 4, hi);
    out[8] = any ? 1 : 0;
  } else if (op == K_LAZY) {   // emu_ls_update's form (the fetch of lane L returns 1000 + L for every word), and the fetched words themselves
    LsPt lo{11, 12, 13, in[0]}, hi{14, 15, 16, in[1]};
    const auto fetch = [&](int, int lane) { return 1000 + lane; };
    const bool any = par == 2 ? ls_update_lazy<false>(false, lo, hi, in[2], in[3], in[4], 0, 1, 2, fetch)
                              : ls_update_lazy<true>(par != 0, lo, hi, in[2], in[3], in[4], 0, 1, 2, fetch);
    out[0] = lo.d0; out[1] = hi.d0;
    out[2] = lo.alpha >= 1000 ? lo.alpha - 1000 : -1;
    out[3] = hi.alpha >= 1000 ? hi.alpha - 1000 : -1;
    out[4] = any ? 1 : 0;
    out[5] = lo.alpha; out[6] = lo.nalpha; out[7] = lo.cost; out[8] = hi.alpha; out[9] = hi.nalpha;
  } else if (op == K_GATE) {   // (lo.d0, hi.d0, kg, kng)
    const LsPt lo{0, 0, 0, in[0]}, hi{0, 0, 0, in[1]};
    const LsGate g = ls_gate(in[2], in[3]);
    const bool cl = ls_converged_lo(lo, g), ch = ls_converged_hi(hi, g);
    out[0] = (ls_converged(lo, hi, in[2], in[3]) ? 1 : 0) | ((cl || ch) ? 2 : 0);
    out[1] = cl ? 1 : 0;
    out[2] = ch ? 1 : 0;
  } else if (op == K_RESULT) {   // (p0.cost, lo.alpha, lo.cost, hi.alpha, hi.cost)
    const LsPt p0{0, 0, in[0], 0}, lo{in[1], 0, in[2], 0}, hi{in[3], 0, in[4], 0};
    float alpha;
    const bool improved = ls_result(p0, lo, hi, alpha);
    out[0] = ubits(alpha);
    out[1] = improved ? 1 : 0;
  }
}

// The update in the form the kernels compile (solver_reg.h: the line search): ONE case per wavefront, every word of it wave-uniform
// (DM_UNIFORM_I), the three trial points in the 16-lane groups that start at lanes 0 / 16 / 32 (lo_next, hi_next, mid), the fetch a
// lane-indexed read of the winner's first lane.  Word k of lane l holds 0x3f800000 + 0x1000 k + l, so a fetch from any other lane shows;
// the slope key of a group is right in its FIRST lane only.  `writer`: the lane that stores the (uniform) result.
template <bool MINMAX, class W>
DIAL_DEV void key_uniform_case(W& w, const int* in, unsigned* out, int rule, bool writer) {
  const int k0 = DM_UNIFORM_I(in[0]), k1 = DM_UNIFORM_I(in[1]), kt[3] = {DM_UNIFORM_I(in[2]), DM_UNIFORM_I(in[3]), DM_UNIFORM_I(in[4])};
  const int rule_u = DM_UNIFORM_I(rule);
  vfloat pk[4];
  w.per_lane_n(pk, [&](int l, float* o) {
    for (int k = 0; k < 3; k++) o[k] = bitsf(0x3f800000 + 0x1000 * k + l);
    const int g = l >> 4;
    o[3] = bitsf(((l & 15) == 0 && g < 3) ? (g == 0 ? kt[0] : (g == 1 ? kt[1] : kt[2])) : 0x7f000000 + l);
  });
  LsPt lo = key_point(1, k0), hi = key_point(2, k1);
  const bool any = ls_update_lazy<MINMAX>(rule_u != 0, lo, hi, fbits(bcast(pk[3], 0)), fbits(bcast(pk[3], 16)), fbits(bcast(pk[3], 32)), 0, 16, 32,
                                          [&](int word, int lane) { return fbits(bcast(pk[word], lane)); });
  if (writer) {
    key_put(out, lo);
    key_put(out + 4, hi);
    out[8] = any ? 1 : 0;
  }
}

DIAL_DEV void trig_case(const float* in, unsigned* out) {
  float s, c, q[4];
  dm::fast_sincos(in[3], s, c);
  dm::axis_angle_to_quat(q, in, in[3]);
  out[0] = ubits(s); out[1] = ubits(c);
  for (int k = 0; k < 4; k++) out[2 + k] = ubits(q[k]);
}

}  // namespace lane
