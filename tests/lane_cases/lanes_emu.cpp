// lanes_emu.cpp -- host side of the lane-local pins (TEST INFRASTRUCTURE ONLY): the cases of lane_cases.h on the emulator build
// (-DDIAL_EMU, -ffp-contract=off), with the same C interface as lanes.hip minus the stream.  Lanes run one after the other, each with
// its own polygon slice, pre-filled like the device's.
#define DIAL_EMU 1
#include "rollout_body.h"   // (-I dial_mpc_amd/csrc: tests/lane_lib.py)
using namespace dial;
#include "lane_cases.h"

extern "C" {

int lane_sizes(int* v) {
  const int s[12] = {lane::G_IN, lane::G_OUT, lane::S_IN, lane::S_OUT, lane::K_IN, lane::K_OUT, lane::U_IN, lane::U_OUT, lane::T_IN, lane::T_OUT,
                     DIAL_BOX_POLY_WORDS, LANE_POLY_STRIDE};
  for (int k = 0; k < 12; k++) v[k] = s[k];
  return 0;
}

int lane_geom(const float* in, unsigned* out, int n, int fill) {
  if (n <= 0) return -1;
  for (size_t i = 0; i < (size_t)n; i++) {
    float poly[DIAL_BOX_POLY_WORDS];
    for (int k = 0; k < DIAL_BOX_POLY_WORDS; k++) poly[k] = __builtin_bit_cast(float, fill ? 0x7fc00000 : 0);
    lane::geom_case(in + i * lane::G_IN, out + i * lane::G_OUT, poly);
  }
  return 0;
}

int lane_seg(const float* in, unsigned* out, int n) {
  if (n <= 0) return -1;
  for (size_t i = 0; i < (size_t)n; i++) lane::seg_case(in + i * lane::S_IN, out + i * lane::S_OUT);
  return 0;
}

int lane_key(const int* in, unsigned* out, int n, int op, int par) {
  if (n <= 0 || op < 0 || op >= lane::K_COUNT) return -1;
  for (size_t i = 0; i < (size_t)n; i++) lane::key_case(in + i * lane::K_IN, out + i * lane::K_OUT, op, par);
  return 0;
}

int lane_key_uniform(const int* in, unsigned* out, int n, int rule, int minmax) {
  if (n <= 0) return -1;
  for (size_t i = 0; i < (size_t)n; i++) {
    Wave w;
    if (minmax) lane::key_uniform_case<true>(w, in + i * lane::U_IN, out + i * lane::U_OUT, rule, true);
    else lane::key_uniform_case<false>(w, in + i * lane::U_IN, out + i * lane::U_OUT, rule, true);
  }
  return 0;
}

int lane_trig(const float* in, unsigned* out, int n) {
  if (n <= 0) return -1;
  for (size_t i = 0; i < (size_t)n; i++) lane::trig_case(in + i * lane::T_IN, out + i * lane::T_OUT);
  return 0;
}

}  // extern "C"
