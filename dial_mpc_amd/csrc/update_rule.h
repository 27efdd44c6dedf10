// update_rule.h -- K4a for the elite update rule (DIAL_UPDATE_ELITE, include/dial_mpc.h): uniform weights on the K best of a plan's B
// candidates, +0 on the rest.  Included by dial_hip.hip (the host side: launcher type, argument checks) and by update_rule.hip (the kernel); the functions of the
// first part are plain C++ (a CPU test compiles them).
//
// The order (best first): by reward, a NaN below every number (-inf included), -0 equal to +0, equal rewards by ascending index.
// The first K candidates in this order are the elites; each gets the fp32 quotient 1.0f / (float)K, bit for bit.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DIAL_UR_HD __host__ __device__ __forceinline__
#else
#define DIAL_UR_HD inline
#endif

namespace dial_update {

// Bit pattern of an fp32 reward -> a key whose UNSIGNED order is the rule's order: every NaN (either sign) -> 0, the lowest key;
// -0 -> the key of +0; otherwise the usual flip (negative: all bits, non-negative: the sign bit).  -inf maps to 0x007fffff > 0.
// Works on the bits, not on a float: the device code is compiled with -fno-honor-nans.
DIAL_UR_HD uint32_t reward_key(uint32_t bits) {
  if ((bits & 0x7fffffffu) > 0x7f800000u) return 0u;
  if (bits == 0x80000000u) bits = 0u;
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

// The correctly rounded fp32 quotient 1.0f / (float)K as a bit pattern, 1 <= K < 2^24, in integer arithmetic: the device build's fp32
// division is not correctly rounded (-fno-hip-fp32-correctly-rounded-divide-sqrt), and every elite must hold the bits the contract names.
// K = 2^e: exact.  Otherwise 1 / K = m 2^-(e + 1) with m = 2^(e + 1) / K in (1, 2): q = m 2^23 rounded to nearest, ties to even; a
// carry to q = 2^24 runs into the exponent field, as it must.
DIAL_UR_HD uint32_t elite_weight_bits(int K) {
  const uint32_t k = (uint32_t)K;
  int e = 0;
  while ((k >> (e + 1)) != 0u) e++;   // 2^e <= k < 2^(e + 1)
  if ((k & (k - 1u)) == 0u) return (uint32_t)(127 - e) << 23;
  const uint64_t num = 1ull << (e + 24);
  uint64_t q = num / k;
  const uint64_t rem = num - q * k;
  if (2u * rem > k || (2u * rem == k && (q & 1u))) q++;
  return ((uint32_t)(126 - e) << 23) + (uint32_t)(q - (1ull << 23));
}

// Elites among the candidates whose key EQUALS the K-th largest key: K less the number of keys above it.  The first that many of
// them in index order are taken (1 <= result <= the number of such candidates).
DIAL_UR_HD int elite_ties_taken(int K, int count_above) { return K - count_above; }

// One digit of the radix select: of the candidates still in play, `above` have a larger digit than bin d and `in_bin` fall into it;
// bin d holds the K'-th largest (K' = remaining) exactly when above < remaining <= above + in_bin.
DIAL_UR_HD bool elite_bin_holds(uint32_t above, uint32_t in_bin, uint32_t remaining) { return above < remaining && remaining <= above + in_bin; }

}   // namespace dial_update

#if defined(__HIPCC__)
#define UR_THREADS 1024
// The kernel lives in a library of its own, libdialupdate.so (update_rule.hip; the IEEE measurement variant links that unit itself), so
// that the code objects of libdialhip.so stay as shipped.  libdialhip.so looks this launcher up in its own directory when the elite
// rule is bound (dial_set_update_rule) and hands it the arguments weights_kernel takes, K in place of the temperature.
#define DIAL_UPDATE_RULE_SYMBOL "dial_update_rule_launch_v1"
typedef hipError_t (*dial_update_rule_launch_fn)(hipStream_t st, int plans, const float* rews, int B, int K, float* weights,
                                                 const float* gathered, int per, float* rews_out);
#endif

#if defined(__HIPCC__) && defined(DIAL_UPDATE_RULE_KERNEL)   // (update_rule.hip alone defines it)
#define UR_BLOCK 4   // 1024-index chunks whose keys a thread holds at once: B <= 4096 keeps every key in registers across the passes

// elite_weights_kernel: weights_kernel's launch shape and arguments, K in place of temp.  One 1024-thread workgroup per plan
// (blockIdx.x); rews_in / weights [plans][B]; `gathered` != nullptr: the packing first pass of the sharded phase B (see weights_kernel).
//   1. Four-pass 8-bit radix select of the K-th largest key T: per pass a 256-bin LDS histogram of the digit of the keys that share
//      the prefix found so far (integer LDS atomics: adds commute, the counts do not depend on arrival order); wavefront 0 then
//      suffix-scans it -- four bins per lane, a 64-lane shuffle scan of the lane totals --, names the one bin that holds the K'-th
//      largest and clears the histogram for the next pass: two barriers per pass.
//      A wavefront whose participating lanes all fall into one bin -- the rule for the leading digits of rewards of one magnitude --
//      adds its count with one atomic instead of up to 64 serialised ones.
//   2. Every key above T is an elite.  Of the keys equal to T the first `ties` in index order are: when all of them are (the usual
//      case, distinct rewards), one compare per candidate; otherwise a running count over consecutive 1024-index chunks -- __ballot /
//      popcount prefix inside a wavefront, the 16 wavefront counts through LDS (double-buffered: one barrier per chunk) -- and the
//      loop stops counting once the quota is met.
// A thread's keys are loaded UR_BLOCK chunks at a time (independent loads in flight together); with B <= UR_BLOCK x 1024 they are
// loaded once and stay in registers, otherwise every pass re-reads the rewards (<= 256 KB, cache resident).  1.2 KB of LDS, no
// scratch.  B from 2 up; K in 1 .. B (the caller checks).  The output depends on the rewards alone.
extern "C" __global__ void __launch_bounds__(UR_THREADS)
elite_weights_kernel(const float* __restrict__ rews_in, int B, int K, float* __restrict__ weights, const float* __restrict__ gathered,
                     int per, float* __restrict__ rews_out) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t sel[3];            // the chosen bin, the candidates still to find inside it, its population
  __shared__ uint32_t wcnt[2][UR_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* rews = rews_in + (size_t)blockIdx.x * B;
  weights += (size_t)blockIdx.x * B;
  if (tid < 256) hist[tid] = 0u;
  if (gathered) {
    const int n_total = B - 1;
    for (int n = tid; n < B; n += UR_THREADS)
      rews_out[n] = n < n_total ? gathered[(size_t)(n / per) * (per + 1) + (n % per)] : gathered[per];
    __threadfence_block();
    rews = rews_out;
  }
  __syncthreads();
  const uint32_t* rbits = reinterpret_cast<const uint32_t*>(rews);
  const int chunks = (B + UR_THREADS - 1) / UR_THREADS;
  const bool resident = chunks <= UR_BLOCK;   // (uniform)
  uint32_t key[UR_BLOCK];
  // keys of chunks c0 .. c0 + UR_BLOCK - 1 (0 past the end: such a candidate never takes part, every use checks n < B)
#define UR_LOAD_KEYS(c0)                                                         \
  _Pragma("unroll") for (int u = 0; u < UR_BLOCK; u++) {                         \
    const int n_ = ((c0) + u) * UR_THREADS + tid;                                \
    key[u] = n_ < B ? dial_update::reward_key(rbits[n_]) : 0u;                   \
  }
  if (resident) { UR_LOAD_KEYS(0) }

  uint32_t prefix = 0u, mask = 0u, remaining = (uint32_t)K, in_bin = 0u;
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int c0 = 0; c0 < chunks; c0 += UR_BLOCK) {
      if (!resident) { UR_LOAD_KEYS(c0) }
#pragma unroll
      for (int u = 0; u < UR_BLOCK; u++) {
        if (c0 + u < chunks) {   // (uniform; every lane of a wavefront runs the ballots together)
          const int n = (c0 + u) * UR_THREADS + tid;
          const bool in = n < B && (key[u] & mask) == prefix;
          const uint32_t bin = (key[u] >> shift) & 255u;
          const unsigned long long act = __ballot(in);
          if (act) {
            const int first = __ffsll((long long)act) - 1;
            const uint32_t fb = (uint32_t)__shfl((int)bin, first, 64);
            if (__ballot(in && bin == fb) == act) {
              if (lane == first) atomicAdd(&hist[fb], (uint32_t)__popcll(act));
            } else if (in) {
              atomicAdd(&hist[bin], 1u);
            }
          }
        }
      }
    }
    __syncthreads();
    if (wv == 0) {   // bins 4 lane .. 4 lane + 3: s = candidates in the bins above this lane's
      uint32_t h[4];
#pragma unroll
      for (int j = 0; j < 4; j++) { h[j] = hist[4 * lane + j]; hist[4 * lane + j] = 0u; }
      const uint32_t own = (h[0] + h[1]) + (h[2] + h[3]);
      uint32_t s = own;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_down((int)s, o, 64);
        if (lane + o < 64) s += t;
      }
      uint32_t above = s - own;
#pragma unroll
      for (int j = 3; j >= 0; j--) {
        if (dial_update::elite_bin_holds(above, h[j], remaining)) { sel[0] = (uint32_t)(4 * lane + j); sel[1] = remaining - above; sel[2] = h[j]; }
        above += h[j];
      }
    }
    __syncthreads();
    prefix |= sel[0] << shift;
    mask |= 255u << shift;
    remaining = sel[1];
    in_bin = sel[2];
    // (sel is rewritten only behind the next pass's first barrier, which every thread reaches after these reads)
  }
  const uint32_t T = prefix;                       // the K-th largest key
  const uint32_t ties = (uint32_t)dial_update::elite_ties_taken(K, K - (int)remaining);   // elites among the keys equal to T
  const uint32_t wbits = dial_update::elite_weight_bits(K);
  uint32_t* wout = reinterpret_cast<uint32_t*>(weights);
  const bool all_ties = ties == in_bin;            // every candidate at the threshold is an elite (uniform)
  uint32_t base = 0u;                              // candidates at the threshold below the current chunk (the same in every thread)
  for (int c0 = 0; c0 < chunks; c0 += UR_BLOCK) {
    if (!resident) { UR_LOAD_KEYS(c0) }
#pragma unroll
    for (int u = 0; u < UR_BLOCK; u++) {
      if (c0 + u < chunks) {
        const int c = c0 + u, n = c * UR_THREADS + tid;
        const bool eq = n < B && key[u] == T;
        bool take = n < B && (key[u] > T || (all_ties && eq));
        if (!all_ties && base < ties) {   // (uniform)
          const unsigned long long m = __ballot(eq);
          if (lane == 0) wcnt[c & 1][wv] = (uint32_t)__popcll(m);
          __syncthreads();
          uint32_t below = 0u, total = 0u;
#pragma unroll
          for (int w = 0; w < UR_THREADS / 64; w++) {
            const uint32_t v = wcnt[c & 1][w];
            below += w < wv ? v : 0u;
            total += v;
          }
          const uint32_t rank = base + below + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
          take = take || (eq && rank < ties);
          base += total;
        }
        if (n < B) wout[n] = take ? wbits : 0u;
      }
    }
  }
#undef UR_LOAD_KEYS
}
#endif
