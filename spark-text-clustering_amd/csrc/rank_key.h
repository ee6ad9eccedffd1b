// rank_key.h — the device pieces every ranked query shares (rank.hip, lda_score.hip, lda_em.hip): the 96-bit
// key and its selected prefix, the digit pick of a radix-selection pass, the rule that ends the passes, the
// block bitonic sort of a candidate list and the (value, index) butterfly over a row's lanes.  Device code only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace stc {
namespace rank {

// ---- the key ---------------------------------------------------------------------------------------------------
// An entry's key is 96 bits: the value's bits made to order like the value (value_key), then the complemented
// index (~index as uint32_t).  Keys of distinct indices are distinct, and their descending order is the ranked
// queries' contract: the larger value first, then the smaller index.  Twelve 8-bit digits, most significant first.
constexpr int kDigits = 12;  // 8 of the value, 4 of the complemented index

// −0 is read as 0, negatives below positives; key_value gives back the double (0 for −0)
template <typename T>
__device__ inline uint64_t value_key(T v) {
  const double x = (double)v;
  const uint64_t b = x == 0.0 ? 0ull : (uint64_t)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline double key_value(uint64_t key) {
  const uint64_t b = (key >> 63) ? (key & 0x7FFFFFFFFFFFFFFFull) : ~key;
  return __longlong_as_double((long long)b);
}
// descending by (value key, ~index): the larger value first, then the smaller index
__device__ inline bool key_before(uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib) {
  return ka > kb || (ka == kb && ia < ib);
}

// The digits a radix selection has fixed so far: nd of them from the top of (hi, lo), the rest 0.  All zero is
// the empty prefix, so a cleared record is a fresh selection.
struct Prefix {
  uint64_t hi;
  uint32_t lo;
  uint32_t nd;
  // the key's next digit, the one this pass counts (nd < kDigits)
  __device__ uint32_t digit(uint64_t khi, uint32_t klo) const {
    return nd < 8 ? (uint32_t)(khi >> (56 - 8 * nd)) & 255u : (klo >> (24 - 8 * (nd - 8))) & 255u;
  }
  // the key's first nd digits equal the prefix's (nd < kDigits)
  __device__ bool matches(uint64_t khi, uint32_t klo) const {
    if (nd == 0) return true;
    if (nd <= 8) return ((khi ^ hi) >> (64 - 8 * nd)) == 0;
    return khi == hi && ((klo ^ lo) >> (32 - 8 * (nd - 8))) == 0;
  }
  // the key's first nd digits are at or above the prefix's (nd <= kDigits: with all twelve, the keys themselves)
  __device__ bool at_or_above(uint64_t khi, uint32_t klo) const {
    if (nd == 0) return true;
    if (nd <= 8) {
      const int sh = 64 - 8 * nd;
      return (khi >> sh) >= (hi >> sh);
    }
    const int sh = 32 - 8 * (nd - 8);
    return khi > hi || (khi == hi && (klo >> sh) >= (lo >> sh));
  }
  __device__ void append(uint32_t d) {
    if (nd < 8) hi |= (uint64_t)d << (56 - 8 * nd);
    else lo |= d << (24 - 8 * (nd - 8));
    nd += 1;
  }
  // The passes end once the keys at or above the prefix (`kept`: those above it and those inside its last digit)
  // fit the caller's candidate list of `capacity` entries, at the latest with all twelve digits, when they are
  // exactly the N asked for.
  __device__ bool done(uint32_t kept, uint32_t capacity) const { return kept <= capacity || nd == kDigits; }
};

// ---- the digit pick --------------------------------------------------------------------------------------------
// One pass's histogram → the digit that holds the N-th key.  h: `copies` histograms of 256 counters, copy c's digit
// d at h[c·pitch + d]; above: the keys above the prefix so far (< N).  Called by all 64 lanes of one wave, which all
// get the result: the digit whose keys take the count to N, the keys above it (the new `above`), the keys inside it.
// Lane l owns digits 255 − 4l … 252 − 4l; a wave prefix sum over the lanes' totals finds the first lane whose digits
// reach N, and that lane walks its four.  Should the counts fall short of N (they do not: N is at most the number
// of candidates) no lane reaches it; lane 63 then answers, and its walk stops at its last digit, 0, with every
// other key counted above — the digit a serial walk from 255 down ends on.
struct DigitPick {
  uint32_t digit, above, in_digit;
};
__device__ inline DigitPick pick_digit(const uint32_t* h, int copies, int pitch, uint32_t above, uint32_t N) {
  const int lane = threadIdx.x & 63;
  uint32_t c[4], tot = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int dg = 255 - 4 * lane - q;
    c[q] = 0;
    for (int w = 0; w < copies; ++w) c[q] += h[w * pitch + dg];
    tot += c[q];
  }
  uint32_t incl = tot;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t o = __shfl_up(incl, off, 64);
    if (lane >= off) incl += o;
  }
  uint32_t before = above + incl - tot;
  const unsigned long long reach = __ballot(before + tot >= N);
  const int owner = reach ? __ffsll((long long)reach) - 1 : 63;
  int q = 0;
  uint32_t in = c[0];
#pragma unroll
  for (int i = 1; i < 4; ++i)  // this lane's walk: on to digit i while the count through digit i − 1 is short of N
    if (q == i - 1 && before + in < N) before += in, in = c[i], q = i;
  DigitPick p;
  p.digit = (uint32_t)__shfl(255 - 4 * lane - q, owner, 64);
  p.above = __shfl(before, owner, 64);
  p.in_digit = __shfl(in, owner, 64);
  return p;
}

// ---- the candidate list's sort ---------------------------------------------------------------------------------
// A bitonic sort of P (a power of two >= 2) pairs (key, idx) into key_before's order, by the 256 threads of a
// block; padding of (0, 0xFFFFFFFF) sorts behind every key (an index is below 2^31).  Ends in a barrier.
// The access order, argued for key (u64) / idx (u32) in LDS: thread p of a step holds the pair
// a = 2p − (p & (stride − 1)), b = a + stride.  Read in that order, lanes l and l + 16 of a 32-lane ds_read group
// would meet on one bank at every stride below 32 (a advances by 32 elements per 16 pairs: the a's of a 64-element
// window are its elements with the stride bit clear).  So lanes with bit 4 set read b first and a second: the first
// instruction then takes the window's first 32 elements with the stride bit clear from lanes 0–15 and its last 32
// with the bit set from lanes 16–31 — all 32 residues mod 32, conflict-free for the u64 reads (banks (a/4) mod 64:
// 32 doubles a row) and the u32 reads and writes (32 banks); at strides >= 32 both halves are contiguous runs.
// ds_write_b64 groups are 16 contiguous lanes on 16 double slots, so the key writes swap on lane bit 3 instead
// (the same argument on a 32-element window).  On a list in global memory the order is harmless.
__device__ inline void block_bitonic_sort(uint64_t* key, uint32_t* idx, uint32_t P) {
  const int tid = threadIdx.x;
  const bool r16 = (tid & 16) != 0, w8 = (tid & 8) != 0;
  for (uint32_t size = 2; size <= P; size <<= 1) {
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
      for (uint32_t p = tid; p < P / 2; p += 256) {
        const uint32_t a = 2 * p - (p & (stride - 1)), b = a + stride;
        const uint32_t x = r16 ? b : a, y = r16 ? a : b;
        const uint64_t kx = key[x], ky = key[y];
        const uint32_t ix = idx[x], iy = idx[y];
        const uint64_t ka = r16 ? ky : kx, kb = r16 ? kx : ky;
        const uint32_t ia = r16 ? iy : ix, ib = r16 ? ix : iy;
        const bool first = (a & size) == 0;  // this run sorts in the contract's order, the next one reversed
        if (key_before(kb, ib, ka, ia) == first) {
          key[w8 ? b : a] = w8 ? ka : kb;
          key[w8 ? a : b] = w8 ? kb : ka;
          idx[x] = r16 ? ia : ib;
          idx[y] = r16 ? ib : ia;
        }
      }
      __syncthreads();
    }
  }
}

// ---- a row's maximum -------------------------------------------------------------------------------------------
// The (value, index) butterfly over the `lanes` (a power of two <= 64) adjacent lanes that hold one row: every lane
// comes in with its own best value and that value's index and leaves with the row's — the larger value, and among
// equal values the larger index if LARGER_INDEX, else the smaller.
template <bool LARGER_INDEX>
__device__ __forceinline__ void row_argmax(int lanes, double& best, int& bj) {
  for (int off = lanes >> 1; off > 0; off >>= 1) {
    const double ov = __shfl_xor(best, off, 64);
    const int oj = __shfl_xor(bj, off, 64);
    const bool take = (ov > best) | ((ov == best) & (LARGER_INDEX ? oj > bj : oj < bj));
    best = take ? ov : best;
    bj = take ? oj : bj;
  }
}

}  // namespace rank
}  // namespace stc
