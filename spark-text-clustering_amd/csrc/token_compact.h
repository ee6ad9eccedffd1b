// token_compact.h — what text_prep.hip and token_stages.hip share: strict UTF-8 decoding, the open-addressing
// stop-word table (FNV-1a), and the compaction of kept tokens into a valid stc_dtok — scans of the kept lengths and
// the kept flags, k_emit (the blob and tok_off, u32 or int64) and k_doc_off (doc_off and the longest document).
// Integer arithmetic only; the one atomic is the longest-document maximum, which is order-independent.
#pragma once

#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "stc_handles.h"

namespace stc {
namespace prep {

constexpr int kBlock = 256;
constexpr uint32_t kBadCp = ~0u;

struct StopSlot {
  uint64_t hash;
  int64_t off;
  int64_t len;  // −1: empty
};

__host__ __device__ inline uint64_t fnv1a(const uint8_t* p, int64_t n) {
  uint64_t h = 0xCBF29CE484222325ull;
  for (int64_t i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001B3ull;
  return h;
}

// length of the UTF-8 sequence a lead byte opens; 0: not a lead (a continuation byte, the overlong leads C0 / C1,
// F5 and above)
__host__ __device__ inline int lead_len(uint32_t b) {
  return b < 0x80u ? 1 : b < 0xC2u ? 0 : b < 0xE0u ? 2 : b < 0xF0u ? 3 : b < 0xF5u ? 4 : 0;
}
// the code point of the n readable bytes at p (n = lead_len(p[0]) > 0), kBadCp unless they are well-formed UTF-8
// (continuation bytes, shortest form, no surrogate, ≤ U+10FFFF)
__host__ __device__ inline uint32_t decode_strict(const uint8_t* p, int n) {
  if (n == 1) return p[0];
  uint32_t cp = p[0] & (0xFFu >> (n + 1));
  for (int q = 1; q < n; ++q) {
    const uint32_t c = p[q];
    if ((c & 0xC0u) != 0x80u) return kBadCp;
    cp = (cp << 6) | (c & 0x3Fu);
  }
  if (n == 3 && (cp < 0x800u || (cp >= 0xD800u && cp <= 0xDFFFu))) return kBadCp;
  if (n == 4 && (cp < 0x10000u || cp > 0x10FFFFu)) return kBadCp;
  return cp;
}
// first byte of [p, p + n) that is not part of well-formed UTF-8, −1 when all of it is
__host__ __device__ inline int64_t first_bad_utf8(const uint8_t* p, int64_t n) {
  for (int64_t i = 0; i < n;) {
    const int l = lead_len(p[i]);
    if (l == 0 || i + l > n || decode_strict(p + i, l) == kBadCp) return i;
    i += l;
  }
  return -1;
}

__device__ inline bool is_stop(const uint8_t* __restrict__ tok, int64_t len, const StopSlot* __restrict__ tab,
                               uint64_t mask, const uint8_t* __restrict__ blob) {
  const uint64_t h = fnv1a(tok, len);
  for (uint64_t s = h & mask;; s = (s + 1) & mask) {  // load ≤ 0.5: an empty slot ends every probe
    const StopSlot e = tab[s];
    if (e.len < 0) return false;
    if (e.hash == h && e.len == len) {
      bool eq = true;
      for (int64_t q = 0; q < len; ++q) eq = eq && blob[e.off + q] == tok[q];
      if (eq) return true;
    }
  }
}

// kept token t → output token idx (keep_pre[t], or t when every token is kept): its bytes and its offset
template <typename OffT, typename StartT = int64_t>
__global__ __launch_bounds__(kBlock) void k_emit(const uint8_t* __restrict__ text, const StartT* __restrict__ tok_start,
                                                 const int64_t* __restrict__ out_off /* n_tok + 1 */,
                                                 const int32_t* __restrict__ keep_pre /* n_tok + 1, or null */,
                                                 int64_t n_tok, uint8_t* __restrict__ out, OffT* __restrict__ tok_off) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t > n_tok) return;
  if (t == n_tok) {  // the closing offset
    tok_off[keep_pre ? keep_pre[n_tok] : n_tok] = (OffT)out_off[n_tok];
    return;
  }
  const int64_t idx = keep_pre ? keep_pre[t] : t;
  if (keep_pre && keep_pre[t + 1] == idx) return;  // dropped
  const int64_t o = out_off[t], len = out_off[t + 1] - o, s = tok_start[t];
  tok_off[idx] = (OffT)o;
  for (int64_t q = 0; q < len; ++q) out[o + q] = text[s + q];
}

static __global__ __launch_bounds__(kBlock) void k_doc_off(const int64_t* __restrict__ raw_doc,
                                                           const int32_t* __restrict__ keep_pre, int64_t n_docs,
                                                           int64_t* __restrict__ doc_off,
                                                           unsigned long long* __restrict__ max_doc) {
  const int64_t d = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (d > n_docs) return;
  const int64_t a = keep_pre[raw_doc[d]];
  doc_off[d] = a;
  if (d < n_docs) atomicMax(max_doc, (unsigned long long)(keep_pre[raw_doc[d + 1]] - a));
}

// ---- host side ------------------------------------------------------------------------------------------------
inline int grid_for(int64_t n) { return (int)std::max<int64_t>(1, ceil_div(n, kBlock)); }

// out[1 .. n] = inclusive sums of in[0 .. n), out[0] = 0
template <typename T>
static void exclusive_sums(hipStream_t s, const T* in, T* out, int64_t n) {
  HIP_CHECK(hipMemsetAsync(out, 0, sizeof(T), s));
  if (n == 0) return;
  DevBuf tmp;
  with_temp(tmp, [&](void* t, size_t& tb) { return hipcub::DeviceScan::InclusiveSum(t, tb, in, out + 1, n, s); });
  HIP_CHECK(hipStreamSynchronize(s));  // tmp dies at scope exit
}

inline void throw_bad_utf8(const char* what, int64_t at) {
  throw Error(STC_ERR_INVALID_ARG, std::string("malformed UTF-8 in ") + what + " at byte offset " + std::to_string(at));
}

}  // namespace prep
}  // namespace stc
