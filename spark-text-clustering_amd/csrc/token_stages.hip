// token_stages.hip — the stages that sit between a tokenizer and a vectorizer and work on device tokens
// (stc_dtok in, stc_dtok out), on gfx950:
//
//   StopWordsRemover  [U] ml.feature.StopWordsRemover.transform   stc_swr_create / stc_swr_tokens
//   NGram             [U] ml.feature.NGram (sliding(n), " ")      stc_ngram_tokens
//
// (the semantics are stated in include/stc.h, "Token stages", and restated in plain Python by
// tests/token_stage_oracle.py).  One lane per input token in every kernel; a document is never walked by one
// wave, so a book of tens of thousands of tokens costs what as many short documents cost.
//
//   k_swr_keep     per token, its bytes held in two registers when it has ≤ 16 of them: case-sensitive — FNV-1a of
//                  the bytes, the stop-word table (token_compact.h's layout) probed, the bytes compared on a hash +
//                  length match; case-insensitive — the same over the token's Java 8 lower case, streamed byte by
//                  byte (ASCII inline, the rest through java_lower.h) with strict UTF-8 checked on the way, the
//                  stream run again against the pre-lowered stop word on a match.  The lowered token is never
//                  written.  → kept flag, kept length
//   k_ngram_mark   per token i: its document's end by binary search in doc_off; a window starts here iff
//                  i + n ≤ that end; its length tok_off[i+n] − tok_off[i] + n − 1
//   (scans)        kept lengths → output byte offsets, kept flags → output token ids
//   k_emit         (token_compact.h) the kept tokens' bytes and offsets; k_ngram_emit: the n tokens of each window
//                  with one U+0020 between them
//   k_doc_off      (token_compact.h) doc_off = the kept-flag prefix at the input's document offsets, and max_doc
//   k_lower_len / k_lower_write   the stop words' lower case at stc_swr_create, by the same streaming routine the
//                  tokens go through: equality of the two holds by construction
//
// Integer arithmetic only; the only atomics are the first-malformed-byte minimum and the longest-document maximum,
// both order-independent, so results are bitwise reproducible.  java_lower.h's tables (case_table.h) have internal
// linkage: this translation unit carries its own copy beside tokenizer.hip's.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <type_traits>

#include "java_lower.h"
#include "stc_handles.h"
#include "token_compact.h"

struct stc_swr {
  stc::Ctx* ctx = nullptr;  // the context that made it; only it may use it
  int device = -1;          // for stc_swr_free, which may run after that context is gone
  int case_sensitive = 0;
  int64_t n_stop = 0;
  int64_t max_stop_len = 0;  // (lowered, unless case-sensitive) longer tokens skip the table
  uint64_t table_mask = 0;   // slots − 1 (a power of two ≥ 2 · n_stop)
  stc::DevBuf stop_blob;     // uint8[the words' bytes], lower-cased on the device unless case-sensitive
  stc::DevBuf stop_tab;      // prep::StopSlot[table_mask + 1]
};

namespace stc {
namespace stages {

using prep::exclusive_sums;
using prep::grid_for;
using prep::kBlock;
using prep::StopSlot;

// Where a lane reads its token's bytes from: global memory, or — tokens of ≤ 16 bytes, nearly all of them — two
// registers filled by five aligned dword loads issued together, so the byte loop does not wait on memory.  (Worth 5 %
// of the keep pass, measured: the pass is bound by its per-byte arithmetic, not by these loads — DESIGN.md §14.  A
// 32-byte window was slower.)
struct FromMemory {
  const uint8_t* p;
  __device__ __forceinline__ uint32_t operator[](int64_t i) const { return p[i]; }
};
struct Window16 {
  uint64_t lo, hi;  // bytes 0–7, 8–15
  __device__ __forceinline__ uint32_t operator[](int64_t i) const {
    return (uint32_t)((i < 8 ? lo : hi) >> (8 * ((uint32_t)i & 7u))) & 0xFFu;
  }
};
// blob[s .. s + 16): reads the aligned dwords from s & ~3 to s + 20 at most — inside the kHashPad bytes every device
// blob keeps behind its end (hashing_tf.hip reads its 32-byte windows the same way)
__device__ __forceinline__ Window16 load_window(const uint8_t* __restrict__ blob, int64_t s) {
  const uint32_t* w = reinterpret_cast<const uint32_t*>(blob + (s & ~int64_t(3)));
  const uint32_t sh = 8u * (uint32_t)(s & 3);
  const uint32_t d0 = w[0], d1 = w[1], d2 = w[2], d3 = w[3], d4 = w[4];
  const uint32_t x0 = __funnelshift_r(d0, d1, sh), x1 = __funnelshift_r(d1, d2, sh), x2 = __funnelshift_r(d2, d3, sh),
                 x3 = __funnelshift_r(d3, d4, sh);
  return Window16{(uint64_t)x0 | ((uint64_t)x1 << 32), (uint64_t)x2 | ((uint64_t)x3 << 32)};
}

// The Java 8 lower case (root locale) of the token tok[0 .. len) as a string of its own — Final_Sigma's context is
// the token — streamed: f(byte) for every output byte in order.  b[i] = tok[i] (see above; the rule-applied
// characters, which look around them, read tok itself).  Returns the offset of the first byte that is not part of
// well-formed UTF-8 (the stream stops there), −1 when there is none.
template <typename Src, typename F>
__device__ __forceinline__ int64_t lower_stream(const Src& b, const uint8_t* __restrict__ tok, int64_t len, F&& f) {
  for (int64_t i = 0; i < len;) {
    const uint32_t b0 = b[i];
    if (b0 < 0x80u) {
      f((b0 >= 0x41u && b0 <= 0x5Au) ? b0 + 0x20u : b0);  // ASCII: A–Z
      ++i;
      continue;
    }
    const int n = prep::lead_len(b0);
    if (n == 0 || i + n > len) return i;
    const uint8_t c[4] = {(uint8_t)b0, (uint8_t)b[i + 1], (uint8_t)(n > 2 ? b[i + 2] : 0u), (uint8_t)(n > 3 ? b[i + 3] : 0u)};
    const uint32_t cp = prep::decode_strict(c, n);
    if (cp == prep::kBadCp) return i;
    const uint32_t lc = tokenizer::lower_cp(cp);
    if (lc == 0u) {  // applied by rule: İ, Σ, the capitals whose lower case has another UTF-8 length
      uint32_t w = 0;
      const int m = tokenizer::special_lower(tok, 0, len, i, cp, &w);
      for (int q = 0; q < m; ++q) f((w >> (8 * q)) & 0xFFu);
    } else {  // a same-length mapping (or none)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (q < n) f(lc == cp ? (uint32_t)c[q] : tokenizer::utf8_byte(lc, n, q));
    }
    i += n;
  }
  return -1;
}

// Is the token b[0 .. len) kept.  Its bytes (case-sensitive) or the bytes of its lower case are streamed once for
// FNV-1a (prep::fnv1a) and their count, the table is probed, and on a hash + length match the stream runs again
// against the stop word (pre-lowered in that mode).  *bad: the first malformed byte of the token (−1: none; only the
// lower-casing looks).
template <typename Src>
__device__ __forceinline__ bool swr_kept(const Src& b, const uint8_t* __restrict__ tok, int64_t len, int case_sensitive,
                                         const StopSlot* __restrict__ tab, uint64_t mask,
                                         const uint8_t* __restrict__ stop_blob, int64_t n_stop, int64_t max_stop_len,
                                         int64_t* bad) {
  *bad = -1;
  if (case_sensitive && (n_stop == 0 || len > max_stop_len)) return true;
  uint64_t h = 0xCBF29CE484222325ull;
  int64_t ll = 0;
  auto hash = [&](uint32_t c) {
    h = (h ^ c) * 0x100000001B3ull;
    ++ll;
  };
  if (case_sensitive) {
    for (int64_t i = 0; i < len; ++i) hash(b[i]);
  } else {
    *bad = lower_stream(b, tok, len, hash);
    if (*bad >= 0 || n_stop == 0 || ll > max_stop_len) return true;
  }
  for (uint64_t s = h & mask;; s = (s + 1) & mask) {  // load ≤ 0.5: an empty slot ends every probe
    const StopSlot e = tab[s];
    if (e.len < 0) return true;
    if (e.hash == h && e.len == ll) {
      bool eq = true;
      int64_t k = 0;
      auto same = [&](uint32_t c) {
        eq = eq && k < ll && stop_blob[e.off + k] == (uint8_t)c;
        ++k;
      };
      if (case_sensitive) {
        for (int64_t i = 0; i < len; ++i) same(b[i]);
      } else {
        lower_stream(b, tok, len, same);
      }
      if (eq) return false;
    }
  }
}

// token t = blob[tok_off[t] .. tok_off[t+1]): kept unless it is a stop word
template <typename OffT>
__global__ __launch_bounds__(kBlock) void k_swr_keep(const uint8_t* __restrict__ blob, const OffT* __restrict__ tok_off,
                                                     int64_t n_tok, const StopSlot* __restrict__ stop_tab,
                                                     uint64_t stop_mask, const uint8_t* __restrict__ stop_blob,
                                                     int64_t n_stop, int64_t max_stop_len, int case_sensitive,
                                                     int64_t* __restrict__ out_len, int32_t* __restrict__ keep,
                                                     unsigned long long* __restrict__ bad) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= n_tok) return;
  const int64_t s = (int64_t)tok_off[t], len = (int64_t)tok_off[t + 1] - s;
  int64_t r = -1;
  bool kept;
  if (len <= 16)
    kept = swr_kept(load_window(blob, s), blob + s, len, case_sensitive, stop_tab, stop_mask, stop_blob, n_stop, max_stop_len, &r);
  else
    kept = swr_kept(FromMemory{blob + s}, blob + s, len, case_sensitive, stop_tab, stop_mask, stop_blob, n_stop, max_stop_len, &r);
  if (r >= 0) atomicMin(bad, (unsigned long long)(s + r));
  out_len[t] = kept ? len : 0;
  keep[t] = kept ? 1 : 0;
}

// the stop words' lower case (stc_swr_create): lengths, then bytes at the scanned offsets
__global__ __launch_bounds__(kBlock) void k_lower_len(const uint8_t* __restrict__ blob, const int64_t* __restrict__ off,
                                                      int64_t n, int64_t* __restrict__ out_len) {
  const int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (w >= n) return;
  int64_t ll = 0;
  lower_stream(FromMemory{blob + off[w]}, blob + off[w], off[w + 1] - off[w], [&](uint32_t) { ++ll; });
  out_len[w] = ll;
}
__global__ __launch_bounds__(kBlock) void k_lower_write(const uint8_t* __restrict__ blob, const int64_t* __restrict__ off,
                                                        int64_t n, const int64_t* __restrict__ out_off,
                                                        uint8_t* __restrict__ out) {
  const int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (w >= n) return;
  int64_t o = out_off[w];
  const int64_t end = out_off[w + 1];
  lower_stream(FromMemory{blob + off[w]}, blob + off[w], off[w + 1] - off[w], [&](uint32_t c) {
    if (o < end) out[o] = (uint8_t)c;  // (always so: the lengths came from the same stream)
    ++o;
  });
}

// input token i opens a window iff i + n ≤ the end of its document
template <typename OffT>
__global__ __launch_bounds__(kBlock) void k_ngram_mark(const OffT* __restrict__ tok_off, const int64_t* __restrict__ doc_off,
                                                       int64_t n_docs, int64_t n_tok, int64_t n,
                                                       int64_t* __restrict__ out_len, int32_t* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_tok) return;
  int64_t lo = 0, hi = n_docs;  // doc_off[lo] ≤ i < doc_off[hi] (doc_off[0] = 0, doc_off[n_docs] = n_tok)
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (doc_off[mid] <= i) lo = mid;
    else hi = mid;
  }
  const bool start = n <= doc_off[hi] - i;  // (then i + n ≤ n_tok: tok_off[i + n] exists)
  out_len[i] = start ? (int64_t)tok_off[i + n] - (int64_t)tok_off[i] + n - 1 : 0;
  keep[i] = start ? 1 : 0;
}

// window i → output token keep_pre[i]: input tokens i … i+n−1 with one U+0020 between them
template <typename OutT, typename InT>
__global__ __launch_bounds__(kBlock) void k_ngram_emit(const uint8_t* __restrict__ blob, const InT* __restrict__ tok_off,
                                                       const int64_t* __restrict__ out_off /* n_tok + 1 */,
                                                       const int32_t* __restrict__ keep_pre /* n_tok + 1 */,
                                                       int64_t n_tok, int64_t n, uint8_t* __restrict__ out,
                                                       OutT* __restrict__ out_tok_off) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i > n_tok) return;
  if (i == n_tok) {  // the closing offset
    out_tok_off[keep_pre[n_tok]] = (OutT)out_off[n_tok];
    return;
  }
  const int64_t idx = keep_pre[i];
  if (keep_pre[i + 1] == idx) return;  // no window starts here
  int64_t o = out_off[i];
  out_tok_off[idx] = (OutT)o;
  int64_t s = (int64_t)tok_off[i];
  for (int64_t q = 0; q < n; ++q) {
    const int64_t e = (int64_t)tok_off[i + q + 1];
    if (q) out[o++] = 0x20u;
    for (; s < e; ++s) out[o++] = blob[s];
  }
}

__global__ __launch_bounds__(kBlock) void k_longest_doc(const int64_t* __restrict__ doc_off, int64_t n_docs,
                                                        unsigned long long* __restrict__ max_doc) {
  const int64_t d = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (d < n_docs) atomicMax(max_doc, (unsigned long long)(doc_off[d + 1] - doc_off[d]));
}

// ---- host side ------------------------------------------------------------------------------------------------
static void single_device(Ctx& c) {
  if (c.coll()) throw Error(STC_ERR_STATE, "token stages: the context is connected to other ranks (the token stages are single-device)");
}

int64_t longest_doc(Ctx& c, const int64_t* d_doc_off, int64_t n_docs) {
  hipStream_t s = c.stream;
  DevBuf m;
  m.reserve(8);
  HIP_CHECK(hipMemsetAsync(m.p, 0, 8, s));
  if (n_docs > 0) {
    k_longest_doc<<<grid_for(n_docs), kBlock, 0, s>>>(d_doc_off, n_docs, m.as<unsigned long long>());
    KERNEL_CHECK();
  }
  int64_t h = 0;
  HIP_CHECK(hipMemcpyAsync(&h, m.p, 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  return h;
}

static stc_swr* swr_create(Ctx& c, const uint8_t* stop_utf8, int64_t n_bytes, const int64_t* stop_off, int64_t n_stop,
                           int case_sensitive) {
  single_device(c);
  STC_REQUIRE(case_sensitive == 0 || case_sensitive == 1, "case_sensitive must be 0 or 1");
  STC_REQUIRE(n_stop >= 0 && n_bytes >= 0, "sizes must be >= 0");
  STC_REQUIRE(n_stop == 0 || stop_off, "stop_off");
  if (n_stop > 0) {
    check_offsets("stop_off", stop_off, n_stop, n_bytes, "n_bytes", true);
    STC_REQUIRE(n_bytes == 0 || stop_utf8, "stop_utf8");
    for (int64_t w = 0; w < n_stop; ++w) {
      const int64_t r = prep::first_bad_utf8(stop_utf8 + stop_off[w], stop_off[w + 1] - stop_off[w]);
      if (r >= 0) prep::throw_bad_utf8("the stop words", stop_off[w] + r);
    }
  } else {
    n_bytes = 0;
  }
  c.use();
  hipStream_t s = c.stream;
  auto p = new_handle<stc_swr>(c);
  p->case_sensitive = case_sensitive;
  p->n_stop = n_stop;
  // the words the table holds: the caller's bytes, or their lower case made by the routine the tokens go through
  std::vector<uint8_t> words(stop_utf8, stop_utf8 + n_bytes);
  std::vector<int64_t> off(1, 0);
  if (n_stop > 0) off.assign(stop_off, stop_off + n_stop + 1);
  if (!case_sensitive && n_stop > 0) {
    DevBuf raw, raw_off, len, low_off, low;
    raw.reserve((size_t)std::max<int64_t>(n_bytes, 1));
    raw_off.reserve(8 * (n_stop + 1));
    len.reserve(8 * n_stop);
    low_off.reserve(8 * (n_stop + 1));
    if (n_bytes) HIP_CHECK(hipMemcpyAsync(raw.p, stop_utf8, n_bytes, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(raw_off.p, stop_off, 8 * (n_stop + 1), hipMemcpyHostToDevice, s));
    k_lower_len<<<grid_for(n_stop), kBlock, 0, s>>>(raw.as<uint8_t>(), raw_off.as<int64_t>(), n_stop, len.as<int64_t>());
    KERNEL_CHECK();
    exclusive_sums(s, len.as<int64_t>(), low_off.as<int64_t>(), n_stop);
    HIP_CHECK(hipMemcpyAsync(off.data(), low_off.p, 8 * (n_stop + 1), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    words.assign((size_t)off[n_stop], 0);
    low.reserve((size_t)std::max<int64_t>(off[n_stop], 1));
    k_lower_write<<<grid_for(n_stop), kBlock, 0, s>>>(raw.as<uint8_t>(), raw_off.as<int64_t>(), n_stop,
                                                      low_off.as<int64_t>(), low.as<uint8_t>());
    KERNEL_CHECK();
    if (!words.empty()) HIP_CHECK(hipMemcpyAsync(words.data(), low.p, words.size(), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));  // the scratch buffers die at scope exit
  }
  int64_t max_len = 0;
  uint64_t slots = 2;
  while (slots < 2 * (uint64_t)n_stop) slots <<= 1;
  std::vector<StopSlot> tab(slots, StopSlot{0, 0, -1});
  for (int64_t w = 0; w < n_stop; ++w) {  // the empty word is a word like any other: Tokenizer yields empty tokens
    const int64_t o = off[w], len = off[w + 1] - o;
    const uint64_t h = prep::fnv1a(words.data() + o, len);
    uint64_t q = h & (slots - 1);
    bool dup = false;
    for (; tab[q].len >= 0; q = (q + 1) & (slots - 1))
      if (tab[q].hash == h && tab[q].len == len && !memcmp(words.data() + tab[q].off, words.data() + o, (size_t)len)) {
        dup = true;
        break;
      }
    if (!dup) tab[q] = StopSlot{h, o, len};
    max_len = std::max(max_len, len);
  }
  p->max_stop_len = max_len;
  p->table_mask = slots - 1;
  p->stop_blob.reserve(std::max<size_t>(words.size(), 1));
  p->stop_tab.reserve(sizeof(StopSlot) * slots);
  if (!words.empty()) HIP_CHECK(hipMemcpyAsync(p->stop_blob.p, words.data(), words.size(), hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(p->stop_tab.p, tab.data(), sizeof(StopSlot) * slots, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipStreamSynchronize(s));  // the host tables die at scope exit
  return p.release();
}

// One allocation for everything a call keeps per input token, and its two result words
struct Scratch {
  DevBuf buf;
  int64_t *out_len, *out_off;  // n: kept lengths; n + 1: their exclusive sums
  int32_t *keep, *keep_pre;    // n: kept flags; n + 1: their exclusive sums
  unsigned long long* small;   // [0] the first malformed byte (all ones: none), [1] the longest document
  Scratch(hipStream_t s, int64_t n) {
    const int64_t w = n + 2;  // 8-byte words per array (the int32 arrays take half of theirs)
    buf.reserve((size_t)(8 * (4 * w + 2)));
    out_len = buf.as<int64_t>();
    out_off = out_len + w;
    keep = reinterpret_cast<int32_t*>(out_off + w);
    keep_pre = reinterpret_cast<int32_t*>(out_off + 2 * w);
    small = reinterpret_cast<unsigned long long*>(out_off + 3 * w);
    HIP_CHECK(hipMemsetAsync(small, 0xFF, 8, s));
    HIP_CHECK(hipMemsetAsync(small + 1, 0, 8, s));
  }
};

// The kept tokens of `in` (sc.out_len / sc.keep, one entry per input token) as device tokens with the invariants
// of stc_tokens_upload: kHashPad zero bytes behind the blob, u32 offsets when they fit, max_doc.
// emit(out32, result) writes the blob and tok_off.  Two waits for the device: the sizes, and the end.
template <typename Emit>
static stc_dtok* compact(Ctx& c, const stc_dtok& in, Scratch& sc, Emit&& emit) {
  hipStream_t s = c.stream;
  const int64_t n_tok = in.n_tok, n_docs = in.n_docs;
  auto t = new_handle<stc_dtok>(c);
  t->n_docs = n_docs;
  t->doc_off.reserve(8 * (n_docs + 1));
  DevBuf tmp;  // hipCUB's, for both scans (they run one after the other on the stream)
  HIP_CHECK(hipMemsetAsync(sc.out_off, 0, 8, s));
  HIP_CHECK(hipMemsetAsync(sc.keep_pre, 0, 4, s));
  if (n_tok > 0) {
    size_t b64 = 0, b32 = 0;
    HIP_CHECK(hipcub::DeviceScan::InclusiveSum(nullptr, b64, sc.out_len, sc.out_off + 1, n_tok, s));
    HIP_CHECK(hipcub::DeviceScan::InclusiveSum(nullptr, b32, sc.keep, sc.keep_pre + 1, n_tok, s));
    tmp.reserve(std::max(b64, b32));
    HIP_CHECK(hipcub::DeviceScan::InclusiveSum(tmp.p, b64, sc.out_len, sc.out_off + 1, n_tok, s));
    HIP_CHECK(hipcub::DeviceScan::InclusiveSum(tmp.p, b32, sc.keep, sc.keep_pre + 1, n_tok, s));
  }
  int64_t n_out = 0, bad = -1;
  int32_t n_keep = 0;
  HIP_CHECK(hipMemcpyAsync(&n_out, sc.out_off + n_tok, 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(&n_keep, sc.keep_pre + n_tok, 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(&bad, sc.small, 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  if (bad != -1) prep::throw_bad_utf8("the tokens", bad);
  t->off32 = n_out + kHashPad <= (int64_t(1) << 32);
  t->utf8.reserve(n_out + kHashPad);
  t->tok_off.reserve((t->off32 ? 4 : 8) * ((int64_t)n_keep + 1));
  HIP_CHECK(hipMemsetAsync(t->utf8.as<uint8_t>() + n_out, 0, kHashPad, s));
  emit(t->off32, *t);
  KERNEL_CHECK();
  prep::k_doc_off<<<grid_for(n_docs + 1), kBlock, 0, s>>>(in.doc_off.as<int64_t>(), sc.keep_pre, n_docs,
                                                          t->doc_off.as<int64_t>(), sc.small + 1);
  KERNEL_CHECK();
  HIP_CHECK(hipMemcpyAsync(&t->max_doc, sc.small + 1, 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));  // the scratch buffers die at scope exit
  t->n_bytes = n_out;
  t->n_tok = n_keep;
  return t.release();
}

static void check_input(Ctx& c, const stc_dtok& in) {
  single_device(c);
  STC_REQUIRE(in.n_tok <= (int64_t(1) << 31) - 1, "at most 2^31-1 tokens per call");
  c.use();
}

// f(dst, src) with the result's and the input's token offsets, each as u32 or int64
template <typename F>
static void with_offsets(bool out32, stc_dtok& t, const stc_dtok& in, F&& f) {
  if (out32 && in.off32) f(t.tok_off.as<uint32_t>(), (const uint32_t*)in.tok_off.p);
  else if (out32) f(t.tok_off.as<uint32_t>(), (const int64_t*)in.tok_off.p);
  else if (in.off32) f(t.tok_off.as<int64_t>(), (const uint32_t*)in.tok_off.p);
  else f(t.tok_off.as<int64_t>(), (const int64_t*)in.tok_off.p);
}

static stc_dtok* swr_tokens(Ctx& c, const stc_swr& p, const stc_dtok& in) {
  check_input(c, in);
  hipStream_t s = c.stream;
  const int64_t n_tok = in.n_tok;
  Scratch sc(s, n_tok);
  if (n_tok > 0) {
    auto run = [&](auto* off) {
      k_swr_keep<<<grid_for(n_tok), kBlock, 0, s>>>(in.utf8.as<uint8_t>(), off, n_tok, p.stop_tab.as<StopSlot>(), p.table_mask,
                                                    p.stop_blob.as<uint8_t>(), p.n_stop, p.max_stop_len, p.case_sensitive,
                                                    sc.out_len, sc.keep, sc.small);
    };
    if (in.off32) run(in.tok_off.as<uint32_t>());
    else run(in.tok_off.as<int64_t>());
    KERNEL_CHECK();
  }
  return compact(c, in, sc, [&](bool out32, stc_dtok& t) {
    with_offsets(out32, t, in, [&](auto* dst, auto* src) {
      using OutT = std::remove_pointer_t<decltype(dst)>;
      using InT = std::remove_const_t<std::remove_pointer_t<decltype(src)>>;
      prep::k_emit<OutT, InT><<<grid_for(n_tok + 1), kBlock, 0, s>>>(in.utf8.as<uint8_t>(), src, sc.out_off, sc.keep_pre, n_tok,
                                                                     t.utf8.as<uint8_t>(), dst);
    });
  });
}

static stc_dtok* ngram_tokens(Ctx& c, const stc_dtok& in, int32_t n) {
  STC_REQUIRE(n >= 1, "n must be >= 1");
  check_input(c, in);
  hipStream_t s = c.stream;
  const int64_t n_tok = in.n_tok;
  Scratch sc(s, n_tok);
  if (n_tok > 0) {
    auto run = [&](auto* off) {
      k_ngram_mark<<<grid_for(n_tok), kBlock, 0, s>>>(off, in.doc_off.as<int64_t>(), in.n_docs, n_tok, (int64_t)n, sc.out_len,
                                                      sc.keep);
    };
    if (in.off32) run(in.tok_off.as<uint32_t>());
    else run(in.tok_off.as<int64_t>());
    KERNEL_CHECK();
  }
  return compact(c, in, sc, [&](bool out32, stc_dtok& t) {
    with_offsets(out32, t, in, [&](auto* dst, auto* src) {
      k_ngram_emit<<<grid_for(n_tok + 1), kBlock, 0, s>>>(in.utf8.as<uint8_t>(), src, sc.out_off, sc.keep_pre, n_tok, (int64_t)n,
                                                          t.utf8.as<uint8_t>(), dst);
    });
  });
}

}  // namespace stages
}  // namespace stc

using namespace stc;

extern "C" {

int stc_swr_create(stc_ctx* ctx, const uint8_t* stop_utf8, int64_t n_bytes, const int64_t* stop_off, int64_t n_stop,
                   int case_sensitive, stc_swr** out) {
  return guard([&] {
    STC_REQUIRE(ctx && out, "ctx/out");
    *out = stages::swr_create(*ctx, stop_utf8, n_bytes, stop_off, n_stop, case_sensitive);
  });
}

int stc_swr_free(stc_swr* p) {
  return guard([&] {
    if (!p) return;
    if (p->device >= 0) (void)hipSetDevice(p->device);
    delete p;
  });
}

int stc_swr_tokens(stc_ctx* ctx, const stc_swr* p, const stc_dtok* in, stc_dtok** out) {
  return guard([&] {
    STC_REQUIRE(ctx && p && in && out, "ctx/swr/tokens/out");
    STC_REQUIRE(p->ctx == ctx, "the stop-word remover belongs to another stc_ctx");
    STC_REQUIRE(in->ctx == ctx, "tokens were uploaded on another stc_ctx");
    *out = stages::swr_tokens(*ctx, *p, *in);
  });
}

int stc_ngram_tokens(stc_ctx* ctx, const stc_dtok* in, int32_t n, stc_dtok** out) {
  return guard([&] {
    STC_REQUIRE(ctx && in && out, "ctx/tokens/out");
    STC_REQUIRE(in->ctx == ctx, "tokens were uploaded on another stc_ctx");
    *out = stages::ngram_tokens(*ctx, *in, n);
  });
}

}  // extern "C"
