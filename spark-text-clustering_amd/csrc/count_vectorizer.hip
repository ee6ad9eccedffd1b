// count_vectorizer.hip — CountVectorizer.fit / CountVectorizerModel.transform for gfx950.
//
// Replaces [U] ml.feature.CountVectorizer (Spark 2.4.3, build.sbt:10), the vocabulary-indexed counting of
// LDAClustering.scala:143-171 (fit: wordCounts.top(vocabSize)) and LDALoader.scala:83-105 (transform: the
// dictionary lookup + per-document counts).  Exact: two tokens are one term iff their bytes are equal.
//
// fit       hash every token (64 bits, aligned dword reads) → stable radix sort of (hash, token index) →
//           run heads (a token starts a run when its hash or its BYTES differ from its predecessor's; a hash
//           run that mixes strings is re-sorted by (hash, bytes, token index), so a collision never merges
//           or splits a term) → count = run length, df = document changes inside the run (one packed scan)
//           → df filter → merge sort of the distinct terms by (count descending, bytes ascending) → cut →
//           gather the kept strings.  The host reads back sizes only.
// model     open-addressing table probed from the term's hash, load ≤ 0.5, built by atomicCAS on the index word;
//           a slot holds the index, the length and the first 16 bytes of its term, so the byte compare of a
//           short term needs no second read; an insert that meets its own string reports a duplicate (the
//           smallest index, whatever the order).
// transform per-token lookup (hash, probe, byte compare) → the indices of every document sorted (one wave per
//           document, wave_sort.h's bitonic network in registers; past 1024 tokens hipcub's segmented radix sort,
//           the hashing::sort_long_docs that HashingTF uses) → run
//           heads and lengths by flat scans → minTF filter → CSR.  No atomics on the CSR, no per-document
//           counters: a run of 2^31−1 equal tokens is one subtraction.
// Integer atomics only, and only where the order cannot show (a kept-term count, the CAS inserts, a min).
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdlib>
#include <memory>

#include "collectives.h"
#include "stc_handles.h"
#include "wave_sort.h"

// CountVectorizerModel: term j is blob[term_off[j] .. term_off[j+1]), index = position
struct stc_cvm {
  stc::Ctx* ctx = nullptr;  // the context that made it; only it may read the buffers (checked at the ABI)
  int device = -1;          // for stc_cv_free, which may run after that context is gone
  int64_t n_terms = 0, n_bytes = 0;
  int hash_bits = 64;       // STC_CV_HASH_BITS at construction: the hash is masked to its low bits everywhere
  bool has_counts = false;  // fitted (count / df hold the corpus statistics) or made from a list (zeros)
  uint64_t table_mask = 0;  // table slots − 1 (a power of two ≥ 2 · n_terms: load ≤ 0.5)
  stc::DevBuf blob;         // uint8[n_bytes + kHashPad]
  stc::DevBuf term_off;     // int64[n_terms + 1]
  stc::DevBuf count, df;    // int64[n_terms]
  stc::DevBuf table;        // Slot[table_mask + 1]: term index (−1 = empty), length, first 16 bytes, blob offset
};

namespace stc {
namespace cv {
namespace {

// tokens on the device: token t is utf8[off[t] .. off[t+1]) with off = off32 when given, else off64; the
// blob carries kHashPad bytes of padding; document d owns tokens [doc_off[d], doc_off[d+1])
struct TokView {
  const uint8_t* utf8 = nullptr;
  const int64_t* off64 = nullptr;
  const uint32_t* off32 = nullptr;
  int64_t n_tok = 0;
  const int64_t* doc_off = nullptr;  // nullptr for index_of
  int64_t n_docs = 0;
  int64_t max_doc = -1;  // the longest document's token count when the upload knows it, −1 otherwise
};

// ---------------------------------------------------------------------------------------
// strings: read as whole aligned dwords and realigned with v_alignbyte (as hashing_tf.hip's k_hash);
// the blobs carry kHashPad bytes of padding, so dword j + 1 of a string never leaves the allocation
// ---------------------------------------------------------------------------------------
struct Str {
  const uint32_t* w;  // the aligned dword holding the first byte
  uint32_t sh;        // the first byte's position in it
  uint32_t n;         // bytes
};
__device__ __forceinline__ Str str_at(const uint8_t* p, uint32_t n) {
  const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3);
  return Str{reinterpret_cast<const uint32_t*>(p - sh), sh, n};
}
template <typename O>
__device__ __forceinline__ Str tok_at(const uint8_t* utf8, const O* off, int64_t t) {
  const O b = off[t], e = off[t + 1];
  return str_at(utf8 + b, (uint32_t)(e - b));
}
// bytes 4j .. 4j+3 (little-endian); bytes at or past the end read as 0
__device__ __forceinline__ uint32_t str_dw(const Str& s, uint32_t j) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (4 * j >= s.n) return 0;
  const uint32_t lo = s.w[j], hi = s.sh ? s.w[j + 1] : 0u;
  const uint32_t v = __builtin_amdgcn_alignbyte(hi, lo, s.sh);
  const uint32_t rem = s.n - 4 * j;
  return rem >= 4 ? v : v & (0xFFFFFFFFu >> (8 * (4 - rem)));
#else
  (void)s;
  (void)j;
  return 0;
#endif
}
__device__ __forceinline__ bool str_eq(const Str& a, const Str& b) {
  if (a.n != b.n) return false;
  for (uint32_t j = 0; 4 * j < a.n; ++j)
    if (str_dw(a, j) != str_dw(b, j)) return false;
  return true;
}
// unsigned bytewise order from dword j0 on, a proper prefix first: the zero padding of the shorter string
// compares below every byte but NUL, and equal padded dwords leave the decision to the length
__device__ __forceinline__ int str_cmp(const Str& a, const Str& b, uint32_t j0) {
  const uint32_t m = a.n < b.n ? a.n : b.n;
  for (uint32_t j = j0; 4 * j < m; ++j) {
    const uint32_t x = __builtin_bswap32(str_dw(a, j)), y = __builtin_bswap32(str_dw(b, j));
    if (x != y) return x < y ? -1 : 1;
  }
  return a.n < b.n ? -1 : (a.n > b.n ? 1 : 0);
}
// 64-bit hash: splitmix64 over the 8-byte words, the length in the seed
__device__ __forceinline__ uint64_t str_hash(const Str& s, uint64_t mask) {
  uint64_t h = 0x9E3779B97F4A7C15ull ^ ((uint64_t)s.n * 0xFF51AFD7ED558CCDull);
  for (uint32_t j = 0; 4 * j < s.n; j += 2)
    h = splitmix64(h ^ ((uint64_t)str_dw(s, j) | ((uint64_t)str_dw(s, j + 1) << 32)));
  return h & mask;
}
// the first 8 bytes big-endian, zero padded: the leading sort key of the byte order
__device__ __forceinline__ uint64_t str_prefix(const Str& s) {
  return ((uint64_t)__builtin_bswap32(str_dw(s, 0)) << 32) | __builtin_bswap32(str_dw(s, 1));
}

// the document of token t: the last d with doc_off[d] <= t (empty documents own no token)
__device__ __forceinline__ int64_t doc_of(const int64_t* __restrict__ doc_off, int64_t n_docs, int64_t t) {
  int64_t lo = 0, hi = n_docs;  // doc_off[lo] <= t < doc_off[hi]
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (doc_off[mid] <= t) lo = mid;
    else hi = mid;
  }
  return lo;
}

int grid_for(int64_t n) { return (int)std::min<int64_t>(std::max<int64_t>(ceil_div(n, 256), 1), 8192); }
#define CV_LOOP(i, n) \
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (n); i += (int64_t)gridDim.x * 256)

// sub-buffers of one grow-only scratch allocation: add() every size, commit(), then at()
struct Arena {
  size_t total = 0;
  char* base = nullptr;
  size_t add(size_t bytes) {
    const size_t o = total;
    total += (bytes + 255) & ~size_t(255);
    return o;
  }
  void commit(DevBuf& b) {
    b.reserve(std::max<size_t>(total, 256));
    base = b.as<char>();
  }
  template <typename T>
  T* at(size_t o) const { return reinterpret_cast<T*>(base + o); }
};

uint64_t mask_of(int bits) { return bits >= 64 ? ~0ull : ((1ull << bits) - 1); }

int hash_bits_env() {
  const char* e = std::getenv("STC_CV_HASH_BITS");
  if (!e || !*e) return 64;
  const int n = std::atoi(e);
  STC_REQUIRE(n >= 1 && n <= 64, "STC_CV_HASH_BITS must be 1..64");
  return n;
}

void single_device(Ctx& c) {
  if (c.coll()) throw Error(STC_ERR_STATE, "cv: the context is connected to other ranks (CountVectorizer is single-device)");
}

template <typename F>
void with_off(const TokView& tk, F&& f) {
  if (tk.off32) f(tk.off32);
  else f(tk.off64);
}

// ---------------------------------------------------------------------------------------
// fit
// ---------------------------------------------------------------------------------------
template <typename O>
__global__ __launch_bounds__(256) void k_cv_hash(const uint8_t* __restrict__ utf8, const O* __restrict__ off,
                                                 int64_t n_tok, uint64_t mask, uint64_t* __restrict__ hk,
                                                 uint32_t* __restrict__ ti) {
  CV_LOOP(t, n_tok) {
    hk[t] = str_hash(tok_at(utf8, off, t), mask);
    ti[t] = (uint32_t)t;
  }
}

struct HashTok {  // the collision fallback's sort key
  uint64_t h;
  uint32_t t, pad;
};
__global__ __launch_bounds__(256) void k_cv_pack(const uint64_t* __restrict__ hk, const uint32_t* __restrict__ ti,
                                                 int64_t n, HashTok* __restrict__ out) {
  CV_LOOP(i, n) out[i] = HashTok{hk[i], ti[i], 0u};
}
__global__ __launch_bounds__(256) void k_cv_unpack(const HashTok* __restrict__ in, int64_t n, uint64_t* __restrict__ hk,
                                                   uint32_t* __restrict__ ti) {
  CV_LOOP(i, n) {
    hk[i] = in[i].h;
    ti[i] = in[i].t;
  }
}
template <typename O>
struct HashTokLess {  // (hash, bytes, token index): a total order, equal strings adjacent and in token order
  const uint8_t* utf8;
  const O* off;
  __host__ __device__ bool operator()(const HashTok& a, const HashTok& b) const {
    if (a.h != b.h) return a.h < b.h;
    const int c = str_cmp(tok_at(utf8, off, a.t), tok_at(utf8, off, b.t), 0);
    return c != 0 ? c < 0 : a.t < b.t;
  }
};

// sorted position i → (run head) << 32 | (head, or another document than the predecessor's); *collide is
// set when two neighbours share a hash and differ in their bytes
template <typename O>
__global__ __launch_bounds__(256) void k_cv_heads(const uint8_t* __restrict__ utf8, const O* __restrict__ off,
                                                  const int64_t* __restrict__ doc_off, int64_t n_docs,
                                                  const uint64_t* __restrict__ hk, const uint32_t* __restrict__ ti,
                                                  int64_t n, int64_t* __restrict__ fl, int32_t* __restrict__ collide) {
  CV_LOOP(i, n) {
    int64_t head = 1, docf = 1;
    if (i > 0) {
      const int64_t t = ti[i], tp = ti[i - 1];
      const bool same_hash = hk[i] == hk[i - 1];
      const bool same = same_hash && str_eq(tok_at(utf8, off, t), tok_at(utf8, off, tp));
      if (same_hash && !same) *collide = 1;
      head = same ? 0 : 1;
      // inside a run the token indices ascend, so the documents do: another one iff t is past tp's
      docf = same ? (doc_off[doc_of(doc_off, n_docs, tp) + 1] <= t ? 1 : 0) : 1;
    }
    fl[i] = (head << 32) | docf;
  }
}

// from the inclusive scan of the flags: term u's first sorted position and the document flags before it
__global__ __launch_bounds__(256) void k_cv_starts(const int64_t* __restrict__ sc, int64_t n, int32_t* __restrict__ start,
                                                   int32_t* __restrict__ dstart) {
  CV_LOOP(i, n) {
    const int64_t v = sc[i], hu = v >> 32;
    if (i == 0 || (sc[i - 1] >> 32) != hu) {
      start[hu - 1] = (int32_t)i;
      dstart[hu - 1] = (int32_t)(v & 0xFFFFFFFF) - 1;
    }
    if (i == n - 1) {
      start[hu] = (int32_t)n;
      dstart[hu] = (int32_t)(v & 0xFFFFFFFF);
    }
  }
}

struct TermKey {
  uint32_t neg;     // 2^31−1 − count (ascending = count descending); 0xFFFFFFFF: dropped by the df filter
  uint32_t rep;     // a token holding the term's bytes
  uint64_t prefix;  // its first 8 bytes, big-endian, zero padded
};
template <typename O>
struct TermLess {
  const uint8_t* utf8;
  const O* off;
  __host__ __device__ bool operator()(const TermKey& a, const TermKey& b) const {
    if (a.neg != b.neg) return a.neg < b.neg;
    if (a.neg == 0xFFFFFFFFu) return false;  // dropped terms: any order
    if (a.prefix != b.prefix) return a.prefix < b.prefix;
    return str_cmp(tok_at(utf8, off, a.rep), tok_at(utf8, off, b.rep), 2) < 0;
  }
};

template <typename O>
__global__ __launch_bounds__(256) void k_cv_keys(const uint8_t* __restrict__ utf8, const O* __restrict__ off,
                                                 const uint32_t* __restrict__ ti, const int32_t* __restrict__ start,
                                                 const int32_t* __restrict__ dstart, int64_t n_terms, double min_df,
                                                 double max_df, TermKey* __restrict__ keys, uint32_t* __restrict__ ids,
                                                 int32_t* __restrict__ n_kept) {
  CV_LOOP(u, n_terms) {
    const int32_t cnt = start[u + 1] - start[u], df = dstart[u + 1] - dstart[u];
    const bool keep = (double)df >= min_df && (double)df <= max_df;
    const uint32_t rep = ti[start[u]];
    keys[u] = TermKey{keep ? 0x7FFFFFFFu - (uint32_t)cnt : 0xFFFFFFFFu, rep, str_prefix(tok_at(utf8, off, rep))};
    ids[u] = (uint32_t)u;
    if (keep) atomicAdd(n_kept, 1);  // a count: the order of the adds cannot show
  }
}

// the kept terms in vocabulary order: their lengths (for the offsets scan), counts and df
template <typename O>
__global__ __launch_bounds__(256) void k_cv_lens(const O* __restrict__ off, const TermKey* __restrict__ keys,
                                                 const uint32_t* __restrict__ ids, const int32_t* __restrict__ start,
                                                 const int32_t* __restrict__ dstart, int64_t n_keep,
                                                 int64_t* __restrict__ len, int64_t* __restrict__ count,
                                                 int64_t* __restrict__ df) {
  CV_LOOP(j, n_keep) {
    const uint32_t u = ids[j], rep = keys[j].rep;
    len[j] = (int64_t)(off[rep + 1] - off[rep]);
    count[j] = start[u + 1] - start[u];
    df[j] = dstart[u + 1] - dstart[u];
  }
}
template <typename O>
__global__ __launch_bounds__(256) void k_cv_gather(const uint8_t* __restrict__ utf8, const O* __restrict__ off,
                                                   const TermKey* __restrict__ keys, int64_t n_keep,
                                                   const int64_t* __restrict__ term_off, uint8_t* __restrict__ blob) {
  CV_LOOP(j, n_keep) {
    const uint8_t* src = utf8 + off[keys[j].rep];
    uint8_t* dst = blob + term_off[j];
    const int64_t n = term_off[j + 1] - term_off[j];
    for (int64_t b = 0; b < n; ++b) dst[b] = src[b];
  }
}

// ---------------------------------------------------------------------------------------
// model: the table
// ---------------------------------------------------------------------------------------
// A slot carries the term's index, its length and its first 16 bytes, so a lookup of a term of ≤ 16 bytes —
// nearly every word — is ONE random 32-byte read: length and bytes are compared in the slot itself, and only
// a longer term's remaining bytes are read from the vocabulary blob.  The hash picks the first slot probed.
struct alignas(32) Slot {
  int32_t idx;      // −1: empty
  uint32_t len;     // the term's bytes
  uint64_t p0, p1;  // its bytes 0..7 and 8..15 (little-endian dwords, zero padded)
  uint64_t off;     // where it starts in the blob
};
__device__ __forceinline__ uint64_t str_qw(const Str& s, uint32_t q) {  // bytes 8q .. 8q+7
  return (uint64_t)str_dw(s, 2 * q) | ((uint64_t)str_dw(s, 2 * q + 1) << 32);
}

__global__ __launch_bounds__(256) void k_cv_insert(const uint8_t* __restrict__ blob, const int64_t* __restrict__ term_off,
                                                   int64_t n_terms, uint64_t mask, uint64_t tmask, Slot* slots,
                                                   int32_t* __restrict__ dup) {
  CV_LOOP(j, n_terms) {
    const Str s = tok_at(blob, term_off, j);
    const uint64_t h = str_hash(s, mask);
    for (uint64_t pos = h & tmask;; pos = (pos + 1) & tmask) {  // load ≤ 0.5: an empty slot exists
      const int32_t old = atomicCAS(&slots[pos].idx, -1, (int32_t)j);
      if (old == -1) break;
      if (str_eq(s, tok_at(blob, term_off, old))) {  // the same string twice: one of the two stays out
        atomicMin(dup, (int32_t)j < old ? (int32_t)j : old);
        break;
      }
    }
  }
}
// once every index is placed: each occupied slot's copy of its term's length, first bytes and offset
__global__ __launch_bounds__(256) void k_cv_fill(Slot* __restrict__ slots, int64_t n_slots, const uint8_t* __restrict__ blob,
                                                 const int64_t* __restrict__ term_off) {
  CV_LOOP(p, n_slots) {
    const int32_t j = slots[p].idx;
    if (j >= 0) {
      const Str s = tok_at(blob, term_off, j);
      slots[p].len = s.n;
      slots[p].p0 = str_qw(s, 0);
      slots[p].p1 = str_qw(s, 1);
      slots[p].off = (uint64_t)term_off[j];
    }
  }
}

// token → term index, or `oov`
template <typename O>
__global__ __launch_bounds__(256) void k_cv_lookup(const uint8_t* __restrict__ utf8, const O* __restrict__ off,
                                                   int64_t n_tok, const uint8_t* __restrict__ blob,
                                                   const Slot* __restrict__ slots, uint64_t mask, uint64_t tmask,
                                                   int32_t oov, int32_t* __restrict__ out) {
  CV_LOOP(t, n_tok) {
    const Str s = tok_at(utf8, off, t);
    const uint64_t h = str_hash(s, mask), p0 = str_qw(s, 0), p1 = str_qw(s, 1);
    int32_t r = oov;
    for (uint64_t pos = h & tmask;; pos = (pos + 1) & tmask) {
      const Slot sl = slots[pos];
      if (sl.idx < 0) break;
      if (sl.len == s.n && sl.p0 == p0 && sl.p1 == p1) {  // the bytes themselves, not a hash of them
        bool same = true;
        if (s.n > 16) {
          const Str v = str_at(blob + sl.off, sl.len);
          for (uint32_t j = 4; same && 4 * j < s.n; ++j) same = str_dw(s, j) == str_dw(v, j);
        }
        if (same) {
          r = sl.idx;
          break;
        }
      }
    }
    out[t] = r;
  }
}

// builds m.table from m.blob / m.term_off; returns the smallest index of a term that occurs twice, or −1
int32_t build_table(Ctx& c, stc_cvm& m) {
  hipStream_t st = c.stream;
  uint64_t slots = 16;
  while (slots < 2 * (uint64_t)m.n_terms) slots <<= 1;
  m.table_mask = slots - 1;
  m.table.reserve(sizeof(Slot) * slots);
  HIP_CHECK(hipMemsetAsync(m.table.p, 0xFF, sizeof(Slot) * slots, st));
  Arena a;
  const size_t o_dup = a.add(4);
  a.commit(c.scratch[0]);
  int32_t dup = INT32_MAX;
  HIP_CHECK(hipMemcpyAsync(a.at<int32_t>(o_dup), &dup, 4, hipMemcpyHostToDevice, st));
  k_cv_insert<<<grid_for(m.n_terms), 256, 0, st>>>(m.blob.as<uint8_t>(), m.term_off.as<int64_t>(), m.n_terms,
                                                    mask_of(m.hash_bits), m.table_mask, m.table.as<Slot>(),
                                                    a.at<int32_t>(o_dup));
  KERNEL_CHECK();
  k_cv_fill<<<grid_for((int64_t)slots), 256, 0, st>>>(m.table.as<Slot>(), (int64_t)slots, m.blob.as<uint8_t>(),
                                                      m.term_off.as<int64_t>());
  KERNEL_CHECK();
  HIP_CHECK(hipMemcpyAsync(&dup, a.at<int32_t>(o_dup), 4, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  return dup == INT32_MAX ? -1 : dup;
}

std::unique_ptr<stc_cvm> new_model(Ctx& c) {
  auto m = new_handle<stc_cvm>(c);
  m->hash_bits = hash_bits_env();
  return m;
}

void lookup(Ctx& c, const stc_cvm& m, const TokView& tk, int32_t oov, int32_t* d_out) {
  if (tk.n_tok == 0) return;
  with_off(tk, [&](const auto* off) {
    k_cv_lookup<<<grid_for(tk.n_tok), 256, 0, c.stream>>>(tk.utf8, off, tk.n_tok, m.blob.as<uint8_t>(),
                                                           m.table.as<Slot>(), mask_of(m.hash_bits), m.table_mask,
                                                           oov, d_out);
  });
  KERNEL_CHECK();
}

// ---------------------------------------------------------------------------------------
// transform: the sorted indices of every document → runs → CSR
// ---------------------------------------------------------------------------------------
// the indices of one document sorted in registers by wave_sort.h's bitonic network (the one HashingTF uses);
// documents past kSortCap tokens go to hipcub's segmented radix sort (hashing::sort_long_docs)
template <int P>
__device__ __forceinline__ void sort_doc(const int32_t* __restrict__ keys, int32_t* __restrict__ sorted, int64_t s,
                                         int n, int lane) {
  int32_t x[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int e = lane * P + p;
    x[p] = e < n ? keys[s + e] : INT32_MAX;  // pads sort last (indices ≤ n_terms < 2^31 − 1)
  }
  bitonic_regs<P>(x, lane);
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int e = lane * P + p;
    if (e < n) sorted[s + e] = x[p];
  }
}
// one wave per document; longer documents are appended to `large` (the order of the list only permutes the
// segments of the radix sort that follows)
__global__ __launch_bounds__(64 * kDocWaves) void k_tf_sort_docs(const int32_t* __restrict__ keys,
                                                                const int64_t* __restrict__ doc_off, int64_t n_docs,
                                                                int32_t* __restrict__ sorted,
                                                                int32_t* __restrict__ large,
                                                                int32_t* __restrict__ n_large) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int64_t d = (int64_t)blockIdx.x * kDocWaves + wv; d < n_docs; d += (int64_t)gridDim.x * kDocWaves) {
    const int64_t s = doc_off[d], n64 = doc_off[d + 1] - s;
    if (n64 > kSortCap) {
      if (lane == 0) large[atomicAdd(n_large, 1)] = (int32_t)d;
      continue;
    }
    const int n = (int)n64;
    if (n == 0) continue;
    with_keys_per_lane<1, kSortCap / 64>(n, [&](auto pc) { sort_doc<decltype(pc)::value>(keys, sorted, s, n, lane); });
  }
}

__global__ __launch_bounds__(256) void k_tf_doc_starts(const int64_t* __restrict__ doc_off, int64_t n_docs,
                                                       int32_t* __restrict__ fl) {
  CV_LOOP(d, n_docs)
    if (doc_off[d + 1] > doc_off[d]) fl[doc_off[d]] = 1;
}
__global__ __launch_bounds__(256) void k_tf_heads(const int32_t* __restrict__ keys, int64_t n, int32_t* __restrict__ fl) {
  CV_LOOP(i, n)
    if (i > 0 && keys[i] != keys[i - 1]) fl[i] = 1;
}
// rid = the inclusive scan of the head flags: run r starts where rid becomes r + 1
__global__ __launch_bounds__(256) void k_tf_starts(const int32_t* __restrict__ rid, int64_t n, int32_t* __restrict__ rstart) {
  CV_LOOP(i, n) {
    const int32_t r = rid[i];
    if (i == 0 || rid[i - 1] != r) rstart[r - 1] = (int32_t)i;
    if (i == n - 1) rstart[r] = (int32_t)n;
  }
}
// keep[r]: in the vocabulary and count >= effectiveMinTF (minTF >= 1 ? minTF : tokenCount * minTF)
__global__ __launch_bounds__(256) void k_tf_keep(const int32_t* __restrict__ keys, const int32_t* __restrict__ rstart,
                                                 int64_t n_runs, const int64_t* __restrict__ doc_off, int64_t n_docs,
                                                 int32_t n_terms, double min_tf, int32_t* __restrict__ keep) {
  CV_LOOP(r, n_runs + 1) {
    int32_t k = 0;
    if (r < n_runs) {
      const int32_t s = rstart[r], len = rstart[r + 1] - s;
      if (keys[s] < n_terms) {
        double eff = min_tf;
        if (min_tf < 1.0) {
          const int64_t d = doc_of(doc_off, n_docs, s);
          eff = (double)(doc_off[d + 1] - doc_off[d]) * min_tf;
        }
        k = (double)len >= eff ? 1 : 0;
      }
    }
    keep[r] = k;  // keep[n_runs] = 0: the exclusive scan's last element is the total
  }
}
__global__ __launch_bounds__(256) void k_tf_indptr(const int64_t* __restrict__ doc_off, int64_t n_docs,
                                                   const int32_t* __restrict__ rid, const int32_t* __restrict__ slot,
                                                   int64_t* __restrict__ indptr) {
  CV_LOOP(d, n_docs + 1) {
    const int64_t p = doc_off[d];
    indptr[d] = slot[p ? rid[p - 1] : 0];  // the kept runs before the document's first run
  }
}
template <typename V>
__global__ __launch_bounds__(256) void k_tf_emit(const int32_t* __restrict__ keys, const int32_t* __restrict__ rstart,
                                                 const int32_t* __restrict__ keep, const int32_t* __restrict__ slot,
                                                 int64_t n_runs, int binary, int32_t* __restrict__ idx,
                                                 V* __restrict__ vals) {
  CV_LOOP(r, n_runs)
    if (keep[r]) {
      const int32_t s = rstart[r], o = slot[r];
      idx[o] = keys[s];
      vals[o] = binary ? V(1) : V(rstart[r + 1] - s);
    }
}

// ---------------------------------------------------------------------------------------
// the model's operations, behind the stc_cv_* entry points below
// ---------------------------------------------------------------------------------------
stc_cvm* fit(Ctx& c, const TokView& tk, int64_t vocab_size, double min_df, double max_df) {
  single_device(c);
  STC_REQUIRE(vocab_size > 0, "vocabSize must be > 0");
  STC_REQUIRE(min_df >= 0.0, "minDF must be >= 0");
  STC_REQUIRE(max_df >= 0.0, "maxDF must be >= 0");
  const double min_cnt = min_df >= 1.0 ? min_df : min_df * (double)tk.n_docs;
  const double max_cnt = max_df >= 1.0 ? max_df : max_df * (double)tk.n_docs;
  STC_REQUIRE(max_cnt >= min_cnt, "maxDF must be >= minDF");
  STC_REQUIRE(tk.n_tok < (int64_t(1) << 31), "at most 2^31-1 tokens per call (split the corpus)");
  c.use();
  auto m = new_model(c);
  m->has_counts = true;
  const char* kEmpty = "The vocabulary size should be > 0. Lower minDF as necessary.";
  STC_REQUIRE(tk.n_tok > 0, kEmpty);
  hipStream_t st = c.stream;
  const int64_t n = tk.n_tok;
  const uint64_t mask = mask_of(m->hash_bits);
  DevBuf& tmp = c.scratch[2];

  Arena a;
  const size_t o_hk = a.add(8 * n), o_hk2 = a.add(8 * n), o_ti = a.add(4 * n), o_ti2 = a.add(4 * n),
               o_fl = a.add(8 * n), o_small = a.add(64);
  a.commit(c.scratch[0]);
  uint64_t* hk = a.at<uint64_t>(o_hk);
  uint64_t* hk2 = a.at<uint64_t>(o_hk2);
  uint32_t* ti = a.at<uint32_t>(o_ti);
  uint32_t* ti2 = a.at<uint32_t>(o_ti2);
  int64_t* fl = a.at<int64_t>(o_fl);
  int32_t* small = a.at<int32_t>(o_small);  // [0] collision seen, [1] kept terms
  HIP_CHECK(hipMemsetAsync(small, 0, 64, st));

  with_off(tk, [&](const auto* off) { k_cv_hash<<<grid_for(n), 256, 0, st>>>(tk.utf8, off, n, mask, hk, ti); });
  KERNEL_CHECK();
  with_temp(tmp, [&](void* t, size_t& tb) {
    return hipcub::DeviceRadixSort::SortPairs(t, tb, hk, hk2, ti, ti2, (int)n, 0, m->hash_bits, st);
  });
  auto heads = [&] {
    with_off(tk, [&](const auto* off) {
      k_cv_heads<<<grid_for(n), 256, 0, st>>>(tk.utf8, off, tk.doc_off, tk.n_docs, hk2, ti2, n, fl, small);
    });
    KERNEL_CHECK();
  };
  heads();
  int32_t collide = 0;
  HIP_CHECK(hipMemcpyAsync(&collide, small, 4, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  if (collide) {  // some hash run mixes strings: order the tokens by (hash, bytes, token index) instead
    DevBuf& pk = c.scratch[3];
    pk.reserve(sizeof(HashTok) * n);
    k_cv_pack<<<grid_for(n), 256, 0, st>>>(hk2, ti2, n, pk.as<HashTok>());
    KERNEL_CHECK();
    with_off(tk, [&](const auto* off) {
      using O = std::remove_cv_t<std::remove_pointer_t<decltype(off)>>;
      HashTokLess<O> less{tk.utf8, off};
      with_temp(tmp, [&](void* t, size_t& tb) {
        return hipcub::DeviceMergeSort::SortKeys(t, tb, pk.as<HashTok>(), (int)n, less, st);
      });
    });
    k_cv_unpack<<<grid_for(n), 256, 0, st>>>(pk.as<HashTok>(), n, hk2, ti2);
    KERNEL_CHECK();
    heads();
  }
  // inclusive scan of (heads << 32 | document flags), in place
  with_temp(tmp, [&](void* t, size_t& tb) { return hipcub::DeviceScan::InclusiveSum(t, tb, fl, fl, (int)n, st); });
  int64_t last = 0;
  HIP_CHECK(hipMemcpyAsync(&last, fl + (n - 1), 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  const int64_t U = last >> 32;  // distinct terms

  Arena b;
  const size_t o_start = b.add(4 * (U + 1)), o_dstart = b.add(4 * (U + 1)), o_keys = b.add(sizeof(TermKey) * U),
               o_ids = b.add(4 * U), o_len = b.add(8 * (U + 1));
  b.commit(c.scratch[1]);
  int32_t* start = b.at<int32_t>(o_start);
  int32_t* dstart = b.at<int32_t>(o_dstart);
  TermKey* keys = b.at<TermKey>(o_keys);
  uint32_t* ids = b.at<uint32_t>(o_ids);
  int64_t* len = b.at<int64_t>(o_len);
  k_cv_starts<<<grid_for(n), 256, 0, st>>>(fl, n, start, dstart);
  KERNEL_CHECK();
  with_off(tk, [&](const auto* off) {
    using O = std::remove_cv_t<std::remove_pointer_t<decltype(off)>>;
    k_cv_keys<<<grid_for(U), 256, 0, st>>>(tk.utf8, off, ti2, start, dstart, U, min_cnt, max_cnt, keys, ids, small + 1);
    TermLess<O> less{tk.utf8, off};
    with_temp(tmp, [&](void* t, size_t& tb) {
      return hipcub::DeviceMergeSort::SortPairs(t, tb, keys, ids, (int)U, less, st);
    });
  });
  KERNEL_CHECK();
  int32_t kept = 0;
  HIP_CHECK(hipMemcpyAsync(&kept, small + 1, 4, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  const int64_t n_keep = std::min<int64_t>(vocab_size, kept);
  STC_REQUIRE(n_keep > 0, kEmpty);

  m->n_terms = n_keep;
  m->term_off.reserve(8 * (n_keep + 1));
  m->count.reserve(8 * n_keep);
  m->df.reserve(8 * n_keep);
  int64_t* term_off = m->term_off.as<int64_t>();
  with_off(tk, [&](const auto* off) {
    k_cv_lens<<<grid_for(n_keep), 256, 0, st>>>(off, keys, ids, start, dstart, n_keep, len, m->count.as<int64_t>(),
                                                m->df.as<int64_t>());
  });
  KERNEL_CHECK();
  HIP_CHECK(hipMemsetAsync(term_off, 0, 8, st));
  with_temp(tmp, [&](void* t, size_t& tb) {
    return hipcub::DeviceScan::InclusiveSum(t, tb, len, term_off + 1, (int)n_keep, st);
  });
  HIP_CHECK(hipMemcpyAsync(&m->n_bytes, term_off + n_keep, 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  m->blob.reserve(m->n_bytes + kHashPad);
  with_off(tk, [&](const auto* off) {
    k_cv_gather<<<grid_for(n_keep), 256, 0, st>>>(tk.utf8, off, keys, n_keep, term_off, m->blob.as<uint8_t>());
  });
  KERNEL_CHECK();
  if (build_table(c, *m) >= 0) throw Error(STC_ERR_STATE, "cv: fit produced one term twice (internal error)");
  return m.release();
}

stc_cvm* from_vocabulary(Ctx& c, const uint8_t* utf8, int64_t n_bytes, const int64_t* term_off, int64_t n_terms) {
  single_device(c);
  STC_REQUIRE(n_terms > 0 && n_terms < (int64_t(1) << 31), "the vocabulary must hold 1..2^31-1 terms");
  STC_REQUIRE(n_bytes >= 0 && term_off && (n_bytes == 0 || utf8), "utf8/term_off");
  check_offsets("term_off", term_off, n_terms, n_bytes, "n_bytes", false);
  c.use();
  auto m = new_model(c);
  hipStream_t st = c.stream;
  m->n_terms = n_terms;
  m->n_bytes = term_off[n_terms];
  m->blob.reserve(m->n_bytes + kHashPad);
  m->term_off.reserve(8 * (n_terms + 1));
  m->count.reserve(8 * n_terms);
  m->df.reserve(8 * n_terms);
  if (m->n_bytes) HIP_CHECK(hipMemcpyAsync(m->blob.p, utf8, m->n_bytes, hipMemcpyHostToDevice, st));
  HIP_CHECK(hipMemcpyAsync(m->term_off.p, term_off, 8 * (n_terms + 1), hipMemcpyHostToDevice, st));
  HIP_CHECK(hipMemsetAsync(m->count.p, 0, 8 * n_terms, st));
  HIP_CHECK(hipMemsetAsync(m->df.p, 0, 8 * n_terms, st));
  const int32_t dup = build_table(c, *m);
  if (dup >= 0) {
    const std::string term(reinterpret_cast<const char*>(utf8) + term_off[dup], (size_t)(term_off[dup + 1] - term_off[dup]));
    throw Error(STC_ERR_INVALID_ARG, "requirement failed: the vocabulary holds the term \"" + term + "\" more than once");
  }
  return m.release();
}

void get(Ctx& c, const stc_cvm& m, uint8_t* utf8_out, int64_t* term_off_out, int64_t* count_out, int64_t* df_out) {
  single_device(c);
  c.use();
  hipStream_t st = c.stream;
  if (utf8_out && m.n_bytes) HIP_CHECK(hipMemcpyAsync(utf8_out, m.blob.p, m.n_bytes, hipMemcpyDeviceToHost, st));
  if (term_off_out) HIP_CHECK(hipMemcpyAsync(term_off_out, m.term_off.p, 8 * (m.n_terms + 1), hipMemcpyDeviceToHost, st));
  if (count_out) HIP_CHECK(hipMemcpyAsync(count_out, m.count.p, 8 * m.n_terms, hipMemcpyDeviceToHost, st));
  if (df_out) HIP_CHECK(hipMemcpyAsync(df_out, m.df.p, 8 * m.n_terms, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
}

void index_of(Ctx& c, const stc_cvm& m, const TokView& tk, int32_t* idx_out) {
  single_device(c);
  STC_REQUIRE(tk.n_tok < (int64_t(1) << 31), "at most 2^31-1 tokens per call (split the corpus)");
  if (tk.n_tok == 0) return;
  c.use();
  DevBuf& out = c.scratch[0];
  out.reserve(4 * tk.n_tok);
  lookup(c, m, tk, -1, out.as<int32_t>());
  HIP_CHECK(hipMemcpyAsync(idx_out, out.p, 4 * tk.n_tok, hipMemcpyDeviceToHost, c.stream));
  HIP_CHECK(hipStreamSynchronize(c.stream));
}

void transform(Ctx& c, const stc_cvm& m, const TokView& tk, double min_tf, int binary, int value_dtype, DCsr& out) {
  single_device(c);
  STC_REQUIRE(min_tf >= 0.0, "minTF must be >= 0");
  STC_REQUIRE(value_dtype == STC_F32 || value_dtype == STC_F64, "value_dtype");
  STC_REQUIRE(tk.n_tok < (int64_t(1) << 31), "at most 2^31-1 tokens per call (split the corpus)");
  c.use();
  hipStream_t st = c.stream;
  const int64_t n = tk.n_tok, n_docs = tk.n_docs;
  out.rows = n_docs;
  out.cols = m.n_terms;
  out.dtype = value_dtype;
  out.nnz = 0;
  out.positive = true;    // counts >= 1 (binary: 1)
  out.unique_ids = true;  // one entry per distinct index
  c.recycle.take(out.indptr, sizeof(int64_t) * (n_docs + 1));
  if (n == 0) {
    HIP_CHECK(hipMemsetAsync(out.indptr.p, 0, sizeof(int64_t) * (n_docs + 1), st));
    return;
  }
  DevBuf& tmp = c.scratch[2];
  Arena a;
  const size_t o_k = a.add(4 * n), o_k2 = a.add(4 * n), o_rid = a.add(4 * n), o_large = a.add(4 * (n_docs + 16));
  a.commit(c.scratch[0]);
  int32_t* k = a.at<int32_t>(o_k);
  int32_t* k2 = a.at<int32_t>(o_k2);
  int32_t* rid = a.at<int32_t>(o_rid);
  int32_t* n_large_d = a.at<int32_t>(o_large);  // word 0: the long documents' count, from word 16: their list
  int32_t* large = n_large_d + 16;
  const int32_t oov = (int32_t)m.n_terms;  // sorts after every index
  lookup(c, m, tk, oov, k);
  HIP_CHECK(hipMemsetAsync(n_large_d, 0, 4, st));
  k_tf_sort_docs<<<(unsigned)std::min<int64_t>(ceil_div(n_docs, kDocWaves), 1 << 14), 64 * kDocWaves, 0, st>>>(
      k, tk.doc_off, n_docs, k2, large, n_large_d);
  KERNEL_CHECK();
  int32_t n_large = 0;
  if (tk.max_doc < 0 || tk.max_doc > kSortCap) {  // (an upload that knows its longest document skips the read-back)
    HIP_CHECK(hipMemcpyAsync(&n_large, n_large_d, 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
  }
  if (n_large > 0) {  // long documents: hipcub's segmented radix sort
    hashing::sort_long_docs(c, k, k2, n, large, n_large, tk.doc_off, oov /* the largest key */, c.scratch[3], tmp);
  }
  HIP_CHECK(hipMemsetAsync(rid, 0, 4 * n, st));
  k_tf_doc_starts<<<grid_for(n_docs), 256, 0, st>>>(tk.doc_off, n_docs, rid);
  KERNEL_CHECK();
  k_tf_heads<<<grid_for(n), 256, 0, st>>>(k2, n, rid);
  KERNEL_CHECK();
  with_temp(tmp, [&](void* t, size_t& tb) { return hipcub::DeviceScan::InclusiveSum(t, tb, rid, rid, (int)n, st); });
  int32_t n_runs = 0;
  HIP_CHECK(hipMemcpyAsync(&n_runs, rid + (n - 1), 4, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));

  Arena b;
  const size_t o_rs = b.add(4 * ((int64_t)n_runs + 1)), o_keep = b.add(4 * ((int64_t)n_runs + 1)),
               o_slot = b.add(4 * ((int64_t)n_runs + 1));
  b.commit(c.scratch[1]);
  int32_t* rstart = b.at<int32_t>(o_rs);
  int32_t* keep = b.at<int32_t>(o_keep);
  int32_t* slot = b.at<int32_t>(o_slot);
  k_tf_starts<<<grid_for(n), 256, 0, st>>>(rid, n, rstart);
  KERNEL_CHECK();
  k_tf_keep<<<grid_for(n_runs + 1), 256, 0, st>>>(k2, rstart, n_runs, tk.doc_off, n_docs, oov, min_tf, keep);
  KERNEL_CHECK();
  with_temp(tmp, [&](void* t, size_t& tb) { return hipcub::DeviceScan::ExclusiveSum(t, tb, keep, slot, n_runs + 1, st); });
  k_tf_indptr<<<grid_for(n_docs + 1), 256, 0, st>>>(tk.doc_off, n_docs, rid, slot, out.indptr.as<int64_t>());
  KERNEL_CHECK();
  int32_t total = 0;
  HIP_CHECK(hipMemcpyAsync(&total, slot + n_runs, 4, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  out.nnz = total;
  c.recycle.take(out.indices, sizeof(int32_t) * std::max<int64_t>(total, 1));
  c.recycle.take(out.values, (value_dtype == STC_F32 ? 4 : 8) * std::max<int64_t>(total, 1));
  if (value_dtype == STC_F32)
    k_tf_emit<float><<<grid_for(n_runs), 256, 0, st>>>(k2, rstart, keep, slot, n_runs, binary, out.indices.as<int32_t>(),
                                                        out.values.as<float>());
  else
    k_tf_emit<double><<<grid_for(n_runs), 256, 0, st>>>(k2, rstart, keep, slot, n_runs, binary, out.indices.as<int32_t>(),
                                                         out.values.as<double>());
  KERNEL_CHECK();
}

void destroy(stc_cvm* m) {
  if (!m) return;
  if (m->device >= 0) {  // queued readers of the model first: the buffers are freed below
    (void)hipSetDevice(m->device);
    (void)hipDeviceSynchronize();
  }
  delete m;
}

void cv_view_upload(const TokenUpload& u, int64_t n_tok, int64_t n_docs, TokView& v) {
  v.utf8 = u.utf8.as<uint8_t>();
  v.off64 = u.tok_off.as<int64_t>();
  v.n_tok = n_tok;
  v.doc_off = u.doc_off.as<int64_t>();
  v.n_docs = n_docs;
  v.max_doc = u.max_doc;
}
void cv_view_tokens(const stc_dtok& t, TokView& v) {
  v.utf8 = t.utf8.as<uint8_t>();
  if (t.off32) v.off32 = t.tok_off.as<uint32_t>();
  else v.off64 = t.tok_off.as<int64_t>();
  v.n_tok = t.n_tok;
  v.doc_off = t.doc_off.as<int64_t>();
  v.n_docs = t.n_docs;
  v.max_doc = t.max_doc;
}

}  // namespace
}  // namespace cv
}  // namespace stc

using namespace stc;

extern "C" {

// ---- C ABI: the pointers are checked and host tokens uploaded (padded as stc_tokens_upload does) here ----

int stc_cv_fit(stc_ctx* ctx, const uint8_t* utf8, int64_t n_bytes, const int64_t* tok_off, int64_t n_tok,
               const int64_t* doc_off, int64_t n_docs, int64_t vocab_size, double min_df, double max_df,
               stc_cvm** out) {
  return guard([&] {
    STC_REQUIRE(ctx && doc_off && out, "ctx/doc_off/out");
    ctx->use();
    TokenUpload u;
    upload_tokens(*ctx, u, utf8, n_bytes, tok_off, n_tok, doc_off, n_docs);
    wait_stream(*ctx, ctx->stream);
    cv::TokView v;
    cv::cv_view_upload(u, n_tok, n_docs, v);
    *out = cv::fit(*ctx, v, vocab_size, min_df, max_df);
  });
}

int stc_cv_fit_tokens(stc_ctx* ctx, const stc_dtok* tokens, int64_t vocab_size, double min_df, double max_df,
                      stc_cvm** out) {
  return guard([&] {
    STC_REQUIRE(ctx && tokens && out, "ctx/tokens/out");
    STC_REQUIRE(tokens->ctx == ctx, "tokens were uploaded on another stc_ctx");
    cv::TokView v;
    cv::cv_view_tokens(*tokens, v);
    *out = cv::fit(*ctx, v, vocab_size, min_df, max_df);
  });
}

int stc_cv_from_vocabulary(stc_ctx* ctx, const uint8_t* utf8, int64_t n_bytes, const int64_t* term_off,
                           int64_t n_terms, stc_cvm** out) {
  return guard([&] {
    STC_REQUIRE(ctx && out, "ctx/out");
    *out = cv::from_vocabulary(*ctx, utf8, n_bytes, term_off, n_terms);
  });
}

int stc_cv_shape(const stc_cvm* model, int64_t* n_terms_out, int64_t* n_bytes_out) {
  return guard([&] {
    STC_REQUIRE(model, "model");
    if (n_terms_out) *n_terms_out = model->n_terms;
    if (n_bytes_out) *n_bytes_out = model->n_bytes;
  });
}

int stc_cv_get(stc_ctx* ctx, const stc_cvm* model, uint8_t* utf8_out, int64_t* term_off_out, int64_t* count_out,
               int64_t* df_out) {
  return guard([&] {
    STC_REQUIRE(ctx && model, "ctx/model");
    STC_REQUIRE(model->ctx == ctx, "the model belongs to another stc_ctx");
    cv::get(*ctx, *model, utf8_out, term_off_out, count_out, df_out);
  });
}

int stc_cv_index_of(stc_ctx* ctx, const stc_cvm* model, const uint8_t* utf8, int64_t n_bytes, const int64_t* tok_off,
                    int64_t n_tok, int32_t* idx_out) {
  return guard([&] {
    STC_REQUIRE(ctx && model && (idx_out || n_tok == 0), "ctx/model/idx_out");
    STC_REQUIRE(model->ctx == ctx, "the model belongs to another stc_ctx");
    ctx->use();
    TokenUpload u;
    upload_tokens(*ctx, u, utf8, n_bytes, tok_off, n_tok, nullptr, 0);
    wait_stream(*ctx, ctx->stream);
    cv::TokView v;
    cv::cv_view_upload(u, n_tok, 0, v);
    v.doc_off = nullptr;
    cv::index_of(*ctx, *model, v, idx_out);
  });
}

int stc_cv_transform_dev(stc_ctx* ctx, const stc_cvm* model, const uint8_t* utf8, int64_t n_bytes,
                         const int64_t* tok_off, int64_t n_tok, const int64_t* doc_off, int64_t n_docs, double min_tf,
                         int binary, int value_dtype, stc_dcsr** out) {
  return guard([&] {
    STC_REQUIRE(ctx && model && doc_off && out, "ctx/model/doc_off/out");
    STC_REQUIRE(model->ctx == ctx, "the model belongs to another stc_ctx");
    STC_REQUIRE(value_dtype == STC_F32 || value_dtype == STC_F64, "value_dtype");
    ctx->use();
    TokenUpload u;
    upload_tokens(*ctx, u, utf8, n_bytes, tok_off, n_tok, doc_off, n_docs);
    wait_stream(*ctx, ctx->stream);
    auto m = new_handle<stc_dcsr>(*ctx);
    cv::TokView v;
    cv::cv_view_upload(u, n_tok, n_docs, v);
    cv::transform(*ctx, *model, v, min_tf, binary, value_dtype, *m);
    wait_stream(*ctx, ctx->stream);  // the uploaded tokens are freed on return
    *out = m.release();
  });
}

int stc_cv_transform_tokens(stc_ctx* ctx, const stc_cvm* model, const stc_dtok* tokens, double min_tf, int binary,
                            int value_dtype, stc_dcsr** out) {
  return guard([&] {
    STC_REQUIRE(ctx && model && tokens && out, "ctx/model/tokens/out");
    STC_REQUIRE(model->ctx == ctx, "the model belongs to another stc_ctx");
    STC_REQUIRE(tokens->ctx == ctx, "tokens were uploaded on another stc_ctx");
    STC_REQUIRE(value_dtype == STC_F32 || value_dtype == STC_F64, "value_dtype");
    auto m = new_handle<stc_dcsr>(*ctx);
    cv::TokView v;
    cv::cv_view_tokens(*tokens, v);
    cv::transform(*ctx, *model, v, min_tf, binary, value_dtype, *m);
    *out = m.release();
  });
}

int stc_cv_free(stc_cvm* model) {
  return guard([&] { cv::destroy(model); });
}

}  // extern "C"
