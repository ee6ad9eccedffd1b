// lda_score.hip — document scores (include/stc.h, "Document scores"): a set of documents scored once, γ kept on the
// device, and the clustering report's questions answered from it.
//
// What a score holds: γ rows×k fp64 (a row marked empty stored as 0), rowsum[r] = Σ_j |γ[r][j]| added sequentially
// in ascending j (−1: empty), each row's main topic and its θ, the per-topic counts; built by two kernels:
//   k_score_widen  reads γ of the E-step's type T (or the uploaded doubles) and the emptiness marks; writes γ as
//                  fp64 and rowsum.  One wave per 64 rows: a tile of 64 rows × 16 topics goes through LDS so that
//                  global reads and writes are row segments while each lane adds its own row in order.
//   k_score_main   reads γ and rowsum; writes topic[r] (the last maximum of θ = γ / rowsum, −1 for an empty row),
//                  weight[r] and adds the rows to count[k] (integer atomics: a block's LDS counters, then global).
// Grouping (stc_score_members, made on first use) is a stable counting sort in three kernels, integers only:
//   k_group_count  reads topic; a wave counts its tile's rows per topic in LDS and writes its k counters.
//   k_group_scan   reads count[k] and the tiles' counters; writes indptr[k+1] and turns every tile's counter into
//                  the position of that tile's first row of the topic.
//   k_group_place  reads topic and those positions; a wave walks its tile 64 rows at a time in row order and
//                  writes members[]: inside a topic the rows ascend, whatever the grid.
// The two ranked lists call rank.h on (γ, rowsum).
//
// Important terms: S_t as a k×V bit set (rank.h's column selection in raw mode over the resident λ, then
// k_terms_bits: integer atomicOr), and k_terms_select, one workgroup per document claimed by ticket:
//   a row of at most kCap entries is loaded whole; a longer one gets rank_key.h's most-significant-digit radix
//   selection over the 96-bit key (value key, ~term), 8 bits a pass, which stops as soon as the keys at or above
//   the selected prefix fit the candidate list (at the latest after 12 digits, when they are exactly the
//   doc_terms first) and collects them; then rank_key.h's bitonic sort of the candidates by the key in LDS, the
//   bit test of the first doc_terms against S_t and an ordered compaction (ballot prefix) of the first max_out.
// Ties at the threshold value are resolved by the key's term digits, so the result does not depend on the order
// of a row's entries (stc_dcsr_upload does not require ascending indices), nor on the ticket order or the atomics:
// counts are integers and the final order is a total order of the keys.
#include "lda_handle.h"
#include "lda_online.h"
#include "rank.h"
#include "rank_key.h"

using namespace stc;

struct stc_dscore {
  stc::Ctx* ctx = nullptr;  // the context that made it; only it may read the buffers
  int device = -1;          // for stc_score_free, which may run after that context is gone
  int64_t rows = 0, nonempty = 0;
  int k = 0;
  DevBuf gamma, rowsum;         // double[rows×k], double[rows]
  DevBuf topic, weight, count;  // int32[rows], double[rows], uint64[k]
  std::vector<int64_t> counts;  // count[] on the host
  // what the queries make on first use
  mutable bool grouped = false;
  mutable DevBuf indptr, members;  // int64[k+1], int64[nonempty]
  mutable rank::Scratch rk;
};

namespace {

constexpr int kWidenCols = 16;  // topics of one LDS tile
constexpr int kGroupTiles = 1024;  // at most this many tiles (waves) group the rows
constexpr int kCap = 2048;         // candidates of one document sorted in LDS: 16 KiB of keys + 8 KiB of terms
constexpr int kHistPitch = 257;    // a wave's 256 digit counters + 1

// ---- widen + row sum -------------------------------------------------------------------------------------------
// LDS: the tile holds `rows` segments of w <= 16 doubles at a pitch of w | 1 doubles.  Reading, lane i adds
// tile[i·pitch + c] for c ascending: the pitch is odd, so the 32 lanes of a ds_read_b64 group sit on 32 different
// double slots of the 64-bank row — conflict-free.  Writing, element e of the tile goes to (e / w)·pitch + e % w:
// at w = 16 a 16-lane ds_write_b64 group writes one whole segment (contiguous, conflict-free); a narrower last
// chunk takes a gap per segment and may pay 2-way on a few groups, once per 64 rows.
template <typename T>
__global__ __launch_bounds__(64) void k_score_widen(const T* src, const int64_t* __restrict__ ptr,
                                                    const uint8_t* __restrict__ empty, int64_t R, int k, double* gamma,
                                                    double* __restrict__ rowsum) {
  __shared__ double tile[64 * (kWidenCols + 1)];
  const int lane = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  const int rows = (int)min((int64_t)64, R - r0);
  const int64_t r = r0 + lane;
  bool is_empty = false;
  if (lane < rows) is_empty = ptr ? ptr[r + 1] == ptr[r] : (empty != nullptr && empty[r] != 0);
  const unsigned long long emask = __ballot(is_empty);
  double s = 0.0;
  for (int c0 = 0; c0 < k; c0 += kWidenCols) {
    const int w = min(kWidenCols, k - c0), pitch = w | 1;
    for (int e = lane; e < rows * w; e += 64) {
      const int rl = e / w, c = e - rl * w;
      const int64_t off = (r0 + rl) * k + c0 + c;
      const double x = ((emask >> rl) & 1ull) ? 0.0 : (double)src[off];
      gamma[off] = x;
      tile[rl * pitch + c] = x;
    }
    __syncthreads();
    if (lane < rows)
      for (int c = 0; c < w; ++c) s += fabs(tile[lane * pitch + c]);
    __syncthreads();
  }
  if (lane < rows) rowsum[r] = is_empty ? -1.0 : s;
}

// ---- main topic ------------------------------------------------------------------------------------------------
// lpr lanes per row (the power of two at or above k, at most 64), 64 / lpr rows per wave; lane j0 of a row walks
// topics j0, j0 + lpr, … ascending with >=, so it keeps its last maximum, and the butterfly prefers the larger θ,
// then the larger topic.  θ is formed as stc_score_topic_distribution forms it.
__global__ __launch_bounds__(256) void k_score_main(const double* __restrict__ gamma, const double* __restrict__ rowsum,
                                                    int64_t R, int k, int lpr, int32_t* __restrict__ topic,
                                                    double* __restrict__ weight, unsigned long long* __restrict__ count) {
  __shared__ uint32_t h[4096];
  for (int i = threadIdx.x; i < k; i += 256) h[i] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, G = 64 / lpr;
  const int j0 = lane & (lpr - 1), slot = lane / lpr;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), waves = (int64_t)gridDim.x * 4;
  for (int64_t base = wave * G; base < R; base += waves * G) {  // wave-uniform
    const int64_t r = base + slot;
    const bool valid = r < R;
    const double s = valid ? rowsum[r] : -1.0;
    double best = -1.0;
    int bj = -1;
    if (valid) {
      for (int j = j0; j < k; j += lpr) {
        double x = gamma[r * k + j];
        if (s > 0.0) x = x / s;
        if (x >= best) best = x, bj = j;
      }
    }
    rank::row_argmax<true>(lpr, best, bj);
    if (valid && j0 == 0) {
      const bool none = s < 0.0 || bj < 0;  // bj < 0: a row of NaN only (unpinned)
      topic[r] = none ? -1 : bj;
      weight[r] = none ? 0.0 : best;
      if (!none) atomicAdd(&h[bj], 1u);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < k; i += 256)
    if (h[i]) atomicAdd(&count[i], (unsigned long long)h[i]);
}

__global__ void k_score_theta(const double* __restrict__ gamma, const double* __restrict__ rowsum, int64_t n, int k,
                              double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double s = rowsum[i / k], x = gamma[i];
  out[i] = s > 0.0 ? x / s : x;
}

// ---- grouping --------------------------------------------------------------------------------------------------
// tile b = rows [b·tile, (b+1)·tile), one wave each; cnt[b·k + t]
__global__ __launch_bounds__(64) void k_group_count(const int32_t* __restrict__ topic, int64_t R, int k, int64_t tile,
                                                    uint32_t* __restrict__ cnt) {
  __shared__ uint32_t h[4096];
  for (int i = threadIdx.x; i < k; i += 64) h[i] = 0;
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * tile, r1 = min(R, r0 + tile);
  for (int64_t r = r0 + threadIdx.x; r < r1; r += 64) {
    const int t = topic[r];
    if (t >= 0) atomicAdd(&h[t], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < k; i += 64) cnt[(int64_t)blockIdx.x * k + i] = h[i];
}

// thread t: indptr[t] = Σ_{u<t} count[u]; pos[b·k + t] = indptr[t] + the rows of topic t in the tiles before b
__global__ void k_group_scan(const unsigned long long* __restrict__ count, int k, int tiles, uint32_t* __restrict__ cnt,
                             int64_t* __restrict__ pos, int64_t* __restrict__ indptr) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= k) return;
  int64_t run = 0;
  for (int u = 0; u < t; ++u) run += (int64_t)count[u];
  indptr[t] = run;
  if (t == k - 1) indptr[k] = run + (int64_t)count[t];
  for (int b = 0; b < tiles; ++b) {
    const uint32_t c = cnt[(int64_t)b * k + t];
    pos[(int64_t)b * k + t] = run;
    run += c;
  }
}

__global__ __launch_bounds__(64) void k_group_place(const int32_t* __restrict__ topic, int64_t R, int k, int64_t tile,
                                                    const int64_t* __restrict__ pos, int64_t* __restrict__ members) {
  __shared__ int64_t next[4096];
  for (int i = threadIdx.x; i < k; i += 64) next[i] = pos[(int64_t)blockIdx.x * k + i];
  __syncthreads();
  const int lane = threadIdx.x;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int64_t r0 = (int64_t)blockIdx.x * tile, r1 = min(R, r0 + tile);
  for (int64_t c0 = r0; c0 < r1; c0 += 64) {  // 64 rows at a time, in row order
    const int64_t r = c0 + lane;
    const int t = r < r1 ? topic[r] : -1;
    bool todo = t >= 0;
    unsigned long long left = __ballot(todo);
    while (left) {  // one topic of the chunk per turn: its rows take consecutive positions in lane order
      const int t0 = __shfl(t, __ffsll((long long)left) - 1, 64);
      const unsigned long long same = __ballot(todo && t == t0);
      if (todo && t == t0) {
        members[next[t0] + __popcll(same & below)] = r;
        todo = false;
      }
      __syncthreads();  // the reads of next[t0] before its update (one wave: a barrier of its own)
      if (lane == 0) next[t0] += __popcll(same);
      __syncthreads();
      left &= ~same;
    }
  }
}

// ---- important terms -------------------------------------------------------------------------------------------
__global__ void k_terms_bits(const int64_t* __restrict__ sel, int64_t n_per_topic, int k, int64_t W,
                             uint32_t* __restrict__ bits) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_per_topic * k) return;
  const int64_t t = i / n_per_topic, w = sel[i];
  atomicOr(&bits[t * W + (w >> 5)], 1u << (w & 31));
}

// a block-uniform value read from LDS, as a scalar
__device__ inline int64_t uniform64(unsigned long long v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return (int64_t)(((unsigned long long)hi << 32) | lo);
}

// LDS of k_terms_select.
//  s_hist: one histogram per wave at a pitch of 257 counters — wave w's digit d sits on bank (w + d) mod 32, so the
//    four waves counting one digit (a row of near-equal values) do not queue on one bank; lanes of one wave that
//    count the same digit are serialised by the atomic unit, which no layout avoids.
//  s_key (u64) / s_idx (u32): the candidate list, in the layout rank_key.h's block_bitonic_sort argues.
template <typename T>
__global__ __launch_bounds__(256) void k_terms_select(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                      const T* __restrict__ values, const int32_t* __restrict__ topic,
                                                      int64_t R, const uint32_t* __restrict__ bits, int64_t W, int DT,
                                                      int max_out, unsigned long long* __restrict__ ticket,
                                                      int32_t* __restrict__ idx_out, double* __restrict__ val_out,
                                                      int32_t* __restrict__ n_out) {
  __shared__ uint64_t s_key[kCap];
  __shared__ uint32_t s_idx[kCap];
  __shared__ uint32_t s_hist[4 * kHistPitch];
  __shared__ unsigned long long s_doc;
  __shared__ uint32_t s_digit, s_above, s_in_digit, s_cnt;
  __shared__ int s_wsum[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  // the ticket loop in k_estep_rows64_pers' form: the claim and the exit test are the loop's own condition and d is
  // made a scalar, so the compiler sees a uniform loop around the barriers (written as for (;;) { if (tid == 0)
  // claim; barrier; if (d >= R) return; … } it split thread 0 from its wave around the first barrier)
  if (tid == 0) s_doc = atomicAdd(ticket, 1ull);
  __syncthreads();
  int64_t d = uniform64(s_doc);
  while (d < R) {
    __syncthreads();  // every thread has read s_doc
    const int64_t e0 = indptr[d], n = indptr[d + 1] - e0;
    const int t = topic[d];
    int found = 0;
    if (t >= 0 && n > 0) {
      uint32_t m;  // candidates in s_key / s_idx
      if (n <= kCap) {
        for (int i = tid; i < (int)n; i += 256) {
          s_key[i] = rank::value_key(values[e0 + i]);
          s_idx[i] = (uint32_t)indices[e0 + i];
        }
        m = (uint32_t)n;
      } else {
        rank::Prefix pre = {0, 0, 0};
        uint32_t above = 0;
        for (;;) {
          for (int i = tid; i < 4 * kHistPitch; i += 256) s_hist[i] = 0;
          __syncthreads();
          for (int64_t i = tid; i < n; i += 256) {
            const uint64_t hi = rank::value_key(values[e0 + i]);
            const uint32_t lo = ~(uint32_t)indices[e0 + i];
            if (pre.matches(hi, lo)) atomicAdd(&s_hist[wave * kHistPitch + pre.digit(hi, lo)], 1u);
          }
          __syncthreads();
          if (wave == 0) {  // the digit that takes the count to DT, over the four waves' histograms
            const rank::DigitPick p = rank::pick_digit(s_hist, 4, kHistPitch, above, (uint32_t)DT);
            if (lane == 0) s_digit = p.digit, s_above = p.above, s_in_digit = p.in_digit;
          }
          __syncthreads();
          pre.append(s_digit);
          above = s_above;
          const bool done = pre.done(above + s_in_digit, (uint32_t)kCap);
          __syncthreads();
          if (done) break;  // block-uniform
        }
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        for (int64_t i = tid; i < n; i += 256) {
          const uint64_t hi = rank::value_key(values[e0 + i]);
          const uint32_t ix = (uint32_t)indices[e0 + i];
          if (!pre.at_or_above(hi, ~ix)) continue;
          const uint32_t p = atomicAdd(&s_cnt, 1u);
          if (p < (uint32_t)kCap) {  // always, unless a row repeats one (value, term) entry past the list
            s_key[p] = hi;
            s_idx[p] = ix;
          }
        }
        __syncthreads();
        m = min(s_cnt, (uint32_t)kCap);
      }
      uint32_t P = 2;
      while (P < m) P <<= 1;
      for (uint32_t i = m + tid; i < P; i += 256) {  // padding sorts behind every key (a term is below 2^31)
        s_key[i] = 0ull;
        s_idx[i] = 0xFFFFFFFFu;
      }
      __syncthreads();
      rank::block_bitonic_sort(s_key, s_idx, P);
      // the first L entries are L_d; those in S_t leave in order, max_out at most
      const int L = (int)min((uint32_t)DT, m);
      const uint32_t* trow = bits + (int64_t)t * W;
      for (int c0 = 0; c0 < L && found < max_out; c0 += 256) {  // block-uniform
        const int i = c0 + tid;
        uint32_t w = 0;
        bool in = false;
        if (i < L) {
          w = s_idx[i];
          in = (trow[w >> 5] >> (w & 31)) & 1u;
        }
        const unsigned long long bal = __ballot(in);
        if (lane == 0) s_wsum[wave] = __popcll(bal);
        __syncthreads();
        int off = found, total = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          off += u < wave ? s_wsum[u] : 0;
          total += s_wsum[u];
        }
        const int p = off + __popcll(bal & below);
        if (in && p < max_out) {
          idx_out[d * max_out + p] = (int32_t)w;
          val_out[d * max_out + p] = rank::key_value(s_key[i]);
        }
        found += total;
        __syncthreads();
      }
      found = min(found, max_out);
    }
    for (int i = found + tid; i < max_out; i += 256) {
      idx_out[d * max_out + i] = -1;
      val_out[d * max_out + i] = 0.0;
    }
    if (tid == 0) {
      n_out[d] = found;
      s_doc = atomicAdd(ticket, 1ull);
    }
    __syncthreads();
    d = uniform64(s_doc);
  }
}

// ---- host ------------------------------------------------------------------------------------------------------
void require_single(const Ctx& c) {
  if (c.coll())
    throw Error(STC_ERR_STATE, "score: the context is connected to other ranks (document scores are single-device)");
}

const stc_dscore& checked(stc_ctx* ctx, const stc_dscore* score) {
  STC_REQUIRE(ctx && score, "ctx/score");
  STC_REQUIRE(score->ctx == ctx, "the score belongs to another stc_ctx");
  require_single(*ctx);
  ctx->use();
  return *score;
}

// rowsum, the main topics and the counts from γ in `src` (T, or the score's own doubles when src == S.gamma.p)
template <typename T>
void finish(stc_dscore& S, const T* src, const int64_t* ptr, const uint8_t* empty) {
  Ctx& c = *S.ctx;
  hipStream_t s = c.stream;
  S.rowsum.reserve(8 * std::max<int64_t>(S.rows, 1));
  S.topic.reserve(4 * std::max<int64_t>(S.rows, 1));
  S.weight.reserve(8 * std::max<int64_t>(S.rows, 1));
  S.count.reserve(8 * (size_t)S.k);
  S.counts.assign((size_t)S.k, 0);
  HIP_CHECK(hipMemsetAsync(S.count.p, 0, 8 * (size_t)S.k, s));
  if (S.rows > 0) {
    k_score_widen<T><<<blocks_for(S.rows, 64), 64, 0, s>>>(src, ptr, empty, S.rows, S.k, S.gamma.as<double>(),
                                                           S.rowsum.as<double>());
    KERNEL_CHECK();
    const int lpr = std::min(pow2_at_least(S.k), 64);
    const int64_t waves = ceil_div(S.rows, 64 / lpr);
    const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(waves, 4), (int64_t)c.cus * 8);
    k_score_main<<<grid, 256, 0, s>>>(S.gamma.as<double>(), S.rowsum.as<double>(), S.rows, S.k, lpr, S.topic.as<int32_t>(),
                                      S.weight.as<double>(), S.count.as<unsigned long long>());
    KERNEL_CHECK();
    HIP_CHECK(hipMemcpyAsync(S.counts.data(), S.count.p, 8 * (size_t)S.k, hipMemcpyDeviceToHost, s));
  }
  wait_stream(c, s);
  S.nonempty = 0;
  for (int64_t n : S.counts) S.nonempty += n;
}

void group(const stc_dscore& S) {
  if (S.grouped) return;
  hipStream_t s = S.ctx->stream;
  S.indptr.reserve(8 * ((size_t)S.k + 1));
  S.members.reserve(8 * std::max<int64_t>(S.nonempty, 1));
  if (S.rows == 0) {
    HIP_CHECK(hipMemsetAsync(S.indptr.p, 0, 8 * ((size_t)S.k + 1), s));
  } else {
    const int64_t tile = std::max<int64_t>(2048, ceil_div(ceil_div(S.rows, kGroupTiles), 64) * 64);
    const int tiles = (int)ceil_div(S.rows, tile);
    DevBuf cnt, pos;
    cnt.reserve(4 * (size_t)tiles * S.k);
    pos.reserve(8 * (size_t)tiles * S.k);
    k_group_count<<<tiles, 64, 0, s>>>(S.topic.as<int32_t>(), S.rows, S.k, tile, cnt.as<uint32_t>());
    KERNEL_CHECK();
    k_group_scan<<<blocks_for(S.k, 256), 256, 0, s>>>(S.count.as<unsigned long long>(), S.k, tiles, cnt.as<uint32_t>(),
                                                      pos.as<int64_t>(), S.indptr.as<int64_t>());
    KERNEL_CHECK();
    k_group_place<<<tiles, 64, 0, s>>>(S.topic.as<int32_t>(), S.rows, S.k, tile, pos.as<int64_t>(), S.members.as<int64_t>());
    KERNEL_CHECK();
    wait_stream(*S.ctx, s);  // cnt / pos are freed here
  }
  S.grouped = true;
}

template <typename T>
void launch_terms(hipStream_t s, const Ctx& c, const DCsr& docs, const int32_t* topic, const uint32_t* bits, int64_t W,
                  int doc_terms, int max_out, unsigned long long* ticket, int32_t* idx, double* val, int32_t* n) {
  const unsigned grid = (unsigned)std::min<int64_t>(docs.rows, (int64_t)c.cus * 4);
  k_terms_select<T><<<grid, 256, 0, s>>>(docs.indptr.as<int64_t>(), docs.indices.as<int32_t>(), docs.values.as<T>(), topic,
                                         docs.rows, bits, W, doc_terms, max_out, ticket, idx, val, n);
  KERNEL_CHECK();
}

}  // namespace

extern "C" {

int stc_lda_score(stc_lda* L, const stc_dcsr* docs, uint64_t gamma_seed, int64_t doc_id_base, const double* gamma0,
                  stc_dscore** out) {
  return guard([&] {
    STC_REQUIRE(L && docs && out, "lda/docs/out");
    STC_REQUIRE(docs->ctx == L->ctx, "the documents belong to another stc_ctx than the LDA handle");
    require_single(*L->ctx);
    L->ctx->use();
    auto S = new_handle<stc_dscore>(*L->ctx);
    S->rows = docs->rows;
    S->k = L->k;
    S->gamma.reserve(8 * std::max<int64_t>(S->rows * S->k, 1));
    const void* g = online::score_gamma(*L, *docs, gamma_seed, doc_id_base, gamma0);
    online::by_infer_type(*L, [&](auto t) {
      finish<decltype(t)>(*S, static_cast<const decltype(t)*>(g), docs->indptr.as<int64_t>(), nullptr);
    });
    *out = S.release();
  });
}

int stc_score_from_gamma(stc_ctx* ctx, const double* gamma, const uint8_t* empty, int64_t rows, int32_t k,
                         stc_dscore** out) {
  return guard([&] {
    STC_REQUIRE(ctx && out && (gamma || rows == 0), "ctx/gamma/out");
    STC_REQUIRE(rows >= 0 && rows < (int64_t(1) << 31), "score: 0 <= rows < 2^31");
    STC_REQUIRE(k >= 2 && k <= 4096, "score: 2 <= k <= 4096");
    require_single(*ctx);
    for (int64_t i = 0; i < rows * k; ++i)
      STC_REQUIRE(gamma[i] >= 0.0 && std::isfinite(gamma[i]), "score: gamma entries must be finite and >= 0");
    ctx->use();
    auto S = new_handle<stc_dscore>(*ctx);
    S->rows = rows;
    S->k = k;
    S->gamma.reserve(8 * std::max<int64_t>(rows * k, 1));
    DevBuf marks;
    if (rows > 0) {
      HIP_CHECK(hipMemcpyAsync(S->gamma.p, gamma, 8 * rows * k, hipMemcpyHostToDevice, ctx->stream));
      if (empty) {
        marks.reserve((size_t)rows);
        HIP_CHECK(hipMemcpyAsync(marks.p, empty, (size_t)rows, hipMemcpyHostToDevice, ctx->stream));
      }
    }
    finish<double>(*S, S->gamma.as<double>(), nullptr, empty ? marks.as<uint8_t>() : nullptr);
    *out = S.release();
  });
}

int stc_score_free(stc_dscore* score) {
  return guard([&] {
    if (!score) return;
    if (score->device >= 0) (void)hipSetDevice(score->device);
    delete score;
  });
}

int stc_score_shape(const stc_dscore* score, int64_t* rows, int32_t* k, int64_t* nonempty) {
  return guard([&] {
    STC_REQUIRE(score, "score");
    if (rows) *rows = score->rows;
    if (k) *k = score->k;
    if (nonempty) *nonempty = score->nonempty;
  });
}

int stc_score_topic_distribution(stc_ctx* ctx, const stc_dscore* score, double* out) {
  return guard([&] {
    const stc_dscore& S = checked(ctx, score);
    const int64_t n = S.rows * S.k;
    if (n > 0 && out) {
      DevBuf th;
      th.reserve(8 * n);
      k_score_theta<<<blocks_for(n, 256), 256, 0, ctx->stream>>>(S.gamma.as<double>(), S.rowsum.as<double>(), n, S.k,
                                                                 th.as<double>());
      KERNEL_CHECK();
      HIP_CHECK(hipMemcpyAsync(out, th.p, 8 * n, hipMemcpyDeviceToHost, ctx->stream));
      wait_stream(*ctx, ctx->stream);
      return;
    }
    wait_stream(*ctx, ctx->stream);
  });
}

int stc_score_main_topics(stc_ctx* ctx, const stc_dscore* score, int32_t* topic_out, double* weight_out,
                          int64_t* count_out) {
  return guard([&] {
    const stc_dscore& S = checked(ctx, score);
    hipStream_t s = ctx->stream;
    if (topic_out && S.rows) HIP_CHECK(hipMemcpyAsync(topic_out, S.topic.p, 4 * S.rows, hipMemcpyDeviceToHost, s));
    if (weight_out && S.rows) HIP_CHECK(hipMemcpyAsync(weight_out, S.weight.p, 8 * S.rows, hipMemcpyDeviceToHost, s));
    wait_stream(*ctx, s);
    if (count_out) std::copy(S.counts.begin(), S.counts.end(), count_out);
  });
}

int stc_score_members(stc_ctx* ctx, const stc_dscore* score, int64_t* indptr_out, int64_t* rows_out) {
  return guard([&] {
    const stc_dscore& S = checked(ctx, score);
    hipStream_t s = ctx->stream;
    group(S);
    if (indptr_out) HIP_CHECK(hipMemcpyAsync(indptr_out, S.indptr.p, 8 * ((size_t)S.k + 1), hipMemcpyDeviceToHost, s));
    if (rows_out && S.nonempty) HIP_CHECK(hipMemcpyAsync(rows_out, S.members.p, 8 * S.nonempty, hipMemcpyDeviceToHost, s));
    wait_stream(*ctx, s);
  });
}

int stc_score_top_topics(stc_ctx* ctx, const stc_dscore* score, int32_t n_topics, int32_t* idx_out, double* weight_out) {
  return guard([&] {
    const stc_dscore& S = checked(ctx, score);
    STC_REQUIRE(n_topics > 0, "score: n_topics > 0");
    STC_REQUIRE(S.k <= 1024, "score: top_topics serves k <= 1024 (the row selection's register slices)");
    hipStream_t s = ctx->stream;
    if (S.rows > 0) {
      const int N = std::min<int>(n_topics, S.k);
      const int64_t total = S.rows * N;
      S.rk.out_row.reserve(4 * total);
      S.rk.out_w.reserve(8 * total);
      rank::select_rows(s, S.gamma.p, false, S.rowsum.as<double>(), S.rows, S.k, N, S.rk.out_row.as<int32_t>(),
                            S.rk.out_w.as<double>());
      if (idx_out) HIP_CHECK(hipMemcpyAsync(idx_out, S.rk.out_row.p, 4 * total, hipMemcpyDeviceToHost, s));
      if (weight_out) HIP_CHECK(hipMemcpyAsync(weight_out, S.rk.out_w.p, 8 * total, hipMemcpyDeviceToHost, s));
    }
    wait_stream(*ctx, s);
  });
}

int stc_score_top_documents(stc_ctx* ctx, const stc_dscore* score, int64_t max_docs, int64_t* n_out, int64_t* row_out,
                            double* weight_out) {
  return guard([&] {
    const stc_dscore& S = checked(ctx, score);
    STC_REQUIRE(max_docs > 0, "score: max_docs > 0");
    hipStream_t s = ctx->stream;
    const int64_t N = std::min(max_docs, S.nonempty), cap = std::min(max_docs, S.rows), total = N * S.k;
    if (N > 0) {
      S.rk.out_row.reserve(8 * total);
      S.rk.out_w.reserve(8 * total);
      rank::select_columns(s, S.rk, S.gamma.p, false, S.rows, S.k, N, S.rowsum.as<double>(), nullptr, 0,
                               S.rk.out_row.as<int64_t>(), S.rk.out_w.as<double>());
      for (int t = 0; t < S.k; ++t) {
        if (row_out)
          HIP_CHECK(hipMemcpyAsync(row_out + t * cap, S.rk.out_row.as<int64_t>() + t * N, 8 * N, hipMemcpyDeviceToHost, s));
        if (weight_out)
          HIP_CHECK(hipMemcpyAsync(weight_out + t * cap, S.rk.out_w.as<double>() + t * N, 8 * N, hipMemcpyDeviceToHost, s));
      }
    }
    wait_stream(*ctx, s);
    if (n_out) *n_out = N;
  });
}

int stc_lda_important_terms(stc_lda* L, const stc_dcsr* docs, const stc_dscore* score, const int32_t* topic_of,
                            int32_t doc_terms, int32_t topic_terms, int32_t max_out, int32_t* idx_out, double* value_out,
                            int32_t* n_out) {
  return guard([&] {
    STC_REQUIRE(L && docs && score, "lda/docs/score");
    STC_REQUIRE(docs->ctx == L->ctx, "the documents belong to another stc_ctx than the LDA handle");
    STC_REQUIRE(score->ctx == L->ctx, "the score belongs to another stc_ctx than the LDA handle");
    require_single(*L->ctx);
    STC_REQUIRE(doc_terms >= 1 && topic_terms >= 1 && max_out >= 1, "terms: doc_terms, topic_terms and max_out must be >= 1");
    STC_REQUIRE(doc_terms <= 1024, "terms: doc_terms <= 1024");
    if (!L->model.has_topics) throw Error(STC_ERR_STATE, "no topics: call stc_lda_init_random or stc_lda_set_topics");
    STC_REQUIRE(score->k == L->k, "terms: the score has another k than the LDA handle");
    STC_REQUIRE(docs->rows == score->rows, "terms: docs must be the matrix that was scored (another row count)");
    STC_REQUIRE(docs->cols == L->V, "document vectors must have vocab_size columns");
    STC_REQUIRE(L->V < (int64_t(1) << 31), "terms: vocab_size < 2^31");
    const int64_t R = docs->rows;
    const int k = L->k;
    if (topic_of)
      for (int64_t d = 0; d < R; ++d)
        STC_REQUIRE(topic_of[d] >= -1 && topic_of[d] < k, "terms: topic_of entries must be -1 or in [0, k)");
    Ctx& c = *L->ctx;
    c.use();
    hipStream_t s = c.stream;
    gather_lambda(*L);
    if (R == 0) {
      wait_stream(c, s);
      return;
    }
    // S_t as bits: word (t, w >> 5), bit w & 31
    const int64_t W = ceil_div(L->V, 32), N = std::min<int64_t>(topic_terms, L->V);
    DevBuf bits, sel_row, sel_w, topics, ticket, d_idx, d_val, d_n;
    rank::Scratch sc;
    bits.reserve(4 * (size_t)W * k);
    if (N == L->V) {
      HIP_CHECK(hipMemsetAsync(bits.p, 0xFF, 4 * (size_t)W * k, s));
    } else {
      HIP_CHECK(hipMemsetAsync(bits.p, 0, 4 * (size_t)W * k, s));
      sel_row.reserve(8 * (size_t)N * k);
      sel_w.reserve(8 * (size_t)N * k);
      rank::select_columns(s, sc, L->model.lam.p, false, L->V, k, N, nullptr, nullptr, 0, sel_row.as<int64_t>(),
                               sel_w.as<double>());
      k_terms_bits<<<blocks_for(N * k, 256), 256, 0, s>>>(sel_row.as<int64_t>(), N, k, W, bits.as<uint32_t>());
      KERNEL_CHECK();
    }
    const int32_t* d_topic = score->topic.as<int32_t>();
    if (topic_of) {
      topics.reserve(4 * (size_t)R);
      HIP_CHECK(hipMemcpyAsync(topics.p, topic_of, 4 * (size_t)R, hipMemcpyHostToDevice, s));
      d_topic = topics.as<int32_t>();
    }
    ticket.reserve(8);
    HIP_CHECK(hipMemsetAsync(ticket.p, 0, 8, s));
    const int64_t total = R * max_out;
    d_idx.reserve(4 * (size_t)total);
    d_val.reserve(8 * (size_t)total);
    d_n.reserve(4 * (size_t)R);
    if (docs->dtype == STC_F32)
      launch_terms<float>(s, c, *docs, d_topic, bits.as<uint32_t>(), W, doc_terms, max_out, ticket.as<unsigned long long>(),
                          d_idx.as<int32_t>(), d_val.as<double>(), d_n.as<int32_t>());
    else
      launch_terms<double>(s, c, *docs, d_topic, bits.as<uint32_t>(), W, doc_terms, max_out, ticket.as<unsigned long long>(),
                           d_idx.as<int32_t>(), d_val.as<double>(), d_n.as<int32_t>());
    if (idx_out) HIP_CHECK(hipMemcpyAsync(idx_out, d_idx.p, 4 * (size_t)total, hipMemcpyDeviceToHost, s));
    if (value_out) HIP_CHECK(hipMemcpyAsync(value_out, d_val.p, 8 * (size_t)total, hipMemcpyDeviceToHost, s));
    if (n_out) HIP_CHECK(hipMemcpyAsync(n_out, d_n.p, 4 * (size_t)R, hipMemcpyDeviceToHost, s));
    wait_stream(c, s);
  });
}

}  // extern "C"
