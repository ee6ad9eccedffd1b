// rank.hip — ranked queries over a resident matrix (rank.h): selection instead of a sort.
//
// Column selection (describeTopics, topDocumentsPerTopic, the important terms' S_t): per topic the N largest of R
// values, ordered by (value descending, row ascending).  Every entry has rank_key.h's 96-bit key (the value's
// order-preserving bits, ~row); all keys of a column are distinct, and the contract's order is the keys' descending
// order.  A most-significant-digit radix selection over that key, 8 bits per pass, 12 passes at most:
//   k_rank_hist   a block reads a tile of kTileRows rows × up to kTopicGroup topics (row segments, coalesced),
//                 counts the current digit of the entries that match the topic's selected prefix in LDS
//                 (integer atomics) and adds its non-zero counters to the topic's global histogram.
//   k_rank_scan   per topic: rank_key.h's digit pick finds the digit that holds the N-th key; it is appended to
//                 the prefix and the histogram cleared.  A topic is done once the keys at or above its prefix
//                 number at most N + kSlack (they fit the candidate list), at the latest after the last digit,
//                 when they number exactly N.  A block all of whose topics are done returns before it reads
//                 anything.
//   k_rank_collect appends every key at or above the prefix to the topic's candidate list (an integer
//                 counter; the list is unordered).
//   k_rank_sort   one block per topic: rank_key.h's bitonic sort of the candidates by the key (in LDS up to
//                 kLdsSort entries, else in the list itself), then the first N leave in the contract's order.
// Counts are integers and the final order is a total order of distinct keys, so the result depends on the
// matrix alone: not on the grid, the tile, timing or the order of the atomics.  A pass reads R·k·sizeof(T)
// bytes (+ 8R in the row-normalised mode); nothing of the matrix is copied, scratch is k·(256 counters +
// a prefix) + k·P candidates + R row sums.  All element offsets are int64.
//
// Row sums (the normalised mode and topTopics' weights): one thread per row, j ascending — the sequential
// order, whatever k.
//
// Row selection (topTopicsPerDocument): the EM pass's lane layouts (lda_em.hip) — KP lanes per row and 64/KP
// rows per wave for k <= 64, NS register slices of 64 topics above — and N rounds of rank_key.h's (value, index)
// butterfly; the winner's owner retires it.
#include "rank.h"

#include "collectives.h"
#include "rank_key.h"
#include "stc_handles.h"

namespace stc {
namespace rank {

namespace {

constexpr int kTileRows = 512;    // rows of one block's tile
constexpr int kTopicGroup = 32;   // topics of one block: 32 × 257 counters = 32.1 KiB of LDS
constexpr int kHistStride = 257;  // a topic's 256 counters + 1: topic t's digit d sits on bank (t + d) mod 32
constexpr int kSlack = 512;       // candidates a topic may keep beyond N (ends the passes early)
constexpr int kLdsSort = 2048;    // candidates sorted in LDS (24 KiB); more are sorted in global memory

struct Sel {
  Prefix prefix;     // the digits selected so far
  uint32_t above;    // keys strictly above the prefix
  uint32_t done;
  uint32_t count;    // k_rank_collect's append counter
};

// entry (r, t)'s key; false: row r is no candidate
template <typename T, bool NORM>
__device__ inline bool make_key(const T* __restrict__ m, const double* __restrict__ rowsum, int64_t r, int t, int k,
                                uint64_t& hi, uint32_t& lo) {
  double x = (double)m[r * k + t];
  if (NORM) {
    const double s = rowsum[r];
    if (s < 0.0) return false;
    if (s > 0.0) x = x / s;
  }
  hi = value_key(x);
  lo = ~(uint32_t)r;
  return true;
}

// the block's topics' selection state → LDS; whether any of them still selects
__device__ inline bool load_group(const Sel* __restrict__ sel, int tg, int width, Sel* s_sel) {
  const bool live = (int)threadIdx.x < width;
  if (live) s_sel[threadIdx.x] = sel[tg + threadIdx.x];
  return __syncthreads_or(live && !s_sel[threadIdx.x].done);
}

template <typename T, bool NORM>
__global__ __launch_bounds__(256) void k_rank_hist(const T* __restrict__ m, const double* __restrict__ rowsum, int64_t R,
                                                   int k, const Sel* __restrict__ sel, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[kTopicGroup * kHistStride];
  __shared__ Sel s_sel[kTopicGroup];
  const int tg = blockIdx.y * kTopicGroup, width = min(k - tg, kTopicGroup);
  if (!load_group(sel, tg, width, s_sel)) return;  // block-uniform
  for (int i = threadIdx.x; i < kTopicGroup * kHistStride; i += 256) h[i] = 0;
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * kTileRows;
  const int rows = (int)min((int64_t)kTileRows, R - r0);
  for (int e = threadIdx.x; e < rows * width; e += 256) {  // a row's `width` topics are contiguous
    const int rl = e / width, tl = e - rl * width;
    const Sel& s = s_sel[tl];
    if (s.done) continue;
    uint64_t hi;
    uint32_t lo;
    if (!make_key<T, NORM>(m, rowsum, r0 + rl, tg + tl, k, hi, lo)) continue;
    if (s.prefix.matches(hi, lo)) atomicAdd(&h[tl * kHistStride + s.prefix.digit(hi, lo)], 1u);
  }
  __syncthreads();
  for (int tl = 0; tl < width; ++tl) {
    const uint32_t c = h[tl * kHistStride + threadIdx.x];
    if (c) atomicAdd(&hist[(int64_t)(tg + tl) * 256 + threadIdx.x], c);
  }
}

// cap: the candidate list's capacity, N + kSlack
__global__ __launch_bounds__(256) void k_rank_scan(Sel* __restrict__ sel, uint32_t* __restrict__ hist, uint32_t N,
                                                   uint32_t cap) {
  __shared__ uint32_t h[256];
  const int t = blockIdx.x;
  if (sel[t].done) return;  // block-uniform
  h[threadIdx.x] = hist[(int64_t)t * 256 + threadIdx.x];
  hist[(int64_t)t * 256 + threadIdx.x] = 0;
  __syncthreads();
  if (threadIdx.x >= 64) return;
  Sel s = sel[t];
  const DigitPick p = pick_digit(h, 1, 0, s.above, N);  // digit 0 if the counts fall short (they do not)
  s.prefix.append(p.digit);
  s.above = p.above;
  s.done = s.prefix.done(p.above + p.in_digit, cap) ? 1u : 0u;
  if (threadIdx.x == 0) sel[t] = s;
}

template <typename T, bool NORM>
__global__ __launch_bounds__(256) void k_rank_collect(const T* __restrict__ m, const double* __restrict__ rowsum,
                                                      int64_t R, int k, Sel* __restrict__ sel, uint32_t P,
                                                      uint64_t* __restrict__ cand_key, uint32_t* __restrict__ cand_row) {
  __shared__ Sel s_sel[kTopicGroup];
  const int tg = blockIdx.y * kTopicGroup, width = min(k - tg, kTopicGroup);
  if ((int)threadIdx.x < width) s_sel[threadIdx.x] = sel[tg + threadIdx.x];
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * kTileRows;
  const int rows = (int)min((int64_t)kTileRows, R - r0);
  for (int e = threadIdx.x; e < rows * width; e += 256) {
    const int rl = e / width, tl = e - rl * width;
    uint64_t hi;
    uint32_t lo;
    if (!make_key<T, NORM>(m, rowsum, r0 + rl, tg + tl, k, hi, lo)) continue;
    if (!s_sel[tl].prefix.at_or_above(hi, lo)) continue;
    const uint32_t pos = atomicAdd(&sel[tg + tl].count, 1u);
    if (pos < P) {  // always: a done topic has at most N + kSlack <= P such keys
      cand_key[(int64_t)(tg + tl) * P + pos] = hi;
      cand_row[(int64_t)(tg + tl) * P + pos] = (uint32_t)(r0 + rl);
    }
  }
}

// P: a power of two >= the topic's candidates
__global__ __launch_bounds__(256) void k_rank_sort(const Sel* __restrict__ sel, uint32_t P, uint64_t* __restrict__ cand_key,
                                                   uint32_t* __restrict__ cand_row, uint32_t N,
                                                   const double* __restrict__ nk, int64_t row0,
                                                   int64_t* __restrict__ out_row, double* __restrict__ out_w) {
  __shared__ uint64_t s_key[kLdsSort];
  __shared__ uint32_t s_row[kLdsSort];
  const int t = blockIdx.x;
  const uint32_t n = min(sel[t].count, P);
  uint64_t* gk = cand_key + (int64_t)t * P;
  uint32_t* gr = cand_row + (int64_t)t * P;
  const bool in_lds = P <= (uint32_t)kLdsSort;  // block-uniform
  // padding sorts behind every key (a row is below 2^31)
  if (in_lds) {
    for (uint32_t i = threadIdx.x; i < P; i += 256) {
      s_key[i] = i < n ? gk[i] : 0ull;
      s_row[i] = i < n ? gr[i] : 0xFFFFFFFFu;
    }
    __syncthreads();
    block_bitonic_sort(s_key, s_row, P);
  } else {
    for (uint32_t i = n + threadIdx.x; i < P; i += 256) {
      gk[i] = 0ull;
      gr[i] = 0xFFFFFFFFu;
    }
    __syncthreads();
    block_bitonic_sort(gk, gr, P);
  }
  for (uint32_t i = threadIdx.x; i < N; i += 256) {
    const double v = key_value(in_lds ? s_key[i] : gk[i]);
    out_row[(int64_t)t * N + i] = row0 + (int64_t)(in_lds ? s_row[i] : gr[i]);
    out_w[(int64_t)t * N + i] = nk ? v / nk[t] : v;
  }
}

template <typename T>
__global__ void k_rank_rowsum(const T* __restrict__ m, const int64_t* __restrict__ ptr, int64_t R, int k,
                              double* __restrict__ rowsum) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  if (ptr && ptr[r + 1] == ptr[r]) {
    rowsum[r] = -1.0;
    return;
  }
  const T* row = m + r * k;
  double s = 0.0;
  for (int j = 0; j < k; ++j) s += (double)row[j];
  rowsum[r] = s;
}

__global__ void k_rank_count(const int64_t* __restrict__ ptr, int64_t R, unsigned long long* __restrict__ count) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool v = r < R && ptr[r + 1] > ptr[r];
  const unsigned long long b = __ballot(v);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(count, (unsigned long long)__popcll(b));
}

// lane = row slot × KP + topic (KP < 64), or NS slices of 64 topics per lane (KP = 64): lda_em.hip's layouts
template <typename T, int KP, int NS>
__global__ __launch_bounds__(256) void k_rank_rows(const T* __restrict__ m, const double* __restrict__ rowsum, int64_t R,
                                                   int k, int N, int32_t* __restrict__ out_idx,
                                                   double* __restrict__ out_w) {
  constexpr int G = 64 / KP;
  const int lane = threadIdx.x & 63;
  const int j0 = lane % KP, slot = lane / KP;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wave * G >= R) return;  // wave-uniform
  const int64_t r = wave * G + slot;
  const bool valid = r < R;
  double x[NS];  // a padding lane, an empty slot and a retired entry carry −1, below every count
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int j = j0 + 64 * i;
    x[i] = (valid && j < k) ? (double)m[r * k + j] : -1.0;
  }
  const double s = valid ? rowsum[r] : 0.0;
  for (int n = 0; n < N; ++n) {  // wave-uniform trip count
    double best = -1.0;
    int bj = j0;
#pragma unroll
    for (int i = 0; i < NS; ++i) {  // ascending j, strict >: the first maximum of this lane
      const bool up = x[i] > best;
      best = up ? x[i] : best;
      bj = up ? j0 + 64 * i : bj;
    }
    row_argmax<false>(KP, best, bj);  // the row's lanes: larger value, then smaller index
#pragma unroll
    for (int i = 0; i < NS; ++i)
      if (j0 + 64 * i == bj) x[i] = -1.0;
    if (valid && j0 == 0) {
      out_idx[r * N + n] = bj;
      out_w[r * N + n] = s > 0.0 ? best / s : best;
    }
  }
}

template <typename T, bool NORM>
void select_columns_as(hipStream_t s, Scratch& sc, const T* m, int64_t R, int k, int64_t N, const double* rowsum,
                       const double* nk, int64_t row0, int64_t* out_row, double* out_w) {
  uint32_t P = 2;
  while ((int64_t)P < N + kSlack) P <<= 1;
  sc.sel.reserve(sizeof(Sel) * (size_t)k);
  sc.hist.reserve(4 * 256 * (size_t)k);
  sc.cand_key.reserve(8 * (size_t)P * k);
  sc.cand_row.reserve(4 * (size_t)P * k);
  Sel* sel = sc.sel.as<Sel>();
  uint32_t* hist = sc.hist.as<uint32_t>();
  HIP_CHECK(hipMemsetAsync(sel, 0, sizeof(Sel) * (size_t)k, s));
  HIP_CHECK(hipMemsetAsync(hist, 0, 4 * 256 * (size_t)k, s));
  const dim3 grid(blocks_for(R, kTileRows), (unsigned)ceil_div(k, kTopicGroup));
  for (int d = 0; d < kDigits; ++d) {
    k_rank_hist<T, NORM><<<grid, 256, 0, s>>>(m, rowsum, R, k, sel, hist);
    KERNEL_CHECK();
    k_rank_scan<<<(unsigned)k, 256, 0, s>>>(sel, hist, (uint32_t)N, (uint32_t)(N + kSlack));
    KERNEL_CHECK();
  }
  k_rank_collect<T, NORM><<<grid, 256, 0, s>>>(m, rowsum, R, k, sel, P, sc.cand_key.as<uint64_t>(),
                                               sc.cand_row.as<uint32_t>());
  KERNEL_CHECK();
  k_rank_sort<<<(unsigned)k, 256, 0, s>>>(sel, P, sc.cand_key.as<uint64_t>(), sc.cand_row.as<uint32_t>(), (uint32_t)N, nk,
                                          row0, out_row, out_w);
  KERNEL_CHECK();
}

template <typename T>
void select_rows_as(hipStream_t s, const T* m, const double* rowsum, int64_t R, int k, int N, int32_t* out_idx,
                    double* out_w) {
  const int kp = pow2_at_least(k);
  const int G = kp < 64 ? 64 / kp : 1;
  const unsigned grid = blocks_for(ceil_div(R, G), 4);
#define STC_RANK_CASE(KP, NS)                                                        \
  k_rank_rows<T, KP, NS><<<grid, 256, 0, s>>>(m, rowsum, R, k, N, out_idx, out_w);   \
  break
  switch (kp) {
    case 2: STC_RANK_CASE(2, 1);
    case 4: STC_RANK_CASE(4, 1);
    case 8: STC_RANK_CASE(8, 1);
    case 16: STC_RANK_CASE(16, 1);
    case 32: STC_RANK_CASE(32, 1);
    case 64: STC_RANK_CASE(64, 1);
    case 128: STC_RANK_CASE(64, 2);
    case 256: STC_RANK_CASE(64, 4);
    case 512: STC_RANK_CASE(64, 8);
    case 1024: STC_RANK_CASE(64, 16);
    default: throw Error(STC_ERR_INVALID_ARG, "em: k out of range");
  }
#undef STC_RANK_CASE
  KERNEL_CHECK();
}

}  // namespace

void row_sums(hipStream_t s, const void* m, bool f32, const int64_t* ptr, int64_t R, int k, double* rowsum) {
  if (R == 0) return;
  if (f32) k_rank_rowsum<float><<<blocks_for(R, 256), 256, 0, s>>>((const float*)m, ptr, R, k, rowsum);
  else k_rank_rowsum<double><<<blocks_for(R, 256), 256, 0, s>>>((const double*)m, ptr, R, k, rowsum);
  KERNEL_CHECK();
}

void count_vertices(hipStream_t s, const int64_t* ptr, int64_t R, int64_t* count) {
  HIP_CHECK(hipMemsetAsync(count, 0, 8, s));
  if (R == 0) return;
  k_rank_count<<<blocks_for(R, 256), 256, 0, s>>>(ptr, R, (unsigned long long*)count);
  KERNEL_CHECK();
}

void select_columns(hipStream_t s, Scratch& sc, const void* m, bool f32, int64_t R, int k, int64_t N,
                    const double* rowsum, const double* nk, int64_t row0, int64_t* out_row, double* out_w) {
  STC_REQUIRE(N >= 1 && N <= R && R < (int64_t(1) << 31), "em rank: 1 <= N <= rows < 2^31");
  if (f32) {
    if (rowsum) select_columns_as<float, true>(s, sc, (const float*)m, R, k, N, rowsum, nullptr, row0, out_row, out_w);
    else select_columns_as<float, false>(s, sc, (const float*)m, R, k, N, nullptr, nk, row0, out_row, out_w);
  } else {
    if (rowsum) select_columns_as<double, true>(s, sc, (const double*)m, R, k, N, rowsum, nullptr, row0, out_row, out_w);
    else select_columns_as<double, false>(s, sc, (const double*)m, R, k, N, nullptr, nk, row0, out_row, out_w);
  }
}

void describe_columns(Ctx& c, Scratch& sc, const void* m, bool f32, int64_t R, int k, int64_t N, const double* nk,
                      int32_t* idx_out, double* weight_out) {
  hipStream_t s = c.stream;
  const int64_t total = N * k;
  sc.out_row.reserve(8 * total);
  sc.out_w.reserve(8 * total);
  select_columns(s, sc, m, f32, R, k, N, nullptr, nk, 0, sc.out_row.as<int64_t>(), sc.out_w.as<double>());
  std::vector<int64_t> rows((size_t)total);
  HIP_CHECK(hipMemcpyAsync(rows.data(), sc.out_row.p, 8 * total, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(weight_out, sc.out_w.p, 8 * total, hipMemcpyDeviceToHost, s));
  wait_stream(c, s);
  std::copy(rows.begin(), rows.end(), idx_out);
}

void select_rows(hipStream_t s, const void* m, bool f32, const double* rowsum, int64_t R, int k, int N,
                 int32_t* out_idx, double* out_w) {
  if (R == 0) return;
  STC_REQUIRE(N >= 1 && N <= k, "em rank: 1 <= N <= k");
  if (f32) select_rows_as<float>(s, (const float*)m, rowsum, R, k, N, out_idx, out_w);
  else select_rows_as<double>(s, (const double*)m, rowsum, R, k, N, out_idx, out_w);
}

}  // namespace rank
}  // namespace stc
