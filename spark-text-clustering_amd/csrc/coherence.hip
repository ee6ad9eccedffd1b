// coherence.hip — topic coherence (include/stc.h "Topic coherence"): the document co-occurrence counts of the
// topics' top terms over a resident corpus (gfx950), and the two measures computed from them on the host.
//
// The reference judges a model by reading each topic's top terms (LDALoader.scala:66-69, 177-187); UMass
// (Mimno et al. 2011) and document-level NPMI put a number on "these terms occur together".  Both are
// functions of df[t][i] and codf[t][i][j] alone, so the device does one integer pass over the corpus and
// everything with a logarithm in it stays on the host.
//
// The pass:
//   slot index   the k·n slots (term, t·64 + i) sorted by term on the host (at most 2^18 of them, and they come
//                from the host), uploaded; first[w] = the first sorted position holding term w, −1 for a term
//                without a slot: one 4-byte gather per corpus entry, a second read only on a hit.
//   k_count      one wave per document, documents drawn sixteen at a time from a ticket counter.  Lanes stride
//                over the row; a hit ORs bit i into the wave's LDS mask[t] and, when the mask was empty, appends
//                t to the wave's touched list.  Then (touched topic, set bit j) pairs spread over the lanes add 1
//                to count[t][j(j+1)/2 + i] for every set bit i <= j, and the touched masks are cleared: a
//                document costs its hits, not k.  The u32 counters are private to the workgroup in LDS when
//                they fit beside the masks of at least four waves, else in slabs in global memory shared by
//                as few workgroups as the slab budget allows.
//   k_reduce     sums the partial triangles into int64 and mirrors them; the diagonal is df.
// Integer adds only: any order gives the same counts, so the result is exact and the same bytes every run.
#include <algorithm>
#include <cmath>

#include "coherence_host.h"
#include "collectives.h"
#include "stc_handles.h"

using namespace stc;

namespace stc {
namespace coherence {

constexpr int kMaxN = 64;                  // one u64 mask per (wave, topic)
constexpr int kMaxK = 4096;                // slot = t·64 + i fits 18 bits
constexpr int64_t kLds = 160 * 1024;       // a CU's LDS, all of it one workgroup's when needed
constexpr int kMaxWaves = 16;
constexpr int kMinLdsWaves = 4;            // fewer waves than this beside LDS counters: the slabs instead
constexpr int kChunk = 16;                 // documents per ticket
constexpr int kUnroll = 4;                 // entries per lane and step of a row
constexpr int64_t kSlabBudget = int64_t(256) << 20;  // bytes of global counter slabs per call

struct Plan {
  bool lds;       // the counters live in LDS
  int waves;      // per workgroup
  size_t bytes;   // dynamic LDS per workgroup
};

// per wave: k u64 masks + k i32 touched + its touched count; the counters: k·n(n+1)/2 u32
static Plan plan(int k, int n) {
  const int64_t tri = (int64_t)n * (n + 1) / 2, per_wave = 12 * (int64_t)k + 4, cnt = 4 * (int64_t)k * tri;
  Plan p;
  const int64_t w = cnt < kLds ? (kLds - cnt) / per_wave : 0;
  p.lds = w >= kMinLdsWaves;
  p.waves = (int)std::min<int64_t>(kMaxWaves, p.lds ? w : kLds / per_wave);  // k = 4096: 3 waves
  p.bytes = (size_t)(p.waves * per_wave + (p.lds ? cnt : 0));
  return p;
}

__global__ __launch_bounds__(256) void k_first(const int2* __restrict__ slots, int n_slots, int32_t* __restrict__ first) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n_slots) return;
  const int w = slots[p].x;
  if (p == 0 || slots[p - 1].x != w) first[w] = p;
}

// one wave wrote LDS and reads it back across its lanes: LDS is in order per wave, the compiler must be too
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

template <typename V>
__global__ __launch_bounds__(kMaxWaves * 64) void k_count(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx, const V* __restrict__ val /* nullptr: all > 0 */,
    int64_t rows, const int32_t* __restrict__ first, const int2* __restrict__ slots, int n_slots, int k, int n,
    int lds_counters, uint32_t* __restrict__ part, int64_t n_slabs, unsigned long long* __restrict__ ticket) {
  extern __shared__ unsigned long long smem[];
  const int tid = threadIdx.x, W = blockDim.x >> 6, wave = tid >> 6, lane = tid & 63;
  const int tri = n * (n + 1) / 2, kt = k * tri;
  unsigned long long* mask = smem + (size_t)wave * k;               // [W][k]
  int32_t* touched_all = reinterpret_cast<int32_t*>(smem + (size_t)W * k);
  int32_t* touched = touched_all + (size_t)wave * k;                // [W][k]
  int32_t* nt = touched_all + (size_t)W * k;                        // [W]
  uint32_t* lcnt = reinterpret_cast<uint32_t*>(nt + W);             // [k·tri] when lds_counters
  for (int i = tid; i < W * k; i += blockDim.x) smem[i] = 0;
  if (tid < W) nt[tid] = 0;
  if (lds_counters)
    for (int i = tid; i < kt; i += blockDim.x) lcnt[i] = 0;
  __syncthreads();
  uint32_t* gcnt = part + ((int64_t)blockIdx.x % n_slabs) * kt;

  for (;;) {
    unsigned long long d0 = 0;
    if (lane == 0) d0 = atomicAdd(ticket, (unsigned long long)kChunk);
    d0 = __shfl(d0, 0);
    if (d0 >= (unsigned long long)rows) break;
    const int nd = (int)std::min<int64_t>(kChunk, rows - (int64_t)d0);
    const int64_t ip = lane <= nd ? indptr[(int64_t)d0 + lane] : 0;  // kChunk + 1 <= 64 lanes
    for (int r = 0; r < nd; ++r) {
      const int64_t e0 = __shfl(ip, r), e1 = __shfl(ip, r + 1);
      // kUnroll entries per lane and step, every load of a stage issued before the first use: a wave works on one
      // short document at a time, so its memory parallelism has to come from inside the row
      for (int64_t eb = e0 + lane; eb < e1; eb += 64 * kUnroll) {
        int32_t w[kUnroll];
        V v[kUnroll];
        int p[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) w[u] = eb + 64 * u < e1 ? idx[eb + 64 * u] : -1;
        if (val != nullptr) {
#pragma unroll
          for (int u = 0; u < kUnroll; ++u) v[u] = eb + 64 * u < e1 ? val[eb + 64 * u] : V(0);
#pragma unroll
          for (int u = 0; u < kUnroll; ++u)
            if (!(v[u] > V(0))) w[u] = -1;  // zeros, negatives and NaN are not occurrences
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) p[u] = w[u] >= 0 ? first[w[u]] : -1;
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          if (p[u] < 0) continue;
          for (int q = p[u]; q < n_slots; ++q) {
            const int2 s = slots[q];
            if (s.x != w[u]) break;
            const int t = s.y >> 6;
            if (atomicOr(&mask[t], 1ull << (s.y & 63)) == 0) touched[atomicAdd(&nt[wave], 1)] = t;
          }
        }
      }
      wave_sync();
      const int ntw = nt[wave];
      if (ntw == 0) continue;
      for (int q = lane; q < ntw * n; q += 64) {  // (touched topic, bit j): add the pairs i <= j
        const int t = touched[q / n], j = q % n;
        const unsigned long long m = mask[t];
        if (!((m >> j) & 1ull)) continue;
        unsigned long long lo = m & (~0ull >> (63 - j));
        const int base = t * tri + j * (j + 1) / 2;
        while (lo) {
          const int i = __ffsll((long long)lo) - 1;
          lo &= lo - 1;
          if (lds_counters)
            atomicAdd(&lcnt[base + i], 1u);
          else
            atomicAdd(&gcnt[base + i], 1u);
        }
      }
      wave_sync();
      for (int q = lane; q < ntw; q += 64) mask[touched[q]] = 0;
      if (lane == 0) nt[wave] = 0;
      wave_sync();
    }
  }
  if (lds_counters) {
    __syncthreads();
    uint32_t* out = part + (int64_t)blockIdx.x * kt;
    for (int i = tid; i < kt; i += blockDim.x) out[i] = lcnt[i];
  }
}

// codf[t][i][j] = Σ_g part[g][t][tri(min, max)], df[t][i] = codf[t][i][i]
__global__ __launch_bounds__(256) void k_reduce(const uint32_t* __restrict__ part, int64_t n_part, int k, int n,
                                                int64_t* __restrict__ df, int64_t* __restrict__ codf) {
  const int64_t total = (int64_t)k * n * n, kt = (int64_t)k * (n * (n + 1) / 2);
  for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
    const int j = (int)(o % n), i = (int)((o / n) % n);
    const int64_t t = o / ((int64_t)n * n);
    const int a = i < j ? i : j, b = i < j ? j : i;
    const int64_t src = t * (n * (n + 1) / 2) + b * (b + 1) / 2 + a;
    int64_t s = 0;
    for (int64_t g = 0; g < n_part; ++g) s += part[g * kt + src];
    codf[o] = s;
    if (i == j) df[t * n + i] = s;
  }
}

static void count(Ctx& c, const DCsr& m, const int32_t* terms, int k, int n, int64_t* df_out, int64_t* codf_out) {
  hipStream_t s = c.stream;
  const int64_t kn = (int64_t)k * n, knn = kn * n, kt = (int64_t)k * (n * (n + 1) / 2);
  std::vector<int2> slots;
  slots.reserve((size_t)kn);
  for (int64_t q = 0; q < kn; ++q) {
    const int32_t w = terms[q];
    if (w == -1) continue;
    if (w < 0 || (int64_t)w >= m.cols)
      throw Error(STC_ERR_INVALID_ARG, "coherence: terms[" + std::to_string(q) + "] = " + std::to_string(w) +
                                           " is neither -1 nor a column of the matrix (" + std::to_string(m.cols) + ")");
    slots.push_back(make_int2(w, (int)((q / n) * 64 + q % n)));
  }
  std::sort(slots.begin(), slots.end(), [](const int2& a, const int2& b) { return a.x != b.x ? a.x < b.x : a.y < b.y; });
  const int n_slots = (int)slots.size();
  if (n_slots == 0 || m.nnz == 0 || m.rows == 0) {
    if (df_out) std::fill(df_out, df_out + kn, int64_t(0));
    if (codf_out) std::fill(codf_out, codf_out + knn, int64_t(0));
    wait_stream(c, s);
    return;
  }
  const Plan p = plan(k, n);
  // at most kMaxWaves waves per CU: two 16-wave workgroups per CU ran the planted corpus's top-10 count 3.3 times
  // slower than one (8.96 against 2.69 ms)
  const int wg_per_cu = (int)std::max<int64_t>(1, std::min<int64_t>(kLds / (int64_t)p.bytes, kMaxWaves / p.waves));
  const int64_t G = std::max<int64_t>(
      1, std::min<int64_t>((int64_t)c.cus * wg_per_cu, ceil_div(ceil_div(m.rows, (int64_t)kChunk), (int64_t)p.waves)));
  const int64_t n_part = p.lds ? G : std::max<int64_t>(1, std::min<int64_t>(G, kSlabBudget / (4 * kt)));

  DevBuf& part = c.scratch[0];
  DevBuf& first = c.scratch[1];
  DevBuf& dslots = c.scratch[2];  // [0, 8): the ticket; the slots behind it
  DevBuf& out = c.scratch[3];     // df (k·n), then codf (k·n·n)
  part.reserve(4 * (size_t)(n_part * kt));
  first.reserve(4 * (size_t)m.cols);
  dslots.reserve(8 + 8 * (size_t)n_slots);
  out.reserve(8 * (size_t)(kn + knn));
  auto* ticket = dslots.as<unsigned long long>();
  const int2* d_slots = reinterpret_cast<const int2*>(ticket + 1);
  HIP_CHECK(hipMemsetAsync(ticket, 0, 8, s));
  HIP_CHECK(hipMemcpyAsync((void*)d_slots, slots.data(), 8 * (size_t)n_slots, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemsetAsync(first.p, 0xFF, 4 * (size_t)m.cols, s));  // −1: no slot
  k_first<<<blocks_for(n_slots), 256, 0, s>>>(d_slots, n_slots, first.as<int32_t>());
  KERNEL_CHECK();
  if (!p.lds) HIP_CHECK(hipMemsetAsync(part.p, 0, 4 * (size_t)(n_part * kt), s));
  const unsigned threads = 64u * (unsigned)p.waves;
  if (m.dtype == STC_F32) {
    HIP_CHECK(hipFuncSetAttribute((const void*)k_count<float>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.bytes));
    k_count<float><<<(unsigned)G, threads, p.bytes, s>>>(
        m.indptr.as<int64_t>(), m.indices.as<int32_t>(), m.positive ? nullptr : m.values.as<float>(), m.rows,
        first.as<int32_t>(), d_slots, n_slots, k, n, p.lds ? 1 : 0, part.as<uint32_t>(), n_part, ticket);
  } else {
    HIP_CHECK(hipFuncSetAttribute((const void*)k_count<double>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.bytes));
    k_count<double><<<(unsigned)G, threads, p.bytes, s>>>(
        m.indptr.as<int64_t>(), m.indices.as<int32_t>(), m.positive ? nullptr : m.values.as<double>(), m.rows,
        first.as<int32_t>(), d_slots, n_slots, k, n, p.lds ? 1 : 0, part.as<uint32_t>(), n_part, ticket);
  }
  KERNEL_CHECK();
  int64_t* d_df = out.as<int64_t>();
  int64_t* d_codf = d_df + kn;
  k_reduce<<<(unsigned)std::min<int64_t>(ceil_div(knn, 256), 8192), 256, 0, s>>>(part.as<uint32_t>(), n_part, k, n, d_df,
                                                                               d_codf);
  KERNEL_CHECK();
  if (df_out) HIP_CHECK(hipMemcpyAsync(df_out, d_df, 8 * (size_t)kn, hipMemcpyDeviceToHost, s));
  if (codf_out) HIP_CHECK(hipMemcpyAsync(codf_out, d_codf, 8 * (size_t)knn, hipMemcpyDeviceToHost, s));
  wait_stream(c, s);  // (the host slot list is read by its copy until here)
}

}  // namespace coherence
}  // namespace stc

extern "C" {

int stc_term_cooccurrence(stc_ctx* ctx, const stc_dcsr* docs, const int32_t* terms, int32_t k, int32_t n, int64_t* df_out,
                          int64_t* codf_out, int64_t* n_docs_out) {
  return guard([&] {
    STC_REQUIRE(ctx && docs && terms, "ctx/docs/terms");
    STC_REQUIRE(docs->ctx == ctx, "the matrix belongs to another stc_ctx");
    STC_REQUIRE(n >= 1 && n <= coherence::kMaxN, "coherence: 1 <= n <= 64 terms per topic");
    STC_REQUIRE(k >= 1 && k <= coherence::kMaxK, "coherence: 1 <= k <= 4096 topics");
    STC_REQUIRE(docs->rows < (int64_t(1) << 32), "coherence: fewer than 2^32 documents per call");
    if (ctx->coll())
      throw Error(STC_ERR_STATE, "coherence: the context is connected to other ranks (the count is single-device)");
    ctx->use();
    coherence::count(*ctx, *docs, terms, k, n, df_out, codf_out);  // (waits for the stream)
    if (n_docs_out) *n_docs_out = docs->rows;
  });
}

int stc_coherence(const int64_t* df, const int64_t* codf, int32_t k, int32_t n, int64_t n_docs, int measure, double eps,
                  double* topic_out, int32_t* pairs_out) {
  return guard([&] {
    const char* bad = coherence::measure_topics(df, codf, k, n, n_docs, measure, eps, topic_out, pairs_out);
    STC_REQUIRE(bad == nullptr, bad);
  });
}

}  // extern "C"
