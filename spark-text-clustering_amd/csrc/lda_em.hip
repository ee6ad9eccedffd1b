// lda_em.hip — [U] EMLDAOptimizer / DistributedLDAModel on the GPU (stc_em_*, include/stc.h).
//
// The corpus is a bipartite graph: every CSR entry (d, w, c ≠ 0) is an edge between document vertex d and
// term vertex w.  State: N_dk (D×k), N_wk (V×k), N_k = Σ_w N_wk.  One iteration sends along every edge the
// message c·γ with γ_j ∝ (N_wk[w][j] + η−1)(N_dk[d][j] + α−1) / (N_k[j] + V(η−1)), normalised over j, and
// every vertex's new counts are the sum of the messages of its edges.
//
// The graph never changes, so create() builds it once in both orientations (the filtered CSR and its
// transpose by a stable radix sort) and an iteration is the same kernel run twice: over rows (→ N_dk',
// gathering N_wk rows) and over columns (→ N_wk', gathering N_dk rows).  Each run recomputes γ; the E×k
// messages are never stored.  logLikelihood and topicAssignments are the row run in further modes (a scalar
// per chunk; per edge the first topic with the largest γ).
//
// Reproducibility: no float atomics.  A vertex's edge list is cut into chunks of kChunk edges; one wave
// sums one chunk (topics across lanes; for k < 64 several edges side by side, folded in a fixed lane
// order) and writes the partial with plain stores; k_em_fixup adds a vertex's partials in chunk order.
// N_k and the two scalars of logLikelihood / logPrior are fixed-shape two-level reductions.  Nothing
// depends on the grid size or on timing.
//
// Several devices (lda_em.h, em_group.hip): a member holds a contiguous shard of the documents with all V
// columns.  Its row pass is the single handle's; its column pass sums the messages of its own edges into
// N_wk' (a term without a local edge: a 0 row), the members' N_wk' are all-reduced, and N_k / inv follow on
// every member from the same sum.  The RNG keys of kInit continue the global CSR order (pos_base), and a
// term vertex exists iff any member has an edge of it (gdeg, all-reduced once at create).
//
// State storage (stc_em_create_as): N_dk / N_wk are double or float arrays.  The kernels that touch them are
// templates on that type; a load widens to double, a store of a new element rounds it once, and everything
// else — counts, α, η, N_k, inv, γ, accumulators, partials, the scalars — is fp64 in the same order in both
// instantiations.  N_k is the fp64 column sum of the stored N_wk.
//
// Ranked queries (describe, top_documents, top_topics): selections over the resident state by rank.hip's
// kernels; this file sizes their scratch, feeds them the state's buffers and copies the lists out.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <vector>

#include "collectives.h"
#include "lda_em.h"
#include "rank.h"
#include "rank_key.h"
#include "stc_handles.h"

namespace stc {
namespace em {

namespace {

constexpr int kChunk = 256;      // edges of one vertex summed by one wave
constexpr int kSumRows = 2048;   // N_wk rows per block of the N_k reduction's first level
constexpr int kSumElems = 4096;  // elements per block of a scalar reduction's first level

// one orientation of the graph: vertices × their edges (the other endpoint, the count)
struct Side {
  int64_t n = 0;                 // vertices (D or V)
  int64_t n_chunks = 0, n_multi = 0;
  DevBuf ptr;                    // int64[n+1]
  DevBuf idx;                    // int32[E] the other endpoint
  DevBuf cnt;                    // double[E]
  DevBuf pos;                    // int64[E] the edge's position in CSR order (columns only; rows: identity)
  DevBuf chunk_vertex;           // int32[n_chunks]
  DevBuf choff;                  // int64[n+1] first chunk of each vertex
  DevBuf moff;                   // int64[n+1] first partial slot of each vertex with more than one chunk
};

struct SideView {
  const int64_t* ptr;
  const int32_t* idx;
  const double* cnt;
  const int64_t* pos;
  const int32_t* chunk_vertex;
  const int64_t* choff;
  const int64_t* moff;
  int64_t n_chunks;
};

enum Mode { kUpdate = 0, kLogLik = 1, kInit = 2, kAssign = 3 };

// T: the state's storage type (double, or float for an STC_F32 handle).  A load widens to double, the store of
// a new count rounds it to T (once); everything between is fp64 in both instantiations.
template <typename T>
struct PassArgs {
  SideView g;
  const T* own;         // n×k counts of this orientation's vertices
  const T* other;       // the gathered side's counts
  double own_add, other_add;  // α−1 / η−1 (as fits the side)
  const double* inv;    // k: 1 / (N_k + V(η−1))
  T* out;               // n×k new counts (vertices with one chunk)
  double* partial;      // n_multi×k (chunks of the others)
  double* scalar;       // kLogLik: one value per chunk
  uint64_t seed;        // kInit
  int64_t pos_base;     // kInit: edges of the corpus before this handle's first (a group member; else 0)
  int k;
  int32_t* assign;      // kAssign: E, one topic per edge (rows only: the edge's position is its CSR position)
};

// Topics across lanes.  KP < 64: 64/KP edges side by side (lane = edge slot × KP + topic), the normalising
// sum a reduction over KP lanes.  KP = 64: NS slices of 64 topics per lane.  The product own·other is the
// same number in both orientations (one rounding, commutative), so both passes see the same γ.
// kAssign (rows only) keeps no sum: per edge the first j with the largest factor, the factor formed as kUpdate
// forms it.  A padding lane or an empty slot carries −1, below every real factor (α, η > 1 make them > 0).
// The fp32 pass stores through two element sizes (T out, double partial), and the compiler kept the byte
// offsets of both and v·k alive across the edge loop: 2 VGPRs more than the fp64 pass, which at 256 topics
// is the step from 7 waves per SIMD to 6.  refresh() hides a value's origin there, so the store addresses
// are formed after the loop.  The fp64 instantiation is left as it was.
template <typename T, typename X>
__device__ inline X refresh(X x) {
  if constexpr (sizeof(T) == 4) asm volatile("" : "+v"(x));
  return x;
}

template <typename T, int KP, int NS, int MODE>
__global__ __launch_bounds__(256) void k_em_pass(const PassArgs<T> a) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= a.g.n_chunks) return;  // wave-uniform
  const int64_t v = a.g.chunk_vertex[c];
  const int64_t c0 = a.g.choff[v], nch = a.g.choff[v + 1] - c0;
  const int64_t s = a.g.ptr[v] + (c - c0) * kChunk;
  const int64_t e = min(s + (int64_t)kChunk, a.g.ptr[v + 1]);
  constexpr int G = 64 / KP;
  const int j0 = lane % KP, slot = lane / KP;
  const int k = a.k;
  double own[NS], inv[NS], acc[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int j = j0 + 64 * i;
    const bool live = j < k;
    own[i] = (MODE != kInit && live) ? (double)a.own[v * k + j] + a.own_add : 0.0;
    inv[i] = (MODE != kInit && live) ? a.inv[j] : 0.0;
    acc[i] = 0.0;
  }
  double ln_s = 0.0, sc = 0.0;
  if (MODE == kLogLik) {  // θ_d's normaliser Σ_j (N_dk[d][j] + α−1)
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < NS; ++i) t += own[i];
#pragma unroll
    for (int o = KP / 2; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    ln_s = log(t);
  }
  for (int64_t base = s; base < e; base += G) {  // wave-uniform trip count
    const int64_t ed = base + slot;
    const bool valid = ed < e;
    const int64_t o = valid ? (int64_t)a.g.idx[ed] : 0;
    if (MODE == kAssign) {
      // every lane loads (a padding lane the last topic, an empty slot row 0), so the NS loads issue together
      const T* row = a.other + o * k;
      double x[NS];
#pragma unroll
      for (int i = 0; i < NS; ++i) x[i] = (double)row[min(j0 + 64 * i, k - 1)];
      double best = -1.0;
      int bj = j0;
#pragma unroll
      for (int i = 0; i < NS; ++i) {  // ascending j, strict >: the first maximum of this lane
        const int j = j0 + 64 * i;
        const double gi = (valid && j < k) ? (own[i] * (x[i] + a.other_add)) * inv[i] : -1.0;
        const bool up = gi > best;
        best = up ? gi : best;
        bj = up ? j : bj;
      }
      rank::row_argmax<false>(KP, best, bj);  // the slot's lanes: larger value, then smaller index
      if (valid && j0 == 0) a.assign[ed] = bj;
      continue;
    }
    const double cn = valid ? a.g.cnt[ed] : 0.0;
    double g[NS], sum = 0.0;
    if (MODE == kInit) {
      const uint64_t st = doc_stream(a.seed, (uint64_t)(valid ? (a.g.pos ? a.g.pos[ed] : ed) + a.pos_base : 0));
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        const int j = j0 + 64 * i;
        g[i] = (valid && j < k) ? rng_uniform(st, (uint64_t)j) : 0.0;
        sum += g[i];
      }
    } else {
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        const int j = j0 + 64 * i;
        g[i] = (valid && j < k) ? (own[i] * ((double)a.other[o * k + j] + a.other_add)) * inv[i] : 0.0;
        sum += g[i];
      }
    }
#pragma unroll
    for (int off = KP / 2; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if (MODE == kLogLik) {
      if (valid) sc += cn * (log(sum) - ln_s);
    } else {
      const double w = valid ? cn / sum : 0.0;
#pragma unroll
      for (int i = 0; i < NS; ++i) acc[i] += w * g[i];
    }
  }
  if (MODE == kAssign) return;
  // fold the edge slots (fixed order), slot 0 holds the chunk's sum
  if (MODE == kLogLik) {
#pragma unroll
    for (int off = KP; off < 64; off <<= 1) sc += __shfl_xor(sc, off, 64);
    if (lane == 0) a.scalar[c] = sc;
    return;
  }
#pragma unroll
  for (int i = 0; i < NS; ++i) {
#pragma unroll
    for (int off = KP; off < 64; off <<= 1) acc[i] += __shfl_xor(acc[i], off, 64);
  }
  if (slot != 0) return;
  const int js = refresh<T>(j0);
  if (nch == 1) {  // the vertex's whole sum: stored as the state stores it
    T* dst = a.out + refresh<T>(v) * k;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int j = js + 64 * i;
      if (j < k) dst[j] = (T)acc[i];
    }
  } else {
    double* dst = a.partial + (a.g.moff[v] + (c - c0)) * k;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int j = js + 64 * i;
      if (j < k) dst[j] = acc[i];
    }
  }
}

// out[v] = Σ partials of v in chunk order (vertices with several chunks), 0 (vertices without an edge)
template <typename T>
__global__ void k_em_fixup(const int64_t* __restrict__ choff, const int64_t* __restrict__ moff,
                           const double* __restrict__ partial, T* __restrict__ out, int64_t n, int k) {
  const int64_t total = n * k;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = t / k;
    const int j = (int)(t - v * k);
    const int64_t nch = choff[v + 1] - choff[v];
    if (nch == 1) continue;
    double s = 0.0;
    const double* p = partial + moff[v] * k + j;
    for (int64_t l = 0; l < nch; ++l) s += p[l * k];
    out[t] = (T)s;
  }
}

// whether vertex v exists: it has an edge here (ptr), or, for a group member's terms, on any member (deg)
__device__ inline bool has_vertex(const int64_t* __restrict__ ptr, const int64_t* __restrict__ deg, int64_t v) {
  return deg ? deg[v] > 0 : ptr[v + 1] > ptr[v];
}

// rows of vertices without an edge ← 0 (an injected state keeps to the graph's vertices)
template <typename T>
__global__ void k_em_mask(const int64_t* __restrict__ ptr, const int64_t* __restrict__ deg, T* __restrict__ x,
                          int64_t n, int k) {
  const int64_t total = n * k;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = t / k;
    if (!has_vertex(ptr, deg, v)) x[t] = (T)0;
  }
}

// deg[v] = the edges of vertex v (a member's term degrees, summed over the members at create)
__global__ void k_em_degree(const int64_t* __restrict__ ptr, int64_t n, int64_t* __restrict__ deg) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v < n) deg[v] = ptr[v + 1] - ptr[v];
}

// N_k, level 1: block b sums rows [b·kSumRows, (b+1)·kSumRows) per topic — tpr lanes across the topics,
// 256/tpr row streams folded in stream order.  The sum is fp64 over the stored values of either storage type.
template <typename T>
__global__ __launch_bounds__(256) void k_em_colsum1(const T* __restrict__ x, int64_t n, int k, int tpr,
                                                    double* __restrict__ part) {
  __shared__ double red[256];
  const int j0 = threadIdx.x % tpr, sub = threadIdx.x / tpr, S = 256 / tpr;
  const int64_t r0 = (int64_t)blockIdx.x * kSumRows, r1 = min(r0 + (int64_t)kSumRows, n);
  for (int jb = 0; jb < k; jb += tpr) {  // block-uniform
    const int j = jb + j0;
    double s = 0.0;
    if (j < k)
      for (int64_t r = r0 + sub; r < r1; r += S) s += (double)x[r * k + j];
    red[threadIdx.x] = s;
    __syncthreads();
    if (sub == 0 && j < k) {
      double t = 0.0;
      for (int q = 0; q < S; ++q) t += red[q * tpr + j0];
      part[(int64_t)blockIdx.x * k + j] = t;
    }
    __syncthreads();
  }
}
// level 2 (one block): N_k[j] = Σ_b part[b][j] in block order, inv[j] = 1 / (N_k[j] + V(η−1))
__global__ void k_em_colsum2(const double* __restrict__ part, int64_t nb, int k, double v_eta, double* __restrict__ nk,
                             double* __restrict__ inv) {
  for (int j = threadIdx.x; j < k; j += blockDim.x) {
    double s = 0.0;
    for (int64_t b = 0; b < nb; ++b) s += part[b * k + j];
    nk[j] = s;
    inv[j] = 1.0 / (s + v_eta);
  }
}

// fixed-shape sum of n doubles: block b folds [b·kSumElems, …) (16 strided elements per thread, then a tree)
__device__ inline double block_tree_sum(double s, double* red) {
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}
__global__ __launch_bounds__(256) void k_em_sum1(const double* __restrict__ x, int64_t n, double* __restrict__ part) {
  __shared__ double red[256];
  const int64_t b0 = (int64_t)blockIdx.x * kSumElems;
  double s = 0.0;
  for (int i = 0; i < kSumElems / 256; ++i) {
    const int64_t e = b0 + threadIdx.x + 256 * i;
    if (e < n) s += x[e];
  }
  s = block_tree_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void k_em_sum2(const double* __restrict__ part, int64_t nb, double* __restrict__ out) {
  __shared__ double red[256];
  double s = 0.0;
  for (int64_t b = threadIdx.x; b < nb; b += 256) s += part[b];
  s = block_tree_sum(s, red);
  if (threadIdx.x == 0) *out = s;
}

// logPrior's per-vertex term Σ_j ln(·): terms ln φ_w[j] (inv given), documents ln θ_d[j]; 0 without an edge
template <typename T>
__global__ void k_em_prior(const int64_t* __restrict__ ptr, const int64_t* __restrict__ deg,
                           const T* __restrict__ x, int64_t n, int k, double add, const double* __restrict__ inv,
                           double* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  double s = 0.0;
  if (has_vertex(ptr, deg, v)) {
    const T* row = x + v * k;
    if (inv) {
      for (int j = 0; j < k; ++j) s += log(((double)row[j] + add) * inv[j]);
    } else {
      double t = 0.0;
      for (int j = 0; j < k; ++j) t += (double)row[j] + add;
      for (int j = 0; j < k; ++j) s += log(((double)row[j] + add) / t);
    }
  }
  out[v] = s;
}

// ---- graph construction (once per handle) ----------------------------------------------------------
__global__ void k_em_flag(const double* __restrict__ val, const int32_t* __restrict__ idx, int64_t nnz, int64_t cols,
                          int64_t* __restrict__ flag, int* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > nnz) return;
  if (i == nnz) {
    flag[i] = 0;
    return;
  }
  flag[i] = val[i] != 0.0 ? 1 : 0;
  if (idx[i] < 0 || (int64_t)idx[i] >= cols) atomicOr(bad, 1);
}
__global__ void k_em_row_ptr(const int64_t* __restrict__ indptr, const int64_t* __restrict__ newpos, int64_t rows,
                             int64_t nnz, int64_t* __restrict__ ptr, int* __restrict__ bad) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r > rows) return;
  const int64_t p = indptr[r];
  if (p < 0 || p > nnz || (r < rows && indptr[r + 1] < p) || (r == 0 && p != 0) || (r == rows && p != nnz)) {
    atomicOr(bad, 2);
    ptr[r] = 0;
    return;
  }
  ptr[r] = newpos[p];
}
__global__ void k_em_compact(const int64_t* __restrict__ indptr, int64_t rows, const int32_t* __restrict__ idx,
                             const double* __restrict__ val, const int64_t* __restrict__ newpos, int64_t nnz,
                             int32_t* __restrict__ eidx, double* __restrict__ ecnt, int32_t* __restrict__ erow,
                             int64_t* __restrict__ iota) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnz || val[i] == 0.0) return;
  int64_t lo = 0, hi = rows;  // the row r with indptr[r] <= i < indptr[r+1]
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (indptr[mid] <= i) lo = mid;
    else hi = mid;
  }
  const int64_t p = newpos[i];
  eidx[p] = idx[i];
  ecnt[p] = val[i];
  erow[p] = (int32_t)lo;
  iota[p] = p;
}
__global__ void k_em_transpose(const int64_t* __restrict__ perm, const int32_t* __restrict__ erow,
                               const double* __restrict__ ecnt, int64_t E, int32_t* __restrict__ cidx,
                               double* __restrict__ ccnt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= E) return;
  const int64_t p = perm[i];
  cidx[i] = erow[p];
  ccnt[i] = ecnt[p];
}
// ptr[w] = the first sorted edge whose term is >= w (w = 0 … V)
__global__ void k_em_col_ptr(const int32_t* __restrict__ sorted, int64_t E, int64_t cols, int64_t* __restrict__ ptr) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w > cols) return;
  int64_t lo = 0, hi = E;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)sorted[mid] < w) lo = mid + 1;
    else hi = mid;
  }
  ptr[w] = lo;
}
__global__ void k_em_chunk_count(const int64_t* __restrict__ ptr, int64_t n, int64_t* __restrict__ nch,
                                 int64_t* __restrict__ nmulti) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v > n) return;
  const int64_t c = v < n ? (ptr[v + 1] - ptr[v] + kChunk - 1) / kChunk : 0;
  nch[v] = c;
  nmulti[v] = c > 1 ? c : 0;
}
__global__ void k_em_chunk_fill(const int64_t* __restrict__ choff, int64_t n, int32_t* __restrict__ chunk_vertex) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  for (int64_t c = choff[v]; c < choff[v + 1]; ++c) chunk_vertex[c] = (int32_t)v;
}

inline unsigned strided_blocks(int64_t n) { return (unsigned)std::min<int64_t>(std::max<int64_t>(1, ceil_div(n, 256)), 1 << 20); }

void excl_scan(hipStream_t s, DevBuf& tmp, const int64_t* in, int64_t* out, int64_t n) {
  with_temp(tmp, [&](void* t, size_t& tb) { return hipcub::DeviceScan::ExclusiveSum(t, tb, in, out, (int)n, s); });
}

template <typename T, int MODE>
void launch_pass(hipStream_t s, const PassArgs<T>& a) {
  if (a.g.n_chunks == 0) return;
  const unsigned grid = blocks_for(a.g.n_chunks, 4);
  const int kp = pow2_at_least(a.k);
#define STC_EM_CASE(KP, NS)                                \
  k_em_pass<T, KP, NS, MODE><<<grid, 256, 0, s>>>(a);      \
  break
  switch (kp) {
    case 2: STC_EM_CASE(2, 1);
    case 4: STC_EM_CASE(4, 1);
    case 8: STC_EM_CASE(8, 1);
    case 16: STC_EM_CASE(16, 1);
    case 32: STC_EM_CASE(32, 1);
    case 64: STC_EM_CASE(64, 1);
    case 128: STC_EM_CASE(64, 2);
    case 256: STC_EM_CASE(64, 4);
    case 512: STC_EM_CASE(64, 8);
    case 1024: STC_EM_CASE(64, 16);
    default: throw Error(STC_ERR_INVALID_ARG, "em: k out of range");
  }
#undef STC_EM_CASE
  KERNEL_CHECK();
}

}  // namespace
}  // namespace em
}  // namespace stc

using namespace stc;
using namespace stc::em;

struct stc_em {
  Ctx* ctx = nullptr;
  int device = -1;       // for stc_em_destroy, which may run after the context is gone
  int k = 0;
  int64_t D = 0, V = 0, E = 0;
  double alpha = 0.0, eta = 0.0;
  bool has_state = false;
  int cur = 0;           // which of the two state copies is current
  Side rows, cols;
  int dtype = STC_F64;   // how N_dk / N_wk are stored: STC_F64, or STC_F32 (rounded when stored, read widened)
  DevBuf ndk[2], nwk[2]; // D×k, V×k of dtype
  DevBuf nk, inv;        // k
  DevBuf partial;        // max(rows.n_multi, cols.n_multi)×k
  DevBuf sum_part;       // first-level partials of the N_k and scalar reductions
  DevBuf scalar;         // per-chunk / per-vertex scalars of logLikelihood / logPrior
  DevBuf result;         // 3 doubles: Σ c ln(φ·θ), Σ ln φ, Σ ln θ
  DevBuf assign;         // int32[E]: topicAssignments' output (allocated by its first call)
  // a member of an stc_em_group (lda_em.h): D, E and the graph are its shard's
  bool member = false;
  int64_t pos_base = 0;  // edges in the earlier shards
  DevBuf gdeg;           // int64[V]: every term's edges over all members (empty: the local graph is the whole one)
  rank::Scratch rk;      // the ranked queries' scratch (rank.h; allocated by their first call)
  int64_t doc_vertices = -1;  // the documents with an edge (counted by the first top_documents)
};

namespace stc {
namespace em {
namespace {

SideView view(const Side& g, bool with_pos) {
  return SideView{g.ptr.as<int64_t>(), g.idx.as<int32_t>(), g.cnt.as<double>(), with_pos ? g.pos.as<int64_t>() : nullptr,
                  g.chunk_vertex.as<int32_t>(), g.choff.as<int64_t>(), g.moff.as<int64_t>(), g.n_chunks};
}

void build_chunks(Ctx& c, Side& g, DevBuf& t0, DevBuf& t1, DevBuf& scan_tmp) {
  hipStream_t s = c.stream;
  t0.reserve(8 * (g.n + 1));
  t1.reserve(8 * (g.n + 1));
  g.choff.reserve(8 * (g.n + 1));
  g.moff.reserve(8 * (g.n + 1));
  k_em_chunk_count<<<blocks_for(g.n + 1), 256, 0, s>>>(g.ptr.as<int64_t>(), g.n, t0.as<int64_t>(), t1.as<int64_t>());
  KERNEL_CHECK();
  excl_scan(s, scan_tmp, t0.as<int64_t>(), g.choff.as<int64_t>(), g.n + 1);
  excl_scan(s, scan_tmp, t1.as<int64_t>(), g.moff.as<int64_t>(), g.n + 1);
  int64_t h[2] = {0, 0};
  HIP_CHECK(hipMemcpyAsync(&h[0], g.choff.as<int64_t>() + g.n, 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(&h[1], g.moff.as<int64_t>() + g.n, 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  g.n_chunks = h[0];
  g.n_multi = h[1];
  g.chunk_vertex.reserve(4 * std::max<int64_t>(g.n_chunks, 1));
  if (g.n > 0) {
    k_em_chunk_fill<<<blocks_for(g.n), 256, 0, s>>>(g.choff.as<int64_t>(), g.n, g.chunk_vertex.as<int32_t>());
    KERNEL_CHECK();
  }
}

// the host code below is written once over the storage type: f(T{}) with T = double or float
template <typename F>
void by_state_type(const stc_em& m, F&& f) {
  if (m.dtype == STC_F32) f(float{});
  else f(double{});
}
size_t state_elem(const stc_em& m) { return m.dtype == STC_F32 ? sizeof(float) : sizeof(double); }

// N_k and the per-iteration constants of state copy `which`, on the device
void refresh_totals(stc_em& m, int which) {
  hipStream_t s = m.ctx->stream;
  const int64_t nb = ceil_div(m.V, kSumRows);
  const int tpr = std::min(pow2_at_least(m.k), 256);
  by_state_type(m, [&](auto t) {
    using T = decltype(t);
    k_em_colsum1<T><<<(unsigned)nb, 256, 0, s>>>(m.nwk[which].as<T>(), m.V, m.k, tpr, m.sum_part.as<double>());
  });
  KERNEL_CHECK();
  k_em_colsum2<<<1, 256, 0, s>>>(m.sum_part.as<double>(), nb, m.k, (double)m.V * (m.eta - 1.0), m.nk.as<double>(),
                                 m.inv.as<double>());
  KERNEL_CHECK();
}

template <typename T, int MODE>
void run_side_as(stc_em& m, bool row_side, int from, int to, uint64_t seed) {
  hipStream_t s = m.ctx->stream;
  const Side& g = row_side ? m.rows : m.cols;
  PassArgs<T> a{};
  a.g = view(g, !row_side);
  a.own = (row_side ? m.ndk[from] : m.nwk[from]).as<T>();
  a.other = (row_side ? m.nwk[from] : m.ndk[from]).as<T>();
  a.own_add = row_side ? m.alpha - 1.0 : m.eta - 1.0;
  a.other_add = row_side ? m.eta - 1.0 : m.alpha - 1.0;
  a.inv = m.inv.as<double>();
  T* out = (row_side ? m.ndk[to] : m.nwk[to]).as<T>();
  a.out = out;
  a.partial = m.partial.as<double>();
  a.scalar = m.scalar.as<double>();
  a.seed = seed;
  a.pos_base = m.pos_base;
  a.k = m.k;
  a.assign = m.assign.as<int32_t>();
  launch_pass<T, MODE>(s, a);
  if (MODE != kLogLik && MODE != kAssign && g.n > 0) {
    k_em_fixup<T><<<strided_blocks(g.n * m.k), 256, 0, s>>>(g.choff.as<int64_t>(), g.moff.as<int64_t>(),
                                                           m.partial.as<double>(), out, g.n, m.k);
    KERNEL_CHECK();
  }
}
template <int MODE>
void run_side(stc_em& m, bool row_side, int from, int to, uint64_t seed) {
  by_state_type(m, [&](auto t) { run_side_as<decltype(t), MODE>(m, row_side, from, to, seed); });
}

void sum_to(stc_em& m, const double* x, int64_t n, double* out) {
  hipStream_t s = m.ctx->stream;
  if (n == 0) {
    HIP_CHECK(hipMemsetAsync(out, 0, 8, s));
    return;
  }
  const int64_t nb = ceil_div(n, kSumElems);
  k_em_sum1<<<(unsigned)nb, 256, 0, s>>>(x, n, m.sum_part.as<double>());
  KERNEL_CHECK();
  k_em_sum2<<<1, 256, 0, s>>>(m.sum_part.as<double>(), nb, out);
  KERNEL_CHECK();
}

// the public entry points serve one device; a connected context's handle is driven by its stc_em_group alone
void require_idle_single(const Ctx& c, bool as_member = false) {
  if (c.coll() && !as_member)
    throw Error(STC_ERR_STATE, "em: the context is connected to other ranks (EM is single-device; several devices: stc_em_group)");
}
void require_state(const stc_em& m) {
  if (!m.has_state) throw Error(STC_ERR_STATE, "em: no state yet (stc_em_init_random or stc_em_set_state first)");
}
const int64_t* global_degrees(const stc_em& m) { return m.gdeg.p ? m.gdeg.as<int64_t>() : nullptr; }

// a member's N_wk' holds the messages of its own edges: the sum over the members is the graph's (fp32 state:
// the members' stored, rounded partials are added in fp32)
void reduce_terms(stc_em& m, int which) {
  if (m.member && m.ctx->coll())
    coll_all_reduce(*m.ctx, m.nwk[which].p, (size_t)(m.V * m.k), m.dtype == STC_F32 ? ncclFloat32 : ncclFloat64,
                    m.ctx->stream);
}

stc_em* create(Ctx& c, const DCsr& in, int32_t k, double doc_concentration, double topic_concentration,
               int state_dtype, bool as_member = false, int64_t pos_base = 0) {
  require_idle_single(c, as_member);
  STC_REQUIRE(state_dtype == STC_F64 || state_dtype == STC_F32, "em: the state dtype must be STC_F64 or STC_F32");
  STC_REQUIRE(in.dtype == STC_F64, "em: the corpus values must be STC_F64");
  STC_REQUIRE(k >= 2 && k <= 1024, "em: 2 <= k <= 1024");
  STC_REQUIRE(in.rows >= 0 && in.cols > 0, "em: corpus shape");
  STC_REQUIRE(in.rows < (int64_t(1) << 31) - 1 && in.cols < (int64_t(1) << 31) - 1 && in.nnz < (int64_t(1) << 31) - 1,
              "em: rows, columns and entries below 2^31 - 1");
  const double alpha = doc_concentration == -1.0 ? 50.0 / k + 1.0 : doc_concentration;
  const double eta = topic_concentration == -1.0 ? 1.1 : topic_concentration;
  STC_REQUIRE(alpha > 1.0, "em: docConcentration must be > 1.0 (or -1 for auto) for EM");
  STC_REQUIRE(eta > 1.0, "em: topicConcentration must be > 1.0 (or -1 for auto) for EM");
  c.use();
  hipStream_t s = c.stream;
  auto m = new_handle<stc_em>(c);
  m->k = k;
  m->D = in.rows;
  m->V = in.cols;
  m->alpha = alpha;
  m->eta = eta;
  m->dtype = state_dtype;
  const int64_t nnz = in.nnz;

  // 1. the edges: entries whose value is not 0, in CSR order
  DevBuf flag, newpos, scan_tmp, bad;
  flag.reserve(8 * (nnz + 1));
  newpos.reserve(8 * (nnz + 1));
  bad.reserve(sizeof(int));
  HIP_CHECK(hipMemsetAsync(bad.p, 0, sizeof(int), s));
  k_em_flag<<<blocks_for(nnz + 1), 256, 0, s>>>(in.values.as<double>(), in.indices.as<int32_t>(), nnz, in.cols,
                                                flag.as<int64_t>(), bad.as<int>());
  KERNEL_CHECK();
  excl_scan(s, scan_tmp, flag.as<int64_t>(), newpos.as<int64_t>(), nnz + 1);
  m->rows.n = m->D;
  m->rows.ptr.reserve(8 * (m->D + 1));
  k_em_row_ptr<<<blocks_for(m->D + 1), 256, 0, s>>>(in.indptr.as<int64_t>(), newpos.as<int64_t>(), m->D, nnz,
                                                    m->rows.ptr.as<int64_t>(), bad.as<int>());
  KERNEL_CHECK();
  int64_t E = 0;
  int h_bad = 0;
  HIP_CHECK(hipMemcpyAsync(&E, newpos.as<int64_t>() + nnz, 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(&h_bad, bad.p, sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  STC_REQUIRE(h_bad == 0, "em: the corpus has a column index out of range or a malformed indptr");
  m->E = E;
  const int64_t E1 = std::max<int64_t>(E, 1);
  DevBuf erow, iota, sorted_term, sort_tmp;
  m->rows.idx.reserve(4 * E1);
  m->rows.cnt.reserve(8 * E1);
  erow.reserve(4 * E1);
  iota.reserve(8 * E1);
  if (nnz > 0) {
    k_em_compact<<<blocks_for(nnz), 256, 0, s>>>(in.indptr.as<int64_t>(), m->D, in.indices.as<int32_t>(),
                                                 in.values.as<double>(), newpos.as<int64_t>(), nnz,
                                                 m->rows.idx.as<int32_t>(), m->rows.cnt.as<double>(),
                                                 erow.as<int32_t>(), iota.as<int64_t>());
    KERNEL_CHECK();
  }

  // 2. the transpose: a stable sort of the edges by term keeps every term's documents in CSR order
  m->cols.n = m->V;
  m->cols.ptr.reserve(8 * (m->V + 1));
  m->cols.idx.reserve(4 * E1);
  m->cols.cnt.reserve(8 * E1);
  m->cols.pos.reserve(8 * E1);
  sorted_term.reserve(4 * E1);
  if (E > 0) {
    int bits = 1;
    while ((int64_t(1) << bits) < m->V) ++bits;
    with_temp(sort_tmp, [&](void* t, size_t& tb) {
      return hipcub::DeviceRadixSort::SortPairs(t, tb, m->rows.idx.as<int32_t>(), sorted_term.as<int32_t>(),
                                                iota.as<int64_t>(), m->cols.pos.as<int64_t>(), (int)E, 0, bits, s);
    });
    k_em_transpose<<<blocks_for(E), 256, 0, s>>>(m->cols.pos.as<int64_t>(), erow.as<int32_t>(), m->rows.cnt.as<double>(),
                                                 E, m->cols.idx.as<int32_t>(), m->cols.cnt.as<double>());
    KERNEL_CHECK();
  }
  k_em_col_ptr<<<blocks_for(m->V + 1), 256, 0, s>>>(sorted_term.as<int32_t>(), E, m->V, m->cols.ptr.as<int64_t>());
  KERNEL_CHECK();

  // 3. the chunk tables of both orientations
  build_chunks(c, m->rows, flag, newpos, scan_tmp);
  build_chunks(c, m->cols, flag, newpos, scan_tmp);

  // 4. state and scratch
  const int64_t kk = k;
  for (int i = 0; i < 2; ++i) {
    m->ndk[i].reserve(state_elem(*m) * std::max<int64_t>(m->D * kk, 1));
    m->nwk[i].reserve(state_elem(*m) * std::max<int64_t>(m->V * kk, 1));
  }
  m->nk.reserve(8 * kk);
  m->inv.reserve(8 * kk);
  m->partial.reserve(8 * std::max<int64_t>(std::max(m->rows.n_multi, m->cols.n_multi) * kk, 1));
  m->sum_part.reserve(8 * std::max<int64_t>({ceil_div(m->V, kSumRows) * kk, ceil_div(m->rows.n_chunks, kSumElems),
                                            ceil_div(m->D, kSumElems), ceil_div(m->V, kSumElems), int64_t(1)}));
  m->scalar.reserve(8 * std::max<int64_t>({m->rows.n_chunks, m->D, m->V, int64_t(1)}));
  m->result.reserve(8 * 3);
  m->member = as_member;
  m->pos_base = pos_base;
  if (as_member && c.coll()) {  // which terms have a vertex is a property of the whole graph
    m->gdeg.reserve(8 * m->V);
    k_em_degree<<<blocks_for(m->V), 256, 0, s>>>(m->cols.ptr.as<int64_t>(), m->V, m->gdeg.as<int64_t>());
    KERNEL_CHECK();
    coll_all_reduce(c, m->gdeg.p, (size_t)m->V, ncclInt64, s);
  }
  wait_stream(c, s);  // the build's temporaries are freed on return
  return m.release();
}

void destroy(stc_em* m) {
  if (!m) return;
  if (m->device >= 0) {  // queued iterations first: the buffers are freed below
    (void)hipSetDevice(m->device);
    (void)hipDeviceSynchronize();
  }
  delete m;
}

void init_random(stc_em& m, uint64_t seed, bool as_member = false) {
  require_idle_single(*m.ctx, as_member);
  m.ctx->use();
  run_side<kInit>(m, true, 0, 0, seed);
  run_side<kInit>(m, false, 0, 0, seed);
  reduce_terms(m, 0);
  m.cur = 0;
  refresh_totals(m, 0);
  m.has_state = true;
}

void check_state_input(const stc_em& m, const double* doc_topics, const double* term_topics) {
  STC_REQUIRE((doc_topics || m.D == 0) && term_topics, "em: doc_topics / term_topics");
  const int64_t nd = m.D * m.k, nw = m.V * m.k;
  for (int64_t i = 0; i < nd; ++i) STC_REQUIRE(doc_topics[i] >= 0.0, "em: doc_topics must be non-negative");
  for (int64_t i = 0; i < nw; ++i) STC_REQUIRE(term_topics[i] >= 0.0, "em: term_topics must be non-negative");
}

// the arrays checked by the caller; no collective: every member is given the same term_topics
void set_state(stc_em& m, const double* doc_topics, const double* term_topics, bool as_member = false) {
  require_idle_single(*m.ctx, as_member);
  m.ctx->use();
  hipStream_t s = m.ctx->stream;
  const int64_t nd = m.D * m.k, nw = m.V * m.k;
  // fp32 state: rounded to nearest on the host (the mask only writes zeros, so its order against the rounding
  // does not matter); the narrow copies live until the stream has been waited for
  std::vector<float> nd32, nw32;
  const void *src_d = doc_topics, *src_w = term_topics;
  if (m.dtype == STC_F32) {
    nd32.assign(doc_topics, doc_topics + nd);
    nw32.assign(term_topics, term_topics + nw);
    src_d = nd32.data();
    src_w = nw32.data();
  }
  const size_t es = state_elem(m);
  if (nd) HIP_CHECK(hipMemcpyAsync(m.ndk[0].p, src_d, es * nd, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(m.nwk[0].p, src_w, es * nw, hipMemcpyHostToDevice, s));
  by_state_type(m, [&](auto t) {
    using T = decltype(t);
    if (nd) k_em_mask<T><<<strided_blocks(nd), 256, 0, s>>>(m.rows.ptr.as<int64_t>(), nullptr, m.ndk[0].as<T>(), m.D, m.k);
    k_em_mask<T><<<strided_blocks(nw), 256, 0, s>>>(m.cols.ptr.as<int64_t>(), global_degrees(m), m.nwk[0].as<T>(), m.V, m.k);
  });
  KERNEL_CHECK();
  m.cur = 0;
  refresh_totals(m, 0);
  wait_stream(*m.ctx, s);  // the caller's arrays are free to change on return
  m.has_state = true;
}

void get_state(stc_em& m, double* doc_topics, double* term_topics, double* totals, double* alpha_out, double* eta_out) {
  if (alpha_out) *alpha_out = m.alpha;
  if (eta_out) *eta_out = m.eta;
  if (!doc_topics && !term_topics && !totals) return;
  require_state(m);
  m.ctx->use();
  hipStream_t s = m.ctx->stream;
  const int64_t nd = doc_topics ? m.D * m.k : 0, nw = term_topics ? m.V * m.k : 0;
  if (totals) HIP_CHECK(hipMemcpyAsync(totals, m.nk.p, 8 * m.k, hipMemcpyDeviceToHost, s));
  if (m.dtype == STC_F32) {  // the stored values widened on the host, which is exact
    std::vector<float> nd32((size_t)nd), nw32((size_t)nw);
    if (nd) HIP_CHECK(hipMemcpyAsync(nd32.data(), m.ndk[m.cur].p, 4 * nd, hipMemcpyDeviceToHost, s));
    if (nw) HIP_CHECK(hipMemcpyAsync(nw32.data(), m.nwk[m.cur].p, 4 * nw, hipMemcpyDeviceToHost, s));
    wait_stream(*m.ctx, s);
    std::copy(nd32.begin(), nd32.end(), doc_topics);
    std::copy(nw32.begin(), nw32.end(), term_topics);
    return;
  }
  if (nd) HIP_CHECK(hipMemcpyAsync(doc_topics, m.ndk[m.cur].p, 8 * nd, hipMemcpyDeviceToHost, s));
  if (nw) HIP_CHECK(hipMemcpyAsync(term_topics, m.nwk[m.cur].p, 8 * nw, hipMemcpyDeviceToHost, s));
  wait_stream(*m.ctx, s);
}

void next(stc_em& m, int32_t n_iterations, bool as_member = false) {
  require_idle_single(*m.ctx, as_member);
  STC_REQUIRE(n_iterations >= 0, "em: n_iterations >= 0");
  require_state(m);
  m.ctx->use();
  for (int32_t it = 0; it < n_iterations; ++it) {
    const int from = m.cur, to = 1 - m.cur;
    run_side<kUpdate>(m, true, from, to, 0);   // N_dk' over rows, gathering N_wk
    run_side<kUpdate>(m, false, from, to, 0);  // N_wk' over columns, gathering N_dk
    reduce_terms(m, to);                       // a group member: + the other members' edges
    refresh_totals(m, to);                     // N_k' and 1 / (N_k' + V(η−1)) for the next reads
    m.cur = to;
  }
}

// h[0] Σ c ln(φ·θ) over the edges, h[1] Σ ln φ over the term vertices, h[2] Σ ln θ over the document vertices
void log_likelihood_parts(stc_em& m, bool want_ll, bool want_prior, double h[3], bool as_member = false) {
  require_idle_single(*m.ctx, as_member);
  require_state(m);
  m.ctx->use();
  hipStream_t s = m.ctx->stream;
  double* res = m.result.as<double>();
  h[0] = h[1] = h[2] = 0.0;
  if (want_ll) {
    run_side<kLogLik>(m, true, m.cur, m.cur, 0);
    sum_to(m, m.scalar.as<double>(), m.rows.n_chunks, res);
  }
  if (want_prior) {
    by_state_type(m, [&](auto t) {
      using T = decltype(t);
      k_em_prior<T><<<blocks_for(m.V), 256, 0, s>>>(m.cols.ptr.as<int64_t>(), global_degrees(m), m.nwk[m.cur].as<T>(), m.V,
                                                    m.k, m.eta - 1.0, m.inv.as<double>(), m.scalar.as<double>());
    });
    KERNEL_CHECK();
    sum_to(m, m.scalar.as<double>(), m.V, res + 1);
    if (m.D > 0) {
      by_state_type(m, [&](auto t) {
        using T = decltype(t);
        k_em_prior<T><<<blocks_for(m.D), 256, 0, s>>>(m.rows.ptr.as<int64_t>(), nullptr, m.ndk[m.cur].as<T>(), m.D, m.k,
                                                      m.alpha - 1.0, nullptr, m.scalar.as<double>());
      });
      KERNEL_CHECK();
    }
    sum_to(m, m.scalar.as<double>(), m.D, res + 2);
  }
  if (want_ll || want_prior) {
    double r[3] = {0, 0, 0};
    HIP_CHECK(hipMemcpyAsync(r, res, sizeof r, hipMemcpyDeviceToHost, s));
    wait_stream(*m.ctx, s);
    if (want_ll) h[0] = r[0];
    if (want_prior) h[1] = r[1], h[2] = r[2];
  }
}

void log_likelihood(stc_em& m, double* ll_out, double* prior_out) {
  double h[3];
  log_likelihood_parts(m, ll_out != nullptr, prior_out != nullptr, h);
  if (ll_out) *ll_out = h[0];
  if (prior_out) *prior_out = (m.eta - 1.0) * h[1] + (m.alpha - 1.0) * h[2];
}

void topic_assignments(stc_em& m, int64_t* indptr_out, int32_t* terms_out, int32_t* topics_out, bool as_member = false) {
  require_idle_single(*m.ctx, as_member);
  require_state(m);
  m.ctx->use();
  hipStream_t s = m.ctx->stream;
  m.assign.reserve(4 * std::max<int64_t>(m.E, 1));
  run_side<kAssign>(m, true, m.cur, m.cur, 0);
  if (!indptr_out && !terms_out && !topics_out) return;  // enqueued like an iteration: nothing to wait for
  if (indptr_out) HIP_CHECK(hipMemcpyAsync(indptr_out, m.rows.ptr.p, 8 * (m.D + 1), hipMemcpyDeviceToHost, s));
  if (terms_out && m.E) HIP_CHECK(hipMemcpyAsync(terms_out, m.rows.idx.p, 4 * m.E, hipMemcpyDeviceToHost, s));
  if (topics_out && m.E) HIP_CHECK(hipMemcpyAsync(topics_out, m.assign.p, 4 * m.E, hipMemcpyDeviceToHost, s));
  wait_stream(*m.ctx, s);
}

// ---- ranked queries (rank.h) -------------------------------------------------------------------------
bool is_f32(const stc_em& m) { return m.dtype == STC_F32; }

// describeTopics: per topic the N = min(max_terms, V) largest N_wk[w][t], (count descending, term ascending),
// weights N_wk[w][t] / N_k[t]
void describe(stc_em& m, int32_t max_terms, int32_t* idx_out, double* weight_out, bool as_member = false) {
  require_idle_single(*m.ctx, as_member);
  STC_REQUIRE(idx_out && weight_out, "em: idx_out / weight_out");
  STC_REQUIRE(max_terms > 0, "em: max_terms > 0");
  require_state(m);
  m.ctx->use();
  rank::describe_columns(*m.ctx, m.rk, m.nwk[m.cur].p, is_f32(m), m.V, m.k, std::min<int64_t>(max_terms, m.V),
                         m.nk.as<double>(), idx_out, weight_out);
}

// topDocumentsPerTopic over this handle's rows: N = min(max_docs, its document vertices) per topic, rows[t·N + i]
// = row0 + row, by (N_dk[d][t] / Σ_j N_dk[d][j] descending, row ascending); returns N
int64_t top_documents(stc_em& m, int64_t max_docs, int64_t row0, std::vector<int64_t>& rows, std::vector<double>& w,
                      bool as_member = false) {
  require_idle_single(*m.ctx, as_member);
  STC_REQUIRE(max_docs > 0, "em: max_docs > 0");
  require_state(m);
  m.ctx->use();
  hipStream_t s = m.ctx->stream;
  if (m.doc_vertices < 0) {
    m.rk.count.reserve(8);
    rank::count_vertices(s, m.rows.ptr.as<int64_t>(), m.D, m.rk.count.as<int64_t>());
    int64_t n = 0;
    HIP_CHECK(hipMemcpyAsync(&n, m.rk.count.p, 8, hipMemcpyDeviceToHost, s));
    wait_stream(*m.ctx, s);
    m.doc_vertices = n;
  }
  const int64_t N = std::min(max_docs, m.doc_vertices), total = N * m.k;
  rows.assign((size_t)total, 0);
  w.assign((size_t)total, 0.0);
  if (N == 0) return 0;
  m.rk.rowsum.reserve(8 * m.D);
  m.rk.out_row.reserve(8 * total);
  m.rk.out_w.reserve(8 * total);
  rank::row_sums(s, m.ndk[m.cur].p, is_f32(m), m.rows.ptr.as<int64_t>(), m.D, m.k, m.rk.rowsum.as<double>());
  rank::select_columns(s, m.rk, m.ndk[m.cur].p, is_f32(m), m.D, m.k, N, m.rk.rowsum.as<double>(), nullptr, row0,
                       m.rk.out_row.as<int64_t>(), m.rk.out_w.as<double>());
  HIP_CHECK(hipMemcpyAsync(rows.data(), m.rk.out_row.p, 8 * total, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(w.data(), m.rk.out_w.p, 8 * total, hipMemcpyDeviceToHost, s));
  wait_stream(*m.ctx, s);
  return N;
}

// topTopicsPerDocument: per row the N = min(n_topics, k) largest N_dk[d][j], (count descending, topic ascending),
// weights N_dk[d][j] / Σ_j N_dk[d][j] (a row whose sum is 0, as a document without a vertex: 0 … N−1, weight 0)
void top_topics(stc_em& m, int32_t n_topics, int32_t* idx_out, double* weight_out, bool as_member = false) {
  require_idle_single(*m.ctx, as_member);
  STC_REQUIRE((idx_out && weight_out) || m.D == 0, "em: idx_out / weight_out");
  STC_REQUIRE(n_topics > 0, "em: n_topics > 0");
  require_state(m);
  if (m.D == 0) return;
  m.ctx->use();
  hipStream_t s = m.ctx->stream;
  const int N = std::min<int>(n_topics, m.k);
  const int64_t total = m.D * N;
  m.rk.rowsum.reserve(8 * m.D);
  m.rk.out_row.reserve(4 * total);
  m.rk.out_w.reserve(8 * total);
  rank::row_sums(s, m.ndk[m.cur].p, is_f32(m), nullptr, m.D, m.k, m.rk.rowsum.as<double>());
  rank::select_rows(s, m.ndk[m.cur].p, is_f32(m), m.rk.rowsum.as<double>(), m.D, m.k, N, m.rk.out_row.as<int32_t>(),
                    m.rk.out_w.as<double>());
  HIP_CHECK(hipMemcpyAsync(idx_out, m.rk.out_row.p, 4 * total, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(weight_out, m.rk.out_w.p, 8 * total, hipMemcpyDeviceToHost, s));
  wait_stream(*m.ctx, s);
}

void shape(const stc_em& m, int32_t* k, int64_t* n_docs, int64_t* vocab, int64_t* n_edges) {
  if (k) *k = m.k;
  if (n_docs) *n_docs = m.D;
  if (vocab) *vocab = m.V;
  if (n_edges) *n_edges = m.E;
}

}  // namespace

// ---- the member side of an stc_em_group (lda_em.h) --------------------------------------------------
stc_em* member_create(Ctx& c, const DCsr& shard, int32_t k, double doc_concentration, double topic_concentration,
                      int state_dtype, int64_t pos_base) {
  return create(c, shard, k, doc_concentration, topic_concentration, state_dtype, true, pos_base);
}
void member_init_random(stc_em& m, uint64_t seed) { init_random(m, seed, true); }
void member_set_state(stc_em& m, const double* doc_topics, const double* term_topics) {
  set_state(m, doc_topics, term_topics, true);
}
void member_next(stc_em& m, int32_t n_iterations) { next(m, n_iterations, true); }
void member_log_likelihood(stc_em& m, double* ll, double* term_prior, double* doc_prior) {
  double h[3];
  log_likelihood_parts(m, ll != nullptr, term_prior || doc_prior, h, true);
  if (ll) *ll = h[0];
  if (term_prior) *term_prior = h[1];
  if (doc_prior) *doc_prior = h[2];
}
void member_topic_assignments(stc_em& m, int64_t* indptr_out, int32_t* terms_out, int32_t* topics_out) {
  topic_assignments(m, indptr_out, terms_out, topics_out, true);
}
void member_describe(stc_em& m, int32_t max_terms, int32_t* idx_out, double* weight_out) {
  describe(m, max_terms, idx_out, weight_out, true);
}
int64_t member_top_documents(stc_em& m, int64_t max_docs, int64_t row0, std::vector<int64_t>& rows,
                             std::vector<double>& weights) {
  return top_documents(m, max_docs, row0, rows, weights, true);
}
void member_top_topics(stc_em& m, int32_t n_topics, int32_t* idx_out, double* weight_out) {
  top_topics(m, n_topics, idx_out, weight_out, true);
}
void member_wait(stc_em& m) {
  m.ctx->use();
  wait_stream(*m.ctx, m.ctx->stream);
}

}  // namespace em
}  // namespace stc

extern "C" {

// ---- C ABI ---------------------------------------------------------------------------------
int stc_em_create_as(stc_ctx* ctx, const stc_dcsr* corpus, int32_t k, double doc_concentration,
                     double topic_concentration, int state_dtype, stc_em** out) {
  return guard([&] {
    STC_REQUIRE(ctx && corpus && out, "ctx/corpus/out");
    STC_REQUIRE(corpus->ctx == ctx, "the corpus belongs to another stc_ctx");
    *out = em::create(*ctx, *corpus, k, doc_concentration, topic_concentration, state_dtype);
  });
}

int stc_em_create(stc_ctx* ctx, const stc_dcsr* corpus, int32_t k, double doc_concentration,
                  double topic_concentration, stc_em** out) {
  return stc_em_create_as(ctx, corpus, k, doc_concentration, topic_concentration, STC_F64, out);
}

int stc_em_state_dtype(const stc_em* m, int* dtype_out) {
  return guard([&] {
    STC_REQUIRE(m && dtype_out, "em/dtype_out");
    *dtype_out = m->dtype;
  });
}

int stc_em_destroy(stc_em* m) {
  return guard([&] { em::destroy(m); });
}

int stc_em_shape(const stc_em* m, int32_t* k, int64_t* n_docs, int64_t* vocab, int64_t* n_edges) {
  return guard([&] {
    STC_REQUIRE(m, "em");
    em::shape(*m, k, n_docs, vocab, n_edges);
  });
}

int stc_em_init_random(stc_em* m, uint64_t seed) {
  return guard([&] {
    STC_REQUIRE(m, "em");
    em::init_random(*m, seed);
  });
}

int stc_em_set_state(stc_em* m, const double* doc_topics, const double* term_topics) {
  return guard([&] {
    STC_REQUIRE(m, "em");
    require_idle_single(*m->ctx);
    em::check_state_input(*m, doc_topics, term_topics);
    em::set_state(*m, doc_topics, term_topics);
  });
}

int stc_em_get_state(stc_em* m, double* doc_topics, double* term_topics, double* totals, double* alpha_out,
                     double* eta_out) {
  return guard([&] {
    STC_REQUIRE(m, "em");
    em::get_state(*m, doc_topics, term_topics, totals, alpha_out, eta_out);
  });
}

int stc_em_next(stc_em* m, int32_t n_iterations) {
  return guard([&] {
    STC_REQUIRE(m, "em");
    em::next(*m, n_iterations);
  });
}

int stc_em_log_likelihood(stc_em* m, double* log_likelihood_out, double* log_prior_out) {
  return guard([&] {
    STC_REQUIRE(m, "em");
    em::log_likelihood(*m, log_likelihood_out, log_prior_out);
  });
}

int stc_em_topic_assignments(stc_em* m, int64_t* indptr_out, int32_t* terms_out, int32_t* topics_out) {
  return guard([&] {
    STC_REQUIRE(m, "em");
    em::topic_assignments(*m, indptr_out, terms_out, topics_out);
  });
}

int stc_em_describe(stc_em* m, int32_t max_terms, int32_t* idx_out, double* weight_out) {
  return guard([&] {
    STC_REQUIRE(m, "em");
    em::describe(*m, max_terms, idx_out, weight_out);
  });
}

int stc_em_top_documents(stc_em* m, int64_t max_docs, int64_t* n_out, int64_t* row_out, double* weight_out) {
  return guard([&] {
    STC_REQUIRE(m, "em");
    STC_REQUIRE(n_out && row_out && weight_out, "em: n_out / row_out / weight_out");
    std::vector<int64_t> rows;
    std::vector<double> w;
    const int64_t N = em::top_documents(*m, max_docs, 0, rows, w), cap = std::min(max_docs, m->D);
    for (int t = 0; t < m->k; ++t) {
      std::copy(rows.begin() + t * N, rows.begin() + (t + 1) * N, row_out + t * cap);
      std::copy(w.begin() + t * N, w.begin() + (t + 1) * N, weight_out + t * cap);
    }
    *n_out = N;
  });
}

int stc_em_top_topics(stc_em* m, int32_t n_topics, int32_t* idx_out, double* weight_out) {
  return guard([&] {
    STC_REQUIRE(m, "em");
    em::top_topics(*m, n_topics, idx_out, weight_out);
  });
}

}  // extern "C"
