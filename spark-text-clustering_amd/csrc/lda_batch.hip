// lda_batch.hip — the minibatch and bookkeeping kernels of an online-LDA step for gfx950: sampling the
// batch ([U] RDD.sample), partitioning its slots into short | long documents, slot permutations, γ₀ draws,
// the iteration statistics and plain sums, and the STC_MIXED list / write-back of the fp64 re-solve.
// None of them is on the hot path; each is a few lines around one grid-stride loop.
#include "lda_kernels.h"
#include "lda_step_kernels.h"

namespace stc {
namespace lda {

template <typename X>
__global__ __launch_bounds__(256) void k_sum(const X* __restrict__ x, int64_t n, double* __restrict__ out) {
  __shared__ double s[256];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) acc += (double)x[i];
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = s[0];
}

template <typename T>
void launch_sum_vals(hipStream_t s, const T* x, int64_t n, double* out) {
  k_sum<T><<<1, 256, 0, s>>>(x, n, out);
  KERNEL_CHECK();
}

__global__ void k_last3(const int32_t* a, const int64_t* b, const int32_t* c, int64_t* out) {
  if (threadIdx.x == 0) {
    out[0] = *a;
    out[1] = *b;
    out[2] = *c;
  }
}
void launch_last3(hipStream_t s, const int32_t* a, const int64_t* b, const int32_t* c, int64_t* out) {
  k_last3<<<1, 64, 0, s>>>(a, b, c, out);
  KERNEL_CHECK();
}

__global__ __launch_bounds__(1024) void k_iter_stats(const int32_t* __restrict__ iters,
                                                     const int32_t* __restrict__ nonempty, int64_t n,
                                                     int max_iter, int64_t* __restrict__ out4,
                                                     int64_t* __restrict__ cum2) {
  // one block (the cumulative counters need no atomics); 1024 threads with 16 loads each in flight
  __shared__ int64_t s[4][16];
  int64_t sum = 0, cap = 0, ne = 0;
  int mx = 0;
  for (int64_t b = 0; b < n; b += 16 * 1024) {
    int it[16], nz[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int64_t i = b + u * 1024 + threadIdx.x;
      it[u] = i < n ? iters[i] : 0;
      nz[u] = i < n ? nonempty[i] : 0;
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      sum += it[u];
      mx = it[u] > mx ? it[u] : mx;
      cap += (it[u] >= max_iter) ? 1 : 0;
      ne += nz[u];
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_xor(sum, o, 64);
    cap += __shfl_xor(cap, o, 64);
    ne += __shfl_xor(ne, o, 64);
    const int m2 = __shfl_xor(mx, o, 64);
    mx = m2 > mx ? m2 : mx;
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s[0][w] = sum;
    s[1][w] = mx;
    s[2][w] = cap;
    s[3][w] = ne;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t r[4] = {0, 0, 0, 0};
    for (int j = 0; j < 16; ++j) {
      r[0] += s[0][j];
      r[1] = s[1][j] > r[1] ? s[1][j] : r[1];
      r[2] += s[2][j];
      r[3] += s[3][j];
    }
    for (int j = 0; j < 4; ++j) out4[j] = r[j];
    if (cum2) {  // cumulative Σ iterations, cap hits
      cum2[0] += r[0];
      cum2[1] += r[2];
    }
  }
}

void launch_iter_stats(hipStream_t s, const int32_t* iters, const int32_t* nonempty, int64_t n,
                       int max_iter, int64_t* out4, int64_t* cum2) {
  k_iter_stats<<<1, 1024, 0, s>>>(iters, nonempty, n, max_iter, out4, cum2);
  KERNEL_CHECK();
}

// RDD.sample(withReplacement, fraction): Poisson(f) (with) or Bernoulli(f) (without) per doc
__global__ __launch_bounds__(256) void k_sample(const int64_t* __restrict__ indptr, int64_t D,
                                                double f, int with_repl, uint64_t seed,
                                                int64_t iteration, int rank, int64_t cap,
                                                int32_t* __restrict__ counts,
                                                int64_t* __restrict__ weights,
                                                int32_t* __restrict__ short_counts) {
  for (int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x; d < D; d += (int64_t)gridDim.x * 256) {
    const uint64_t st = doc_stream(seed ^ 0x5DEECE66Dull, train_doc_key(iteration, rank, d));
    const double u = rng_uniform(st, 0);
    int c = 0;
    if (with_repl) {
      double p = exp(-f), F = p;
      while (u > F && c < 64) {
        ++c;
        p *= f / c;
        F += p;
      }
    } else {
      c = u < f ? 1 : 0;
    }
    const int64_t nnz = indptr[d + 1] - indptr[d];
    counts[d] = c;
    weights[d] = (int64_t)c * nnz;
    short_counts[d] = nnz <= cap ? c : 0;
  }
}

void launch_sample(hipStream_t s, const int64_t* indptr, int64_t D, double fraction, int with_repl,
                   uint64_t seed, int64_t iteration, int rank, int64_t cap, int32_t* counts,
                   int64_t* weights, int32_t* short_counts) {
  int64_t g = ceil_div(D, 256);
  k_sample<<<(unsigned)(g > 8192 ? 8192 : g), 256, 0, s>>>(indptr, D, fraction, with_repl, seed,
                                                           iteration, rank, cap, counts, weights,
                                                           short_counts);
  KERNEL_CHECK();
}

// Members in doc order (raw position = count_incl[d] − c + j), written to partitioned slots:
// short docs (nnz <= cap) first, long docs after n_short.  All INCLUSIVE scans.
__global__ __launch_bounds__(256) void k_fill_batch(const int64_t* __restrict__ indptr, int64_t D,
                                                    int64_t cap, const int32_t* __restrict__ counts,
                                                    const int32_t* __restrict__ count_incl,
                                                    const int32_t* __restrict__ short_incl,
                                                    int64_t n_short, int32_t* __restrict__ batch_p,
                                                    int32_t* __restrict__ orig_p,
                                                    int64_t* __restrict__ nnz_p) {
  for (int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x; d < D; d += (int64_t)gridDim.x * 256) {
    const int c = counts[d];
    if (c == 0) continue;
    const int64_t nnz = indptr[d + 1] - indptr[d];
    const int64_t raw0 = (int64_t)count_incl[d] - c;
    const int64_t sh_before = (int64_t)short_incl[d] - (nnz <= cap ? c : 0);
    const int64_t slot0 = nnz <= cap ? sh_before : n_short + (raw0 - sh_before);
    for (int j = 0; j < c; ++j) {
      batch_p[slot0 + j] = (int32_t)d;
      orig_p[slot0 + j] = (int32_t)(raw0 + j);
      nnz_p[slot0 + j] = nnz;
    }
  }
}

void launch_fill_batch(hipStream_t s, const int64_t* indptr, int64_t D, int64_t cap,
                       const int32_t* counts, const int32_t* count_incl,
                       const int32_t* short_incl, int64_t n_short, int32_t* batch_p,
                       int32_t* orig_p, int64_t* nnz_p) {
  int64_t g = ceil_div(D, 256);
  k_fill_batch<<<(unsigned)(g > 8192 ? 8192 : g), 256, 0, s>>>(indptr, D, cap, counts, count_incl,
                                                               short_incl, n_short, batch_p, orig_p,
                                                               nnz_p);
  KERNEL_CHECK();
}

// slots [0, n) reordered by idx: out[i] = in[idx[i]] for the slot arrays
__global__ __launch_bounds__(256) void k_permute_slots(const int32_t* __restrict__ idx, int64_t n,
                                                       const int32_t* __restrict__ batch, const int32_t* __restrict__ orig,
                                                       const int64_t* __restrict__ nnz, int32_t* __restrict__ batch2,
                                                       int32_t* __restrict__ orig2, int64_t* __restrict__ nnz2) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int32_t j = idx[i];
    batch2[i] = batch[j];
    orig2[i] = orig[j];
    nnz2[i] = nnz[j];
  }
}
__global__ __launch_bounds__(256) void k_iota(int32_t* __restrict__ x, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) x[i] = (int32_t)i;
}
void launch_permute_slots(hipStream_t s, const int32_t* idx, int64_t n, const int32_t* batch, const int32_t* orig,
                          const int64_t* nnz, int32_t* batch2, int32_t* orig2, int64_t* nnz2) {
  if (n == 0) return;
  const int64_t g = ceil_div(n, 256);
  k_permute_slots<<<(unsigned)(g > 4096 ? 4096 : g), 256, 0, s>>>(idx, n, batch, orig, nnz, batch2, orig2, nnz2);
  KERNEL_CHECK();
}
void launch_iota(hipStream_t s, int32_t* x, int64_t n) {
  if (n == 0) return;
  const int64_t g = ceil_div(n, 256);
  k_iota<<<(unsigned)(g > 4096 ? 4096 : g), 256, 0, s>>>(x, n);
  KERNEL_CHECK();
}

// host-injected membership: flags + stable partition into [short | long] slots
__global__ __launch_bounds__(256) void k_part_flags(const int64_t* __restrict__ indptr,
                                                    const int32_t* __restrict__ batch, int64_t n,
                                                    int64_t cap, int64_t* __restrict__ nnz_out,
                                                    int32_t* __restrict__ short_flag) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t r = batch ? (int64_t)batch[i] : i;  // nullptr: identity rows
    const int64_t nnz = indptr[r + 1] - indptr[r];
    nnz_out[i] = nnz;
    short_flag[i] = nnz <= cap ? 1 : 0;
  }
}

void launch_part_flags(hipStream_t s, const int64_t* indptr, const int32_t* batch, int64_t n,
                       int64_t cap, int64_t* nnz_out, int32_t* short_flag) {
  if (n == 0) return;
  int64_t g = ceil_div(n, 256);
  k_part_flags<<<(unsigned)(g > 4096 ? 4096 : g), 256, 0, s>>>(indptr, batch, n, cap, nnz_out, short_flag);
  KERNEL_CHECK();
}

__global__ __launch_bounds__(256) void k_part_scatter(const int32_t* __restrict__ batch,
                                                      const int64_t* __restrict__ nnz, int64_t n,
                                                      const int32_t* __restrict__ short_flag,
                                                      const int32_t* __restrict__ short_incl,
                                                      int32_t* __restrict__ batch_p,
                                                      int32_t* __restrict__ orig_p,
                                                      int64_t* __restrict__ nnz_p) {
  const int64_t n_short = n > 0 ? short_incl[n - 1] : 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t sh = short_incl[i];
    const int64_t slot = short_flag[i] ? sh - 1 : n_short + (i - sh);
    batch_p[slot] = batch ? batch[i] : (int32_t)i;
    orig_p[slot] = (int32_t)i;
    nnz_p[slot] = nnz[i];
  }
}

void launch_part_scatter(hipStream_t s, const int32_t* batch, const int64_t* nnz, int64_t n,
                         const int32_t* short_flag, const int32_t* short_incl, int32_t* batch_p,
                         int32_t* orig_p, int64_t* nnz_p) {
  if (n == 0) return;
  int64_t g = ceil_div(n, 256);
  k_part_scatter<<<(unsigned)(g > 4096 ? 4096 : g), 256, 0, s>>>(batch, nnz, n, short_flag, short_incl,
                                                                 batch_p, orig_p, nnz_p);
  KERNEL_CHECK();
}

// γ₀ of a launch's members ahead of the E-step: one thread per (slot, topic), the counter RNG each
// E-step kernel would otherwise run in its prologue (the same gamma_sample, key and stream), written
// member-major for EStepArgs::gamma0.  The E-step prologues are latency-bound per document and the team
// kernels drew every topic of the document in every member; here the draws fill the chip.
template <typename T>
__global__ __launch_bounds__(256) void k_gamma0(const int32_t* __restrict__ batch, const int32_t* __restrict__ orig,
                                                int64_t n, int k, uint64_t seed, int64_t iteration, int rank,
                                                int key_mode, int64_t doc_id_base, double shape, T* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * k) return;
  const int64_t slot = i / k;
  const int t = (int)(i - slot * k);
  const int64_t mem = orig ? (int64_t)orig[slot] : slot;
  const int64_t row = batch ? (int64_t)batch[slot] : slot;
  const uint64_t key = key_mode == 0 ? train_doc_key(iteration, rank, mem) : (uint64_t)(doc_id_base + row);
  out[mem * k + t] = (T)gamma_sample(doc_stream(seed, key), t, shape);
}

template <typename T>
void launch_gamma0(hipStream_t s, const int32_t* batch, const int32_t* orig, int64_t n, int k, uint64_t seed,
                   int64_t iteration, int rank, int key_mode, int64_t doc_id_base, double shape, T* out) {
  if (n <= 0) return;
  k_gamma0<T><<<(unsigned)ceil_div(n * k, (int64_t)256), 256, 0, s>>>(batch, orig, n, k, seed, iteration, rank,
                                                                      key_mode, doc_id_base, shape, out);
  KERNEL_CHECK();
}

// ---- STC_MIXED: the fp64 re-solve of the fp32 E-step's slowly converging documents -------------------
// slots whose member is non-empty and took more than `thr` fp32 iterations: those with nnz ≤ cap64 (the fp64
// fast kernels' row capacity) from position 0 up (count cnt[0]), the others from position n − 1 down
// (count cnt[1]); each position holds the slot's row, member, entry offset and the slot itself.  The order
// within a list is the atomics' (every document's outputs are its own, so results do not depend on it).
__global__ void k_mixed_list(const int64_t* __restrict__ indptr, const int32_t* __restrict__ batch,
                             const int32_t* __restrict__ orig, const int64_t* __restrict__ bptr,
                             const int32_t* __restrict__ iters, const int32_t* __restrict__ nonempty, int64_t n,
                             int thr, int64_t cap64, int32_t* __restrict__ lbatch, int32_t* __restrict__ lorig,
                             int64_t* __restrict__ lbptr, int32_t* __restrict__ lslot, int32_t* __restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t mem = orig ? orig[i] : (int32_t)i;
  if (!nonempty[mem] || iters[mem] <= thr) return;
  const int64_t row = batch ? batch[i] : i;
  const int64_t nnz = indptr[row + 1] - indptr[row];
  const int64_t j = nnz <= cap64 ? (int64_t)atomicAdd(&cnt[0], 1) : n - 1 - (int64_t)atomicAdd(&cnt[1], 1);
  lbatch[j] = (int32_t)row;
  lorig[j] = mem;
  lbptr[j] = bptr ? bptr[i] : indptr[row];
  lslot[j] = (int32_t)i;
}
void launch_mixed_list(hipStream_t s, const int64_t* indptr, const int32_t* batch, const int32_t* orig,
                       const int64_t* bptr, const int32_t* iters, const int32_t* nonempty, int64_t n, int thr,
                       int64_t cap64, int32_t* lbatch, int32_t* lorig, int64_t* lbptr, int32_t* lslot, int32_t* cnt) {
  HIP_CHECK(hipMemsetAsync(cnt, 0, 2 * sizeof(int32_t), s));
  if (n <= 0) return;
  k_mixed_list<<<(unsigned)ceil_div(n, (int64_t)256), 256, 0, s>>>(indptr, batch, orig, bptr, iters, nonempty, n, thr,
                                                                  cap64, lbatch, lorig, lbptr, lslot, cnt);
  KERNEL_CHECK();
}
// the re-solved documents' fp64 outputs into the fp32 step buffers: eθ' and E[log θ] per slot, r and the
// sstats sort value (slot, fp32 r) per entry, γ per member (when given); one workgroup per listed document
// (list positions [0, ms) and [n − ml, n))
__global__ __launch_bounds__(256) void k_mixed_fixup(const int64_t* __restrict__ indptr, const int32_t* __restrict__ lbatch,
                                                     const int32_t* __restrict__ lorig, const int64_t* __restrict__ lbptr,
                                                     const int32_t* __restrict__ lslot, int64_t n, int ms, int ml, int k,
                                                     int kp, const double* __restrict__ eth64,
                                                     const double* __restrict__ elogth64, const double* __restrict__ r64,
                                                     const double* __restrict__ gamma64, float* __restrict__ eth,
                                                     float* __restrict__ elogth, float* __restrict__ r,
                                                     uint64_t* __restrict__ vals, float* __restrict__ gamma) {
  const int jj = blockIdx.x;
  const int64_t j = jj < ms ? jj : n - ml + (jj - ms);
  const int64_t slot = lslot[j], mem = lorig[j], row = lbatch[j], e0 = lbptr[j];
  const int64_t nnz = indptr[row + 1] - indptr[row];
  for (int t = threadIdx.x; t < kp; t += blockDim.x) {
    eth[slot * kp + t] = (float)eth64[j * kp + t];
    if (t < k) {
      elogth[slot * k + t] = (float)elogth64[j * k + t];
      if (gamma) gamma[mem * k + t] = (float)gamma64[mem * k + t];
    }
  }
  for (int64_t e = threadIdx.x; e < nnz; e += blockDim.x) {
    const float rv = (float)r64[e0 + e];
    r[e0 + e] = rv;
    if (vals) vals[e0 + e] = entry_val<float>(slot, e0 + e, rv);
  }
}
void launch_mixed_fixup(hipStream_t s, const int64_t* indptr, const int32_t* lbatch, const int32_t* lorig,
                        const int64_t* lbptr, const int32_t* lslot, int64_t n, int ms, int ml, int k, int kp,
                        const double* eth64, const double* elogth64, const double* r64, const double* gamma64,
                        float* eth, float* elogth, float* r, uint64_t* vals, float* gamma) {
  if (ms + ml <= 0) return;
  k_mixed_fixup<<<(unsigned)(ms + ml), 256, 0, s>>>(indptr, lbatch, lorig, lbptr, lslot, n, ms, ml, k, kp, eth64,
                                                    elogth64, r64, gamma64, eth, elogth, r, vals, gamma);
  KERNEL_CHECK();
}

#define STC_INSTANTIATE(T)                                                                        \
  template void launch_gamma0<T>(hipStream_t, const int32_t*, const int32_t*, int64_t, int, uint64_t, int64_t, \
                                 int, int, int64_t, double, T*);                                  \
  template void launch_sum_vals<T>(hipStream_t, const T*, int64_t, double*);

STC_INSTANTIATE(float)
STC_INSTANTIATE(double)

}  // namespace lda
}  // namespace stc
