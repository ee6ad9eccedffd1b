// lda_step_kernels.h — host-side launch API of the online-LDA step outside the E-step: the sstats SpMM
// (lda_sstats.hip), the M-step and the bound's topics part (lda_mstep.hip) and the batch / bookkeeping
// kernels (lda_batch.hip).  The E-step kernels' API is lda_kernels.h.
#pragma once

#include "stc_internal.h"

namespace stc {
namespace lda {

constexpr int kChunk = 256;           // sorted entries per wave in the sstats segmented SpMM
constexpr int kRowsPerBlock = 64;     // terms per workgroup in the λ update
constexpr int kLogphatBlocks = 2048;

// ---- lda_batch.hip ---------------------------------------------------------------------

// Batch partition: slots [0, n_short) = members with nnz <= cap (wave kernel), then the rest.
void launch_part_flags(hipStream_t s, const int64_t* indptr, const int32_t* batch, int64_t n,
                       int64_t cap, int64_t* nnz_out, int32_t* short_flag);
void launch_part_scatter(hipStream_t s, const int32_t* batch, const int64_t* nnz, int64_t n,
                         const int32_t* short_flag, const int32_t* short_incl, int32_t* batch_p,
                         int32_t* orig_p, int64_t* nnz_p);
void launch_sample(hipStream_t s, const int64_t* indptr, int64_t D, double fraction, int with_repl,
                   uint64_t seed, int64_t iteration, int rank, int64_t cap, int32_t* counts,
                   int64_t* weights, int32_t* short_counts);
// writes partitioned slots: batch_p (row), orig_p (raw member position), nnz_p
void launch_fill_batch(hipStream_t s, const int64_t* indptr, int64_t D, int64_t cap,
                       const int32_t* counts, const int32_t* count_incl,
                       const int32_t* short_incl, int64_t n_short, int32_t* batch_p,
                       int32_t* orig_p, int64_t* nnz_p);
// out[0..2] = {*a, *b, *c} (the inclusive scans' totals for one readback)
void launch_last3(hipStream_t s, const int32_t* a, const int64_t* b, const int32_t* c, int64_t* out);
void launch_permute_slots(hipStream_t s, const int32_t* idx, int64_t n, const int32_t* batch, const int32_t* orig,
                          const int64_t* nnz, int32_t* batch2, int32_t* orig2, int64_t* nnz2);
void launch_iota(hipStream_t s, int32_t* x, int64_t n);
template <typename T>
void launch_sum_vals(hipStream_t s, const T* x, int64_t n, double* out);
void launch_iter_stats(hipStream_t s, const int32_t* iters, const int32_t* nonempty, int64_t n,
                       int max_iter, int64_t* out4 /* sum, max, caphits, nonempty */,
                       int64_t* cum2 /* += Σiters, caphits; may be null */);
// γ₀ of n slots' members (gamma_sample, keyed as the E-step kernels key it) into out[member·k + t]
template <typename T>
void launch_gamma0(hipStream_t s, const int32_t* batch, const int32_t* orig, int64_t n, int k, uint64_t seed,
                   int64_t iteration, int rank, int key_mode, int64_t doc_id_base, double shape, T* out);
// STC_MIXED (lda_online.hip mixed_resolve): the fp32 E-step's documents past `thr` iterations, listed for the fp64
// re-solve (nnz ≤ cap64 from position 0 up, cnt[0]; the rest from n − 1 down, cnt[1]) ...
void launch_mixed_list(hipStream_t s, const int64_t* indptr, const int32_t* batch, const int32_t* orig,
                       const int64_t* bptr, const int32_t* iters, const int32_t* nonempty, int64_t n, int thr,
                       int64_t cap64, int32_t* lbatch, int32_t* lorig, int64_t* lbptr, int32_t* lslot, int32_t* cnt);
// ... and their fp64 outputs written back into the fp32 step buffers (γ when gamma is given)
void launch_mixed_fixup(hipStream_t s, const int64_t* indptr, const int32_t* lbatch, const int32_t* lorig,
                        const int64_t* lbptr, const int32_t* lslot, int64_t n, int ms, int ml, int k, int kp,
                        const double* eth64, const double* elogth64, const double* r64, const double* gamma64,
                        float* eth, float* elogth, float* r, uint64_t* vals, float* gamma);

// ---- lda_sstats.hip --------------------------------------------------------------------

// The multi-GPU stat layout for a reduce-scatter per vocabulary sub-chunk (lda_online.hip train_tail): rank
// r's slice [r·vs, (r+1)·vs) is cut into nsub sub-chunks of vsj rows (the last one the rest), and
// sub-chunk j of every slice is stored together, in rank order, at physical rows [n·j·vsj, …) — so
// sub-chunk j is ONE contiguous reduce-scatter of n pieces.  sub ≥ 0 restricts an sstats launch to the
// terms of sub-chunk j (the entries, their sort order and the chunk grid are the whole launch's, so
// every row's fp64 sum associates exactly as in the single launch); sub < 0: canonical rows, every term.
struct StatMap {
  uint32_t vs = 0, vsj = 0;
  int n = 1, nsub = 1, sub = -1;
};
__host__ __device__ __forceinline__ int stat_sub(const StatMap& m, uint32_t v) {
  const uint32_t j = (v % m.vs) / m.vsj;
  return j < (uint32_t)(m.nsub - 1) ? (int)j : m.nsub - 1;
}
// (rank, sub-chunk) group of a term: the groups are contiguous term ranges, in term order
__host__ __device__ __forceinline__ uint32_t stat_group(const StatMap& m, uint32_t v) {
  return (v / m.vs) * (uint32_t)m.nsub + (uint32_t)stat_sub(m, v);
}
__host__ __device__ __forceinline__ int64_t stat_row(const StatMap& m, uint32_t v) {
  if (m.sub < 0) return (int64_t)v;
  const uint32_t r = v / m.vs, rem = v - r * m.vs;
  const int j = stat_sub(m, v);
  const int64_t w = j < m.nsub - 1 ? (int64_t)m.vsj : (int64_t)m.vs - (int64_t)(m.nsub - 1) * m.vsj;
  return (int64_t)m.n * j * m.vsj + (int64_t)r * w + (rem - (int64_t)j * m.vsj);
}

// stamp (one rank, canonical rows only; may be null): stamp[v] = sid for every row v this launch writes, so
// the M-step can tell this step's rows from stale ones and stat needs no clearing (launch_lambda_eeb)
template <typename T>
void launch_sstats(hipStream_t s, const uint32_t* skeys, const uint64_t* svals, int64_t E,
                   const T* r, const T* eth, int kp, T* stat, T* headbuf, T* tailbuf,
                   const StatMap& map = StatMap{}, int32_t* stamp = nullptr, int32_t sid = 0);
void launch_entry_pairs(hipStream_t s, const int64_t* indptr, const int32_t* indices, const int32_t* batch,
                        const int64_t* bptr, int64_t n, uint32_t* keys, uint64_t* vals);
template <typename T>
void launch_unscale_stat(hipStream_t s, const T* stat, const double* logscale, const double* psic, int64_t V,
                         int k, int kp, double* out_vk);

// ---- lda_mstep.hip ---------------------------------------------------------------------

// the fused M-step pass (update = true: λ update; both: expElogβ' rows, logscale, colsum partials)
// Bp64 (STC_MIXED, T = float only; may be null): the same rows in fp64 at the same m_v, for the re-solve.
// stamp (may be null): rows with stamp[v] ≠ sid take stat = 0 without reading stat / Bp (launch_sstats)
template <typename T>
void launch_lambda_eeb(hipStream_t s, bool update, double* lam, const T* stat, T* Bp, double* logscale,
                       int64_t V, int k, int kp, double rho, double scale, double eta, const double* gate,
                       double* colpart, int64_t nblocks, double* Bp64 = nullptr, const int32_t* stamp = nullptr,
                       int32_t sid = 0);
// colsum (block order), psic[0, k) = ψ(colsum), psic[k, 2k) = exp(−ψ(colsum))
void launch_colsum_reduce(hipStream_t s, const double* colpart, int64_t nblocks, int k,
                          const double* gate, double* colsum, double* psic);
template <typename T>
void launch_logphat(hipStream_t s, const T* elogth, const int32_t* nonempty, int64_t n, int k,
                    double* small /* k+1 */, double* part /* kLogphatBlocks × (k+1) scratch */);
void launch_update_alpha(hipStream_t s, double* alpha, const double* small, int k, double rho);
void launch_init_lambda(hipStream_t s, double* lam, int64_t V, int k, uint64_t seed, double shape);
void launch_topics_bound(hipStream_t s, const double* lam, const double* colsum, int64_t V, int k,
                         double eta, double* partials, int64_t nblocks);
void launch_to_f32(hipStream_t s, const double* in, float* out, int64_t n);

}  // namespace lda
}  // namespace stc
