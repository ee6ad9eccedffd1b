// lda_mstep.hip — the M-step of online variational-Bayes LDA and the bound's topics part for gfx950
// (K8–K12 of SURVEY.md §7).
//
// Each kernel restates one upstream function of spark-mllib 2.4.3 (TextClustering/build.sbt:10),
// reached from lda.run(corpus) at LDAClustering.scala:61:
//   k_lambda_eeb     [U] submitMiniBatch `statsSum ⊙ expElogβᵀ` + updateLambda, and in the same
//                    pass the rows of exp(LDAUtils.dirichletExpectation(λ)) (+ .t)
//   k_update_alpha   [U] updateAlpha (Newton step on α)
//   k_topics_bound   [U] logLikelihoodBound topicsPart
// with the model's λ₀ draw and its exports (topic-major λ, fp32 copies).  The row-scaled expElogβ' is
// lda.hip's numerics note.
#include <algorithm>

#include "estep_common.h"
#include "lda_step_kernels.h"

namespace stc {
namespace lda {

// ---------------------------------------------------------------------------------------
// M-step.  λ is fp64 V×k (term-major, Spark's topicsMatrix orientation); rows of RB terms per
// workgroup, lanes over topics, fixed-order per-topic partial sums (deterministic colsum).
// ---------------------------------------------------------------------------------------

// expElogβ'[v][t] = exp(ψ(λ_vt) − m_v), m_v ≈ max_t ψ(λ_vt): the ROW-scaled part of Spark's
// exp(dirichletExpectation(λ)) — the per-topic factor exp(−ψ(Σ_v λ_vt)) is applied to eθ by the
// E-step (EStepArgs::psic), so a row needs only its own λ and the pass fuses with the λ update.
// m_v only has to be common to the row and to logscale, not the exact maximum: the fp32 build takes
// it from an fp32 DPP max and evaluates the exponential as 2^n · 2^f with the integer/fraction split
// done in fp64, so the fp32 argument never loses the bits of a large |ψ(λ)|.  The fp64 build takes
// m_v = ψ(max_t λ_vt) (ψ is increasing: one ψ per row instead of one per element) and evaluates
// exp(ψ(λ) − m_v) as exp_digamma_minus_d, without a logarithm per element (round 6: config 5's
// M-step was fp64-VALU-bound, 2,934 → 2,337 instructions per row at k = 2000).
__device__ __forceinline__ float exp_scaled(double x, float) {
  const double y = x * 1.4426950408889634;  // log2 e
  const double n = floor(y);
  return __builtin_amdgcn_ldexpf(__builtin_amdgcn_exp2f((float)(y - n)), (int)n);
}
__device__ __forceinline__ double exp_scaled(double x, double) { return exp(x); }
__device__ __forceinline__ double row_max(double m, float) {
  return (double)wave_max_dpp((float)m);
}
__device__ __forceinline__ double row_max(double m, double) { return wave_max(m); }

// The M-step in ONE pass over the vocabulary rows ([U] submitMiniBatch `statsSum ⊙ expElogβᵀ` +
// updateLambda, then the next minibatch's expElogβ): per row v
//   λ_v ← (1−ρ)λ_v + ρ(stat_v ⊙ Bp_v·D/|B| + η)     (UPDATE; stat ⊙ Bp = Spark's batchResult, §4)
//   Bp_v ← exp(ψ(λ_v) − m_v), logscale_v = m_v      (the next E-step's rows)
// and per block of kRowsPerBlock rows the per-topic partials of Σ_v λ_vt (colpart), reduced by
// k_colsum_reduce in block order.  One wave per row (lane = topic mod 64, Q topics per lane), the
// four waves of a block take rows w, w+4, …; the block's partials are added in wave order, so colsum
// is identical for any vocabulary slicing that keeps the blocks (§6).  UPDATE = false: colsum
// partials and Bp of the current λ (set_topics / init_random).
// five workgroups per CU (≤ 102 VGPRs, no spills; the default budget took 106 and four): the pass is
// latency-bound, one row in flight per wave — M-step 0.361 → 0.330 ms at the headline (6: 48 B of scratch
// per lane, 0.41 ms; the next row's loads issued before this row's ψ / exp, measured slower)
template <typename T, int Q, bool UPDATE>
__global__ __launch_bounds__(256, 5) void k_lambda_eeb(double* __restrict__ lam, const T* __restrict__ stat,
                                                    T* __restrict__ Bp, double* __restrict__ logscale,
                                                    int64_t V, int k, int kp, double rho, double scale,
                                                    double eta, const double* __restrict__ gate,
                                                    double* __restrict__ colpart, double* __restrict__ Bp64,
                                                    const int32_t* __restrict__ stamp, int32_t sid) {
  if (gate && !(gate[0] > 0.0)) return;  // Spark: no non-empty docs ⇒ no update
  __shared__ double s_acc[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t v0 = (int64_t)blockIdx.x * kRowsPerBlock;
  constexpr int QC = Q < 4 ? Q : 4;  // topics per lane whose loads are issued together
  double acc[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) acc[q] = 0.0;
  for (int i = w; i < kRowsPerBlock; i += 4) {
    const int64_t v = v0 + i;
    if (v >= V) break;
    double e[Q];
    double m = -INFINITY;
    // a row no sstats launch of this step wrote (stamp ≠ sid) holds stale sums: read as 0, as the cleared
    // stat row was (0·Bp·scale + η = η bit for bit), and its stat / Bp bytes are not fetched
    const bool live = !UPDATE || !stamp || stamp[v] == sid;
#pragma unroll
    for (int q0 = 0; q0 < Q; q0 += QC) {
      double lv[QC], sv[QC], bv[QC];
#pragma unroll
      for (int j = 0; j < QC; ++j) {
        const int t = lane + 64 * (q0 + j);
        lv[j] = t < k ? lam[v * k + t] : 1.0;
        if (UPDATE) {
          sv[j] = live && t < k ? (double)stat[v * kp + t] : 0.0;
          bv[j] = live && t < k ? (double)Bp[v * kp + t] : 0.0;
        }
      }
#pragma unroll
      for (int j = 0; j < QC; ++j) {
        const int q = q0 + j, t = lane + 64 * q;
        double nl = lv[j];
        if (UPDATE) nl = (1.0 - rho) * nl + rho * (sv[j] * bv[j] * scale + eta);
        if (t < k) {
          if (UPDATE) lam[v * k + t] = nl;
          acc[q] += nl;
        }
        if constexpr (sizeof(T) == 8) {  // ψ is increasing: max_t ψ(λ_vt) = ψ(max_t λ_vt)
          e[q] = nl;
          if (t < k) m = fmax(m, nl);
        } else {
          e[q] = t < k ? digamma_fast_d(nl) : -INFINITY;
          m = fmax(m, e[q]);
        }
      }
    }
    m = row_max(m, T());
    T* br = Bp + v * kp;
    if constexpr (sizeof(T) == 8) {  // one ψ per row, and exp(ψ(λ) − m_v) without a logarithm per element
      m = digamma_fast_d(m);
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const int t = lane + 64 * q;
        if (t < kp) br[t] = t < k ? exp_digamma_minus_d(e[q], m) : 0.0;
      }
    } else {
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const int t = lane + 64 * q;
        if (t < kp) br[t] = t < k ? exp_scaled(e[q] - m, T()) : T(0);
      }
    }
    if constexpr (sizeof(T) == 4) {  // STC_MIXED: the fp64 rows of the re-solve, at the same m_v
      if (Bp64) {
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          const int t = lane + 64 * q;
          if (t < kp) Bp64[v * kp + t] = t < k ? exp(e[q] - m) : 0.0;
        }
      }
    }
    if (lane == 0) logscale[v] = m;
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    s_acc[w][lane] = acc[q];
    __syncthreads();
    const int t = lane + 64 * q;
    if (w == 0 && t < k)
      colpart[(int64_t)blockIdx.x * k + t] = ((s_acc[0][lane] + s_acc[1][lane]) + s_acc[2][lane]) + s_acc[3][lane];
    __syncthreads();
  }
}

// The same pass for many topics (kp > 256): a row per WORKGROUP — thread i owns topics i + 256·j — so
// the loads of a row are spread over 256 lanes instead of one wave's Q·3 registers, and the next row's
// loads are issued before this row's ψ/exp work (software pipelined).  The row max crosses the four
// waves through LDS (double-buffered by row parity: one barrier per row).  Each topic's colsum partial
// is one thread's running sum over the block's rows in row order.
template <typename T, int Q, bool UPDATE>
__global__ __launch_bounds__(256, Q <= 8 ? 3 : 1) void k_lambda_eeb_wide(double* __restrict__ lam, const T* __restrict__ stat,
                                                         T* __restrict__ Bp, double* __restrict__ logscale,
                                                         int64_t V, int k, int kp, double rho, double scale,
                                                         double eta, const double* __restrict__ gate,
                                                         double* __restrict__ colpart, double* __restrict__ Bp64,
                                                         const int32_t* __restrict__ stamp, int32_t sid) {
  if (gate && !(gate[0] > 0.0)) return;
  __shared__ double s_max[2][4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t v0 = (int64_t)blockIdx.x * kRowsPerBlock;
  const int nrow = (int)((V - v0) < kRowsPerBlock ? (V - v0 > 0 ? V - v0 : 0) : kRowsPerBlock);
  double acc[Q], lv[Q], sv[Q], bv[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) acc[q] = 0.0;
  auto load = [&](int64_t v) {
    const bool live = !UPDATE || !stamp || stamp[v] == sid;  // (as k_lambda_eeb)
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int t = tid + 256 * q;
      lv[q] = t < k ? lam[v * k + t] : 1.0;
      if (UPDATE) {
        sv[q] = live && t < k ? (double)stat[v * kp + t] : 0.0;
        bv[q] = live && t < k ? (double)Bp[v * kp + t] : 0.0;
      }
    }
  };
  if (nrow > 0) load(v0);
  for (int i = 0; i < nrow; ++i) {
    const int64_t v = v0 + i;
    double e[Q];
    double m = -INFINITY;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int t = tid + 256 * q;
      double nl = lv[q];
      if (UPDATE) nl = (1.0 - rho) * nl + rho * (sv[q] * bv[q] * scale + eta);
      if (t < k) {
        if (UPDATE) lam[v * k + t] = nl;
        acc[q] += nl;
      }
      e[q] = nl;
    }
    if (i + 1 < nrow) load(v + 1);  // the next row's loads fly during this row's ψ / exp
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int t = tid + 256 * q;
      if constexpr (sizeof(T) == 8) {  // (as k_lambda_eeb) the row max of λ, one ψ per row
        if (t < k) m = fmax(m, e[q]);
      } else {
        e[q] = t < k ? digamma_fast_d(e[q]) : -INFINITY;
        m = fmax(m, e[q]);
      }
    }
    m = row_max(m, T());
    if (lane == 0) s_max[i & 1][w] = m;
    __syncthreads();
    m = fmax(fmax(s_max[i & 1][0], s_max[i & 1][1]), fmax(s_max[i & 1][2], s_max[i & 1][3]));
    T* br = Bp + v * kp;
    if constexpr (sizeof(T) == 8) {
      m = digamma_fast_d(m);
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const int t = tid + 256 * q;
        if (t < kp) br[t] = t < k ? exp_digamma_minus_d(e[q], m) : 0.0;
      }
    } else {
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const int t = tid + 256 * q;
        if (t < kp) br[t] = t < k ? exp_scaled(e[q] - m, T()) : T(0);
      }
    }
    if constexpr (sizeof(T) == 4) {  // STC_MIXED: the fp64 rows of the re-solve, at the same m_v
      if (Bp64) {
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          const int t = tid + 256 * q;
          if (t < kp) Bp64[v * kp + t] = t < k ? exp(e[q] - m) : 0.0;
        }
      }
    }
    if (tid == 0) logscale[v] = m;
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int t = tid + 256 * q;
    if (t < k) colpart[(int64_t)blockIdx.x * k + t] = acc[q];
  }
}

template <typename T>
void launch_lambda_eeb(hipStream_t s, bool update, double* lam, const T* stat, T* Bp, double* logscale,
                       int64_t V, int k, int kp, double rho, double scale, double eta, const double* gate,
                       double* colpart, int64_t nblocks, double* Bp64, const int32_t* stamp, int32_t sid) {
  if (nblocks <= 0) return;
  if (kp > 256) {  // a row per workgroup
    const int qw = (kp + 255) / 256;
#define STC_LEEBW(QQ)                                                                                    \
  do {                                                                                                   \
    if (update)                                                                                          \
      k_lambda_eeb_wide<T, QQ, true><<<(unsigned)nblocks, 256, 0, s>>>(lam, stat, Bp, logscale, V, k, kp, \
                                                                        rho, scale, eta, gate, colpart,   \
                                                                        Bp64, stamp, sid);               \
    else                                                                                                 \
      k_lambda_eeb_wide<T, QQ, false><<<(unsigned)nblocks, 256, 0, s>>>(lam, stat, Bp, logscale, V, k,    \
                                                                         kp, rho, scale, eta, gate, colpart, \
                                                                         Bp64, stamp, sid);              \
  } while (0)
    if (qw <= 2) STC_LEEBW(2);
    else if (qw <= 4) STC_LEEBW(4);
    else if (qw <= 8) STC_LEEBW(8);
    else if (qw <= 16) STC_LEEBW(16);
    else throw Error(STC_ERR_INVALID_ARG, "k > 4096 topics is not supported");
#undef STC_LEEBW
    KERNEL_CHECK();
    return;
  }
  const int q = (kp + 63) / 64;
#define STC_LEEB(QQ)                                                                                    \
  do {                                                                                                  \
    if (update)                                                                                         \
      k_lambda_eeb<T, QQ, true><<<(unsigned)nblocks, 256, 0, s>>>(lam, stat, Bp, logscale, V, k, kp,   \
                                                                   rho, scale, eta, gate, colpart, Bp64, stamp, sid); \
    else                                                                                                \
      k_lambda_eeb<T, QQ, false><<<(unsigned)nblocks, 256, 0, s>>>(lam, stat, Bp, logscale, V, k, kp,  \
                                                                    rho, scale, eta, gate, colpart, Bp64, stamp, sid); \
  } while (0)
  if (q <= 1) STC_LEEB(1);
  else if (q <= 2) STC_LEEB(2);
  else STC_LEEB(4);
#undef STC_LEEB
  KERNEL_CHECK();
}

// colsum_t = Σ_b colpart[b][t] in block order, psic_t = ψ(colsum_t) (the E-step's per-topic factor of
// expElogβ) and psic_{k+t} = exp(−ψ(colsum_t))
__global__ __launch_bounds__(256) void k_colsum_reduce(const double* __restrict__ colpart,
                                                       int64_t nblocks, int k,
                                                       const double* __restrict__ gate,
                                                       double* __restrict__ colsum, double* __restrict__ psic) {
  if (gate && !(gate[0] > 0.0)) return;
  __shared__ double s[256];
  const int t = blockIdx.x;
  double acc = 0.0;
  for (int64_t b = threadIdx.x; b < nblocks; b += 256) acc += colpart[b * k + t];
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    colsum[t] = s[0];
    const double pc = digamma_fast_d(s[0]);
    psic[t] = pc;
    psic[k + t] = exp(-pc);  // the fp32 kernels' multiplier (an fp32 exponent argument would lose its low bits)
  }
}

void launch_colsum_reduce(hipStream_t s, const double* colpart, int64_t nblocks, int k,
                          const double* gate, double* colsum, double* psic) {
  k_colsum_reduce<<<k, 256, 0, s>>>(colpart, nblocks, k, gate, colsum, psic);
  KERNEL_CHECK();
}

// logphat = Σ_docs E[log θ_d] (fixed order) ; small[k] = #non-empty docs.  Two passes: kLogphatBlocks
// blocks each sum a contiguous range of docs with lanes along the (coalesced) topic rows, then one
// block adds the block partials in block order — the same tree every run.
template <typename T>
__global__ __launch_bounds__(256) void k_logphat_part(const T* __restrict__ elogth,
                                                      const int32_t* __restrict__ nonempty, int64_t n,
                                                      int k, double* __restrict__ part) {
  // block b sums docs [b·per, (b+1)·per) for column t = threadIdx.x (+256·c): four independent loads
  // in flight per thread, the rows of a step contiguous across the block's threads
  const int64_t per = (n + gridDim.x - 1) / gridDim.x;
  const int64_t i0 = (int64_t)blockIdx.x * per, i1 = i0 + per < n ? i0 + per : n;
  for (int t = threadIdx.x; t <= k; t += 256) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t i = i0; i < i1; i += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t iu = i + u;
        if (iu < i1) acc[u] += t < k ? (double)elogth[iu * k + t] : (double)nonempty[iu];
      }
    }
    part[(int64_t)blockIdx.x * (k + 1) + t] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  }
}
// column t's kLogphatBlocks partials: 256 threads × (kLogphatBlocks / 256) loads, then a fixed tree
__global__ __launch_bounds__(256) void k_logphat_final(const double* __restrict__ part, int nb, int k,
                                                       double* __restrict__ small) {
  __shared__ double s[256];
  const int t = blockIdx.x;
  double acc = 0.0;
  for (int b = threadIdx.x; b < nb; b += 256) acc += part[(int64_t)b * (k + 1) + t];
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) small[t] = s[0];
}

template <typename T>
void launch_logphat(hipStream_t s, const T* elogth, const int32_t* nonempty, int64_t n, int k,
                    double* small, double* part) {
  k_logphat_part<T><<<kLogphatBlocks, 256, 0, s>>>(elogth, nonempty, n, k, part);
  KERNEL_CHECK();
  k_logphat_final<<<k + 1, 256, 0, s>>>(part, kLogphatBlocks, k, small);
  KERNEL_CHECK();
}

// updateAlpha: one Newton step; applied only when every α_t + ρ·dα_t > 0
__global__ __launch_bounds__(256) void k_update_alpha(double* __restrict__ alpha,
                                                      const double* __restrict__ small, int k,
                                                      double rho) {
  extern __shared__ double s_g[];  // gradf[k], q[k]
  __shared__ double s_r[4 * 4];
  const double N = small[k];
  if (!(N > 0.0)) return;
  double* s_q = s_g + k;
  double asum = 0.0, z = 0.0, dz = -INFINITY;
  for (int t = threadIdx.x; t < k; t += 256) asum += alpha[t];
  block_reduce3(asum, z, dz, s_r);
  const double psis = digamma_t<double>(asum);
  double a1 = 0.0, a2 = 0.0;
  for (int t = threadIdx.x; t < k; t += 256) {
    const double al = alpha[t];
    const double g = N * (-(digamma_t<double>(al) - psis) + small[t] / N);
    const double q = -N * trigamma_d(al);
    s_g[t] = g;
    s_q[t] = q;
    a1 += g / q;
    a2 += 1.0 / q;
  }
  double dz2 = -INFINITY;
  block_reduce3(a1, a2, dz2, s_r);
  const double c = N * trigamma_d(asum);
  const double b = a1 / (1.0 / c + a2);
  double bad = 0.0, z2 = 0.0, dz3 = -INFINITY;
  for (int t = threadIdx.x; t < k; t += 256) {
    const double da = -(s_g[t] - b) / s_q[t];
    s_g[t] = da;
    if (!(rho * da + alpha[t] > 0.0)) bad += 1.0;
  }
  block_reduce3(bad, z2, dz3, s_r);
  if (bad == 0.0)
    for (int t = threadIdx.x; t < k; t += 256) alpha[t] += rho * s_g[t];
}

void launch_update_alpha(hipStream_t s, double* alpha, const double* small, int k, double rho) {
  // gradf and q: 16·k B, 64 KiB at k = 4096 beside the kernel's static words — past the default limit of a
  // launch from k = 4089, so the largest request (k ≤ 4096, stc_lda_create) is registered once
  static bool set = false;
  if (!set) {
    HIP_CHECK(hipFuncSetAttribute((const void*)k_update_alpha, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(2 * sizeof(double) * 4096)));
    set = true;
  }
  k_update_alpha<<<1, 256, 2 * sizeof(double) * k, s>>>(alpha, small, k, rho);
  KERNEL_CHECK();
}

// λ₀ ~ Gamma(shape, 1/shape) i.i.d., keyed by the k×V element index (identical on every rank)
__global__ __launch_bounds__(256) void k_init_lambda(double* __restrict__ lam, int64_t V, int k,
                                                     uint64_t seed, double shape) {
  const int64_t total = V * k;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t v = e / k;
    const int t = (int)(e - v * k);
    lam[e] = gamma_sample(doc_stream(seed, (uint64_t)t * (uint64_t)V + (uint64_t)v), 0, shape);
  }
}

void launch_init_lambda(hipStream_t s, double* lam, int64_t V, int k, uint64_t seed, double shape) {
  k_init_lambda<<<2048, 256, 0, s>>>(lam, V, k, seed, shape);
  KERNEL_CHECK();
}

// topicsPart of logLikelihoodBound: Σ(η−λ)·Elogβ + Σ(lgamma λ − lgamma η) over the V×k elements; the
// per-topic Σ_k (lgamma(ηV) − lgamma Σ_v λ_vk) term is added on the host (lda_online.hip topics_part)
__global__ __launch_bounds__(256) void k_topics_bound(const double* __restrict__ lam,
                                                      const double* __restrict__ colsum, int64_t V,
                                                      int k, double eta, double* __restrict__ partials) {
  extern __shared__ double s_psic[];
  __shared__ double s_r[16];
  for (int t = threadIdx.x; t < k; t += 256) s_psic[t] = digamma_t<double>(colsum[t]);
  __syncthreads();
  const int64_t total = V * k;
  const double lge = lgamma(eta);
  double acc = 0.0, z = 0.0, dz = -INFINITY;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int t = (int)(e % k);
    const double l = lam[e];
    const double eb = digamma_t<double>(l) - s_psic[t];
    acc += (eta - l) * eb + (lgamma(l) - lge);
  }
  block_reduce3(acc, z, dz, s_r);
  if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

void launch_topics_bound(hipStream_t s, const double* lam, const double* colsum, int64_t V, int k,
                         double eta, double* partials, int64_t nblocks) {
  k_topics_bound<<<(unsigned)nblocks, 256, sizeof(double) * k, s>>>(lam, colsum, V, k, eta, partials);
  KERNEL_CHECK();
}

__global__ void k_to_f32(const double* __restrict__ in, float* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = (float)in[i];
}
void launch_to_f32(hipStream_t s, const double* in, float* out, int64_t n) {
  if (n <= 0) return;
  k_to_f32<<<(unsigned)std::min<int64_t>(ceil_div(n, (int64_t)256), 65536), 256, 0, s>>>(in, out, n);
  KERNEL_CHECK();
}

#define STC_INSTANTIATE(T)                                                                        \
  template void launch_lambda_eeb<T>(hipStream_t, bool, double*, const T*, T*, double*, int64_t, int, \
                                     int, double, double, double, const double*, double*, int64_t, double*, \
                                     const int32_t*, int32_t);                                    \
  template void launch_logphat<T>(hipStream_t, const T*, const int32_t*, int64_t, int, double*, double*);

STC_INSTANTIATE(float)
STC_INSTANTIATE(double)

}  // namespace lda
}  // namespace stc
