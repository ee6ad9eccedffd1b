// lda.hip — the workgroup E-step of online variational-Bayes LDA for gfx950 (K6 of SURVEY.md §7): the
// kernel for documents past the fast kernels' row capacity (lda_grid.hip, lda_rows64.hip, lda_wide.hip,
// lda_team64.hip).  The rest of a step is in lda_sstats.hip, lda_mstep.hip and lda_batch.hip.
//
// It restates one upstream function of spark-mllib 2.4.3 (TextClustering/build.sbt:10), reached from
// lda.run(corpus) at LDAClustering.scala:61 and toLocal.topicDistribution at LDALoader.scala:108:
//   k_estep          [U] OnlineLDAOptimizer.variationalTopicInference (+ LocalLDAModel
//                    logLikelihoodBound corpusPart when BOUND)
//
// Numerics: expElogβ is stored ROW-SCALED and without its per-topic factor,
// Bp[v][t] = exp(ψ(λ_vt) − m_v) with m_v = max_t ψ(λ_vt); the E-step iterates with
// eθ' = exp(ψ(γ_t) − ψ(max γ) − ψ(Σ_v λ_vt)).  Bp·eθ' = e^{-m_v}·expElogβ·exp(ψ(γ) − ψ(max γ)), so
// both scales cancel exactly in γ ← eθ ⊙ Bᵀ(cts/(B·eθ)) + α and in batchResult = stat ⊙ expElogβ:
// the recursion is Spark's, but nothing underflows in fp32 (Spark's unscaled exp(Elogβ) reaches
// 1e-50 for rare terms).  The bound adds m_v and max E[log θ] back in fp64.
#include "estep_common.h"

namespace stc {
namespace lda {

template <typename T>
struct VecOf;
template <>
struct VecOf<float> {
  typedef float type __attribute__((ext_vector_type(4)));
  static constexpr int W = 4;
};
template <>
struct VecOf<double> {
  typedef double type __attribute__((ext_vector_type(2)));
  static constexpr int W = 2;
};

// Spark adds 1e-100 to φ = B·eθ (unscaled).  In the row/doc-scaled space that epsilon becomes
// ε'_n = 1e-100 / (exp(m_v)·exp(max E[log θ])) = exp(kLogEps − m_v − lmax), kLogEps = ln(1e-100)
// (estep_common.h): it keeps Spark's behaviour for terms whose unscaled expElogβ underflows (they
// contribute nothing in Spark).
template <typename T>
__device__ __forceinline__ T eps_floor() { return T(1.17549435e-38); }  // FLT_MIN (f32 only)
template <>
__device__ __forceinline__ double eps_floor<double>() { return 0.0; }
// BOUND: a dot product below this may have lost products to underflow (each below FLT_MIN / DBL_MIN, so all k of
// them are a negligible part of a dot at the floor); such a row's token term is evaluated in log space
template <typename T>
__device__ __forceinline__ T lse_floor() { return T(1e-25); }
template <>
__device__ __forceinline__ double lse_floor<double>() { return 1e-280; }

template <typename T, typename VT>
__device__ __forceinline__ T hsum(VT v);
template <>
__device__ __forceinline__ float hsum<float, VecOf<float>::type>(VecOf<float>::type v) {
  return (v.x + v.y) + (v.z + v.w);
}
template <>
__device__ __forceinline__ double hsum<double, VecOf<double>::type>(VecOf<double>::type v) {
  return v.x + v.y;
}

__device__ __forceinline__ float exp_t(float x) { return __expf(x); }
__device__ __forceinline__ float psi_t(float x) { return digamma_fast(x); }
__device__ __forceinline__ double psi_t(double x) { return digamma_t<double>(x); }
__device__ __forceinline__ double exp_t(double x) { return exp(x); }
// eθ' = exp(x − ψc_t): fp64 subtracts ψc_t in the argument, fp32 multiplies by exp(−ψc_t) (EStepArgs::psic)
__device__ __forceinline__ double exp_minus_psic(double x, const double* psic, int k, int t) {
  (void)k;
  return exp(x - psic[t]);
}
__device__ __forceinline__ float exp_minus_psic(float x, const double* psic, int k, int t) {
  return __expf(x) * (float)psic[k + t];
}

template <typename T>
__host__ __device__ constexpr int part_elems(int kp) {
  return (256 * VecOf<T>::W > kp) ? 256 * VecOf<T>::W : kp;
}

template <typename T>
size_t estep_lds_bytes(int kp, int lds_rows, int P) {
  size_t b = 0;
  b += 2 * (size_t)kp * sizeof(T);                 // eth, gam
  b += (size_t)part_elems<T>(kp) * sizeof(T);      // partial column sums
  b += 16 * sizeof(double);                        // reduction scratch
  b += (size_t)lds_rows * sizeof(int32_t);         // ids   (lds_rows % 4 == 0)
  b += 3 * (size_t)lds_rows * sizeof(T);           // cts, r, ln(1e-100) − m_v
  b += (size_t)lds_rows * P * sizeof(T);           // the document block B
  return b;
}

template <typename T>
int estep_lds_rows(int k, int kp, int P) {
  (void)k;
  const size_t fixed = estep_lds_bytes<T>(kp, 0, P);
  const size_t per_row = sizeof(int32_t) + 3 * sizeof(T) + (size_t)P * sizeof(T);
  if (fixed >= (size_t)kLdsBudget) return 0;
  int rows = (int)(((size_t)kLdsBudget - fixed) / per_row);
  return rows & ~3;
}

// ---------------------------------------------------------------------------------------
// K6: the E-step.  One 256-thread workgroup per document; the hardware dispatcher balances the
// data-dependent trip counts.  LDS=true keeps the gathered nnz×k block in LDS (rows padded to
// P with P/W odd ⇒ conflict-free row-per-lane ds_read_b128); LDS=false streams it from L2.
// Per inner iteration: φ_n = B_n·eθ' (row per lane), r_n = cts_n/φ_n, s = Bᵀr (column groups ×
// row subsets, partials in LDS), γ = eθ'⊙s + α, eθ' = exp(ψ(γ) − ψ(max γ)), meanΔγ ≤ 1e-3 stops.
// ---------------------------------------------------------------------------------------
template <typename T, bool STATS, bool BOUND, bool LDS>
__device__ __forceinline__ void estep_doc(const EStepArgs<T>& a, unsigned char* smem, int64_t slot,
                                          int64_t mem, int64_t row, int64_t s0, int nnz, int64_t e0) {
  using VT = typename VecOf<T>::type;
  constexpr int W = VecOf<T>::W;
  const int tid = threadIdx.x;
  const int k = a.k, kp = a.kp, ncg = kp / W, P = a.P;
  const int rows_cap = a.lds_rows;

  T* s_eth = reinterpret_cast<T*>(smem);
  T* s_gam = s_eth + kp;
  T* s_part = s_gam + kp;
  double* s_red = reinterpret_cast<double*>(s_part + part_elems<T>(kp));
  int32_t* s_ids = reinterpret_cast<int32_t*>(s_red + 16);
  T* s_cts = reinterpret_cast<T*>(s_ids + rows_cap);
  T* s_r = s_cts + rows_cap;
  T* s_lse = s_r + rows_cap;
  T* s_B = s_lse + rows_cap;

  const int32_t* ids = LDS ? s_ids : a.indices + s0;
  const T* cts = LDS ? s_cts : a.values + s0;
  T* rr = LDS ? s_r : a.r + e0;

  // -- load ids / counts (LDS) and detect an all-zero document (Spark's numNonzeros == 0)
  int nz = 0;
  for (int n = tid; n < nnz; n += kBlock) {
    const int32_t id = a.indices[s0 + n];
    const T c = a.values[s0 + n];
    if (LDS) {
      s_ids[n] = id;
      s_cts[n] = c;
      s_lse[n] = (T)(kLogEps - a.logscale[id]);
    }
    nz |= (c != T(0));
  }
  const bool nonempty = __syncthreads_or(nz) != 0;
  if (!nonempty) {
    for (int t = tid; t < k; t += kBlock) {
      if (a.gamma) a.gamma[mem * k + t] = T(0);
      if (STATS) a.elogth[slot * k + t] = T(0);
    }
    if (STATS)
      for (int t = tid; t < kp; t += kBlock) a.eth[slot * kp + t] = T(0);
    for (int n = tid; n < nnz; n += kBlock) {
      a.r[e0 + n] = T(0);
      if (STATS) {
        a.keys[e0 + n] = (uint32_t)a.indices[s0 + n];
        a.vals[e0 + n] = entry_val<T>(slot, e0 + n, T(0));
      }
    }
    if (tid == 0) {
      if (a.iters) a.iters[mem] = 0;
      if (a.nonempty) a.nonempty[mem] = 0;
      if (BOUND) a.bound[mem] = 0.0;
    }
    return;
  }

  // -- gather the document block B[n][:] = Bp[ids[n]][:] into LDS
  if (LDS) {
    const int total = nnz * ncg;
#pragma unroll 4
    for (int w = tid; w < total; w += kBlock) {
      const int n = w / ncg;
      const int c = w - n * ncg;
      const VT v = *reinterpret_cast<const VT*>(a.Bp + (int64_t)s_ids[n] * kp + c * W);
      *reinterpret_cast<VT*>(s_B + n * P + c * W) = v;
    }
  }

  // -- γ₀ (injected or counter RNG) and eθ'
  uint64_t stream = 0;
  if (!a.gamma0) {
    const uint64_t key = a.key_mode == 0 ? train_doc_key(a.iteration, a.rank, mem)
                                         : (uint64_t)(a.doc_id_base + row);
    stream = doc_stream(a.seed, key);
  }
  double gsum = 0.0, gmax = -INFINITY, dummy = 0.0;
  for (int t = tid; t < kp; t += kBlock) {
    T g = T(0);
    if (t < k) {
      g = a.gamma0 ? a.gamma0[mem * k + t] : (T)gamma_sample(stream, t, a.gamma_shape);
      gsum += (double)g;
      gmax = fmax(gmax, (double)g);
    }
    s_gam[t] = g;
  }
  block_reduce3(gsum, dummy, gmax, s_red);
  T lmax = psi_t((T)gmax) - psi_t((T)gsum);  // max_t E[log θ_t]
  {
    const T psimax = psi_t((T)gmax);
    for (int t = tid; t < kp; t += kBlock)
      s_eth[t] = t < k ? exp_minus_psic(psi_t(s_gam[t]) - psimax, a.psic, k, t) : T(0);
  }
  __syncthreads();

  const int R = ncg >= kBlock ? 1 : kBlock / ncg;  // row subsets in the Bᵀr product
  const int nwork = R * ncg;
  int it = 0;
  bool done = false;
  double b_tok = 0.0, c_tok = 0.0;  // BOUND: Σ cts·(log φ'_n + m_v), Σ cts
  while (true) {
    // Phase A: φ_n = B_n · eθ', r_n = cts_n / φ_n
    for (int n = tid; n < nnz; n += kBlock) {
      const T* Brow = LDS ? s_B + n * P : a.Bp + (int64_t)ids[n] * kp;
      VT acc = (VT)T(0);
      for (int c = 0; c < ncg; ++c)
        acc += *reinterpret_cast<const VT*>(Brow + c * W) * *reinterpret_cast<const VT*>(s_eth + c * W);
      const T dot = hsum<T, VT>(acc);
      const T lse = LDS ? s_lse[n] : (T)(kLogEps - a.logscale[ids[n]]);
      const T phi = dot + fmax(exp_t(lse - lmax), eps_floor<T>());
      const T cn = cts[n];
      rr[n] = cn / phi;
      // logSumExp: no epsilon (with λ at hand the token terms are taken after the loop instead, see there)
      if (BOUND && !a.lam && (done || it >= a.max_iter) && cn != T(0)) {
        b_tok += (double)cn * ((double)log(fmax(dot, eps_floor<T>())) + a.logscale[ids[n]]);
        c_tok += (double)cn;
      }
    }
    __syncthreads();
    if (done || it >= a.max_iter) break;

    // Phase B: partial column sums s_j[c] = Σ_{n ≡ j mod R} B[n][c]·r_n
    for (int w = tid; w < nwork; w += kBlock) {
      const int c = w % ncg;
      const int j = w / ncg;
      VT acc = (VT)T(0);
      for (int n = j; n < nnz; n += R) {
        const T* Brow = LDS ? s_B + n * P : a.Bp + (int64_t)ids[n] * kp;
        acc += *reinterpret_cast<const VT*>(Brow + c * W) * rr[n];
      }
      *reinterpret_cast<VT*>(s_part + j * kp + c * W) = acc;
    }
    __syncthreads();

    // Phase C: γ ← eθ' ⊙ s + α ; Σ|Δγ|, Σγ, max γ
    double dsum = 0.0;
    gsum = 0.0;
    gmax = -INFINITY;
    for (int t = tid; t < k; t += kBlock) {
      T s = T(0);
      for (int j = 0; j < R; ++j) s += s_part[j * kp + t];
      const T g = s_eth[t] * s + (T)a.alpha[t];
      dsum += fabs((double)g - (double)s_gam[t]);
      s_gam[t] = g;
      gsum += (double)g;
      gmax = fmax(gmax, (double)g);
    }
    block_reduce3(dsum, gsum, gmax, s_red);

    // Phase D: eθ' = exp(ψ(γ) − ψ(max γ)) ; meanGammaChange = Σ|Δγ| / k
    const T psimax = psi_t((T)gmax);
    lmax = psimax - psi_t((T)gsum);
    for (int t = tid; t < k; t += kBlock) s_eth[t] = exp_minus_psic(psi_t(s_gam[t]) - psimax, a.psic, k, t);
    ++it;
    done = dsum / (double)k <= 1e-3;
    __syncthreads();
  }

  // -- outputs
  const double psisum = digamma_t<double>(gsum);
  for (int t = tid; t < k; t += kBlock) {
    if (a.gamma) a.gamma[mem * k + t] = s_gam[t];
    if (STATS) a.elogth[slot * k + t] = (T)(digamma_t<double>((double)s_gam[t]) - psisum);
  }
  if (STATS) {
    for (int t = tid; t < kp; t += kBlock) a.eth[slot * kp + t] = s_eth[t];
    for (int n = tid; n < nnz; n += kBlock) {
      const T rv = LDS ? s_r[n] : a.r[e0 + n];  // the L2 path wrote r before the block barrier
      if (LDS) a.r[e0 + n] = rv;
      a.keys[e0 + n] = (uint32_t)ids[n];
      a.vals[e0 + n] = entry_val<T>(slot, e0 + n, rv);
    }
  }
  if (tid == 0) {
    if (a.iters) a.iters[mem] = it;
    if (a.nonempty) a.nonempty[mem] = 1;
  }
  if (BOUND) {
    // E[log p(doc|θ,β)] = Σ_n cts_n (log φ'_n + m_v + max E[log θ]);  E[log p(θ|α) − log q(θ|γ)]
    const double elog_max = digamma_t<double>(gmax) - psisum;
    double topic = 0.0, asum = 0.0, dummy2 = -INFINITY;
    for (int t = tid; t < k; t += kBlock) {
      const double g = (double)s_gam[t], al = a.alpha[t];
      const double el = digamma_t<double>(g) - psisum;
      topic += (al - g) * el + (lgamma(g) - lgamma(al));
      asum += al;
    }
    // With λ at hand (a.lam) the token terms are formed here, from the last pass's dot products computed once
    // more, so that one comparison decides a row's form: log(dot) + m_v as above, or — a dot under lse_floor has
    // lost products to underflow — [U] logLikelihoodBound's own cnt · logSumExp_t(E[log θ_t] + E[log β_vt]) with
    // E[log β_vt] = ψ(λ_vt) − ψ(Σ_v λ_vt).  The block takes a round's marked rows one at a time.  Block-uniform.
    double lse_tok = 0.0;
    if (a.lam) {
      for (int base = 0; base < nnz; base += kBlock) {
        const int n = base + tid;
        T mark = T(0);
        if (n < nnz && cts[n] != T(0)) {
          const T* Brow = LDS ? s_B + n * P : a.Bp + (int64_t)ids[n] * kp;
          VT acc = (VT)T(0);
          for (int c = 0; c < ncg; ++c)
            acc += *reinterpret_cast<const VT*>(Brow + c * W) * *reinterpret_cast<const VT*>(s_eth + c * W);
          const T dot = hsum<T, VT>(acc);
          if (dot < lse_floor<T>()) {
            mark = cts[n];
          } else {
            b_tok += (double)cts[n] * ((double)log(dot) + a.logscale[ids[n]]);
            c_tok += (double)cts[n];
          }
        }
        if (!__syncthreads_or(mark != T(0))) continue;
        s_part[tid] = mark;  // (free since the last Phase C)
        __syncthreads();
        for (int i = 0; i < kBlock && base + i < nnz; ++i) {
          const T cn = s_part[i];
          if (cn == T(0)) continue;
          const double* lrow = a.lam + (int64_t)ids[base + i] * k;
          double mx = -INFINITY, z0 = 0.0, z1 = 0.0;
          for (int t = tid; t < k; t += kBlock)
            mx = fmax(mx, (digamma_t<double>(lrow[t]) - a.psic[t]) + (digamma_t<double>((double)s_gam[t]) - psisum));
          block_reduce3(z0, z1, mx, s_red);
          double se = 0.0, dm = -INFINITY;
          for (int t = tid; t < k; t += kBlock)
            se += exp((digamma_t<double>(lrow[t]) - a.psic[t]) + (digamma_t<double>((double)s_gam[t]) - psisum) - mx);
          block_reduce3(se, z1, dm, s_red);
          lse_tok += (double)cn * (mx + log(se));
        }
        __syncthreads();  // s_part is rewritten by the next round
      }
    }
    double tok = b_tok + c_tok * elog_max;
    block_reduce3(tok, topic, dummy2, s_red);
    double as2 = asum, z = 0.0, dz = -INFINITY;
    block_reduce3(as2, z, dz, s_red);
    if (tid == 0) a.bound[mem] = (tok + lse_tok) + topic + (lgamma(as2) - lgamma(gsum));
  }
}

template <typename T, bool STATS, bool BOUND>
__global__ __launch_bounds__(kBlock) void k_estep(EStepArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  if ((int64_t)blockIdx.x >= a.n) return;
  const int64_t slot = a.slot0 + blockIdx.x;
  const int64_t mem = a.orig ? (int64_t)a.orig[slot] : slot;
  const int64_t row = a.batch ? (int64_t)a.batch[slot] : slot;
  const int64_t s0 = a.indptr[row];
  const int nnz = (int)(a.indptr[row + 1] - s0);
  const int64_t e0 = a.bptr ? a.bptr[slot] : s0;
  if (nnz <= a.lds_rows)
    estep_doc<T, STATS, BOUND, true>(a, smem, slot, mem, row, s0, nnz, e0);
  else
    estep_doc<T, STATS, BOUND, false>(a, smem, slot, mem, row, s0, nnz, e0);
}

// a kernel's dynamic-LDS limit: kLdsBudget, which holds every launch that keeps block rows in LDS — or, where
// the fixed arrays alone pass it (fp64 kp > 3408: 24·kp + 128 B, 98,432 B at kp = 4096, lds_rows = 0), their
// size.  `have` is the kernel's registered limit (0: none yet).
static void reserve_estep_lds(const void* kern, size_t lds, size_t& have) {
  if (lds <= have) return;
  const size_t want = lds > (size_t)kLdsBudget ? lds : (size_t)kLdsBudget;
  HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want));
  have = want;
}

template <typename T>
void launch_estep(hipStream_t s, const EStepArgs<T>& a, bool stats, bool bound) {
  if (a.n == 0) return;
  const size_t lds = estep_lds_bytes<T>(a.kp, a.lds_rows, a.P);
  const dim3 grid((unsigned)a.n);
  if (stats) {
    static size_t have = 0;
    reserve_estep_lds((const void*)k_estep<T, true, false>, lds, have);
    k_estep<T, true, false><<<grid, kBlock, lds, s>>>(a);
  } else if (bound) {
    static size_t have = 0;
    reserve_estep_lds((const void*)k_estep<T, false, true>, lds, have);
    k_estep<T, false, true><<<grid, kBlock, lds, s>>>(a);
  } else {
    static size_t have = 0;
    reserve_estep_lds((const void*)k_estep<T, false, false>, lds, have);
    k_estep<T, false, false><<<grid, kBlock, lds, s>>>(a);
  }
  KERNEL_CHECK();
}

#define STC_INSTANTIATE(T)                                                     \
  template size_t estep_lds_bytes<T>(int, int, int);                           \
  template int estep_lds_rows<T>(int, int, int);                               \
  template void launch_estep<T>(hipStream_t, const EStepArgs<T>&, bool, bool);

STC_INSTANTIATE(float)
STC_INSTANTIATE(double)

}  // namespace lda
}  // namespace stc
