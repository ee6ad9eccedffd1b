// estep_common.h — the device math of the LDA kernels, seen only by the translation units that use it
// (lda.hip, lda_grid.hip, lda_rows64.hip, lda_wide.hip, lda_team64.hip, lda_sstats.hip, lda_mstep.hip):
// Breeze's digamma / trigamma and their fast forms, the wave64 / block reductions with the permlane
// swaps, and — for the register-resident E-step kernels — Spark's φ epsilon in log space, the packed-FMA
// operand type, the reduce-scatter helpers and the diagnostic s_memtime stamps.
#pragma once

#include "lda_kernels.h"

namespace stc {

// ---------------------------------------------------------------------------------------
// Breeze 0.13.2 digamma / trigamma (recurrence to x > 5 + asymptotic series).
// ---------------------------------------------------------------------------------------
template <typename R>
__host__ __device__ inline R digamma_t(R x) {
  R r = 0;
  while (x <= R(5)) {
    r -= R(1) / x;
    x += R(1);
  }
  const R f = R(1) / (x * x);
  const R t = f * (R(-1.0 / 12.0) + f * (R(1.0 / 120.0) + f * (R(-1.0 / 252.0) + f * (R(1.0 / 240.0) +
              f * (R(-1.0 / 132.0) + f * (R(691.0 / 32760.0) + f * (R(-1.0 / 12.0) + f * R(3617.0) / R(8160.0))))))));
  return r + log(x) - R(0.5) / x + t;
}
// ln x for positive normal x: v_log_f32 (log2) · ln 2, without the denormal-range fixup __logf carries
__device__ __forceinline__ float ln_pos(float x) { return __builtin_amdgcn_logf(x) * 0.69314718055994531f; }
// fp32 digamma for the E-step inner loop: ψ(x) = ψ(x+4) − 1/x − (3x²+12x+11)/((x+1)(x+2)(x+3))
// unconditionally (no data-dependent loop ⇒ no lane divergence; the three shifted reciprocals share
// one v_rcp_f32, 1/x keeps its own for the small-γ end), v_log_f32, and Breeze's asymptotic series
// at x+4 ≥ 4 (first omitted term < 2e-9).  Accuracy vs the shift-6 form: tools/dg_check.py.
__device__ inline float digamma_fast(float x) {
  const float num = fmaf(fmaf(3.f, x, 12.f), x, 11.f);
  const float den = fmaf(fmaf(x + 6.f, x, 11.f), x, 6.f);
  const float r = __builtin_amdgcn_rcpf(x) + num * __builtin_amdgcn_rcpf(den);
  const float y = x + 4.f;
  const float iy = __builtin_amdgcn_rcpf(y);
  const float f = iy * iy;
  const float t = f * (-1.f / 12.f + f * (1.f / 120.f + f * (-1.f / 252.f + f * (1.f / 240.f + f * (-1.f / 132.f)))));
  return ln_pos(y) - 0.5f * iy + t - r;
}

// fp64 1/q from v_rcp_f64 and two Newton steps (≤ 1 ulp apart from the correctly rounded quotient)
__device__ __forceinline__ double rcp_nr(double q) {
  double r = __builtin_amdgcn_rcp(q);
  r = fma(r, fma(-q, r, 1.0), r);
  return fma(r, fma(-q, r, 1.0), r);
}
// Breeze evaluates its 8-term asymptotic series S8 at y_B = x + ⌊5 − x⌋ + 1 ∈ (5, 6]; the fast forms
// below evaluate it at x + 6 ∈ (6, 11] (one rational for the six recurrence terms).  S8's truncation
// error E(y) = ψ(y) − S8(y) reaches 8e-13 at y = 5, which a slowly-dying topic of a long E-step
// amplifies past 1e-7 relative, so the difference E(x + 6) − E(y_B) is added back: E(y) = f⁹·P(f),
// f = 1/y², P fitted to 7e-18 absolute on y ∈ [5, 11.5] (tools/fit_breeze_digamma.py).
__device__ __forceinline__ double breeze_trunc(double iy) {
  const double f = iy * iy, f2 = f * f, f4 = f2 * f2;
  return f4 * f4 * f * (-3.053401198888146 + f * (26.284421368293753 + f * (-260.94994774566294 +
                        f * (2372.137971404805 + f * -12318.55039822477))));
}
__device__ __forceinline__ double breeze_shift_fix(double x, double iy6, bool sh) {
  const double yb = sh ? x + (floor(5.0 - x) + 1.0) : 6.0;  // E needs ~1e-4 relative: raw v_rcp_f64
  return breeze_trunc(iy6) - breeze_trunc(__builtin_amdgcn_rcp(yb));
}
// fp64 digamma for the M-step's V×k elements, branch-free: Breeze's recurrence Σ_{i<6} 1/(x+i) for
// x ≤ 5 as one rational Q'(x)/Q(x), Q = x(x+1)…(x+5), the same 8-term asymptotic series at y = x + 6
// (or y = x when x > 5, where Breeze does not shift) and breeze_shift_fix.  Agrees with
// digamma_t<double> to a few ulp; the loop form costs a divergent chain of up to six fp64 divisions.
__device__ inline double digamma_fast_d(double x) {
  const bool sh = x <= 5.0;
  const double q = ((((((x + 15.0) * x + 85.0) * x + 225.0) * x + 274.0) * x + 120.0) * x);
  const double p = (((((6.0 * x + 75.0) * x + 340.0) * x + 675.0) * x + 548.0) * x + 120.0);
  const double iq = rcp_nr(sh ? q : 1.0);
  double c = p * iq;
  c = fma(fma(-q, c, p), iq, c);  // one residual correction of p/q
  const double y = sh ? x + 6.0 : x;
  const double iy = rcp_nr(y);
  const double f = iy * iy;
  const double t = f * (-1.0 / 12.0 + f * (1.0 / 120.0 + f * (-1.0 / 252.0 + f * (1.0 / 240.0 +
                   f * (-1.0 / 132.0 + f * (691.0 / 32760.0 + f * (-1.0 / 12.0 + f * (3617.0 / 8160.0))))))));
  return (sh ? breeze_shift_fix(x, iy, sh) - c : 0.0) + log(y) - 0.5 * iy + t;
}
// exp(ψ(x) − cst) for the fp64 E-step's eθ = exp(ψ(γ) − ψ(Σγ)), without the logarithm: with ψ(x) =
// ln y − 0.5/y + t(y) − s(x) as in digamma_fast_d, exp(ψ(x) − cst) = y · exp(t − 0.5/y − s − cst).
__device__ inline double exp_digamma_minus_d(double x, double cst) {
  const bool sh = x <= 5.0;
  const double q = ((((((x + 15.0) * x + 85.0) * x + 225.0) * x + 274.0) * x + 120.0) * x);
  const double p = (((((6.0 * x + 75.0) * x + 340.0) * x + 675.0) * x + 548.0) * x + 120.0);
  const double iq = rcp_nr(sh ? q : 1.0);
  double c = p * iq;
  c = fma(fma(-q, c, p), iq, c);
  const double y = sh ? x + 6.0 : x;
  const double iy = rcp_nr(y);
  const double f = iy * iy;
  const double t = f * (-1.0 / 12.0 + f * (1.0 / 120.0 + f * (-1.0 / 252.0 + f * (1.0 / 240.0 +
                   f * (-1.0 / 132.0 + f * (691.0 / 32760.0 + f * (-1.0 / 12.0 + f * (3617.0 / 8160.0))))))));
  return y * exp(((sh ? breeze_shift_fix(x, iy, sh) - c : 0.0) - 0.5 * iy + t) - cst);
}

__host__ __device__ inline double trigamma_d(double x) {
  double r = 0;
  while (x <= 5.0) {
    r += 1.0 / (x * x);
    x += 1.0;
  }
  const double f = 1.0 / (x * x);
  const double t = f * (1 / 6.0 + f * (-1 / 30.0 + f * (1 / 42.0 + f * (-1 / 30.0 + f * (5 / 66.0 +
                   f * (-691 / 2730.0 + f * (7 / 6.0 - f * 3617 / 510.0)))))));
  return r + 1.0 / x + f / 2.0 + t / x;
}

// ---------------------------------------------------------------------------------------
// Wave64 / block reductions
// ---------------------------------------------------------------------------------------
// fp32 wave64 all-reduce without LDS: two permlane swaps (across 32 / 16 lanes) and four DPP
// involutions inside each 16-lane row (row_mirror, row_half_mirror, quad_perm 1032 and 2301).
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  // all-lanes-valid permutations only (mirrors, quad_perm): bound_ctrl never fires, no `old` operand
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
// v_readlane of a float / double (wave-uniform lane index)
__device__ __forceinline__ float readlane_t(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
__device__ __forceinline__ double readlane_t(double v, int l) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), l);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
// max of two non-negative floats as an unsigned compare of their bits (no NaN canonicalisation)
__device__ __forceinline__ float max_nonneg(float a, float b) {
  return __builtin_bit_cast(float, max(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b)));
}
// Compiler hazard (ROCm 7.2 hipcc, gfx950): with __builtin_amdgcn_permlane{16,32}_swap the compiler
// sometimes reads the FIRST result register for both results (`v_add v0, v0, v0` after the swap;
// seen whenever both operands carry the same value, even through an opaque copy).  The swaps are
// therefore issued as inline asm with both registers in/out; `s_nop 1` covers the VALU-write →
// permlane-read hazard the compiler inserts for the builtin.  `volatile` keeps the compiler from
// re-materialising a swap inside a divergent branch (inactive partner lanes ⇒ garbage).
__device__ __forceinline__ void pswap32(unsigned& x, unsigned& y) {
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(x), "+v"(y));
}
__device__ __forceinline__ void pswap16(unsigned& x, unsigned& y) {
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(x), "+v"(y));
}
__device__ __forceinline__ float swap32_pair(float v, bool add, float w) {
  unsigned x = __builtin_bit_cast(unsigned, v), y = __builtin_bit_cast(unsigned, w);
  pswap32(x, y);
  const float a = __builtin_bit_cast(float, x), b = __builtin_bit_cast(float, y);
  return add ? a + b : fmaxf(a, b);
}
__device__ __forceinline__ float swap16_pair(float v, bool add, float w) {
  unsigned x = __builtin_bit_cast(unsigned, v), y = __builtin_bit_cast(unsigned, w);
  pswap16(x, y);
  const float a = __builtin_bit_cast(float, x), b = __builtin_bit_cast(float, y);
  return add ? a + b : fmaxf(a, b);
}
// Batched swaps: up to four independent swaps behind one hazard nop.
template <bool D32>
__device__ __forceinline__ void pswap_4(unsigned& a0, unsigned& b0, unsigned& a1, unsigned& b1, unsigned& a2,
                                        unsigned& b2, unsigned& a3, unsigned& b3) {
  if constexpr (D32)
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\tv_permlane32_swap_b32 %2, %3\n\t"
                 "v_permlane32_swap_b32 %4, %5\n\tv_permlane32_swap_b32 %6, %7"
                 : "+v"(a0), "+v"(b0), "+v"(a1), "+v"(b1), "+v"(a2), "+v"(b2), "+v"(a3), "+v"(b3));
  else
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\tv_permlane16_swap_b32 %2, %3\n\t"
                 "v_permlane16_swap_b32 %4, %5\n\tv_permlane16_swap_b32 %6, %7"
                 : "+v"(a0), "+v"(b0), "+v"(a1), "+v"(b1), "+v"(a2), "+v"(b2), "+v"(a3), "+v"(b3));
}
template <bool D32>
__device__ __forceinline__ void pswap_2(unsigned& a0, unsigned& b0, unsigned& a1, unsigned& b1) {
  if constexpr (D32)
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\tv_permlane32_swap_b32 %2, %3"
                 : "+v"(a0), "+v"(b0), "+v"(a1), "+v"(b1));
  else
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\tv_permlane16_swap_b32 %2, %3"
                 : "+v"(a0), "+v"(b0), "+v"(a1), "+v"(b1));
}
template <bool D32>
__device__ __forceinline__ void pswap_1(unsigned& a0, unsigned& b0) {
  if constexpr (D32) pswap32(a0, b0);
  else pswap16(a0, b0);
}
// reduce-scatter step over lane distance 32 (D32) or 16, N pairs: lanes with the role bit clear
// keep the xs set, the others the ys set; out[i] = this lane's kept value + the partner's
template <bool D32, int N>
__device__ __forceinline__ void swap_add_n(const float* xs, const float* ys, float* out) {
  unsigned x[N], y[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    x[i] = __builtin_bit_cast(unsigned, xs[i]);
    y[i] = __builtin_bit_cast(unsigned, ys[i]);
  }
  constexpr int N4 = N / 4 * 4;
#pragma unroll
  for (int b = 0; b < N4; b += 4) pswap_4<D32>(x[b], y[b], x[b + 1], y[b + 1], x[b + 2], y[b + 2], x[b + 3], y[b + 3]);
  if constexpr (N - N4 >= 2) pswap_2<D32>(x[N4], y[N4], x[N4 + 1], y[N4 + 1]);
  if constexpr ((N - N4) % 2 == 1) pswap_1<D32>(x[N - 1], y[N - 1]);
#pragma unroll
  for (int i = 0; i < N; ++i) out[i] = __builtin_bit_cast(float, x[i]) + __builtin_bit_cast(float, y[i]);
}
// three wave all-reduces at once (Σ a, Σ b, max c ≥ 0): the swaps share their hazard nops
__device__ __forceinline__ void wave_reduce3(float& a, float& b, float& c) {
  {
    unsigned a0 = __builtin_bit_cast(unsigned, a), a1 = a0, b0 = __builtin_bit_cast(unsigned, b), b1 = b0,
             c0 = __builtin_bit_cast(unsigned, c), c1 = c0, d0 = 0, d1 = 0;
    pswap_4<true>(a0, a1, b0, b1, c0, c1, d0, d1);
    a = __builtin_bit_cast(float, a0) + __builtin_bit_cast(float, a1);
    b = __builtin_bit_cast(float, b0) + __builtin_bit_cast(float, b1);
    c = max_nonneg(__builtin_bit_cast(float, c0), __builtin_bit_cast(float, c1));
  }
  {
    unsigned a0 = __builtin_bit_cast(unsigned, a), a1 = a0, b0 = __builtin_bit_cast(unsigned, b), b1 = b0,
             c0 = __builtin_bit_cast(unsigned, c), c1 = c0, d0 = 0, d1 = 0;
    pswap_4<false>(a0, a1, b0, b1, c0, c1, d0, d1);
    a = __builtin_bit_cast(float, a0) + __builtin_bit_cast(float, a1);
    b = __builtin_bit_cast(float, b0) + __builtin_bit_cast(float, b1);
    c = max_nonneg(__builtin_bit_cast(float, c0), __builtin_bit_cast(float, c1));
  }
  a += dpp_f<0x140>(a);
  b += dpp_f<0x140>(b);
  c = max_nonneg(c, dpp_f<0x140>(c));
  a += dpp_f<0x141>(a);
  b += dpp_f<0x141>(b);
  c = max_nonneg(c, dpp_f<0x141>(c));
  a += dpp_f<0xB1>(a);
  b += dpp_f<0xB1>(b);
  c = max_nonneg(c, dpp_f<0xB1>(c));
  a += dpp_f<0x4E>(a);
  b += dpp_f<0x4E>(b);
  c = max_nonneg(c, dpp_f<0x4E>(c));
}
__device__ __forceinline__ float wave_sum_dpp(float v) {
  v = swap32_pair(v, true, v);
  v = swap16_pair(v, true, v);
  v += dpp_f<0x140>(v);  // row_mirror
  v += dpp_f<0x141>(v);  // row_half_mirror
  v += dpp_f<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_f<0x4E>(v);   // quad_perm [2,3,0,1]
  return v;
}
__device__ __forceinline__ float wave_max_dpp(float v) {
  v = swap32_pair(v, false, v);
  v = swap16_pair(v, false, v);
  v = fmaxf(v, dpp_f<0x140>(v));
  v = fmaxf(v, dpp_f<0x141>(v));
  v = fmaxf(v, dpp_f<0xB1>(v));
  v = fmaxf(v, dpp_f<0x4E>(v));
  return v;
}

template <typename R>
__device__ inline R wave_sum(R v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <typename R>
__device__ inline R wave_max(R v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

namespace lda {

// ---------------------------------------------------------------------------------------
// Block (256 threads = 4 waves) reduction of (sum, sum, max) in a fixed order: deterministic.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void block_reduce3(double& a, double& b, double& c, double* s_red) {
  a = wave_sum(a);
  b = wave_sum(b);
  c = wave_max(c);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_red[w * 4 + 0] = a;
    s_red[w * 4 + 1] = b;
    s_red[w * 4 + 2] = c;
  }
  __syncthreads();
  a = (s_red[0] + s_red[4]) + (s_red[8] + s_red[12]);
  b = (s_red[1] + s_red[5]) + (s_red[9] + s_red[13]);
  c = fmax(fmax(s_red[2], s_red[6]), fmax(s_red[10], s_red[14]));
  __syncthreads();
}

constexpr double kLogEps = -230.25850929940458;  // ln(1e-100): Spark's φ epsilon (see lda.hip)
constexpr float kTiny = 1.17549435e-38f;         // FLT_MIN

typedef float f2 __attribute__((ext_vector_type(2)));  // v_pk_fma_f32 operand pair

constexpr int hup(int n) { return (n + 1) / 2; }

// reduce-scatter step through a DPP involution (row_mirror / row_half_mirror / quad_perm): lanes
// with the role bit clear keep topic set X, the others Y; the partner sends the set it drops.
template <int CTRL>
__device__ __forceinline__ float rs_dpp(float x, float y, bool hi) {
  const float keep = hi ? y : x;
  const float send = hi ? x : y;
  return keep + dpp_f<CTRL>(send);
}
// DPP controls (all lanes valid): row_mirror i↔15−i, row_half_mirror i↔7−i, row_ror:8 i↔i^8 (in a
// 16-lane row), quad_perm [3,2,1,0] i↔i^3, [1,0,3,2] i↔i^1, [2,3,0,1] i↔i^2
constexpr int DPP_ROW_MIRROR = 0x140, DPP_ROW_HALF_MIRROR = 0x141, DPP_ROW_ROR8 = 0x128,
              DPP_QP_3210 = 0x1B, DPP_QP_1032 = 0xB1, DPP_QP_2301 = 0x4E;

// ---- fp64 cross-lane helpers (lda_rows64.hip, lda_wide.hip): a double moves as two dwords
typedef unsigned long long u64;

__device__ __forceinline__ unsigned lo32(double v) { return (unsigned)__builtin_bit_cast(u64, v); }
__device__ __forceinline__ unsigned hi32(double v) { return (unsigned)(__builtin_bit_cast(u64, v) >> 32); }
__device__ __forceinline__ double mkd(unsigned lo, unsigned hi) {
  return __builtin_bit_cast(double, ((u64)hi << 32) | lo);
}
// 64-bit DPP move as two 32-bit moves (all-lanes-valid permutations only)
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_mov_dpp((int)lo32(v), CTRL, 0xF, 0xF, true);
  const unsigned hi = (unsigned)__builtin_amdgcn_mov_dpp((int)hi32(v), CTRL, 0xF, 0xF, true);
  return mkd(lo, hi);
}
template <int CTRL>
__device__ __forceinline__ double rs_dpp_d(double x, double y, bool hi) {
  const double keep = hi ? y : x;
  const double send = hi ? x : y;
  return keep + dpp_d<CTRL>(send);
}
// reduce-scatter over lane distance 32 (D32) or 16 for N double pairs: both dwords of each value go
// through one v_permlane*_swap each (two values per hazard nop)
template <bool D32, int N>
__device__ __forceinline__ void swap_add_nd(const double* xs, const double* ys, double* out) {
  unsigned xl[N], xh[N], yl[N], yh[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    xl[i] = lo32(xs[i]);
    xh[i] = hi32(xs[i]);
    yl[i] = lo32(ys[i]);
    yh[i] = hi32(ys[i]);
  }
  constexpr int N2 = N / 2 * 2;
#pragma unroll
  for (int b = 0; b < N2; b += 2)
    pswap_4<D32>(xl[b], yl[b], xh[b], yh[b], xl[b + 1], yl[b + 1], xh[b + 1], yh[b + 1]);
  if constexpr (N % 2 == 1) pswap_2<D32>(xl[N - 1], yl[N - 1], xh[N - 1], yh[N - 1]);
#pragma unroll
  for (int i = 0; i < N; ++i) out[i] = mkd(xl[i], xh[i]) + mkd(yl[i], yh[i]);
}
// The s-partial reduce-scatter of the grid E-steps (lda_rows64.hip, lda_team64.hip): lane = tl + 8·rl holds
// x[p] for its topic lane's KL ≤ 16 topics (zero-padded to 16); the eight row lanes rl (lane bits 3, 4, 5)
// are summed in a fixed order — bit 5 by permlane32 swaps, bit 4 by permlane16 swaps, bit 3 by row_ror:8 —
// so that lane (tl, rl) returns the wave sums of topics 2·rl and 2·rl + 1 of its topic lane.
__device__ __forceinline__ void rs_rows8(const double (&x)[16], int lane, double& s0, double& s1) {
  double a[8], b[4];
  swap_add_nd<true, 8>(x, x + 8, a);   // bit 5: topics [0, 8) | [8, 16)
  swap_add_nd<false, 4>(a, a + 4, b);  // bit 4: [0, 4) | [4, 8) of those
  const bool h3 = (lane & 8) != 0;     // bit 3: {0, 1} | {2, 3}
  s0 = rs_dpp_d<DPP_ROW_ROR8>(b[0], b[2], h3);
  s1 = rs_dpp_d<DPP_ROW_ROR8>(b[1], b[3], h3);
}

// fp64 wave64 all-reduce (sum) without LDS
__device__ __forceinline__ double wave_sum_d(double v) {
  {
    unsigned a = lo32(v), b = a, c = hi32(v), d = c;
    pswap_2<true>(a, b, c, d);
    v = mkd(a, c) + mkd(b, d);
  }
  {
    unsigned a = lo32(v), b = a, c = hi32(v), d = c;
    pswap_2<false>(a, b, c, d);
    v = mkd(a, c) + mkd(b, d);
  }
  v += dpp_d<DPP_ROW_MIRROR>(v);
  v += dpp_d<DPP_ROW_HALF_MIRROR>(v);
  v += dpp_d<DPP_QP_1032>(v);
  v += dpp_d<DPP_QP_2301>(v);
  return v;
}

// Diagnostic build only (make stamp → libstc_stamp.so, tools/stamp_estep.py): s_memtime stamps at
// the phase boundaries of the inner loop, summed per phase over every wave of a launch.  The
// product library compiles STAMP(i) to nothing.
#ifdef STC_STAMP
constexpr int kStamps = 12;
// one copy per translation unit (no relocatable device code): each TU exports its own reader
static __device__ unsigned long long g_stamps[kStamps];
__device__ __forceinline__ unsigned long long stamp_now() {
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}
#define STAMP_DECL unsigned long long st_acc[::stc::lda::kStamps] = {}, st_last = ::stc::lda::stamp_now();
#define STAMP(i)                                         \
  do {                                                   \
    const unsigned long long t_ = ::stc::lda::stamp_now(); \
    st_acc[i] += t_ - st_last;                           \
    st_last = t_;                                        \
  } while (0)
#define STAMP_FLUSH                                                  \
  if ((threadIdx.x & 63) == 0)                                       \
    for (int i_ = 0; i_ < ::stc::lda::kStamps; ++i_) atomicAdd(&::stc::lda::g_stamps[i_], st_acc[i_]);
// diagnostic reader: copies (and optionally clears) this TU's per-phase cycle sums
#define STC_STAMP_READER(NAME)                                                                  \
  extern "C" int NAME(unsigned long long* out, int n, int reset) {                              \
    if (n > ::stc::lda::kStamps) n = ::stc::lda::kStamps;                                       \
    if (hipDeviceSynchronize() != hipSuccess) return 3;                                         \
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(::stc::lda::g_stamps), n * sizeof(unsigned long long)) != hipSuccess) \
      return 3;                                                                                 \
    if (reset) {                                                                                \
      unsigned long long z[::stc::lda::kStamps] = {};                                           \
      if (hipMemcpyToSymbol(HIP_SYMBOL(::stc::lda::g_stamps), z, sizeof(z)) != hipSuccess) return 3; \
    }                                                                                           \
    return 0;                                                                                   \
  }
#else
#define STAMP_DECL
#define STAMP(i)
#define STAMP_FLUSH
#define STC_STAMP_READER(NAME)
#endif

}  // namespace lda
}  // namespace stc
