// wave_sort.h — one wave sorts up to 1024 int32 keys in registers (device only): the bitonic network of
// hashing_tf.hip (HashingTF's documents, the E-step row order) and count_vectorizer.hip (k_tf_sort_docs),
// the heads of its sorted runs, and the choice of keys per lane from a document's length.
//
// Layout: 64·P keys, P per lane, element lane·P + p in register p of the lane.  Pads are INT32_MAX, so
// they sort last.
//
// bench.py ties profiles/r06_featurisation_pmc.json to the bytes of hashing_tf.hip, idf.hip and
// stc_internal.h only: a change to this header alone does not invalidate that profile, so re-measure it
// (tools/gpu.sh feat) after one.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

namespace stc {

constexpr int kSortCap = 1024;  // ≤ 16 keys per lane; longer documents go to hipcub's segmented radix sort
constexpr int kDocWaves = 4;    // documents in flight per workgroup of the per-document kernels (one per wave)

// x from lane ^ lx without the LDS crossbar where a DPP pattern exists (round 4: every shuffle of the
// network was a ds_bpermute, ~60 % of the sort): xor 1 / 2 quad_perm, xor 4 = half-row mirror (xor 7)
// after quad_perm xor 3, xor 8 = row rotate by 8; xor 16 ds_swizzle (no address VGPR); xor 32 bpermute.
__device__ __forceinline__ int32_t shfl_xor_dpp(int32_t v, int lx) {
  switch (lx) {
    case 1: return __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, false);   // quad_perm [1,0,3,2]
    case 2: return __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]
    case 4: return __builtin_amdgcn_mov_dpp(__builtin_amdgcn_mov_dpp(v, 0x1B, 0xF, 0xF, false),  // [3,2,1,0]
                                            0x141, 0xF, 0xF, false);     // row_half_mirror
    case 8: return __builtin_amdgcn_mov_dpp(v, 0x128, 0xF, 0xF, false);  // row_ror:8
    case 16: return __builtin_amdgcn_ds_swizzle(v, 0x401F);              // and 0x1F, xor 0x10
    default: return __shfl_xor(v, lx, 64);
  }
}

// Σ over the wave of a per-lane count in [0, P] from bit-sliced ballots (scalar popcounts, no shuffles)
template <int P>
__device__ __forceinline__ int wave_sum_small(int v) {
  int tot = 0;
#pragma unroll
  for (int b = 0; (1 << b) <= P; ++b) tot += __popcll(__ballot((v >> b) & 1)) << b;
  return tot;
}
// the exclusive prefix of such a count over the lanes below this one
template <int P>
__device__ __forceinline__ int wave_excl_small(int v) {
  int pre = 0;
#pragma unroll
  for (int b = 0; (1 << b) <= P; ++b) {
    const uint64_t m = __ballot((v >> b) & 1);
    pre += (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)) << b;
  }
  return pre;
}

// partners at distance j ≥ P across lanes (lane ^ (j / P), same register), j < P inside the lane
template <int P>
__device__ __forceinline__ void bitonic_regs(int32_t (&x)[P], int lane) {
  constexpr int m = 64 * P;  // fully unrolled: every partner distance is a constant
#pragma unroll
  for (int k = 2; k <= m; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (j >= P) {
        const int lx = j / P;
#pragma unroll
        for (int p = 0; p < P; ++p) {
          const int e = lane * P + p;
          const int32_t o = shfl_xor_dpp(x[p], lx);
          const bool lower = (e & j) == 0, asc = (e & k) == 0;
          x[p] = (lower == asc) ? min(x[p], o) : max(x[p], o);
        }
      } else {
#pragma unroll
        for (int p = 0; p < P; ++p) {
          const int q = p ^ j;
          if (q > p) {
            const int e = lane * P + p;
            const bool asc = (e & k) == 0;
            const int32_t a = x[p], b = x[q];
            x[p] = asc ? min(a, b) : max(a, b);
            x[q] = asc ? max(a, b) : min(a, b);
          }
        }
      }
    }
  }
}

// the distinct keys among the first n of the sorted keys (wave total): element lane·P + p heads a run when
// it differs from its predecessor.  (hashing_tf.hip's emit_runs needs the flags themselves and keeps its
// own loop: built on a shared one, k_doc_hash_emit's register allocation moved.)
template <int P>
__device__ __forceinline__ int count_runs(const int32_t (&x)[P], int n, int lane) {
  const int32_t prev_last = __shfl_up(x[P - 1], 1, 64);
  int heads = 0;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int q = lane * P + p;
    const int32_t prev = p == 0 ? prev_last : x[p - 1];
    heads += (q < n && (q == 0 || x[p] != prev)) ? 1 : 0;
  }
  return wave_sum_small<P>(heads);
}

// f(integral_constant<int, P>) for the keys per lane of a document of n ≤ 64·HI keys: the smallest power of
// two P in [LO, HI] with 64·P ≥ n
template <int P, int LO, int HI>
using KeysPerLane = std::integral_constant<int, (P < LO ? LO : (P > HI ? HI : P))>;
template <int LO, int HI, typename F>
__device__ __forceinline__ void with_keys_per_lane(int n, F&& f) {
  static_assert(LO >= 1 && LO <= HI && HI <= kSortCap / 64, "powers of two in [1, 16]");
  // one flat chain (a recursive form cost k_tf_sort_docs two VGPRs and a wave of occupancy); the branches
  // outside [LO, HI) are constant-false, and clamping their P keeps them from instantiating f anew
  if (LO <= 1 && 1 < HI && n <= 64) f(KeysPerLane<1, LO, HI>{});
  else if (LO <= 2 && 2 < HI && n <= 128) f(KeysPerLane<2, LO, HI>{});
  else if (LO <= 4 && 4 < HI && n <= 256) f(KeysPerLane<4, LO, HI>{});
  else if (LO <= 8 && 8 < HI && n <= 512) f(KeysPerLane<8, LO, HI>{});
  else f(KeysPerLane<HI, LO, HI>{});
}

}  // namespace stc
