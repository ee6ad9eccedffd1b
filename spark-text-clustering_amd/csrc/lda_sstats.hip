// lda_sstats.hip — the sufficient statistics of an online-LDA step for gfx950 (K7 of SURVEY.md §7).
//
// It restates one upstream function of spark-mllib 2.4.3 (TextClustering/build.sbt:10), reached from
// lda.run(corpus) at LDAClustering.scala:61:
//   k_sstats/k_fixup [U] submitMiniBatch `stat(::, ids) += sstats` + treeReduce (per device)
// with the (term, slot) pairs an fp64 launch sorts beside the E-step (k_entry_pairs) and Spark's own
// sstats recovered from the scaled stat (k_unscale_stat; the scaling is lda.hip's numerics note).
#include "estep_common.h"
#include "lda_step_kernels.h"

namespace stc {
namespace lda {

// ---------------------------------------------------------------------------------------
// Sufficient statistics: stat[v][:] = Σ_{entries of term v} r_e · eθ'[doc(e)][:]  — a
// segmented SpMM over the batch's (term, slot) pairs radix-sorted by term.  One wave per chunk of
// kChunk sorted entries, lanes over topics; runs that cross chunk edges go to head/tail partials
// that k_fixup adds in chunk order.  Plain stores, no atomics, bitwise reproducible.
// Topics are processed in slabs of 64·Q columns (blockIdx.y, the slow grid dimension): each wave
// keeps kU·Q gathered eθ' values in flight without spilling at any k, and the waves running
// together share one slab of eθ' (≤ 100 MB at 50k docs) in the MALL.
// ---------------------------------------------------------------------------------------
template <typename T, int Q>
__global__ __launch_bounds__(256) void k_sstats(const uint32_t* __restrict__ skeys,
                                                const uint64_t* __restrict__ svals, int64_t E,
                                                const T* __restrict__ r,
                                                const T* __restrict__ eth, int kp, T* __restrict__ stat,
                                                T* __restrict__ headbuf, T* __restrict__ tailbuf,
                                                int64_t nchunks, StatMap map, int32_t* __restrict__ stamp,
                                                int32_t sid) {
  const int c0 = (int)blockIdx.y * 64 * Q;  // this slab's first topic column
  // kU entries in flight per wave: their (term, r, doc) are read out of the lanes that loaded them
  // (v_readlane: wave-uniform, so the eθ' row address is scalar) and their eθ' rows are all requested
  // before the first is accumulated — the gathers are served by L2 / MALL, and one row at a time
  // left the wave waiting a full round trip per entry.
  constexpr int kU = 8;
  const int lane = threadIdx.x & 63;
  const int64_t chunk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (chunk >= nchunks) return;
  const int64_t p0 = chunk * kChunk;
  const int64_t p1 = (p0 + kChunk < E) ? p0 + kChunk : E;
  const uint32_t first = skeys[p0], last = skeys[p1 - 1];
  const bool part = map.sub >= 0;  // a sub-chunk launch: only its terms' rows (StatMap)
  // a chunk inside one (rank, sub-chunk) term range of another launch has nothing of this one's
  if (part && stat_group(map, first) == stat_group(map, last) && stat_sub(map, first) != map.sub) return;
  const bool start_mid = p0 > 0 && skeys[p0 - 1] == first;
  const bool cont = p1 < E && skeys[p1] == last;
  T acc[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) acc[q] = T(0);
  uint32_t cur = first;
  auto flush = [&](uint32_t v) {
    T* dst;
    if (part && stat_sub(map, v) != map.sub) {  // another launch's row: drop it
#pragma unroll
      for (int q = 0; q < Q; ++q) acc[q] = T(0);
      return;
    }
    if (v == first && start_mid) {
      dst = headbuf + chunk * kp;
    } else if (v == last && cont) {
      dst = tailbuf + chunk * kp;
    } else {
      dst = stat + stat_row(map, v) * kp;
      if (stamp && blockIdx.y == 0 && lane == 0) stamp[v] = sid;  // row v holds this step's sums
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int col = c0 + lane + 64 * q;
      if (col < kp) dst[col] = acc[q];
      acc[q] = T(0);
    }
  };
  for (int64_t pb = p0; pb < p1; pb += 64) {
    const int64_t p = pb + lane;
    uint32_t kv = cur;
    T rv = T(0);
    int32_t dv = 0;
    if (p < p1) kv = skeys[p];
    // this launch's entries (a sub-chunk launch gathers nothing for the other terms)
    const bool mine = p < p1 && (!part || stat_sub(map, kv) == map.sub);
    const uint64_t mmask = part ? __ballot(mine) : ~0ull;
    if (mine) {  // (slot, r) travel with the sorted keys (entry_val); fp64 gathers r[e]
      const uint64_t pv = svals[p];
      dv = (int32_t)(pv >> 32);
      if constexpr (sizeof(T) == 4) rv = __builtin_bit_cast(T, (uint32_t)pv);
      else rv = r[(uint32_t)pv];
    }
    const int cnt = (int)((p1 - pb) < 64 ? (p1 - pb) : 64);
    for (int j0 = 0; j0 < cnt; j0 += kU) {
      uint32_t vk[kU];
      T rk[kU];
      T e[kU][Q];
#pragma unroll
      for (int u = 0; u < kU; ++u) {  // lanes past cnt hold (cur, 0, doc 0): harmless to add
        const int jj = j0 + u < 64 ? j0 + u : 63;
        vk[u] = (uint32_t)__builtin_amdgcn_readlane((int)kv, jj);
        rk[u] = readlane_t(rv, jj);
        const T* er = eth + (int64_t)__builtin_amdgcn_readlane(dv, jj) * kp;
        const bool mu = (mmask >> jj) & 1;  // wave-uniform
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          const int col = c0 + lane + 64 * q;
          e[u][q] = col < kp && mu ? er[col] : T(0);
        }
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        if (j0 + u < cnt) {
          if (vk[u] != cur) {
            flush(cur);
            cur = vk[u];
          }
#pragma unroll
          for (int q = 0; q < Q; ++q) acc[q] += rk[u] * e[u][q];
        }
      }
    }
  }
  flush(cur);
}

// Full tiles: kTile consecutive chunks all inside one run (the entries just before and just after the
// tile carry the same term, so — the keys being sorted — every entry of the tile does).  Each such tile's
// head partials are summed here, in chunk order, one wave per tile, into the tail row of its first chunk
// (an interior chunk's tail row is otherwise unused: k_sstats writes its whole sum to the head row).
// k_fixup's owner then steps over a full tile with one add, so the run of a frequent term (thousands
// of chunks at the headline corpus) costs its owner tens of dependent round trips, not hundreds.
constexpr int kTile = 32;
template <typename T, int Q>
__global__ __launch_bounds__(256) void k_fixup_tiles(const uint32_t* __restrict__ skeys, int64_t E, int kp,
                                                     const T* __restrict__ headbuf, T* __restrict__ tailbuf,
                                                     int64_t nchunks, StatMap map) {
  constexpr int kG = 32 / Q;
  const int c0 = (int)blockIdx.y * 64 * Q;
  const int lane = threadIdx.x & 63;
  const int64_t cb = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * kTile;
  if (cb == 0 || cb + kTile >= nchunks) return;  // an entry before the tile and one after it
  const uint32_t key = skeys[cb * kChunk - 1];
  if (skeys[(cb + kTile) * kChunk] != key) return;
  if (map.sub >= 0 && stat_sub(map, key) != map.sub) return;  // another sub-chunk launch's row
  T acc[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) acc[q] = T(0);
  for (int g0 = 0; g0 < kTile; g0 += kG) {
    T h[kG][Q];
#pragma unroll
    for (int g = 0; g < kG; ++g)
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const int col = c0 + lane + 64 * q;
        h[g][q] = col < kp ? headbuf[(cb + g0 + g) * kp + col] : T(0);
      }
#pragma unroll
    for (int g = 0; g < kG; ++g)
#pragma unroll
      for (int q = 0; q < Q; ++q) acc[q] += h[g][q];
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int col = c0 + lane + 64 * q;
    if (col < kp) tailbuf[cb * kp + col] = acc[q];
  }
}

template <typename T, int Q>
__global__ __launch_bounds__(256) void k_fixup(const uint32_t* __restrict__ skeys, int64_t E,
                                               int kp, T* __restrict__ stat,
                                               const T* __restrict__ headbuf,
                                               const T* __restrict__ tailbuf, int64_t nchunks,
                                               StatMap map, int32_t* __restrict__ stamp, int32_t sid) {
  // the run's owner (the chunk where it starts) adds the partials of the chunks the run covers, in
  // chunk order: chunk by chunk up to a kTile boundary, then whole full tiles (k_fixup_tiles' sums),
  // then chunk by chunk to the run's end.  kG chunks / tiles are fetched at a time (keys and partials).
  constexpr int kG = 32 / Q;
  const int c0 = (int)blockIdx.y * 64 * Q;  // this slab's first topic column
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= nchunks) return;
  const int64_t p0 = c * kChunk;
  const int64_t p1 = (p0 + kChunk < E) ? p0 + kChunk : E;
  const uint32_t first = skeys[p0], last = skeys[p1 - 1];
  const bool start_mid = p0 > 0 && skeys[p0 - 1] == first;
  const bool cont = p1 < E && skeys[p1] == last;
  if (!cont || (first == last && start_mid)) return;  // owner = chunk where the run starts
  if (map.sub >= 0 && stat_sub(map, last) != map.sub) return;  // another sub-chunk launch's row
  T acc[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int col = c0 + lane + 64 * q;
    acc[q] = col < kp ? tailbuf[c * kp + col] : T(0);
  }
  bool more = true;
  int64_t cb = c + 1;
  // chunk by chunk over [cb, stop) while the run goes on.  The run's extent within a batch of kG chunks
  // comes from their end keys first (chunk cb is in the run; cb + g is when cb + g − 1 went on past its
  // end), and only those chunks' partials are read — most runs end in the chunk after their owner, and
  // reading kG partials for each of them was ≈ 0.4 GB per launch at the headline
  auto chunks = [&](int64_t stop) {
    while (more && cb < stop) {
      const int m = stop - cb < kG ? (int)(stop - cb) : kG;
      bool go[kG];
      T h[kG][Q];
#pragma unroll
      for (int g = 0; g < kG; ++g) {  // chunk cb+g (all `last` when in the run) goes on past its end?
        const int64_t c2 = cb + g < nchunks ? cb + g : nchunks - 1;
        const int64_t q1 = (c2 * kChunk + kChunk < E) ? c2 * kChunk + kChunk : E;
        go[g] = q1 < E && skeys[q1] == last;
      }
#pragma unroll
      for (int q = 0; q < Q; ++q) {  // chunk cb's partial, with the keys
        const int col = c0 + lane + 64 * q;
        h[0][q] = col < kp ? headbuf[cb * kp + col] : T(0);
      }
      int n_in = 1;       // chunks of this batch in the run
      bool gl = go[0];    // the last of them goes on past its end
#pragma unroll
      for (int g = 1; g < kG; ++g)
        if (n_in == g && g < m && go[g - 1]) {
          n_in = g + 1;
          gl = go[g];
        }
#pragma unroll
      for (int g = 1; g < kG; ++g)
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          const int col = c0 + lane + 64 * q;
          h[g][q] = g < n_in && col < kp ? headbuf[(cb + g) * kp + col] : T(0);
        }
#pragma unroll
      for (int g = 0; g < kG; ++g)
        if (g < n_in)
#pragma unroll
          for (int q = 0; q < Q; ++q) acc[q] += h[g][q];
      more = gl;
      cb += n_in;
    }
  };
  chunks((c + kTile) / kTile * kTile < nchunks ? (c + kTile) / kTile * kTile : nchunks);
  // whole tiles: cb is a tile boundary and the run reached it (the entry before cb is `last`), so the
  // tile is full — k_fixup_tiles summed it — exactly when the entry after it is `last` too
  while (more && cb + kTile < nchunks) {
    bool full[kG];
    T h[kG][Q];
#pragma unroll
    for (int g = 0; g < kG; ++g) {
      const int64_t t = cb + (int64_t)g * kTile;
      const int64_t tc = t < nchunks ? t : nchunks - 1;
      full[g] = t + kTile < nchunks && skeys[(t + kTile) * kChunk] == last;
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const int col = c0 + lane + 64 * q;
        h[g][q] = col < kp ? tailbuf[tc * kp + col] : T(0);
      }
    }
    bool tiles = true;
#pragma unroll
    for (int g = 0; g < kG; ++g) {
      if (tiles && full[g]) {
#pragma unroll
        for (int q = 0; q < Q; ++q) acc[q] += h[g][q];
        cb += kTile;
      } else {
        tiles = false;
      }
    }
    if (!tiles) break;
  }
  chunks(nchunks);
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int col = c0 + lane + 64 * q;
    if (col < kp) stat[stat_row(map, last) * kp + col] = acc[q];
  }
  if (stamp && blockIdx.y == 0 && lane == 0) stamp[last] = sid;
}

template <typename T, int Q>
static void sstats_q(hipStream_t s, const uint32_t* skeys, const uint64_t* svals, int64_t E,
                     const T* r, const T* eth, int kp, T* stat, T* headbuf, T* tailbuf, const StatMap& map,
                     int32_t* stamp, int32_t sid) {
  const int64_t nchunks = ceil_div(E, kChunk);
  const dim3 grid((unsigned)ceil_div(nchunks, 4), (unsigned)ceil_div(kp, 64 * Q));
  k_sstats<T, Q><<<grid, 256, 0, s>>>(skeys, svals, E, r, eth, kp, stat, headbuf, tailbuf, nchunks, map, stamp,
                                      sid);
  KERNEL_CHECK();
  const int64_t ntiles = ceil_div(nchunks, (int64_t)kTile);
  if (ntiles > 1) {
    k_fixup_tiles<T, Q><<<dim3((unsigned)ceil_div(ntiles, 4), grid.y), 256, 0, s>>>(skeys, E, kp, headbuf, tailbuf,
                                                                                   nchunks, map);
    KERNEL_CHECK();
  }
  k_fixup<T, Q><<<grid, 256, 0, s>>>(skeys, E, kp, stat, headbuf, tailbuf, nchunks, map, stamp, sid);
  KERNEL_CHECK();
}

template <typename T>
void launch_sstats(hipStream_t s, const uint32_t* skeys, const uint64_t* svals, int64_t E,
                   const T* r, const T* eth, int kp, T* stat, T* headbuf, T* tailbuf, const StatMap& map,
                   int32_t* stamp, int32_t sid) {
  if (E == 0) return;
  if (stamp && map.sub >= 0) throw Error(STC_ERR_INVALID_ARG, "sstats: row stamps with a sub-chunk map");
  if (kp > 4096) throw Error(STC_ERR_INVALID_ARG, "k > 4096 topics is not supported");
  if (map.sub >= 0 && (map.vs == 0 || map.vsj == 0 || map.nsub < 1 || map.sub >= map.nsub ||
                       (uint64_t)(map.nsub - 1) * map.vsj >= map.vs))
    throw Error(STC_ERR_INVALID_ARG, "sstats: bad sub-chunk map");
  // slab width: ≤ 4 (fp64) / 8 (fp32) columns per lane — the whole row when it is that narrow
  const int q = (kp + 63) / 64;
  constexpr int QMAX = sizeof(T) == 8 ? 4 : 8;
  if (q <= 1) sstats_q<T, 1>(s, skeys, svals, E, r, eth, kp, stat, headbuf, tailbuf, map, stamp, sid);
  else if (q <= 2) sstats_q<T, 2>(s, skeys, svals, E, r, eth, kp, stat, headbuf, tailbuf, map, stamp, sid);
  else if (q <= 4 || QMAX == 4) sstats_q<T, 4>(s, skeys, svals, E, r, eth, kp, stat, headbuf, tailbuf, map, stamp, sid);
  else sstats_q<T, QMAX>(s, skeys, svals, E, r, eth, kp, stat, headbuf, tailbuf, map, stamp, sid);
}

// The sstats pairs of an fp64 launch built from the batch alone (lda_online.hip estep_and_stats, presort): entry
// e = bptr[slot] + n of slot `slot` is the slot's n-th CSR entry, with key its term and value entry_val(slot, e) —
// exactly what the rows E-step kernels write in their close phase (fp64 carries the entry index, not r), so the
// radix sort can run beside the E-step instead of after it.  One wave per slot.
__global__ __launch_bounds__(256) void k_entry_pairs(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                     const int32_t* __restrict__ batch, const int64_t* __restrict__ bptr,
                                                     int64_t n, uint32_t* __restrict__ keys, uint64_t* __restrict__ vals) {
  const int lane = threadIdx.x & 63;
  for (int64_t slot = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6; slot < n; slot += ((int64_t)gridDim.x * 256) >> 6) {
    const int64_t row = batch[slot], s0 = indptr[row], nnz = indptr[row + 1] - s0, e0 = bptr[slot];
    for (int64_t j = lane; j < nnz; j += 64) {
      keys[e0 + j] = (uint32_t)indices[s0 + j];
      vals[e0 + j] = entry_val<double>(slot, e0 + j, 0.0);
    }
  }
}
void launch_entry_pairs(hipStream_t s, const int64_t* indptr, const int32_t* indices, const int32_t* batch,
                        const int64_t* bptr, int64_t n, uint32_t* keys, uint64_t* vals) {
  if (n == 0) return;
  const int64_t g = ceil_div(n, 4);
  k_entry_pairs<<<(unsigned)(g > 8192 ? 8192 : g), 256, 0, s>>>(indptr, indices, batch, bptr, n, keys, vals);
  KERNEL_CHECK();
}

// Spark's sstats from the scaled stat: stat'_vt = stat_vt · e^{m_v} · e^{−ψc_t} (r carries e^{m_v},
// eθ the per-topic e^{−ψ(colsum_t)}), so stat_vt = stat'_vt · exp(ψc_t − m_v)
template <typename T>
__global__ __launch_bounds__(256) void k_unscale_stat(const T* __restrict__ stat,
                                                      const double* __restrict__ logscale,
                                                      const double* __restrict__ psic, int64_t V,
                                                      int k, int kp, double* __restrict__ out) {
  const int64_t total = V * k;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t v = e / k;
    const int t = (int)(e - v * k);
    out[e] = (double)stat[v * kp + t] * exp(psic[t] - logscale[v]);
  }
}

template <typename T>
void launch_unscale_stat(hipStream_t s, const T* stat, const double* logscale, const double* psic, int64_t V,
                         int k, int kp, double* out_vk) {
  k_unscale_stat<T><<<4096, 256, 0, s>>>(stat, logscale, psic, V, k, kp, out_vk);
  KERNEL_CHECK();
}

#define STC_INSTANTIATE(T)                                                                        \
  template void launch_sstats<T>(hipStream_t, const uint32_t*, const uint64_t*, int64_t, const T*, \
                                 const T*, int, T*, T*, T*, const StatMap&, int32_t*, int32_t);   \
  template void launch_unscale_stat<T>(hipStream_t, const T*, const double*, const double*, int64_t, int, \
                                       int, double*);

STC_INSTANTIATE(float)
STC_INSTANTIATE(double)

}  // namespace lda
}  // namespace stc
