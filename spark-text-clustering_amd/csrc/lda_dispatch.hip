// lda_dispatch.hip — which kernel runs these slots: the choice and launch of every E-step kernel family
// (launch_split), γ₀, the mixed mode's fp64 re-solve, and the E-step + sstats of one launch (estep_and_stats).
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cmath>
#include <string>
#include <vector>

#include "lda_handle.h"

namespace stc::online {

// The sstats pairs' radix sort by term (u32 keys, u64 values): rocprim's onesweep at STC_SORT_BITS bits (11: slower)
// per pass (gfx950's tuned block shape, 1024 threads × 8 items)
#ifndef STC_SORT_BITS
#define STC_SORT_BITS 9  // 18-bit term ids (V = 2^18) in two passes: sstats phase −75 µs headline, −90 µs planted vs 8
#endif
using TermSortConfig = rocprim::radix_sort_config<
    rocprim::default_config, rocprim::default_config,
    rocprim::radix_sort_onesweep_config<rocprim::kernel_config<1024, 8>, rocprim::kernel_config<1024, 8>, STC_SORT_BITS,
                                        rocprim::block_radix_rank_algorithm::match>>;
hipError_t term_sort(void* tmp, size_t& bytes, const uint32_t* kin, uint32_t* kout, const uint64_t* vin, uint64_t* vout,
                     int64_t n, int bits, hipStream_t s) {
  return rocprim::radix_sort_pairs<TermSortConfig>(tmp, bytes, kin, kout, vin, vout, (size_t)n, 0u, (unsigned)bits, s);
}

template <typename T>
lda::EStepArgs<T> estep_args(stc_lda& L) {
  lda::EStepArgs<T> a;
  a.k = L.k;
  a.kp = L.kp;
  a.P = L.P;
  a.lds_rows = L.lds_rows;
  a.Bp = L.model.Bp.as<T>();
  if constexpr (std::is_same<T, double>::value) {
    if (L.mixed) {  // the fp64 re-solve / inference of a mixed handle: the fp64 rows and workgroup shape
      a.Bp = L.model.Bp64.as<double>();
      a.P = L.mix.P64;
      a.lds_rows = L.mix.lds_rows64;
    }
  }
  a.logscale = L.model.logscale.as<double>();
  a.psic = L.model.psic.as<double>();
  a.alpha = L.model.alpha.as<double>();
  a.seed = L.cfg.seed;
  a.rank = L.ctx->rank;
  a.gamma_shape = L.cfg.gamma_shape;
  a.max_iter = L.cfg.max_inner_iter;
  a.stop_thr = lda::stop_threshold(L.k);
  return a;
}
template lda::EStepArgs<float> estep_args<float>(stc_lda&);
template lda::EStepArgs<double> estep_args<double>(stc_lda&);

// estep_args plus everything that decides which entry of r, keys and vals belongs to which term of a training
// launch.  The fp32 pass (estep_and_stats) and the mixed mode's fp64 re-solve (mixed_resolve) both start from
// it, so they cannot differ in it: entry e0 + n of a document is the same term in r64, in the fixup's sort values
// and in the fp32 pass's keys, which the fixup leaves in place.  The row order is the many-topic kernel's (none
// at k ≤ 128, where the fp32 grid kernel writes CSR positions; the workgroup kernel reads none in either pass).
template <typename T>
static lda::EStepArgs<T> train_args(stc_lda& L, int64_t iteration) {
  lda::EStepArgs<T> a = estep_args<T>(L);
  a.indptr = L.corpus->indptr.as<int64_t>();
  a.indices = L.corpus->indices.as<int32_t>();
  a.order = L.mb.order_for == L.corpus ? L.mb.order.as<int32_t>() : nullptr;
  a.iteration = iteration;
  a.key_mode = 0;
  a.iters = L.mb.iters.as<int32_t>();
  a.nonempty = L.mb.nonempty.as<int32_t>();
  return a;
}

// team for the many-topic kernel: enough CUs that a document of `mean_rows` rows stays resident.
// k ≤ 512: rows split (k_estep_wide_mc), P = ⌈1.05·rows / resident rows⌉ ≤ 4 (config 4, k = 500:
// fp64 P = 4, fp32 P = 2).  k > 512: topics split (k_estep_wide_tc), members of up to 1024 topics, when
// the one-CU kernel cannot keep the rows resident (config 5, k = 2000: fp64 P = 2; fp32 stays one CU).
// P = 1: the one-CU kernel.  STC_WIDE_TEAM=n forces P = n.
struct TeamChoice {
  int P = 1;
  bool topics = false;
  bool grid = false;  // the fp64 topic-split grid kernel (lda_team64.hip k_estep_tgrid64)
};
template <typename T>
static TeamChoice team_choice(const stc_lda& L, double mean_rows, int64_t max_row) {
  const double need = 1.05 * mean_rows;
  const int force = L.sw.team_force;
  if (force == 1) return {1, false};
  // fp64: the topic-split team with the rows64 grid in every member (members of 104 topics) when every
  // document of the corpus fits its 448 rows (config 4: k = 500, P = 5, 371 ± 10 rows); STC_TGRID=0: off
  if constexpr (std::is_same<T, double>::value) {
    const int P = lda::tgrid64_members(L.kp);
    if (L.sw.tgrid && force == 0 && P >= 2 && P <= 8 && max_row >= 0 && max_row <= lda::tgrid64_row_cap())
      return {P, true, true};
    if (L.sw.tgrid_require)
      throw Error(STC_ERR_STATE, "STC_TGRID=2: the fp64 grid team kernel cannot take this launch (k " + std::to_string(L.k) +
                                     ", longest document " + std::to_string(max_row) + " rows)");
  }
  if (L.k <= 512) {
    if (force > 1) return {force, false};
    const int P = (int)std::ceil(need / std::max(lda::wide_resident_rows<T>(L.k), 1));
    return {std::max(1, std::min(P, 4)), false};
  }
  if (force > 1) return {std::max(force, (L.k + 2047) / 2048), true};
  // only when a quarter or more of the rows would be re-streamed: a few streamed rows cost the one-CU
  // kernel less than a member's exchange (config 5 planted state, fp32: 47 resident of ≈ 47 rows, one
  // CU 2.2× faster than P = 2 at 3 inner iterations)
  if (lda::wide_resident_rows<T>(L.k) >= 0.75 * mean_rows) return {1, false};
  // two members of up to 1024 topics: measured at config 5 (k = 2000, fp64, E-step per minibatch) P = 2
  // 44.0 ms, one CU 53.7, P = 3 (a member without topics) 71.2, P = 4 61.9 — a member's exchange
  // latency is fixed, so the fewest members that hold the block win
  return {std::max(2, std::min(4, (L.k + 1023) / 1024)), true};
}

// The team kernel's timeout word: a member whose partner never arrived (a block that was not
// co-resident after all, e.g. another process holding CUs) gave up instead of hanging, and so did its
// team.  launch_split() reads the word right after the launch and, when it is set, runs the same slots
// again on the one-CU kernel inside the same call: the step completes with the one-CU kernel's results
// (which every member of a group or every rank gets on its own, so no rank's state can diverge).
// debug knob STC_TEAM_FAULT=m: member m of team 0 never publishes (its partners time out quickly)
static int team_fault_member() {
  return env_int("STC_TEAM_FAULT", -1, INT_MIN, INT_MAX);
}

template <typename T>
static bool launch_wide_team(stc_lda& L, const lda::EStepArgs<T>& w, bool stats, TeamChoice tc, int64_t max_row) {
  const int P = tc.P;
  Ctx& c = *L.ctx;
  hipStream_t s = c.stream;
  int cus = 0;
  HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c.device));
  lda::WideTeam wt;
  wt.P = P;
  wt.blocks = 8 * P * (cus / (8 * P));
  if (wt.blocks <= 0) return false;  // fewer CUs than one team per XCD group: the one-CU kernel
  const int teams = wt.blocks / P;
  // granules per member: rows split, the s partials + Σ r·φ; topics split, the φ partials + Σ|Δγ| + Σγ
  wt.xstride = tc.grid ? lda::tgrid64_xstride() : std::max<int64_t>(L.kp + 1, 512 + 2);
  const size_t xbytes = 16 * (size_t)teams * 2 * P * (size_t)wt.xstride;
  L.team.team_words.reserve(16);
  L.team.team_x.reserve(xbytes);
  wt.tmo = L.team.team_words.as<unsigned>();
  wt.xbuf = L.team.team_x.p;
  wt.fault_member = team_fault_member();
  wt.max_row = max_row <= INT32_MAX ? (int)max_row : -1;
  if (wt.fault_member >= 0) wt.spin_limit = 1u << 14;
  // every polled word zeroed before every launch: the timeout word, and the granules' epoch tags
  // (a tag left by an earlier launch could equal an epoch this launch waits for)
  HIP_CHECK(hipMemsetAsync(L.team.team_words.p, 0, 16, s));
  HIP_CHECK(hipMemsetAsync(L.team.team_x.p, 0, xbytes, s));
  bool ok;
  if constexpr (std::is_same<T, double>::value) {
    ok = tc.grid ? lda::launch_estep_tgrid64(s, w, stats, wt)
                 : tc.topics ? lda::launch_estep_wide_tc<T>(s, w, stats, wt) : lda::launch_estep_wide_mc<T>(s, w, stats, wt);
  } else {
    ok = tc.topics ? lda::launch_estep_wide_tc<T>(s, w, stats, wt) : lda::launch_estep_wide_mc<T>(s, w, stats, wt);
  }
  if (ok) HIP_CHECK(hipMemcpyAsync(L.own.htmo.get(), wt.tmo, sizeof(unsigned), hipMemcpyDeviceToHost, s));
  if (!ok && tc.grid && L.sw.tgrid_require) throw Error(STC_ERR_STATE, "STC_TGRID=2: the grid team could not be resident");
  return ok;
}

// fast kernel on slots [0, n_short), workgroup kernel on [n_short, n); mean_rows = the launch's mean
// entries per document (the many-topic kernel's team size).  T is the launch's arithmetic, not the handle's: a
// mixed handle runs both.
template <typename T>
void launch_split(stc_lda& L, const DCsr& m, lda::EStepArgs<T> a, int64_t n, int64_t n_short, bool stats, bool bound,
                  double mean_rows) {
  hipStream_t s = L.ctx->stream;
  int64_t* kcount = L.tm.kcount;
  if (n_short > 0) {
    lda::EStepArgs<T> w = a;
    w.slot0 = 0;
    w.n = n_short;
    const TeamChoice tc = use_wide<T>(L.k) && !bound ? team_choice<T>(L, mean_rows, m.max_row) : TeamChoice{};
    const bool team = tc.P > 1 && launch_wide_team<T>(L, w, stats, tc, m.max_row);
    if (team) {  // launched (a grid that could not be resident falls through to the one-CU kernel)
      kcount[tc.grid ? STC_KC_TGRID64 : tc.topics ? STC_KC_WIDE_TC : STC_KC_WIDE_MC] += 1;
      wait_stream(*L.ctx, s);
      if (*L.own.htmo.get()) {  // a team gave up: the same slots on the one-CU kernel (it rewrites every output)
        *L.own.htmo.get() = 0;
        kcount[STC_KC_TEAM_FALLBACK] += 1;
        kcount[STC_KC_WIDE] += 1;
        lda::launch_estep_wide<T>(s, w, stats, bound);
      }
    } else if (use_wide<T>(L.k)) {
      kcount[STC_KC_WIDE] += 1;
      lda::launch_estep_wide<T>(s, w, stats, bound);
    } else {  // the dtype's grid family: fp32 grid, fp64 rows64 (which counts its long-document pass)
      constexpr bool f32 = std::is_same<T, float>::value;
      const bool long_docs = m.max_row < 0 || m.max_row > (f32 ? lda::grid_onchip_rows(L.k) : lda::rows64_onchip_rows(L.k));
      // the long-document list (count word + slots) and, past it, the resident grid's ticket word
      L.mb.long_list.reserve(4 * (size_t)(n_short + 2));
      w.long_list = L.mb.long_list.as<int32_t>();
      kcount[f32 ? STC_KC_GRID : STC_KC_ROWS64] += 1;
      if (!f32 && long_docs) kcount[STC_KC_ROWS64_LONG] += 1;
      if constexpr (f32) lda::launch_estep_grid(s, w, stats, bound, long_docs);
      else lda::launch_estep_rows64(s, w, stats, bound, long_docs);
    }
  }
  if (n > n_short) {
    a.slot0 = n_short;
    a.n = n - n_short;
    kcount[STC_KC_WORKGROUP] += 1;
    lda::launch_estep<T>(s, a, stats, bound);
  }
}
template void launch_split<float>(stc_lda&, const DCsr&, lda::EStepArgs<float>, int64_t, int64_t, bool, bool, double);
template void launch_split<double>(stc_lda&, const DCsr&, lda::EStepArgs<double>, int64_t, int64_t, bool, bool, double);

template <typename T>
const T* upload_gamma0(stc_lda& L, const double* gamma0, int64_t n) {
  if (!gamma0 || n == 0) return nullptr;
  std::vector<T> h((size_t)(n * L.k));
  for (size_t j = 0; j < h.size(); ++j) {
    STC_REQUIRE(gamma0[j] > 0.0, "gamma0 entries must be > 0");
    h[j] = (T)gamma0[j];
  }
  L.mb.g0.reserve(sizeof(T) * h.size());
  HIP_CHECK(hipMemcpyAsync(L.mb.g0.p, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice, L.ctx->stream));
  wait_stream(*L.ctx, L.ctx->stream);  // h dies at scope exit
  return L.mb.g0.as<T>();
}
template const float* upload_gamma0<float>(stc_lda&, const double*, int64_t);
template const double* upload_gamma0<double>(stc_lda&, const double*, int64_t);

// STC_MIXED with an injected γ₀: its fp64 copy for the re-solve (the fp32 E-step reads the rounded one)
const double* mixed_gamma0(stc_lda& L, const double* gamma0, int64_t n) {
  if (!L.mixed || !gamma0 || n == 0) return nullptr;
  L.mix.g0_64.reserve(sizeof(double) * n * L.k);
  HIP_CHECK(hipMemcpyAsync(L.mix.g0_64.p, gamma0, sizeof(double) * n * L.k, hipMemcpyHostToDevice, L.ctx->stream));
  wait_stream(*L.ctx, L.ctx->stream);  // (the caller's buffer)
  return L.mix.g0_64.as<double>();
}

// γ₀ of the n partitioned slots' members from the counter RNG, keyed as the E-step kernels key it
// (key_mode 0: train_doc_key(iteration, rank, member); 1: doc_id_base + row), into mb.g0gen
template <typename T>
const T* gen_gamma0(stc_lda& L, hipStream_t s, int64_t n, uint64_t seed, int64_t iteration, int key_mode,
                    int64_t base) {
  if (n == 0) return nullptr;
  L.mb.g0gen.reserve(sizeof(T) * n * L.k);
  lda::launch_gamma0<T>(s, L.mb.batch.as<int32_t>(), L.mb.orig.as<int32_t>(), n, L.k, seed, iteration, L.ctx->rank,
                        key_mode, base, L.cfg.gamma_shape, L.mb.g0gen.as<T>());
  return L.mb.g0gen.as<T>();
}
template const float* gen_gamma0<float>(stc_lda&, hipStream_t, int64_t, uint64_t, int64_t, int, int64_t);
template const double* gen_gamma0<double>(stc_lda&, hipStream_t, int64_t, uint64_t, int64_t, int, int64_t);

// STC_MIXED: after the fp32 E-step over the n slots, the documents whose fp32 fixed point took more than
// mixed_thr iterations are re-solved in fp64 — the same γ₀ (the training key drawn in the kernel, or the
// injected fp64 γ₀ g0_64), the fp64 expElogβ' rows (Bp64) and the corpus's fp64 values — and their eθ',
// E[log θ], r, sstats sort values, iteration counts (and γ) replace the fp32 ones before logphat and
// sstats read them.  One host readback (the two list counts) sizes the fp64 launches.  Why the fp32
// iteration count selects them: DESIGN.md §4 (mixed mode).
static void mixed_resolve(stc_lda& L, int64_t n, int64_t E, int64_t iteration, const double* g0_64, bool want_gamma) {
  if (n == 0) return;
  const DCsr& m = *L.corpus;
  hipStream_t s = L.ctx->stream;
  auto& B = L.mb;
  auto& X = L.mix;
  X.m_batch.reserve(4 * n);
  X.m_orig.reserve(4 * n);
  X.m_slot.reserve(4 * n);
  X.m_bptr.reserve(8 * n);
  X.m_cnt.reserve(2 * sizeof(int32_t));
  int32_t* hm = L.own.hmcnt.get();
  lda::launch_mixed_list(s, m.indptr.as<int64_t>(), B.batch.as<int32_t>(), B.orig.as<int32_t>(), B.bptr.as<int64_t>(),
                         B.iters.as<int32_t>(), B.nonempty.as<int32_t>(), n, X.mixed_thr, X.cap64,
                         X.m_batch.as<int32_t>(), X.m_orig.as<int32_t>(), X.m_bptr.as<int64_t>(), X.m_slot.as<int32_t>(),
                         X.m_cnt.as<int32_t>());
  HIP_CHECK(hipMemcpyAsync(hm, X.m_cnt.p, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  wait_stream(*L.ctx, s);
  const int ms = hm[0], ml = hm[1];
  if (ms + ml == 0) return;
  L.tm.kcount[STC_KC_MIXED_RESOLVES] += 1;
  L.tm.kcount[STC_KC_MIXED_DOCS] += ms + ml;
  X.eth64.reserve(8 * n * L.kp);
  X.elogth64.reserve(8 * n * L.k);
  X.r64.reserve(8 * std::max<int64_t>(E, 1));
  X.keys64.reserve(4 * std::max<int64_t>(E, 1));
  X.vals64.reserve(8 * std::max<int64_t>(E, 1));
  if (want_gamma) X.gamma64.reserve(8 * n * L.k);
  lda::EStepArgs<double> a = train_args<double>(L, iteration);  // (estep_args: Bp64 and the fp64 workgroup shape)
  a.values = m.values.as<double>();
  a.gamma0 = g0_64;
  a.gamma = want_gamma ? X.gamma64.as<double>() : nullptr;
  a.r = X.r64.as<double>();
  a.keys = X.keys64.as<uint32_t>();  // (the fp64 sort values are the fp64 layout's: scratch, rewritten by the fixup)
  a.vals = X.vals64.as<uint64_t>();
  const double mean_rows = (double)E / (double)n;
  const auto resolve = [&](int64_t off, int64_t cnt, int64_t n_short) {  // list entries [off, off + cnt)
    lda::EStepArgs<double> w = a;
    w.batch = X.m_batch.as<int32_t>() + off;
    w.orig = X.m_orig.as<int32_t>() + off;
    w.bptr = X.m_bptr.as<int64_t>() + off;
    w.eth = X.eth64.as<double>() + off * L.kp;
    w.elogth = X.elogth64.as<double>() + off * L.k;
    launch_split<double>(L, m, w, cnt, n_short, true, false, mean_rows);
  };
  if (ms > 0) resolve(0, ms, ms);      // the documents the fp64 fast kernels hold
  if (ml > 0) resolve(n - ml, ml, 0);  // the longer ones: the workgroup kernel
  lda::launch_mixed_fixup(s, m.indptr.as<int64_t>(), X.m_batch.as<int32_t>(), X.m_orig.as<int32_t>(),
                          X.m_bptr.as<int64_t>(), X.m_slot.as<int32_t>(), n, ms, ml, L.k, L.kp, X.eth64.as<double>(),
                          X.elogth64.as<double>(), X.r64.as<double>(), want_gamma ? X.gamma64.as<double>() : nullptr,
                          B.eth.as<float>(), B.elogth.as<float>(), B.r.as<float>(), B.vals.as<uint64_t>(),
                          want_gamma ? B.gamma.as<float>() : nullptr);
}

// E-step over the n partitioned slots (mb.batch / orig / bptr), then logphat / non-empty count into
// mb.small and the term-sorted sstats SpMM into model.stat (V×kp, row-scaled).  split: a training step of a
// sharded handle — stat in the sub-chunk layout, one sstats launch per sub-chunk (ev_ss[j] after each).
template <typename T>
void estep_and_stats(stc_lda& L, int64_t n, int64_t n_short, int64_t E, const T* g0, int64_t iteration, bool split,
                     const double* g0_64, bool want_gamma) {
  hipStream_t s = L.ctx->stream;
  auto& B = L.mb;
  auto& M = L.model;
  lda::EStepArgs<T> a = train_args<T>(L, iteration);
  a.values = L.mixed ? L.mix.vals32.as<T>() : L.corpus->values.as<T>();
  // mixed: the fp32 pass stops a document at mixed_thr + 1 iterations — it is re-solved in fp64 anyway, so the
  // fp32 iterations past the threshold (up to ≈ 300 per such document at the bench state) are not spent
  if (L.mixed) a.max_iter = std::min(a.max_iter, L.mix.mixed_thr + 1);
  a.batch = B.batch.as<int32_t>();
  a.orig = B.orig.as<int32_t>();
  a.bptr = B.bptr.as<int64_t>();
  a.gamma0 = g0;
  a.gamma = B.gamma.as<T>();
  a.eth = B.eth.as<T>();
  a.elogth = B.elogth.as<T>();
  a.r = B.r.as<T>();
  a.keys = B.keys.as<uint32_t>();
  a.vals = B.vals.as<uint64_t>();
  record(L, 1);
  // fp64 on the rows kernels (k ≤ 104, every slot on them): an entry's sort value carries its index, not r, so
  // the (term, slot) pairs and their radix sort depend on the batch alone — they run on another stream beside the
  // E-step, whose blocks take the CU slots the resident grid frees as it drains, instead of after it
  bool presort = false;
  if constexpr (std::is_same<T, double>::value)
    presort = L.sw.presort && !L.mixed && !use_wide<double>(L.k) && n_short == n && E > 0;
  hipStream_t ss = nullptr;
  if (presort) {
    // a process with several handles runs past the device's hardware queues (GPU_MAX_HW_QUEUES) when each adds
    // a stream, and a stream sharing a queue waits behind unrelated work: the side stream (next()'s draws,
    // which then queue behind the sort) is used when it exists, else a lowest-priority stream of the sort's own
    ss = L.own.side.s ? L.own.side.s : L.own.sort_stream.get(hipStreamNonBlocking, true);
    HIP_CHECK(hipEventRecord(L.own.ev_ps0.get(), s));  // the batch and its entry offsets are built; skeys / svals free
    HIP_CHECK(hipStreamWaitEvent(ss, L.own.ev_ps0.get(), 0));
    a.keys = nullptr;  // (the E-step kernels leave the pairs alone)
    a.vals = nullptr;
  }
  launch_split<T>(L, *L.corpus, a, n, n_short, true, false, n > 0 ? (double)E / (double)n : 0.0);
  if (presort) {  // enqueued after the E-step launch, so the resident grid is dispatched first
    lda::launch_entry_pairs(ss, L.corpus->indptr.as<int64_t>(), L.corpus->indices.as<int32_t>(),
                            B.batch.as<int32_t>(), B.bptr.as<int64_t>(), n, B.keys.as<uint32_t>(), B.vals.as<uint64_t>());
    size_t tb = B.sort_tmp.bytes;
    HIP_CHECK(term_sort(B.sort_tmp.p, tb, B.keys.as<uint32_t>(), B.skeys.as<uint32_t>(), B.vals.as<uint64_t>(),
                        B.svals.as<uint64_t>(), E, bits_for(L.V), ss));
    HIP_CHECK(hipEventRecord(L.own.ev_sorted.get(), ss));
  }
  if constexpr (std::is_same<T, float>::value) {
    if (L.mixed) mixed_resolve(L, n, E, iteration, g0_64, want_gamma);
  }
  if (L.own.ev_est.e) HIP_CHECK(hipEventRecord(L.own.ev_est.e, s));  // the batch buffers are free (next_impl)
  record(L, 2);
  // logphat first: its all-reduce rides with the first stat sub-chunk of a sharded step
  if (n > 0) {
    lda::launch_logphat<T>(s, B.elogth.as<T>(), B.nonempty.as<int32_t>(), n, L.k, B.small.as<double>(),
                             B.lpart.as<double>());
    lda::launch_iter_stats(s, B.iters.as<int32_t>(), B.nonempty.as<int32_t>(), n, L.cfg.max_inner_iter,
                           B.stats4.as<int64_t>(), B.cum2.as<int64_t>());
  } else {
    HIP_CHECK(hipMemsetAsync(B.small.p, 0, sizeof(double) * (L.k + 1), s));
    HIP_CHECK(hipMemsetAsync(B.stats4.p, 0, sizeof(int64_t) * 4, s));
  }
  // a training step of one rank stamps its rows instead of clearing stat (the M-step reads unstamped rows as
  // zero); sharded steps clear it — the reduce-scatter sums every row of every rank
  M.step_stamped = split && !sharded(L);
  if (M.step_stamped) {
    M.stamp_seq = M.stamp_seq == INT32_MAX ? 0 : M.stamp_seq + 1;  // (never −1, the fresh array's value)
    M.step_sid = M.stamp_seq;
  } else {
    HIP_CHECK(hipMemsetAsync(M.stat.p, 0, sizeof(T) * M.vpad * L.kp, s));  // padded rows stay zero
  }
  if (presort) {
    HIP_CHECK(hipStreamWaitEvent(s, L.own.ev_sorted.e, 0));
  } else if (E > 0) {
    size_t tb = B.sort_tmp.bytes;
    HIP_CHECK(term_sort(B.sort_tmp.p, tb, B.keys.as<uint32_t>(), B.skeys.as<uint32_t>(), B.vals.as<uint64_t>(),
                        B.svals.as<uint64_t>(), E, bits_for(L.V), s));
  }
  const lda::StatMap lay = split ? stat_layout(L) : lda::StatMap{};
  if (lay.nsub <= 1) {
    lda::launch_sstats<T>(s, B.skeys.as<uint32_t>(), B.svals.as<uint64_t>(), E, B.r.as<T>(), B.eth.as<T>(), L.kp,
                          M.stat.as<T>(), B.headbuf.as<T>(), B.tailbuf.as<T>(), lda::StatMap{},
                          M.step_stamped ? M.rowstamp.as<int32_t>() : nullptr, M.step_sid);
  } else {
    for (int j = 0; j < lay.nsub; ++j) {
      lda::StatMap m = lay;
      m.sub = j;
      lda::launch_sstats<T>(s, B.skeys.as<uint32_t>(), B.svals.as<uint64_t>(), E, B.r.as<T>(), B.eth.as<T>(),
                            L.kp, M.stat.as<T>(), B.headbuf.as<T>(), B.tailbuf.as<T>(), m);
      HIP_CHECK(hipEventRecord(L.own.ev_ss[j].get(), s));
    }
  }
  record(L, 3);
}
template void estep_and_stats<float>(stc_lda&, int64_t, int64_t, int64_t, const float*, int64_t, bool, const double*, bool);
template void estep_and_stats<double>(stc_lda&, int64_t, int64_t, int64_t, const double*, int64_t, bool, const double*,
                                      bool);

}  // namespace stc::online
