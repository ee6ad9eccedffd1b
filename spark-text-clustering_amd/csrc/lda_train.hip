// lda_train.hip — a training step around the E-step: the vocabulary layout and the model refresh, the minibatch
// builder and sampler, the M-step slices and the two step tails, stc_lda_step / stc_lda_next's bodies, and what
// stc_group reads and sets of its members (lda_online.h).
//
// Host-side control flow mirrors [U] OnlineLDAOptimizer.submitMiniBatch (spark-mllib 2.4.3):
//   iteration += 1 → E-step over the batch (K6) → stat (K sstats) → treeReduce ≙ RCCL all-reduce
//   → batchResult = stat ⊙ expElogβ, updateLambda (K7) → expElogβ (K8) → updateAlpha.
// One host sync per step (to size the sort for the batch's entry count); everything else is
// stream-ordered on the context's HIP stream.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <vector>

#include "lda_handle.h"
#include "lda_online.h"

using namespace stc;
using namespace stc::online;

// ---- what stc_group reads and sets of its members (lda_online.h) ----
void stc::set_group_knobs(stc_lda& L, bool force_coll, int tail_fault) {
  if (force_coll) L.tail.force_coll = true;
  L.tail.tail_fault = tail_fault;
}
const DCsr* stc::corpus(const stc_lda& L) { return L.corpus; }
void stc::forget_corpus(stc_lda& L) {
  L.corpus = nullptr;
  L.mb.order_for = nullptr;
  L.draw.pre_valid = false;
}
hipStream_t stc::side_stream(const stc_lda& L) { return L.own.side.s; }
// the CSR value dtype a handle reads (a mixed handle: the fp64 values, and an fp32 copy it makes itself)
int stc::corpus_dtype(const stc_lda& L) { return L.mixed ? STC_F64 : L.dtype; }
// A call that failed after queuing the next draw on the side stream (before train_tail ordered the main
// stream behind it) leaves that draw in flight: wait for it and drop it, so nothing samples into the same
// count buffers concurrently and the next call draws synchronously.
void stc::settle_side(stc_lda& L) {
  if (!L.draw.samp_pending) return;
  L.ctx->use();
  wait_stream(*L.ctx, L.own.side.s);
  L.draw.samp_pending = false;
  L.draw.pre_inflight = false;
  L.draw.pre_valid = false;
}
// the full λ on every rank after sharded M-steps: an all-gather of the slices (collective — every
// rank calls the reader, as every executor calls ldaNext)
void stc::gather_lambda(stc_lda& L) {
  if (!L.model.lam_stale) return;
  Ctx& c = *L.ctx;
  const size_t cnt = (size_t)(L.model.Vs * L.k);
  coll_all_gather(c, L.model.lam.as<double>() + (size_t)c.rank * cnt, L.model.lam.p, cnt, ncclFloat64, c.stream);
  wait_stream(c, c.stream);
  L.model.lam_stale = false;
}

namespace stc::online {

void record(stc_lda& L, int slot) {
  if (L.tm.timing) HIP_CHECK(hipEventRecord(L.own.ev[L.tm.ev_set][slot].e, L.ctx->stream));
}

// add the phase times of an event set whose step has completed (left pending otherwise)
static void harvest(stc_lda& L, int set) {
  if (!L.tm.ev_pending[set]) return;
  if (hipEventQuery(L.own.ev[set][5].e) != hipSuccess) return;
  for (int p = 0; p < 5; ++p) {
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, L.own.ev[set][p].e, L.own.ev[set][p + 1].e));
    L.tm.acc_ms[p] += ms;
  }
  L.tm.timed_steps += 1;
  L.tm.ev_pending[set] = false;
}
// before a step records into the current set: a set is reused three steps later, long complete
static void claim_event_set(stc_lda& L) {
  if (!L.tm.timing || !L.tm.ev_pending[L.tm.ev_set]) return;
  wait_event(*L.ctx, L.own.ev[L.tm.ev_set][5].e);
  harvest(L, L.tm.ev_set);
}
void harvest_all(stc_lda& L) {
  for (int set = 0; set < 3; ++set) harvest(L, set);
}

// the vocabulary slices of the M-step: shards = the RCCL ranks (or STC_VIRTUAL_SHARDS on one GPU).
// λ, expElogβ', logscale and stat are padded to shards·Vs rows (the RCCL reduce-scatter / all-gather
// chunks); the padded rows of stat are zero, those of λ / Bp never read.  Called before a step; a
// change of shard count (comm initialised after the handle) keeps λ and recomputes the rest.
void ensure_layout(stc_lda& L) {
  auto& M = L.model;
  const int want = sharded(L) ? L.ctx->n_ranks : M.virt;
  if (want == M.shards && M.Vs > 0) return;
  if (M.lam_stale) throw Error(STC_ERR_STATE, "the shard count changed after sharded steps");
  const int64_t RB = lda::kRowsPerBlock;
  const int64_t Vs = ceil_div(ceil_div(L.V, (int64_t)want), RB) * RB;
  const int64_t vpad = Vs * want;
  if ((size_t)(8 * vpad * L.k) > M.lam.bytes) {  // grow λ, keeping its V·k prefix
    DevBuf tmp;
    tmp.reserve(8 * vpad * L.k);
    if (M.lam.p) {
      HIP_CHECK(hipMemcpyAsync(tmp.p, M.lam.p, 8 * L.V * L.k, hipMemcpyDeviceToDevice, L.ctx->stream));
      wait_stream(*L.ctx, L.ctx->stream);
    }
    swap(tmp, M.lam);
  }
  M.Bp.reserve(arith_size(L) * vpad * L.kp);
  if (L.mixed) M.Bp64.reserve(8 * vpad * L.kp);
  M.stat.reserve(arith_size(L) * vpad * L.kp);
  M.logscale.reserve(8 * vpad);
  M.colpart.reserve(8 * (vpad / RB) * L.k);
  if ((size_t)(4 * vpad) > M.rowstamp.bytes) {  // a new stamp array: no row is this step's
    M.rowstamp.reserve(4 * vpad);
    HIP_CHECK(hipMemsetAsync(M.rowstamp.p, 0xFF, M.rowstamp.bytes, L.ctx->stream));
    M.stamp_seq = 0;
  }
  M.shards = want;
  M.Vs = Vs;
  M.vpad = vpad;
  M.lam_stale = false;
}
void relayout(stc_lda& L) {
  const int old = L.model.shards;
  const int64_t vs = L.model.Vs;
  ensure_layout(L);
  if ((old != L.model.shards || vs != L.model.Vs) && L.model.has_topics) refresh(L);
}

// expElogβ', logscale, colsum and ψ(colsum) from λ
void refresh(stc_lda& L) {
  hipStream_t s = L.ctx->stream;
  auto& M = L.model;
  by_arith_type(L, [&](auto t) {
    using T = decltype(t);
    lda::launch_lambda_eeb<T>(s, false, M.lam.as<double>(), nullptr, M.Bp.as<T>(), M.logscale.as<double>(), L.V, L.k,
                              L.kp, 0.0, 0.0, 0.0, nullptr, M.colpart.as<double>(), M.nblocks_m,
                              L.mixed ? M.Bp64.as<double>() : nullptr);
  });
  lda::launch_colsum_reduce(s, M.colpart.as<double>(), M.nblocks_m, L.k, nullptr, M.colsum.as<double>(),
                            M.psic.as<double>());
  M.has_topics = true;
}

template <typename T>
void ensure_batch(stc_lda& L, int64_t n, int64_t E, bool from_next) {
  if (!from_next) L.draw.prep_side = false;
  const size_t ts = sizeof(T);
  auto& B = L.mb;
  B.batch_raw.reserve(4 * (n + 1));
  B.batch.reserve(4 * (n + 1));
  B.orig.reserve(4 * (n + 1));
  B.flags.reserve(4 * (n + 1));
  B.sincl.reserve(4 * (n + 1));
  B.bptr.reserve(8 * (n + 1));
  B.bnnz.reserve(8 * (n + 1));
  B.nnzp.reserve(8 * (n + 1));
  B.gamma.reserve(ts * n * L.k);
  B.eth.reserve(ts * n * L.kp);
  B.elogth.reserve(ts * n * L.k);
  B.iters.reserve(4 * n);
  B.nonempty.reserve(4 * n);
  B.r.reserve(ts * E);
  B.keys.reserve(4 * E);
  B.vals.reserve(8 * E);
  B.skeys.reserve(4 * E);
  B.svals.reserve(8 * E);
  const int64_t nchunks = ceil_div(E, lda::kChunk) + 1;
  B.headbuf.reserve(ts * nchunks * L.kp);
  B.tailbuf.reserve(ts * nchunks * L.kp);
  B.lpart.reserve(sizeof(double) * lda::kLogphatBlocks * (L.k + 1));
  const auto sort = [&](void* t, size_t& tb) {
    return term_sort(t, tb, B.keys.as<uint32_t>(), B.skeys.as<uint32_t>(), B.vals.as<uint64_t>(), B.svals.as<uint64_t>(),
                     std::max<int64_t>(E, 1), bits_for(L.V), L.ctx->stream);
  };
  with_temp(B.sort_tmp, sort, false);  // sized only: the step sorts its own entry count
}
template void ensure_batch<float>(stc_lda&, int64_t, int64_t, bool);
template void ensure_batch<double>(stc_lda&, int64_t, int64_t, bool);

template <typename X>
static void incl_scan(stc_lda& L, const X* in, X* out, int64_t n, hipStream_t s = nullptr, DevBuf* tmp = nullptr) {
  if (n <= 0) return;
  if (!s) s = L.ctx->stream;
  if (!tmp) tmp = &L.mb.scan_tmp;
  with_temp(*tmp, [&](void* t, size_t& tb) { return hipcub::DeviceScan::InclusiveSum(t, tb, in, out, (int)n, s); });
}

// bptr[0] = 0, bptr[i+1] = Σ_{j<=i} nnz_p[j]  (entry offsets of the partitioned slots)
static void slot_offsets(stc_lda& L, int64_t n, hipStream_t s = nullptr, DevBuf* tmp = nullptr) {
  if (!s) s = L.ctx->stream;
  HIP_CHECK(hipMemsetAsync(L.mb.bptr.p, 0, sizeof(int64_t), s));
  incl_scan<int64_t>(L, L.mb.nnzp.as<int64_t>(), L.mb.bptr.as<int64_t>() + 1, n, s, tmp);
}

// Partition members (raw = row ids on device, or nullptr for identity rows) into
// [nnz <= wave cap | rest] slots: fills mb.batch, mb.orig, mb.nnzp.  One host sync (E, n_short).
Part partition(stc_lda& L, const int64_t* indptr, const int32_t* raw, int64_t n) {
  hipStream_t s = L.ctx->stream;
  auto& B = L.mb;
  Part p;
  if (n == 0) return p;
  lda::launch_part_flags(s, indptr, raw, n, L.wave_cap, B.bnnz.as<int64_t>(), B.flags.as<int32_t>());
  incl_scan<int64_t>(L, B.bnnz.as<int64_t>(), B.bptr.as<int64_t>() + 1, n);  // temp: total E
  incl_scan<int32_t>(L, B.flags.as<int32_t>(), B.sincl.as<int32_t>(), n);
  int32_t ns = 0;
  HIP_CHECK(hipMemcpyAsync(&p.E, B.bptr.as<int64_t>() + n, 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(&ns, B.sincl.as<int32_t>() + (n - 1), 4, hipMemcpyDeviceToHost, s));
  wait_stream(*L.ctx, s);
  p.n_short = ns;
  lda::launch_part_scatter(s, raw, B.bnnz.as<int64_t>(), n, B.flags.as<int32_t>(), B.sincl.as<int32_t>(),
                           B.batch.as<int32_t>(), B.orig.as<int32_t>(), B.nnzp.as<int64_t>());
  return p;
}

// the fast kernel's slots [0, n_short) in descending nnz: the longest documents start first, so the
// launch does not end on a few long documents started late (longest-processing-time-first).  Each
// slot keeps its member index (orig: γ₀ keys, outputs), so results only change in the summation
// order of sstats within a term.
static void order_slots(stc_lda& L, int64_t n_short, hipStream_t s = nullptr) {
  // measured: no gain at 50k docs per launch (≈ 100 documents per workgroup slot, the tail is
  // short), +0.13 ms of sorting; kept for small per-rank minibatches (strong scaling), where a
  // launch is only a few documents deep
  if (!L.sw.sort_docs || n_short < 2 || n_short > 16384) return;
  if (!s) s = L.ctx->stream;
  auto& B = L.mb;
  B.o_keys.reserve(8 * n_short);
  B.o_keys2.reserve(8 * n_short);
  B.o_idx.reserve(4 * n_short);
  B.o_idx2.reserve(4 * n_short);
  B.o_batch.reserve(4 * n_short);
  B.o_orig.reserve(4 * n_short);
  B.o_nnz.reserve(8 * n_short);
  HIP_CHECK(hipMemcpyAsync(B.o_keys.p, B.nnzp.p, 8 * n_short, hipMemcpyDeviceToDevice, s));
  lda::launch_iota(s, B.o_idx.as<int32_t>(), n_short);
  with_temp(B.o_tmp, [&](void* t, size_t& tb) {
    return hipcub::DeviceRadixSort::SortPairsDescending(t, tb, B.o_keys.as<int64_t>(), B.o_keys2.as<int64_t>(),
                                                        B.o_idx.as<int32_t>(), B.o_idx2.as<int32_t>(), (int)n_short, 0, 16, s);
  });
  lda::launch_permute_slots(s, B.o_idx2.as<int32_t>(), n_short, B.batch.as<int32_t>(), B.orig.as<int32_t>(),
                            B.nnzp.as<int64_t>(), B.o_batch.as<int32_t>(), B.o_orig.as<int32_t>(),
                            B.o_nnz.as<int64_t>());
  HIP_CHECK(hipMemcpyAsync(B.batch.p, B.o_batch.p, 4 * n_short, hipMemcpyDeviceToDevice, s));
  HIP_CHECK(hipMemcpyAsync(B.orig.p, B.o_orig.p, 4 * n_short, hipMemcpyDeviceToDevice, s));
  HIP_CHECK(hipMemcpyAsync(B.nnzp.p, B.o_nnz.p, 8 * n_short, hipMemcpyDeviceToDevice, s));
}

// the many-topic kernel's row order for the training corpus: the corpus's document frequencies,
// then each row's entries by ascending df (once per set_corpus)
void ensure_order(stc_lda& L) {
  const bool wide = by_arith_type(L, [&](auto t) { return use_wide<decltype(t)>(L.k); });
  if (!L.sw.hot_order || L.wave_cap <= 0 || !wide || L.mb.order_for == L.corpus) return;
  const DCsr& m = *L.corpus;
  L.mb.order.reserve(4 * std::max<int64_t>(m.nnz, 1));
  L.mb.order_df.reserve(8 * m.cols);
  idf::doc_freq(*L.ctx, m, L.mb.order_df.as<int64_t>());
  hashing::row_order_by_df(*L.ctx, m, L.mb.order_df.as<int64_t>(), L.mb.order.as<int32_t>());
  L.mb.order_for = L.corpus;
}

// the stat sub-chunk layout of a sharded step (lda_kernels.h StatMap; nsub = 1: one reduce-scatter):
// at most rs_chunks sub-chunks of whole λ-update blocks, the last one the rest of the slice
lda::StatMap stat_layout(const stc_lda& L) {
  lda::StatMap m;
  const int64_t nb = L.model.Vs / lda::kRowsPerBlock;
  if (!sharded(L) || L.tail.rs_chunks <= 1 || nb < 2) return m;
  const int64_t per = ceil_div(nb, (int64_t)L.tail.rs_chunks);
  m.vs = (uint32_t)L.model.Vs;
  m.vsj = (uint32_t)(per * lda::kRowsPerBlock);
  m.n = L.model.shards;
  m.nsub = (int)ceil_div(nb, per);
  return m;
}

void require_ready(stc_lda& L) {
  if (!L.corpus) throw Error(STC_ERR_STATE, "no corpus: call stc_lda_set_corpus first");
  if (!L.model.has_topics) throw Error(STC_ERR_STATE, "no topics: call stc_lda_init_random or stc_lda_set_topics");
}

// sub-chunk j: (first canonical row within a slice, rows)
static std::pair<int64_t, int64_t> stat_sub_rows(const lda::StatMap& m, int j) {
  const int64_t w = j < m.nsub - 1 ? (int64_t)m.vsj : (int64_t)m.vs - (int64_t)(m.nsub - 1) * m.vsj;
  return {(int64_t)j * m.vsj, w};
}

// the fused M-step pass over one vocabulary slice r, rows [r·Vs, r·Vs + vn): λ update, the next
// expElogβ' rows + logscale, and colsum partials at λ-update block r·Vs/RB, where the one-GPU
// reduction has them.  Nothing in it needs the new colsum (ψ(colsum) is the E-step's per-topic factor).
template <typename T>
static void mstep_slice(stc_lda& L, int r, double rho, double scale, const double* gate) {
  auto& M = L.model;
  const int64_t v0 = (int64_t)r * M.Vs, vn = std::max<int64_t>(0, std::min(L.V - v0, M.Vs));
  const int64_t nbs = M.Vs / lda::kRowsPerBlock;
  lda::launch_lambda_eeb<T>(L.ctx->stream, true, M.lam.as<double>() + v0 * L.k, M.stat.as<T>() + v0 * L.kp,
                            M.Bp.as<T>() + v0 * L.kp, M.logscale.as<double>() + v0, vn, L.k, L.kp, rho, scale,
                            L.eta, gate, M.colpart.as<double>() + (int64_t)r * nbs * L.k, nbs,
                            L.mixed ? M.Bp64.as<double>() + v0 * L.kp : nullptr,
                            M.step_stamped ? M.rowstamp.as<int32_t>() + v0 : nullptr, M.step_sid);
}
// the same pass over sub-chunk j of slice r, whose summed stat rows sit at the sub-chunk layout's
// physical rows (stat_layout); λ / expElogβ' / logscale / colsum partials at their canonical rows
template <typename T>
static void mstep_sub(stc_lda& L, const lda::StatMap& m, int r, int j, double rho, double scale, const double* gate) {
  auto& M = L.model;
  const auto [off, w] = stat_sub_rows(m, j);
  const int64_t v0 = (int64_t)r * M.Vs + off, vn = std::max<int64_t>(0, std::min(L.V - v0, w));
  const int64_t phys = (int64_t)m.n * j * m.vsj + (int64_t)r * w;
  lda::launch_lambda_eeb<T>(L.ctx->stream, true, M.lam.as<double>() + v0 * L.k, M.stat.as<T>() + phys * L.kp,
                            M.Bp.as<T>() + v0 * L.kp, M.logscale.as<double>() + v0, vn, L.k, L.kp, rho, scale,
                            L.eta, gate, M.colpart.as<double>() + (v0 / lda::kRowsPerBlock) * L.k,
                            w / lda::kRowsPerBlock, L.mixed ? M.Bp64.as<double>() + v0 * L.kp : nullptr);
}

// ---- what the two tails below share ----
// the step's learning rate ρ_t, the corpus / batch scale and the device word that gates an empty batch
// (L.iteration: already this step's)
struct StepRates {
  double rho, scale;
  const double* gate;
};
static StepRates step_rates(const stc_lda& L) {
  const double batch_size = std::ceil(L.cfg.mini_batch_fraction * (double)L.corpus_total);
  return {std::pow(L.cfg.tau0 + (double)L.iteration, -L.cfg.kappa), (double)L.corpus_total / batch_size,
          L.mb.small.as<double>() + L.k};
}

// the prefetched draw's counts (dcnt; word 3 = its global size once stream q's work is done) to the host:
// the next call waits for ev_pre instead of draining a stream
static void publish_draw(stc_lda& L, hipStream_t q) {
  HIP_CHECK(hipMemcpyAsync(L.own.hpre.get(), L.draw.dcnt.p, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, q));
  HIP_CHECK(hipEventRecord(L.own.ev_pre.get(), q));
  L.draw.pre_inflight = false;
  L.draw.pre_valid = true;
}

// after a rank's slice update: the group of all-gathers and the colsum reduce (train_tail's comment)
template <typename T>
static void gather_slices(stc_lda& L, const double* gate) {
  Ctx& c = *L.ctx;
  hipStream_t s = c.stream;
  auto& M = L.model;
  const size_t nbs = (size_t)(M.Vs / lda::kRowsPerBlock), cnt = (size_t)(M.Vs * L.kp);
  coll_group_start(c);
  coll_all_gather(c, M.colpart.as<double>() + (size_t)c.rank * nbs * L.k, M.colpart.p, nbs * L.k, ncclFloat64, s);
  coll_all_gather(c, M.Bp.as<T>() + (size_t)c.rank * cnt, M.Bp.p, cnt, RcclType<T>, s);
  if (L.mixed) coll_all_gather(c, M.Bp64.as<double>() + (size_t)c.rank * cnt, M.Bp64.p, cnt, ncclFloat64, s);
  coll_all_gather(c, M.logscale.as<double>() + (size_t)c.rank * M.Vs, M.logscale.p, (size_t)M.Vs, ncclFloat64, s);
  coll_group_end(c);
  lda::launch_colsum_reduce(s, M.colpart.as<double>(), M.shards * (int64_t)nbs, L.k, gate, M.colsum.as<double>(),
                            M.psic.as<double>());
  M.lam_stale = true;
}

// updateAlpha, the step's timing and counters, and the caller's statistics
static void train_finish(stc_lda& L, const StepRates& sr, int64_t n, int64_t E, stc_step_stats* st) {
  hipStream_t s = L.ctx->stream;
  if (L.cfg.optimize_doc_concentration)
    lda::launch_update_alpha(s, L.model.alpha.as<double>(), L.mb.small.as<double>(), L.k, sr.rho);
  record(L, 5);
  if (L.tm.timing) {
    L.tm.ev_pending[L.tm.ev_set] = true;
    L.tm.ev_set = (L.tm.ev_set + 1) % 3;
  }
  L.tm.cum_docs += n;
  L.tm.cum_entries += E;
  if (st) {
    int64_t h4[4] = {0, 0, 0, 0};
    double ne = 0.0;
    // a copy to pageable memory can block in the runtime: behind collectives, wait (polling) first
    if (L.ctx->comm) wait_stream(*L.ctx, s);
    HIP_CHECK(hipMemcpyAsync(h4, L.mb.stats4.p, sizeof(h4), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&ne, L.mb.small.as<double>() + L.k, sizeof(double), hipMemcpyDeviceToHost, s));
    wait_stream(*L.ctx, s);
    st->batch_docs = n;
    st->batch_entries = E;
    st->inner_iters = h4[0];
    st->inner_iters_max = (int32_t)h4[1];
    st->cap_hits = (int32_t)h4[2];
    st->nonempty_docs = (int64_t)ne;
    st->rho = sr.rho;
  }
}

// train_tail's N-rank form with rs_chunks > 1 (stat_layout: nsub sub-chunks): sstats ran once per sub-chunk
// (estep_and_stats split) and recorded ev_ss[j]; the reduce-scatter of sub-chunk j (one contiguous buffer in
// that layout) runs on cstream as soon as ev_ss[j] fires — under the sstats launches of j+1… — with the
// logphat / count all-reduce in sub-chunk 0's group, and the main stream runs the M-step of sub-chunk j under
// the reduce-scatter of j+1.  Each element is summed over the same ranks in the same way as by the single
// reduce-scatter, and sstats builds every row exactly as the single launch does, so the result is the
// unchunked step's.
template <typename T>
static void train_tail_split(stc_lda& L, const lda::StatMap& lay, bool had_samp, int64_t n, int64_t E,
                      stc_step_stats* st) {
  Ctx& c = *L.ctx;
  hipStream_t s = c.stream, cs = L.own.cstream.get();
  if (had_samp) HIP_CHECK(hipStreamWaitEvent(cs, L.own.ev_samp.e, 0));  // the next draw's count (side stream)
  for (int j = 0; j < lay.nsub; ++j) {
    HIP_CHECK(hipStreamWaitEvent(cs, L.own.ev_ss[j].e, 0));
    const int64_t w = stat_sub_rows(lay, j).second;
    T* chunk = L.model.stat.as<T>() + (int64_t)lay.n * j * lay.vsj * L.kp;
    coll_group_start(c);
    coll_reduce_scatter(c, chunk, chunk + (int64_t)c.rank * w * L.kp, (size_t)(w * L.kp), RcclType<T>, cs);
    if (j == 0) {
      coll_all_reduce(c, L.mb.small.p, (size_t)(L.k + 1), ncclFloat64, cs);
      if (L.draw.pre_inflight) coll_all_reduce(c, L.draw.dcnt.as<int64_t>() + 3, 1, ncclInt64, cs);
    }
    coll_group_end(c);
    if (j == 0 && L.draw.pre_inflight) publish_draw(L, cs);
    HIP_CHECK(hipEventRecord(L.own.ev_rs[j].get(), cs));
  }
  L.iteration += 1;
  const StepRates sr = step_rates(L);
  for (int j = 0; j < lay.nsub; ++j) {
    HIP_CHECK(hipStreamWaitEvent(s, L.own.ev_rs[j].e, 0));
    if (j == 0) record(L, 4);  // the statistics of sub-chunk 0 and the logphat / count sums are in
    mstep_sub<T>(L, lay, c.rank, j, sr.rho, sr.scale, sr.gate);
  }
  gather_slices<T>(L, sr.gate);
  train_finish(L, sr, n, E, st);
}

// [U] submitMiniBatch tail: the stats merge (treeReduce ≙ RCCL), updateLambda, updateAlpha.
//  * one GPU: the fused λ update + expElogβ' pass over all rows, then colsum and ψ(colsum).
//  * N ranks: reduce-scatter of stat (each rank receives the summed rows of its vocabulary slice) and
//    the logphat / count all-reduce in one group; the slice's fused λ update + expElogβ' pass; ONE
//    group of all-gathers — the per-block colsum partials (k doubles per 64 rows), expElogβ' and
//    logscale — then colsum reduced in the one-GPU block order, so it is identical on every rank.
//    λ stays sharded (lam_stale) until a reader gathers it.  Per rank: stat (N−1)/N·V·kp·T bytes
//    out, expElogβ' the same in, against 2(N−1)/N for an all-reduce, and 1/N of the M-step work.
template <typename T>
static void train_tail(stc_lda& L, int64_t n, int64_t E, stc_step_stats* st) {
  Ctx& c = *L.ctx;
  hipStream_t s = c.stream;
  auto& M = L.model;
  const bool ranks = sharded(L);
  const lda::StatMap lay = stat_layout(L);
  if (L.tail.tail_fault > 0 && --L.tail.tail_fault == 0) {
    throw Error(STC_ERR_STATE, "injected member failure between sstats and the reduce-scatter (STC_GROUP_STEP_FAULT)");
  }
  const bool had_samp = L.draw.samp_pending;
  if (L.draw.samp_pending) {  // the next draw's counts (side stream) feed this step's collective / readback
    HIP_CHECK(hipStreamWaitEvent(s, L.own.ev_samp.e, 0));
    L.draw.samp_pending = false;
  }
  if (ranks && lay.nsub > 1) {
    train_tail_split<T>(L, lay, had_samp, n, E, st);
    return;
  }
  if (c.coll()) {
    coll_group_start(c);
    if (ranks) {
      const size_t cnt = (size_t)(M.Vs * L.kp);
      coll_reduce_scatter(c, M.stat.p, M.stat.as<T>() + (size_t)c.rank * cnt, cnt, RcclType<T>, s);
    }
    coll_all_reduce(c, L.mb.small.p, (size_t)(L.k + 1), ncclFloat64, s);
    if (L.draw.pre_inflight)  // the next draw's global batch size (word 3), for the next call
      coll_all_reduce(c, L.draw.dcnt.as<int64_t>() + 3, 1, ncclInt64, s);
    coll_group_end(c);
  }
  if (L.draw.pre_inflight) publish_draw(L, s);
  record(L, 4);
  L.iteration += 1;
  const StepRates sr = step_rates(L);
  if (ranks) {
    mstep_slice<T>(L, c.rank, sr.rho, sr.scale, sr.gate);
    gather_slices<T>(L, sr.gate);
  } else {  // one GPU: all slices here (one unless STC_VIRTUAL_SHARDS)
    for (int r = 0; r < M.shards; ++r) mstep_slice<T>(L, r, sr.rho, sr.scale, sr.gate);
    lda::launch_colsum_reduce(s, M.colpart.as<double>(), M.shards * (M.Vs / lda::kRowsPerBlock), L.k, sr.gate,
                              M.colsum.as<double>(), M.psic.as<double>());
  }
  train_finish(L, sr, n, E, st);
}

// sample draw `draw` on the device: per-doc counts (Poisson / Bernoulli), their scans, and (n, E,
// n_short) into dcnt words 0–2, word 3 = n (all-reduced to the global n by the caller)
static void sample_draw(stc_lda& L, int64_t draw, hipStream_t s, DevBuf* tmp) {
  Ctx& c = *L.ctx;
  auto& W = L.draw;
  const int64_t D = L.corpus->rows;
  if (D > 0) {
    lda::launch_sample(s, L.corpus->indptr.as<int64_t>(), D, L.cfg.mini_batch_fraction,
                       L.cfg.sample_with_replacement, L.cfg.seed, draw, c.rank, L.wave_cap,
                       W.s_counts.as<int32_t>(), W.s_weights.as<int64_t>(), W.s_short.as<int32_t>());
    incl_scan<int32_t>(L, W.s_counts.as<int32_t>(), W.s_cincl.as<int32_t>(), D, s, tmp);
    incl_scan<int64_t>(L, W.s_weights.as<int64_t>(), W.s_wincl.as<int64_t>(), D, s, tmp);
    incl_scan<int32_t>(L, W.s_short.as<int32_t>(), W.s_sincl.as<int32_t>(), D, s, tmp);
    // (n, E, n_short) from the scans' last elements: one kernel packs them, one copy to pinned memory
    lda::launch_last3(s, W.s_cincl.as<int32_t>() + (D - 1), W.s_wincl.as<int64_t>() + (D - 1),
                      W.s_sincl.as<int32_t>() + (D - 1), W.dcnt.as<int64_t>());
  } else {  // a rank without documents still takes part in every collective
    HIP_CHECK(hipMemsetAsync(W.dcnt.p, 0, 3 * sizeof(int64_t), s));
  }
  HIP_CHECK(hipMemcpyAsync(W.dcnt.as<int64_t>() + 3, W.dcnt.p, sizeof(int64_t), hipMemcpyDeviceToDevice, s));
}

// host-injected membership → partitioned slots on the device; returns the partition
template <typename T>
Part upload_members(stc_lda& L, const int64_t* ids, int64_t n) {
  std::vector<int32_t> h((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    STC_REQUIRE(ids[i] >= 0 && ids[i] < L.corpus->rows, "batch doc id out of range");
    h[(size_t)i] = (int32_t)ids[i];
  }
  ensure_batch<T>(L, n, 0);
  if (n > 0)
    HIP_CHECK(hipMemcpyAsync(L.mb.batch_raw.p, h.data(), 4 * n, hipMemcpyHostToDevice, L.ctx->stream));
  Part p = partition(L, L.corpus->indptr.as<int64_t>(), L.mb.batch_raw.as<int32_t>(), n);  // syncs
  ensure_batch<T>(L, n, p.E);
  slot_offsets(L, n);
  return p;
}
template Part upload_members<float>(stc_lda&, const int64_t*, int64_t);
template Part upload_members<double>(stc_lda&, const int64_t*, int64_t);

template <typename T>
void step_ids(stc_lda& L, const int64_t* ids, int64_t n, const double* gamma0, stc_step_stats* st) {
  require_ready(L);
  relayout(L);
  ensure_order(L);
  claim_event_set(L);
  record(L, 0);
  const Part p = upload_members<T>(L, ids, n);
  if (L.tm.timing) harvest_all(L);  // partition() drained the stream
  const T* g0 = upload_gamma0<T>(L, gamma0, n);
  if (!g0) g0 = gen_gamma0<T>(L, L.ctx->stream, n, L.cfg.seed, L.iteration + 1, 0, 0);
  estep_and_stats<T>(L, n, p.n_short, p.E, g0, L.iteration + 1, true, mixed_gamma0(L, gamma0, n));
  train_tail<T>(L, n, p.E, st);
}
template void step_ids<float>(stc_lda&, const int64_t*, int64_t, const double*, stc_step_stats*);
template void step_ids<double>(stc_lda&, const int64_t*, int64_t, const double*, stc_step_stats*);

// [U] OnlineLDAOptimizer.next(): sample a minibatch (device-side), `if (batch.isEmpty()) return this`
// on the GLOBAL batch, else submitMiniBatch.  Draw d's membership is sampled while step d−1 runs
// (after its fill_batch, so the count buffers are free) and its global size is all-reduced with
// step d−1's statistics; the host then waits only on that collective's event — the GPU is still
// busy with step d−1's M-step when step d is enqueued.  The first draw (or one after an empty
// batch, set_corpus or init_random) is sampled and counted synchronously.
template <typename T>
void next_impl(stc_lda& L, stc_step_stats* st) {
  require_ready(L);
  settle_side(L);
  relayout(L);
  ensure_order(L);
  Ctx& c = *L.ctx;
  hipStream_t s = c.stream;
  auto& W = L.draw;
  auto& O = L.own;
  const int64_t D = L.corpus->rows;
  W.s_counts.reserve(4 * D);
  W.s_weights.reserve(8 * D);
  W.s_short.reserve(4 * D);
  W.s_cincl.reserve(4 * D);
  W.s_wincl.reserve(8 * D);
  W.s_sincl.reserve(4 * D);
  W.dcnt.reserve(4 * sizeof(int64_t));
  const int64_t draw = ++W.draws;
  claim_event_set(L);
  record(L, 0);
  int64_t cnt[4];
  // the prefetched draw's batch is built on the side stream (behind its sampling, and behind the previous
  // step's E-step — ev_est), under the previous step's M-step and all-gathers
  const bool prefetched = W.pre_valid && W.pre_draw == draw;
  const bool on_side = prefetched && W.prep_side && O.side.s && O.ev_est.e;
  if (prefetched) {
    wait_event(*L.ctx, O.ev_pre.e);
    std::copy(O.hpre.p, O.hpre.p + 4, cnt);
  } else {
    sample_draw(L, draw, s, &L.mb.scan_tmp);
    if (c.coll()) coll_all_reduce(c, W.dcnt.as<int64_t>() + 3, 1, ncclInt64, s);
    HIP_CHECK(hipMemcpyAsync(O.hcnt.get(), W.dcnt.p, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    wait_stream(*L.ctx, s);
    std::copy(O.hcnt.p, O.hcnt.p + 4, cnt);
  }
  W.pre_valid = false;
  const int64_t n = cnt[0], E = cnt[1], ns32 = cnt[2], n_global = cnt[3];
  if (L.tm.timing) harvest_all(L);
  // Spark's next(): `if (batch.isEmpty()) return this` — no iteration increment
  if (n_global == 0) {
    if (st) *st = stc_step_stats{};
    return;
  }
  ensure_batch<T>(L, n, E, true);
  const hipStream_t ps = on_side ? O.side.s : s;
  if (on_side) HIP_CHECK(hipStreamWaitEvent(ps, O.ev_est.e, 0));
  if (n > 0)
    lda::launch_fill_batch(ps, L.corpus->indptr.as<int64_t>(), D, L.wave_cap, W.s_counts.as<int32_t>(),
                           W.s_cincl.as<int32_t>(), W.s_sincl.as<int32_t>(), ns32, L.mb.batch.as<int32_t>(),
                           L.mb.orig.as<int32_t>(), L.mb.nnzp.as<int64_t>());
  order_slots(L, ns32, ps);
  slot_offsets(L, n, ps, on_side ? &W.side_scan_tmp : &L.mb.scan_tmp);
  const T* g0 = gen_gamma0<T>(L, ps, n, L.cfg.seed, L.iteration + 1, 0, 0);
  // the next draw, on the side stream beside this step's E-step, counted with this step's collective
  const hipStream_t side = O.side.get();  // (the first next() makes it)
  O.ev_est.get();  // from here on estep_and_stats records it
  HIP_CHECK(hipEventRecord(O.ev_fill.get(), ps));  // this draw's counts consumed and its batch built
  HIP_CHECK(hipStreamWaitEvent(on_side ? s : side, O.ev_fill.e, 0));
  sample_draw(L, draw + 1, side, &W.side_scan_tmp);
  HIP_CHECK(hipEventRecord(O.ev_samp.get(), side));
  W.samp_pending = true;
  W.pre_draw = draw + 1;
  if (c.coll()) {
    W.pre_inflight = true;  // the global size rides on this step's collective (train_tail reads it back)
  } else {
    // one rank: the draw's size is already global — read it back on the side stream as soon as it is sampled
    // (during this step's E-step), so the next call enqueues its batch preparation at once and the side stream
    // builds it under this step's sstats and M-step; read back in train_tail, after the E-step and sstats, the
    // preparation only started under the M-step and the next E-step waited for it (the "sample" phase, 0.29 ms)
    publish_draw(L, side);
  }
  estep_and_stats<T>(L, n, ns32, E, g0, L.iteration + 1, true);
  train_tail<T>(L, n, E, st);
  W.prep_side = true;
}
template void next_impl<float>(stc_lda&, stc_step_stats*);
template void next_impl<double>(stc_lda&, stc_step_stats*);

}  // namespace stc::online
