// lda_handle.h — struct stc_lda and what the three translation units behind the stc_lda_* entry points share:
// lda_dispatch.hip (which kernel runs these slots), lda_train.hip (a training step around the E-step) and
// lda_online.hip (the C ABI and the readers).  Private to those three and to lda_score.hip (the document scores,
// which read γ, λ and the handle's shape); no kernel file includes it.
#pragma once

#include <type_traits>

#include "collectives.h"
#include "lda_kernels.h"
#include "lda_step_kernels.h"
#include "stc_handles.h"

// Members by the code that owns them.  Release order: members go last-declared first, so `own`, the last group
// and the only one with streams, events or pinned words, is gone before any DevBuf of the groups above is freed.
struct stc_lda {
  stc::Ctx* ctx = nullptr;
  stc_lda_config cfg{};
  int k = 0, kp = 0, P = 0, lds_rows = 0;
  int64_t V = 0;
  // STC_MIXED: dtype STC_F32 inside the library plus `mixed` — the fp32 E-step, then the documents past
  // mix.mixed_thr fp32 iterations re-solved in fp64 (mixed_resolve)
  int dtype = STC_F32;
  bool mixed = false;
  double eta = 0.0;
  int64_t iteration = 0;
  const stc::DCsr* corpus = nullptr;
  int64_t corpus_total = 0;
  int64_t wave_cap = 0;  // docs with nnz <= wave_cap run the register-resident E-step of the (k, dtype)

  // λ and what the M-step derives from it (ensure_layout, refresh, the M-step slices)
  struct Model {
    stc::DevBuf lam, Bp, logscale, colsum, psic, colpart, alpha;
    stc::DevBuf Bp64;  // mixed: the fp64 expElogβ' rows the M-step writes beside Bp
    // M-step sharding over the vocabulary (multi-GPU): rank r owns λ / expElogβ rows [r·Vs, (r+1)·Vs);
    // Vs is a multiple of the λ-update block so the per-block colsum partials (and hence colsum) are
    // bit-identical to the one-GPU reduction.  virt > 1 runs the same slices on one GPU without
    // collectives (STC_VIRTUAL_SHARDS, for testing the slicing).
    int shards = 1, virt = 1;
    int64_t Vs = 0, vpad = 0, nblocks_m = 0;
    // the step's statistic, laid out as λ.  One rank: sstats stamps the rows it writes (rowstamp[v] = the step's
    // id) and the M-step reads the other rows as zero, so stat is not cleared every step (V·kp·T bytes: 4.2 GB
    // at config 5)
    stc::DevBuf stat, rowstamp;
    int32_t stamp_seq = 0, step_sid = 0;
    bool step_stamped = false;
    bool lam_stale = false;  // rows outside this rank's slice are out of date (sharded M-step)
    bool has_topics = false;
  } model;

  // one launch's documents: slot lists, per-slot and per-entry outputs, the sstats sort (ensure_batch)
  struct Batch {
    stc::DevBuf batch_raw, batch, orig, flags, sincl, bptr, bnnz, nnzp, g0, gamma, eth, elogth, iters, nonempty, r, keys,
        vals, skeys, svals, headbuf, tailbuf, sort_tmp, scan_tmp, small, stats4, cum2, lpart;
    stc::DevBuf g0gen;      // γ₀ drawn ahead of the E-step (lda::launch_gamma0) when the caller injects none
    stc::DevBuf long_list;  // rows / grid kernels: the launch's long documents (count word + slot offsets)
    stc::DevBuf o_keys, o_keys2, o_idx, o_idx2, o_batch, o_orig, o_nnz, o_tmp;  // slot ordering (order_slots)
    // many-topic kernel: per-entry row order, rarest terms first (lda_wide.hip), for `order_for`
    stc::DevBuf order, order_df;
    const stc::DCsr* order_for = nullptr;
    stc::DevBuf bound, scal, dtmp;  // the readers' scratch (infer_impl, topics_part, estep_only)
  } mb;

  // STC_MIXED: the fp64 re-solve's shape, lists and outputs (mixed_resolve); vals32 is the fp32 copy of the
  // corpus's fp64 values that the fp32 E-step reads
  struct Mixed {
    int mixed_thr = 500;
    int P64 = 0, lds_rows64 = 0;  // the fp64 workgroup kernel's LDS pitch / rows at this kp
    int64_t cap64 = 0;            // the fp64 fast kernels' row capacity (longer documents: the workgroup kernel)
    stc::DevBuf vals32, m_batch, m_orig, m_bptr, m_slot, m_cnt, eth64, elogth64, r64, keys64, vals64, gamma64, g0_64;
  } mix;

  // minibatch draws (sample_draw, next_impl): Spark's next() advances its generator on every call, empty
  // batches included
  struct Draw {
    stc::DevBuf s_counts, s_weights, s_short, s_cincl, s_wincl, s_sincl, dcnt, side_scan_tmp;
    int64_t draws = 0;
    // the next draw is sampled on the side stream, concurrently with this step's E-step (it reads only
    // indptr and writes only the s_* buffers, which this step's fill_batch has consumed)
    bool samp_pending = false;
    // next(): the prefetched draw's batch (fill, slot order, offsets) is built on the side stream once the
    // previous step's E-step has read the batch buffers (ev_est), under that step's M-step and all-gathers.
    // prep_side: the last user of the batch buffers was next() (any other call's ensure_batch clears it).
    bool prep_side = false;
    // prefetch: the next draw's membership is sampled during this step and its global size rides on
    // this step's collective, so the next call waits on an event instead of draining the stream
    bool pre_valid = false, pre_inflight = false;
    int64_t pre_draw = 0;
  } draw;

  // sharded steps (train_tail): stat reduce-scattered in rs_chunks vocabulary sub-chunks on cstream, each as
  // soon as its sstats launch is done, and the M-step of sub-chunk j under the reduce-scatter of j+1
  // (STC_RS_CHUNKS, 1: one reduce-scatter after the whole stat)
  struct Tail {
    int rs_chunks = 4;
    bool force_coll = false;  // STC_COLLECTIVE_MSTEP=1: the RCCL slice path even on a 1-rank communicator (tests)
    int tail_fault = 0;  // test knob (STC_GROUP_STEP_FAULT): the tail_fault-th next step throws before its reduce-scatter
  } tail;

  // many-topic documents larger than one CU: the team kernels' polled words and exchange granules (launch_wide_team)
  struct Team {
    stc::DevBuf team_words, team_x;
  } team;

  // phase timing (record / harvest) and the counters the getters report
  struct Timing {
    bool timing = false;
    int ev_set = 0;
    bool ev_pending[3] = {false, false, false};
    double acc_ms[5] = {0, 0, 0, 0, 0};
    int64_t timed_steps = 0;
    int64_t cum_docs = 0, cum_entries = 0;
    int64_t kcount[STC_KC_N] = {};  // E-step launches per kernel family (stc_lda_kernel_counts)
  } tm;

  // the STC_* switches stc_lda_create reads once
  struct Switches {
    bool sort_docs = true;  // STC_SORT_DOCS=0 keeps sampling order
    // fp64 rows kernels: the sstats pairs built and radix-sorted beside the E-step (estep_and_stats), on the side
    // stream when the handle has one, else on sort_stream; STC_PRESORT=0 sorts them after the E-step
    bool presort = true;
    bool hot_order = true;  // STC_HOT_ORDER=0: CSR order
    int team_force = 0;     // STC_WIDE_TEAM=n forces a team of n CUs per many-topic document (1: the one-CU kernel)
    bool tgrid = true;  // fp64 many-topic documents: the topic-split grid team kernel when they fit (STC_TGRID=0: off)
    bool tgrid_require = false;  // STC_TGRID=2 (tests): a many-topic fp64 launch that cannot take it is an error
  } sw;

  // The streams, events and pinned host words, each made on first use (stc_handles.h): the timing events, the
  // pinned words, then each stream after its events.  stc_lda_destroy drains the main stream, side and cstream
  // first; sort_stream needs no drain, because every call that uses it makes the main stream wait for ev_sorted
  // before it returns, so the drained main stream has seen the sort's end.
  struct Owners {
    stc::Stream sort_stream;  // lowest priority; made when the presort runs on a handle that has no side stream
    stc::Event ev_sorted, ev_ps0;
    stc::Stream cstream;  // made by the first chunked sharded tail
    stc::Event ev_rs[16], ev_ss[16];
    stc::Stream side;  // made by the first next()
    stc::Event ev_est, ev_samp, ev_fill, ev_pre;
    stc::Pinned<unsigned> htmo;          // the team kernel's timeout word
    stc::Pinned<int64_t, 4> hpre, hcnt;  // a draw's (n, E, n_short, global n): prefetched / read synchronously
    stc::Pinned<int32_t, 2> hmcnt;       // mixed_resolve's two list counts
    stc::Event ev[3][6];                 // phase timing (made in stc_lda_create, timing on)
  } own;
};

namespace stc::online {

// ---- one dispatch on the handle's precision ----
// the arithmetic type of training and stc_lda_estep (a mixed handle: float, its re-solve apart)
template <typename F>
auto by_arith_type(const stc_lda& L, F&& f) {
  if (L.dtype == STC_F32) return f(float{});
  return f(double{});
}
// the arithmetic type of bound() and topic_distribution(): a mixed handle infers in fp64
template <typename F>
auto by_infer_type(const stc_lda& L, F&& f) {
  if (L.dtype == STC_F32 && !L.mixed) return f(float{});
  return f(double{});
}
inline size_t arith_size(const stc_lda& L) {
  return by_arith_type(L, [](auto t) { return sizeof(t); });
}

template <typename T>
constexpr ncclDataType_t RcclType = std::is_same<T, float>::value ? ncclFloat32 : ncclFloat64;
// the register-resident kernel for the (k, T): the grid kernels up to k = 128 (fp32) / 104 (fp64), the
// topics-across-lanes kernel (lda_wide.hip) beyond; fast_row_cap: the longest document that kernel takes
template <typename T>
int grid_family_cap(int k) { return std::is_same<T, float>::value ? lda::grid_row_cap(k) : lda::rows64_row_cap(k); }
template <typename T>
bool use_wide(int k) { return grid_family_cap<T>(k) == 0; }
template <typename T>
int fast_row_cap(int k) { return use_wide<T>(k) ? lda::wide_row_cap(k) : grid_family_cap<T>(k); }

inline int bits_for(int64_t n) {
  int b = 1;
  while ((int64_t(1) << b) < n) ++b;
  return b;
}
// a step's M-step is sharded over the ranks (reduce-scatter, slice update, all-gather)
inline bool sharded(const stc_lda& L) { return L.ctx->coll() && (L.ctx->n_ranks > 1 || L.tail.force_coll); }

struct Part {
  int64_t E = 0, n_short = 0;
};

// ---- lda_dispatch.hip (the templates instantiated there for float and double) ----
hipError_t term_sort(void* tmp, size_t& bytes, const uint32_t* kin, uint32_t* kout, const uint64_t* vin, uint64_t* vout,
                     int64_t n, int bits, hipStream_t s);
template <typename T>
lda::EStepArgs<T> estep_args(stc_lda& L);
template <typename T>
void launch_split(stc_lda& L, const DCsr& m, lda::EStepArgs<T> a, int64_t n, int64_t n_short, bool stats, bool bound,
                  double mean_rows);
template <typename T>
const T* upload_gamma0(stc_lda& L, const double* gamma0, int64_t n);
const double* mixed_gamma0(stc_lda& L, const double* gamma0, int64_t n);
template <typename T>
const T* gen_gamma0(stc_lda& L, hipStream_t s, int64_t n, uint64_t seed, int64_t iteration, int key_mode, int64_t base);
template <typename T>
void estep_and_stats(stc_lda& L, int64_t n, int64_t n_short, int64_t E, const T* g0, int64_t iteration,
                     bool split = false, const double* g0_64 = nullptr, bool want_gamma = false);

// ---- lda_train.hip (likewise) ----
void record(stc_lda& L, int slot);  // phase timing: event `slot` of the current set
void harvest_all(stc_lda& L);
void ensure_layout(stc_lda& L);
void relayout(stc_lda& L);
void refresh(stc_lda& L);
void ensure_order(stc_lda& L);
void require_ready(stc_lda& L);
lda::StatMap stat_layout(const stc_lda& L);
Part partition(stc_lda& L, const int64_t* indptr, const int32_t* raw, int64_t n);
template <typename T>
void ensure_batch(stc_lda& L, int64_t n, int64_t E, bool from_next = false);
template <typename T>
Part upload_members(stc_lda& L, const int64_t* ids, int64_t n);
template <typename T>
void step_ids(stc_lda& L, const int64_t* ids, int64_t n, const double* gamma0, stc_step_stats* st);
template <typename T>
void next_impl(stc_lda& L, stc_step_stats* st);


// ---- lda_online.hip ----
// the E-step of stc_lda_topic_distribution over `docs`; returns γ on the device (rows×k of by_infer_type's type,
// the handle's mb.gamma: valid until the handle's next call), enqueued on the context's stream
const void* score_gamma(stc_lda& L, const DCsr& docs, uint64_t seed, int64_t base, const double* gamma0);

}  // namespace stc::online
