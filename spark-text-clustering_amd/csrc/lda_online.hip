// lda_online.hip — the stc_lda_* entry points (include/stc.h) of the online-LDA handle: create (which reads
// every STC_* switch of a handle) and destroy, the model's setters and getters, and the readers — the E-step
// alone, inference (topic distribution, the bound) and describe.  One submitMiniBatch per stc_lda_step /
// stc_lda_next: lda_train.hip; the kernel chosen for a launch: lda_dispatch.hip; struct stc_lda: lda_handle.h.
#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#include "lda_handle.h"
#include "lda_online.h"
#include "rank.h"

using namespace stc;
using namespace stc::online;

namespace {

// γ of the n slots' members (the launch's dtype) to the host, widened to double
template <typename T>
void read_gamma(stc_lda& L, int64_t n, double* gamma_out) {
  if (!gamma_out || n <= 0) return;
  hipStream_t s = L.ctx->stream;
  std::vector<T> g((size_t)(n * L.k));
  HIP_CHECK(hipMemcpyAsync(g.data(), L.mb.gamma.p, sizeof(T) * g.size(), hipMemcpyDeviceToHost, s));
  wait_stream(*L.ctx, s);
  for (size_t j = 0; j < g.size(); ++j) gamma_out[j] = (double)g[j];
}

template <typename T>
void estep_only(stc_lda& L, const int64_t* ids, int64_t n, const double* gamma0, double* gamma_out,
                double* stat_out, int32_t* iters_out) {
  require_ready(L);
  relayout(L);
  ensure_order(L);
  hipStream_t s = L.ctx->stream;
  const Part p = upload_members<T>(L, ids, n);
  // γ₀ drawn inside the E-step kernel when not injected (no n×k buffer: ADVICE r5); the pre-drawn form
  // (gen_gamma0) is used only by the training steps, where it was measured to help
  const T* g0 = upload_gamma0<T>(L, gamma0, n);
  const bool t = L.tm.timing;
  L.tm.timing = false;
  estep_and_stats<T>(L, n, p.n_short, p.E, g0, L.iteration + 1, false, mixed_gamma0(L, gamma0, n), gamma_out != nullptr);
  L.tm.timing = t;
  read_gamma<T>(L, n, gamma_out);
  if (iters_out && n > 0) {
    HIP_CHECK(hipMemcpyAsync(iters_out, L.mb.iters.p, 4 * n, hipMemcpyDeviceToHost, s));
  }
  if (stat_out) {
    L.mb.dtmp.reserve(sizeof(double) * L.V * L.k);
    lda::launch_unscale_stat<T>(s, L.model.stat.as<T>(), L.model.logscale.as<double>(), L.model.psic.as<double>(), L.V,
                                L.k, L.kp, L.mb.dtmp.as<double>());
    HIP_CHECK(hipMemcpyAsync(stat_out, L.mb.dtmp.p, sizeof(double) * L.V * L.k, hipMemcpyDeviceToHost, s));
  }
  wait_stream(*L.ctx, s);
}

// the E-step over other documents than the training corpus (so no row order), keyed by doc_id_base + row
template <typename T>
void infer_impl(stc_lda& L, const DCsr& docs, uint64_t seed, int64_t base, const double* gamma0,
                bool bound, double* gamma_out, double* out4 /* corpus, tokens */, bool keep_gamma = false) {
  if (!L.model.has_topics) throw Error(STC_ERR_STATE, "no topics: call stc_lda_init_random or stc_lda_set_topics");
  STC_REQUIRE(docs.cols == L.V, "document vectors must have vocab_size columns");
  STC_REQUIRE(docs.dtype == corpus_dtype(L), "document CSR dtype must match the LDA dtype (STC_F64 for STC_MIXED)");
  hipStream_t s = L.ctx->stream;
  auto& B = L.mb;
  const int64_t n = docs.rows;
  ensure_batch<T>(L, n, 0);
  B.r.reserve(sizeof(T) * std::max<int64_t>(docs.nnz, 1));
  B.bound.reserve(sizeof(double) * std::max<int64_t>(n, 1));
  B.scal.reserve(sizeof(double) * 8);
  const Part p = partition(L, docs.indptr.as<int64_t>(), nullptr, n);
  const T* g0 = upload_gamma0<T>(L, gamma0, n);  // nullptr: drawn inside the E-step kernel (as estep_only)
  lda::EStepArgs<T> a = estep_args<T>(L);
  a.indptr = docs.indptr.as<int64_t>();
  a.indices = docs.indices.as<int32_t>();
  a.values = docs.values.as<T>();
  a.batch = B.batch.as<int32_t>();
  a.orig = B.orig.as<int32_t>();
  a.bptr = nullptr;  // entry slots = the rows' CSR positions
  a.gamma0 = g0;
  a.seed = seed;
  a.key_mode = 1;
  a.doc_id_base = base;
  a.r = B.r.as<T>();
  a.gamma = (gamma_out || keep_gamma) ? B.gamma.as<T>() : nullptr;  // keep_gamma: γ stays in mb.gamma (score_gamma)
  a.iters = B.iters.as<int32_t>();
  a.bound = bound ? B.bound.as<double>() : nullptr;
  a.lam = bound && !L.model.lam_stale ? L.model.lam.as<double>() : nullptr;
  launch_split<T>(L, docs, a, n, p.n_short, false, bound, n > 0 ? (double)docs.nnz / (double)n : 0.0);
  read_gamma<T>(L, n, gamma_out);
  if (bound) {
    double h[3] = {0, 0, 0};
    HIP_CHECK(hipMemsetAsync(B.scal.p, 0, sizeof(double) * 3, s));
    if (n > 0) lda::launch_sum_vals<double>(s, B.bound.as<double>(), n, B.scal.as<double>());
    if (docs.nnz > 0) lda::launch_sum_vals<T>(s, docs.values.as<T>(), docs.nnz, B.scal.as<double>() + 1);
    HIP_CHECK(hipMemcpyAsync(h, B.scal.p, sizeof(double) * 2, hipMemcpyDeviceToHost, s));
    wait_stream(*L.ctx, s);
    out4[0] = h[0];
    out4[1] = h[1];
  }
}

// [U] logLikelihoodBound topicsPart: the per-element sum over the rows this rank holds current (its
// slice when λ is sharded — the caller all-reduces it — else all rows), and separately the
// per-topic normaliser terms Σ_k (lgamma(η·V) − lgamma(Σ_v λ_vk)) from the global colsum (added once).
void topics_part(stc_lda& L, double* elem_part, double* norm_part) {
  hipStream_t s = L.ctx->stream;
  auto& B = L.mb;
  const int64_t nb = 1024;
  B.dtmp.reserve(sizeof(double) * (nb + 1));
  B.scal.reserve(sizeof(double) * 8);
  int64_t v0 = 0, vn = L.V;
  if (L.model.lam_stale) {
    v0 = (int64_t)L.ctx->rank * L.model.Vs;
    vn = std::max<int64_t>(0, std::min(L.V - v0, L.model.Vs));
  }
  HIP_CHECK(hipMemsetAsync(B.dtmp.p, 0, sizeof(double) * nb, s));
  if (vn > 0)
    lda::launch_topics_bound(s, L.model.lam.as<double>() + v0 * L.k, L.model.colsum.as<double>(), vn, L.k, L.eta,
                             B.dtmp.as<double>(), nb);
  lda::launch_sum_vals<double>(s, B.dtmp.as<double>(), nb, B.scal.as<double>() + 3);
  double part = 0.0;
  std::vector<double> cs((size_t)L.k);
  HIP_CHECK(hipMemcpyAsync(&part, B.scal.as<double>() + 3, sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(cs.data(), L.model.colsum.p, sizeof(double) * L.k, hipMemcpyDeviceToHost, s));
  wait_stream(*L.ctx, s);
  // sumEta = η·V (Dirichlet normaliser of q(β_k|λ_k) minus that of p(β_k|η))
  const double lg_sum_eta = std::lgamma(L.eta * (double)L.V);
  double norm = 0.0;
  for (int t = 0; t < L.k; ++t) norm += lg_sum_eta - std::lgamma(cs[(size_t)t]);
  *elem_part = part;
  *norm_part = norm;
}

}  // namespace

// lda_score.hip's E-step: stc_lda_topic_distribution's, with γ (rows×k of the infer type) left in mb.gamma
const void* stc::online::score_gamma(stc_lda& L, const DCsr& docs, uint64_t seed, int64_t base, const double* gamma0) {
  by_infer_type(L, [&](auto t) {
    infer_impl<decltype(t)>(L, docs, seed, base, gamma0, false, nullptr, nullptr, true);
  });
  return L.mb.gamma.p;
}

extern "C" {

// ---- LDA ----------------------------------------------------------------------------------
void stc_lda_config_default(stc_lda_config* c) {
  if (!c) return;
  *c = stc_lda_config{};
  c->k = 10;
  c->vocab_size = 1 << 18;
  c->doc_concentration = nullptr;
  c->doc_concentration_len = 0;
  c->topic_concentration = -1.0;
  c->tau0 = 1024.0;
  c->kappa = 0.51;
  c->mini_batch_fraction = 0.05;
  c->gamma_shape = 100.0;
  c->optimize_doc_concentration = 1;
  c->sample_with_replacement = 1;
  c->seed = 0;
  c->dtype = STC_F64;  // Spark computes the E-step in Double
  c->max_inner_iter = 0;
}

int stc_lda_create(stc_ctx* ctx, const stc_lda_config* cfg, stc_lda** out) {
  return guard([&] {
    STC_REQUIRE(ctx && cfg && out, "ctx/cfg/out");
    // [U] LDA / OnlineLDAOptimizer setter validation
    STC_REQUIRE(cfg->k > 1, "LDA k (number of clusters) must be > 1");
    STC_REQUIRE(cfg->k <= 4096, "k <= 4096");
    STC_REQUIRE(cfg->vocab_size > 0 && cfg->vocab_size <= (int64_t(1) << 31), "vocab_size in (0, 2^31]");
    STC_REQUIRE(cfg->tau0 > 0, "LDA tau0 must be positive");
    STC_REQUIRE(cfg->kappa > 0, "LDA kappa must be positive");
    STC_REQUIRE(cfg->mini_batch_fraction > 0.0 && cfg->mini_batch_fraction <= 1.0,
                "miniBatchFraction must be in range (0,1]");
    STC_REQUIRE(cfg->gamma_shape > 1.0 / 3.0, "gammaShape must be > 1/3");
    STC_REQUIRE(cfg->dtype == STC_F32 || cfg->dtype == STC_F64 || cfg->dtype == STC_MIXED, "dtype");
    STC_REQUIRE(cfg->mixed_resolve_iters >= 0, "mixed_resolve_iters must be >= 0");
    STC_REQUIRE(cfg->max_inner_iter >= 0, "max_inner_iter must be >= 0");
    ctx->use();
    auto L = std::make_unique<stc_lda>();
    L->ctx = ctx;
    L->cfg = *cfg;
    if (L->cfg.max_inner_iter == 0) L->cfg.max_inner_iter = 100000;
    L->k = cfg->k;
    L->V = cfg->vocab_size;
    // STC_MIXED: the fp32 pipeline (dtype STC_F32 inside the library) plus the fp64 re-solve (mixed_resolve)
    L->mixed = cfg->dtype == STC_MIXED;
    L->dtype = L->mixed ? STC_F32 : cfg->dtype;
    L->mix.mixed_thr = cfg->mixed_resolve_iters > 0 ? cfg->mixed_resolve_iters : 500;
    const int W = L->dtype == STC_F32 ? 4 : 2;
    L->kp = (int)ceil_div(L->k, W) * W;
    L->P = ((L->kp / W) % 2 == 1) ? L->kp : L->kp + W;  // P/W odd: conflict-free b128 rows
    L->lds_rows = by_arith_type(*L, [&](auto t) { return lda::estep_lds_rows<decltype(t)>(L->k, L->kp, L->P); });
    if (L->mixed) {  // the fp64 workgroup kernel's shape at the fp32 row pitch, and the fp64 fast-kernel capacity
      L->mix.P64 = ((L->kp / 2) % 2 == 1) ? L->kp : L->kp + 2;
      L->mix.lds_rows64 = lda::estep_lds_rows<double>(L->k, L->kp, L->mix.P64);
      const int c64 = fast_row_cap<double>(L->k);
      L->mix.cap64 = c64 > 0 ? c64 : -1;
    }
    // docs with nnz <= wave_cap run the register-resident kernel (fp32: lda_grid.hip, fp64:
    // lda_rows64.hip), the rest the workgroup kernel (lda.hip); −1: no slot is "short" (not even empty)
    const int cap = by_arith_type(*L, [&](auto t) { return fast_row_cap<decltype(t)>(L->k); });
    L->wave_cap = (!env_flag("STC_DISABLE_WAVE", false) && cap > 0) ? cap : -1;
    // α / η resolution ([U] OnlineLDAOptimizer.initialize)
    std::vector<double> alpha((size_t)L->k);
    const int alen = cfg->doc_concentration ? cfg->doc_concentration_len : 0;
    if (alen == 0 || (alen == 1 && cfg->doc_concentration[0] == -1.0)) {
      std::fill(alpha.begin(), alpha.end(), 1.0 / L->k);
    } else if (alen == 1) {
      STC_REQUIRE(cfg->doc_concentration[0] >= 0, "docConcentration must be >= 0");
      std::fill(alpha.begin(), alpha.end(), cfg->doc_concentration[0]);
    } else {
      STC_REQUIRE(alen == L->k, "docConcentration must have length 1 or k");
      for (int t = 0; t < L->k; ++t) {
        STC_REQUIRE(cfg->doc_concentration[t] >= 0, "docConcentration entries must be >= 0");
        alpha[(size_t)t] = cfg->doc_concentration[t];
      }
    }
    if (cfg->topic_concentration == -1.0) L->eta = 1.0 / L->k;
    else {
      STC_REQUIRE(cfg->topic_concentration >= 0, "topicConcentration must be >= 0");
      L->eta = cfg->topic_concentration;
    }
    L->cfg.doc_concentration = nullptr;
    L->cfg.doc_concentration_len = 0;
    L->model.nblocks_m = ceil_div(L->V, lda::kRowsPerBlock);
    L->model.virt = env_int("STC_VIRTUAL_SHARDS", 1, 1, 64);
    L->sw.hot_order = env_flag("STC_HOT_ORDER", true);
    L->sw.sort_docs = env_flag("STC_SORT_DOCS", true);
    L->sw.presort = env_int("STC_PRESORT", 1, 0, 1) != 0;
    L->sw.team_force = env_int("STC_WIDE_TEAM", 0, 0, 8);
    L->sw.tgrid = env_flag("STC_TGRID", true);
    L->sw.tgrid_require = env_first("STC_TGRID") == '2';
    L->tail.force_coll = env_flag("STC_COLLECTIVE_MSTEP", false);
    L->tail.rs_chunks = env_int("STC_RS_CHUNKS", 4, 1, 16);
    ensure_layout(*L);  // λ, Bp, stat, logscale, colpart for the current shard count
    L->model.colsum.reserve(8 * L->k);
    L->model.psic.reserve(16 * L->k);  // ψ(colsum), exp(−ψ(colsum))
    L->model.alpha.reserve(8 * L->k);
    L->mb.small.reserve(8 * (L->k + 1));
    L->mb.stats4.reserve(8 * 4);
    L->mb.cum2.reserve(8 * 2);
    HIP_CHECK(hipMemsetAsync(L->mb.cum2.p, 0, 16, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(L->model.alpha.p, alpha.data(), 8 * L->k, hipMemcpyHostToDevice, ctx->stream));
    wait_stream(*ctx, ctx->stream);
    for (auto& s : L->own.ev)
      for (auto& e : s) HIP_CHECK(hipEventCreate(&e.e));
    *out = L.release();
  });
}

int stc_lda_destroy(stc_lda* lda) {
  return guard([&] {
    if (!lda) return;
    (void)hipSetDevice(lda->ctx->device);
    // queued work first (with a communicator: a bounded wait; a collective that never completes is
    // aborted with its communicator, which releases its kernels, so the destroy returns)
    Ctx& c = *lda->ctx;
    for (hipStream_t q : {c.stream, lda->own.side.s, lda->own.cstream.s}) {
      if (!q) continue;
      try {
        wait_stream(c, q);
      } catch (const Error&) {
        abort_comm(c);
      }
      (void)hipStreamSynchronize(q);
    }
    delete lda;
  });
}

int stc_lda_set_corpus(stc_lda* L, const stc_dcsr* corpus, int64_t corpus_size_total) {
  return guard([&] {
    STC_REQUIRE(L && corpus, "lda/corpus");
    STC_REQUIRE(corpus->ctx == L->ctx, "the corpus belongs to another stc_ctx than the LDA handle");
    STC_REQUIRE(corpus->cols == L->V, "corpus must have vocab_size columns");
    STC_REQUIRE(corpus->dtype == corpus_dtype(*L), "corpus value dtype must match the LDA dtype (STC_F64 for STC_MIXED)");
    STC_REQUIRE(corpus->rows < (int64_t(1) << 31), "at most 2^31-1 documents per rank");
    STC_REQUIRE(corpus_size_total >= corpus->rows && corpus_size_total > 0,
                "corpus_size_total must be >= this rank's rows and > 0");
    settle_side(*L);  // a draw still being sampled reads the previous corpus
    if (L->mixed) {  // the fp32 copy of the values the fp32 E-step reads
      L->ctx->use();
      L->mix.vals32.reserve(4 * std::max<int64_t>(corpus->nnz, 1));
      lda::launch_to_f32(L->ctx->stream, corpus->values.as<double>(), L->mix.vals32.as<float>(), corpus->nnz);
      wait_stream(*L->ctx, L->ctx->stream);
    }
    L->corpus = corpus;
    L->corpus_total = corpus_size_total;
    L->draw.pre_valid = false;  // a prefetched draw sampled the previous corpus
    L->mb.order_for = nullptr;
  });
}

int stc_lda_init_random(stc_lda* L, uint64_t seed) {
  return guard([&] {
    STC_REQUIRE(L, "lda");
    L->ctx->use();
    lda::launch_init_lambda(L->ctx->stream, L->model.lam.as<double>(), L->V, L->k, seed, L->cfg.gamma_shape);
    L->model.lam_stale = false;
    refresh(*L);
    L->iteration = 0;
    L->draw.draws = 0;  // a fresh generator, as Spark's initialize()
    L->draw.pre_valid = false;
    wait_stream(*L->ctx, L->ctx->stream);
  });
}

int stc_lda_set_topics(stc_lda* L, const double* topics, int layout) {
  return guard([&] {
    STC_REQUIRE(L && topics, "lda/topics");
    STC_REQUIRE(layout == STC_LAYOUT_VK || layout == STC_LAYOUT_KV, "layout");
    L->ctx->use();
    const int64_t n = L->V * L->k;
    std::vector<double> h((size_t)n);
    for (int64_t v = 0; v < L->V; ++v)
      for (int t = 0; t < L->k; ++t) {
        const double x = layout == STC_LAYOUT_VK ? topics[v * L->k + t] : topics[(int64_t)t * L->V + v];
        STC_REQUIRE(x > 0.0 && std::isfinite(x), "topics entries must be finite and > 0");
        h[(size_t)(v * L->k + t)] = x;
      }
    HIP_CHECK(hipMemcpyAsync(L->model.lam.p, h.data(), 8 * n, hipMemcpyHostToDevice, L->ctx->stream));
    L->model.lam_stale = false;
    refresh(*L);
    wait_stream(*L->ctx, L->ctx->stream);
  });
}

int stc_lda_get_topics(stc_lda* L, double* out, int layout) {
  return guard([&] {
    STC_REQUIRE(L && out, "lda/out");
    STC_REQUIRE(layout == STC_LAYOUT_VK || layout == STC_LAYOUT_KV, "layout");
    STC_REQUIRE(L->model.has_topics, "no topics yet");
    L->ctx->use();
    gather_lambda(*L);
    const int64_t n = L->V * L->k;
    if (layout == STC_LAYOUT_VK) {
      HIP_CHECK(hipMemcpyAsync(out, L->model.lam.p, 8 * n, hipMemcpyDeviceToHost, L->ctx->stream));
      wait_stream(*L->ctx, L->ctx->stream);
    } else {
      std::vector<double> h((size_t)n);
      HIP_CHECK(hipMemcpyAsync(h.data(), L->model.lam.p, 8 * n, hipMemcpyDeviceToHost, L->ctx->stream));
      wait_stream(*L->ctx, L->ctx->stream);
      for (int64_t v = 0; v < L->V; ++v)
        for (int t = 0; t < L->k; ++t) out[(int64_t)t * L->V + v] = h[(size_t)(v * L->k + t)];
    }
  });
}

int stc_lda_set_alpha(stc_lda* L, const double* alpha) {
  return guard([&] {
    STC_REQUIRE(L && alpha, "lda/alpha");
    for (int t = 0; t < L->k; ++t) STC_REQUIRE(alpha[t] >= 0, "alpha entries must be >= 0");
    L->ctx->use();
    HIP_CHECK(hipMemcpyAsync(L->model.alpha.p, alpha, 8 * L->k, hipMemcpyHostToDevice, L->ctx->stream));
    wait_stream(*L->ctx, L->ctx->stream);
  });
}

int stc_lda_get_alpha(stc_lda* L, double* alpha_out) {
  return guard([&] {
    STC_REQUIRE(L && alpha_out, "lda/alpha_out");
    L->ctx->use();
    HIP_CHECK(hipMemcpyAsync(alpha_out, L->model.alpha.p, 8 * L->k, hipMemcpyDeviceToHost, L->ctx->stream));
    wait_stream(*L->ctx, L->ctx->stream);
  });
}

int stc_lda_get_eta(stc_lda* L, double* eta_out) {
  return guard([&] {
    STC_REQUIRE(L && eta_out, "lda/eta_out");
    *eta_out = L->eta;
  });
}

int stc_lda_shape(const stc_lda* L, int32_t* k_out, int64_t* vocab_out) {
  return guard([&] {
    STC_REQUIRE(L, "lda");
    if (k_out) *k_out = L->k;
    if (vocab_out) *vocab_out = L->V;
  });
}

int stc_lda_get_iteration(stc_lda* L, int64_t* it) {
  return guard([&] {
    STC_REQUIRE(L && it, "lda/it");
    *it = L->iteration;
  });
}

int stc_lda_step(stc_lda* L, const int64_t* ids, int64_t n, const double* gamma0, stc_step_stats* st) {
  return guard([&] {
    STC_REQUIRE(L && (ids || n == 0) && n >= 0, "lda/ids");
    L->ctx->use();
    by_arith_type(*L, [&](auto t) { step_ids<decltype(t)>(*L, ids, n, gamma0, st); });
  });
}

int stc_lda_next(stc_lda* L, stc_step_stats* st) {
  return guard([&] {
    STC_REQUIRE(L, "lda");
    L->ctx->use();
    by_arith_type(*L, [&](auto t) { next_impl<decltype(t)>(*L, st); });
  });
}

int stc_lda_estep(stc_lda* L, const int64_t* ids, int64_t n, const double* gamma0, double* gamma_out,
                  double* stat_out, int32_t* iters_out) {
  return guard([&] {
    STC_REQUIRE(L && (ids || n == 0) && n >= 0, "lda/ids");
    L->ctx->use();
    by_arith_type(*L, [&](auto t) { estep_only<decltype(t)>(*L, ids, n, gamma0, gamma_out, stat_out, iters_out); });
  });
}

int stc_lda_bound(stc_lda* L, const stc_dcsr* docs, uint64_t gamma_seed, int64_t doc_id_base,
                  const double* gamma0, double* bound_out, double* corpus_part_out,
                  double* topics_part_out, double* token_count_out) {
  return guard([&] {
    STC_REQUIRE(L && docs, "lda/docs");
    STC_REQUIRE(docs->ctx == L->ctx, "the documents belong to another stc_ctx than the LDA handle");
    L->ctx->use();
    double h[3] = {0, 0, 0};
    double norm = 0;
    const bool sharded = L->model.lam_stale;
    by_infer_type(*L, [&](auto t) {
      infer_impl<decltype(t)>(*L, *docs, gamma_seed, doc_id_base, gamma0, true, nullptr, h);
    });
    topics_part(*L, h + 2, &norm);
    // corpusPart and the token count are sums over the ranks' documents; the topics part's element
    // sum too when λ is sharded (each rank holds its slice), else it is already complete everywhere
    allreduce_host(*L->ctx, h, sharded ? 3 : 2);
    const double tp = h[2] + norm;
    if (bound_out) *bound_out = h[0] + tp;
    if (corpus_part_out) *corpus_part_out = h[0];
    if (topics_part_out) *topics_part_out = tp;
    if (token_count_out) *token_count_out = h[1];
  });
}

int stc_lda_topic_distribution(stc_lda* L, const stc_dcsr* docs, uint64_t gamma_seed,
                               int64_t doc_id_base, const double* gamma0, double* out) {
  return guard([&] {
    STC_REQUIRE(L && docs && (out || docs->rows == 0), "lda/docs/out");
    STC_REQUIRE(docs->ctx == L->ctx, "the documents belong to another stc_ctx than the LDA handle");
    L->ctx->use();
    by_infer_type(*L, [&](auto t) {
      infer_impl<decltype(t)>(*L, *docs, gamma_seed, doc_id_base, gamma0, false, out, nullptr);
    });
    for (int64_t i = 0; i < docs->rows; ++i) {  // normalize(gamma, 1.0); zeros for empty docs
      double* g = out + i * L->k;
      double sum = 0.0;
      for (int t = 0; t < L->k; ++t) sum += std::fabs(g[t]);
      if (sum > 0.0)
        for (int t = 0; t < L->k; ++t) g[t] /= sum;
    }
  });
}

int stc_lda_describe(stc_lda* L, int32_t max_terms, int32_t* idx_out, double* weight_out) {
  return guard([&] {
    STC_REQUIRE(L && idx_out && weight_out, "lda/idx_out/weight_out");
    STC_REQUIRE(max_terms > 0, "maxTermsPerTopic must be > 0");
    STC_REQUIRE(L->model.has_topics, "no topics yet");
    // the API's documented limit by now, no kernel's: the selection takes any V < 2^31 with int64 offsets
    STC_REQUIRE(L->V * L->k < (int64_t(1) << 31), "describe: V*k must be < 2^31");
    L->ctx->use();
    gather_lambda(*L);
    // per topic the N heaviest λ[w][t], ties by ascending term (Scala's stable sortBy(-w)); the weight is
    // normalize(topic, 1.0): λ[w][t] / colsum[t] (λ > 0)
    rank::Scratch sc;
    rank::describe_columns(*L->ctx, sc, L->model.lam.p, false, L->V, L->k, std::min<int64_t>(max_terms, L->V),
                           L->model.colsum.as<double>(), idx_out, weight_out);
  });
}

int stc_lda_enable_timing(stc_lda* L, int on) {
  return guard([&] {
    STC_REQUIRE(L, "lda");
    L->tm.timing = on != 0;
    for (double& a : L->tm.acc_ms) a = 0.0;
    L->tm.timed_steps = 0;
    L->tm.ev_pending[0] = L->tm.ev_pending[1] = L->tm.ev_pending[2] = false;
  });
}

int stc_lda_kernel_counts(stc_lda* L, int64_t out[STC_KC_N]) {
  return guard([&] {
    STC_REQUIRE(L && out, "lda/out");
    std::copy(L->tm.kcount, L->tm.kcount + STC_KC_N, out);
  });
}

int stc_lda_phase_times(stc_lda* L, double* ms_out, int64_t* steps_out) {
  return guard([&] {
    STC_REQUIRE(L && ms_out, "lda/ms_out");
    L->ctx->use();
    wait_stream(*L->ctx, L->ctx->stream);
    harvest_all(*L);
    for (int p = 0; p < 5; ++p) ms_out[p] = L->tm.timed_steps ? L->tm.acc_ms[p] / (double)L->tm.timed_steps : 0.0;
    if (steps_out) *steps_out = L->tm.timed_steps;
  });
}

int stc_lda_counters(stc_lda* L, int64_t out[4]) {
  return guard([&] {
    STC_REQUIRE(L && out, "lda/out");
    L->ctx->use();
    int64_t c2[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(c2, L->mb.cum2.p, 16, hipMemcpyDeviceToHost, L->ctx->stream));
    wait_stream(*L->ctx, L->ctx->stream);
    out[0] = L->tm.cum_docs;
    out[1] = L->tm.cum_entries;
    out[2] = c2[0];
    out[3] = c2[1];
  });
}

}  // extern "C"
