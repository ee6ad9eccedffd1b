// group.hip — stc_group: one process driving N devices (stc_init(device_ids, n)).  The JVM runs the
// reference in ONE process (Spark local[*], LDATraining.scala:7), so its drop-in needs the N GPUs of the node behind
// one handle: N contexts joined by one communicator (ncclCommInitAll over distinct devices; the in-process transport
// of collectives.h when every member shares one device), N LDA handles over contiguous document shards (balanced by
// entries), each call run on one host thread per member.  Built on the public ABI, collectives.h and the member
// accessors of lda_online.h.
#include <cstdlib>

#include "group_common.h"
#include "lda_online.h"

using namespace stc;

struct stc_group : GroupBase {
  std::vector<stc_lda*> lda;
  std::vector<stc_dcsr*> shard;
  std::vector<int64_t> row0;  // first corpus row of each member's shard (n + 1 entries)
  int64_t rows = 0, cols = 0, k = 0;  // the corpus's shape; the members' topic count
  int dtype = STC_F64;
};

extern "C" {

int stc_group_create(const int* device_ids, int n_devices, const stc_lda_config* cfg, stc_group** out) {
  return guard([&] {
    STC_REQUIRE(device_ids && cfg && out, "device_ids/cfg/out");
    auto g = std::make_unique<stc_group>();
    struct Cleanup {
      stc_group* g;
      ~Cleanup() {
        if (!g) return;
        for (auto* l : g->lda) (void)stc_lda_destroy(l);
        for (auto* c : g->ctx) (void)stc_destroy(c);
      }
    } cleanup{g.get()};
    // STC_GROUP_RCCL=1 (group_common.h) also runs the collective (vocabulary-sliced) M-step with one member
    const bool rccl1 = open_members(*g, device_ids, n_devices);
    // test knob STC_GROUP_STEP_FAULT=i[:s]: member i's s-th step (default the first) fails, after its E-step
    // and sstats and before its reduce-scatter (its peers' collectives then never complete: the RCCL
    // failure path)
    const char* sf = getenv("STC_GROUP_STEP_FAULT");
    const int step_fault = sf && sf[0] ? atoi(sf) : -1;
    const char* sfc = sf ? std::strchr(sf, ':') : nullptr;
    const int step_fault_at = sfc ? std::max(1, atoi(sfc + 1)) : 1;
    for (int i = 0; i < n_devices; ++i) {
      stc_lda* l = nullptr;
      member_ok(stc_lda_create(g->ctx[(size_t)i], cfg, &l));
      // rccl1: the sliced M-step and its collectives on a 1-rank communicator too
      set_group_knobs(*l, rccl1, i == step_fault ? step_fault_at : 0);
      g->lda.push_back(l);
    }
    g->dtype = corpus_dtype(*g->lda[0]);  // the shards' value dtype
    g->k = cfg->k;
    g->row0.assign((size_t)n_devices + 1, 0);
    cleanup.g = nullptr;
    *out = g.release();
  });
}

int stc_group_destroy(stc_group* g) {
  return guard([&] {
    if (!g) return;
    for (auto* l : g->lda) (void)stc_lda_destroy(l);
    for (auto* d : g->shard) (void)stc_dcsr_free(d);
    close_members(*g);
    delete g;
  });
}

int stc_group_size(const stc_group* g, int* n_out) {
  return guard([&] {
    STC_REQUIRE(g && n_out, "group/n_out");
    *n_out = g->n();
  });
}

int stc_group_transport(const stc_group* g, int* transport_out) {
  return guard([&] {
    STC_REQUIRE(g && transport_out, "group/transport_out");
    *transport_out = g->transport;
  });
}

int stc_group_member(stc_group* g, int i, stc_lda** lda_out) {
  return guard([&] {
    STC_REQUIRE(g && lda_out && i >= 0 && i < g->n(), "group/member index");
    *lda_out = g->lda[(size_t)i];
  });
}

int stc_group_set_corpus(stc_group* g, int64_t n_rows, int64_t n_cols, const int64_t* indptr, const int32_t* indices,
                         const double* values) {
  return guard([&] {
    STC_REQUIRE(g, "group");
    check_host_csr(n_rows, n_cols, indptr, indices, values);
    const std::vector<int64_t> r0 = shard_rows(indptr, n_rows, g->n());
    std::vector<stc_dcsr*> shard((size_t)g->n(), nullptr);
    try {
      // every shard uploaded before any member is switched to it: a failed upload (out of memory) leaves
      // every member on its previous shard
      const char* fe = getenv("STC_GROUP_UPLOAD_FAULT");  // debug knob: member i's upload fails (tests)
      const int fault = fe ? atoi(fe) : -1;
      for_members(*g, [&](int i) {
        if (i == fault) throw Error(STC_ERR_OOM, "injected shard upload failure (STC_GROUP_UPLOAD_FAULT)");
        shard[(size_t)i] = upload_rows(g->ctx[(size_t)i], r0[(size_t)i], r0[(size_t)i + 1], n_cols, indptr, indices,
                                       values, g->dtype);
      });
      for_members(*g, [&](int i) { member_ok(stc_lda_set_corpus(g->lda[(size_t)i], shard[(size_t)i], n_rows)); });
    } catch (...) {
      // members already switched go back to their previous shard (or to none) before the new ones are freed
      for (int i = 0; i < g->n(); ++i) {
        stc_lda* l = g->lda[(size_t)i];
        if (!shard[(size_t)i] || corpus(*l) != shard[(size_t)i]) continue;
        stc_dcsr* old = (size_t)i < g->shard.size() ? g->shard[(size_t)i] : nullptr;
        if (!old || stc_lda_set_corpus(l, old, g->rows) != STC_OK) forget_corpus(*l);
      }
      for (auto* d : shard) (void)stc_dcsr_free(d);
      throw;
    }
    for (auto* d : g->shard) (void)stc_dcsr_free(d);
    g->shard = shard;
    g->row0 = r0;
    g->rows = n_rows;
    g->cols = n_cols;
  });
}

int stc_group_release_corpus(stc_group* g) {
  return guard([&] {
    STC_REQUIRE(g, "group");
    require_usable(*g);
    for (int i = 0; i < g->n(); ++i) {
      stc_lda* l = g->lda[(size_t)i];
      g->ctx[(size_t)i]->use();
      settle_side(*l);
      wait_stream(*g->ctx[(size_t)i], g->ctx[(size_t)i]->stream);
      forget_corpus(*l);
    }
    for (auto* d : g->shard) (void)stc_dcsr_free(d);
    g->shard.clear();
    g->rows = 0;
  });
}

int stc_group_init_random(stc_group* g, uint64_t seed) {
  return guard([&] {
    STC_REQUIRE(g, "group");
    for_members(*g, [&](int i) { member_ok(stc_lda_init_random(g->lda[(size_t)i], seed)); });
  });
}

int stc_group_set_topics(stc_group* g, const double* topics, int layout) {
  return guard([&] {
    STC_REQUIRE(g && topics, "group/topics");
    for_members(*g, [&](int i) { member_ok(stc_lda_set_topics(g->lda[(size_t)i], topics, layout)); });
  });
}

int stc_group_get_topics(stc_group* g, double* topics_out, int layout) {
  return guard([&] {
    STC_REQUIRE(g && topics_out, "group/topics_out");
    // gathering the sharded λ is collective: member 0 copies it out, the others only take part
    for_members(*g, [&](int i) {
      if (i == 0) member_ok(stc_lda_get_topics(g->lda[0], topics_out, layout));
      else gather_lambda(*g->lda[(size_t)i]);
    });
  });
}

int stc_group_get_alpha(stc_group* g, double* alpha_out) {
  return guard([&] {
    STC_REQUIRE(g && alpha_out, "group/alpha_out");
    require_usable(*g);
    g->ctx[0]->use();
    member_ok(stc_lda_get_alpha(g->lda[0], alpha_out));  // α is replicated on every member
  });
}

int stc_group_get_iteration(stc_group* g, int64_t* iteration_out) {
  return guard([&] {
    STC_REQUIRE(g && iteration_out, "group/iteration_out");
    member_ok(stc_lda_get_iteration(g->lda[0], iteration_out));
  });
}

int stc_group_synchronize(stc_group* g) {
  return guard([&] {
    STC_REQUIRE(g, "group");
    require_usable(*g);
    for (int i = 0; i < g->n(); ++i) {
      g->ctx[(size_t)i]->use();
      wait_stream(*g->ctx[(size_t)i], g->ctx[(size_t)i]->stream);
      if (hipStream_t side = side_stream(*g->lda[(size_t)i])) wait_stream(*g->ctx[(size_t)i], side);  // the next draw
    }
  });
}

static void merge_stats(stc_step_stats* out, const std::vector<stc_step_stats>& st) {
  if (!out) return;
  *out = stc_step_stats{};
  for (const auto& s : st) {
    out->batch_docs += s.batch_docs;
    out->batch_entries += s.batch_entries;
    out->inner_iters += s.inner_iters;
    out->inner_iters_max = std::max(out->inner_iters_max, s.inner_iters_max);
    out->cap_hits += s.cap_hits;
  }
  out->nonempty_docs = st[0].nonempty_docs;  // already summed over the members
  out->rho = st[0].rho;
}

int stc_group_next(stc_group* g, stc_step_stats* stats) {
  return guard([&] {
    STC_REQUIRE(g, "group");
    std::vector<stc_step_stats> st((size_t)g->n());
    for_members(*g, [&](int i) { member_ok(stc_lda_next(g->lda[(size_t)i], stats ? &st[(size_t)i] : nullptr)); });
    merge_stats(stats, st);
  });
}

int stc_group_step(stc_group* g, const int64_t* batch_doc_ids, int64_t n, const double* gamma0, stc_step_stats* stats) {
  return guard([&] {
    STC_REQUIRE(g && (batch_doc_ids || n == 0) && n >= 0, "group/batch_doc_ids");
    const int m = g->n();
    const int64_t k = g->k;
    std::vector<std::vector<int64_t>> ids((size_t)m);
    std::vector<std::vector<double>> g0((size_t)m);
    for (int64_t j = 0; j < n; ++j) {
      const int64_t d = batch_doc_ids[j];
      STC_REQUIRE(d >= 0 && d < g->rows, "batch doc id out of range");
      const int q = (int)(std::upper_bound(g->row0.begin(), g->row0.end(), d) - g->row0.begin()) - 1;
      ids[(size_t)q].push_back(d - g->row0[(size_t)q]);
      if (gamma0) g0[(size_t)q].insert(g0[(size_t)q].end(), gamma0 + j * k, gamma0 + (j + 1) * k);
    }
    std::vector<stc_step_stats> st((size_t)m);
    for_members(*g, [&](int i) {
      const auto& v = ids[(size_t)i];
      member_ok(stc_lda_step(g->lda[(size_t)i], v.data(), (int64_t)v.size(), gamma0 ? g0[(size_t)i].data() : nullptr,
                             stats ? &st[(size_t)i] : nullptr));
    });
    merge_stats(stats, st);
  });
}

int stc_group_describe(stc_group* g, int32_t max_terms, int32_t* idx_out, double* weight_out) {
  return guard([&] {
    STC_REQUIRE(g && idx_out && weight_out, "group/idx_out/weight_out");
    for_members(*g, [&](int i) {
      if (i == 0) member_ok(stc_lda_describe(g->lda[0], max_terms, idx_out, weight_out));
      else gather_lambda(*g->lda[(size_t)i]);
    });
  });
}

int stc_group_bound(stc_group* g, int64_t n_rows, int64_t n_cols, const int64_t* indptr, const int32_t* indices,
                    const double* values, uint64_t gamma_seed, int64_t doc_id_base, const double* gamma0,
                    double* bound_out, double* corpus_part_out, double* topics_part_out, double* token_count_out) {
  return guard([&] {
    STC_REQUIRE(g && bound_out, "group/bound_out");
    check_host_csr(n_rows, n_cols, indptr, indices, values);
    const std::vector<int64_t> r0 = shard_rows(indptr, n_rows, g->n());
    const int64_t k = g->k;
    double res[4] = {0, 0, 0, 0};
    for_members(*g, [&](int i) {
      const int64_t lo = r0[(size_t)i], hi = r0[(size_t)i + 1];
      stc_dcsr* d = upload_rows(g->ctx[(size_t)i], lo, hi, n_cols, indptr, indices, values, g->dtype);
      double r[4] = {0, 0, 0, 0};
      // every member's γ₀ keys continue the global row numbering (doc_id_base + row), so the bound is
      // the one a single handle computes over all rows
      const int rc = stc_lda_bound(g->lda[(size_t)i], d, gamma_seed, doc_id_base + lo, gamma0 ? gamma0 + lo * k : nullptr,
                                   &r[0], &r[1], &r[2], &r[3]);
      (void)stc_dcsr_free(d);
      member_ok(rc);
      if (i == 0) std::copy(r, r + 4, res);  // the bound is all-reduced: every member holds the total
    });
    *bound_out = res[0];
    if (corpus_part_out) *corpus_part_out = res[1];
    if (topics_part_out) *topics_part_out = res[2];
    if (token_count_out) *token_count_out = res[3];
  });
}

int stc_group_topic_distribution(stc_group* g, int64_t n_rows, int64_t n_cols, const int64_t* indptr,
                                 const int32_t* indices, const double* values, uint64_t gamma_seed,
                                 int64_t doc_id_base, const double* gamma0, double* out) {
  return guard([&] {
    STC_REQUIRE(g && out, "group/out");
    check_host_csr(n_rows, n_cols, indptr, indices, values);
    const std::vector<int64_t> r0 = shard_rows(indptr, n_rows, g->n());
    const int64_t k = g->k;
    for_members(*g, [&](int i) {
      const int64_t lo = r0[(size_t)i], hi = r0[(size_t)i + 1];
      stc_dcsr* d = upload_rows(g->ctx[(size_t)i], lo, hi, n_cols, indptr, indices, values, g->dtype);
      const int rc = stc_lda_topic_distribution(g->lda[(size_t)i], d, gamma_seed, doc_id_base + lo,
                                                gamma0 ? gamma0 + lo * k : nullptr, out + lo * k);
      (void)stc_dcsr_free(d);
      member_ok(rc);
    });
  });
}

}  // extern "C"
