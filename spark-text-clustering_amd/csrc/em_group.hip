// em_group.hip — stc_em_group: the EM optimizer over N devices from one process (include/stc.h).
//
// Documents are sharded as stc_group_set_corpus shards them (contiguous row ranges balanced by entries); member
// i owns one stc_em over its rows with all V columns (lda_em.h).  N_dk stays on the member, N_wk / N_k / inv
// are replicated: an iteration is the member's row pass, its column pass over its own edges and one all-reduce
// of N_wk'.  The scalars of logLikelihood / logPrior are added here in member order; topicAssignments are
// concatenated in member order, which is the global CSR order.  Contexts, communicator, member threads and the
// failure path are group_common.h's, shared with stc_group.
#include "group_common.h"
#include "lda_em.h"

using namespace stc;

struct stc_em_group : GroupBase {
  std::vector<stc_em*> em;
  std::vector<int64_t> row0;   // first corpus row of each member's shard (n + 1 entries)
  std::vector<int64_t> edge0;  // first edge (non-zero entry, CSR order) of each member's shard (n + 1 entries)
  int32_t k = 0;
  int64_t D = 0, V = 0;
  double alpha = 0.0, eta = 0.0;
  bool has_state = false;
};

namespace {

void require_state(const stc_em_group& g) {
  if (!g.has_state)
    throw Error(STC_ERR_STATE, "em group: no state yet (stc_em_group_init_random or stc_em_group_set_state first)");
}

void destroy(stc_em_group* g) {
  if (!g) return;
  for (auto* m : g->em) (void)stc_em_destroy(m);
  close_members(*g);
  delete g;
}

}  // namespace

extern "C" {

int stc_em_group_create_as(const int* device_ids, int n_devices, int64_t n_rows, int64_t n_cols, const int64_t* indptr,
                           const int32_t* indices, const double* values, int32_t k, double doc_concentration,
                           double topic_concentration, int state_dtype, stc_em_group** out) {
  return guard([&] {
    STC_REQUIRE(device_ids && out, "device_ids/out");
    // stc_em_create_as's checks, here so that every member passes or none starts
    STC_REQUIRE(state_dtype == STC_F64 || state_dtype == STC_F32, "em: the state dtype must be STC_F64 or STC_F32");
    STC_REQUIRE(k >= 2 && k <= 1024, "em: 2 <= k <= 1024");
    check_host_csr(n_rows, n_cols, indptr, indices, values);
    STC_REQUIRE(n_rows < (int64_t(1) << 31) - 1 && n_cols < (int64_t(1) << 31) - 1 && indptr[n_rows] < (int64_t(1) << 31) - 1,
                "em: rows, columns and entries below 2^31 - 1");
    STC_REQUIRE(doc_concentration == -1.0 || doc_concentration > 1.0,
                "em: docConcentration must be > 1.0 (or -1 for auto) for EM");
    STC_REQUIRE(topic_concentration == -1.0 || topic_concentration > 1.0,
                "em: topicConcentration must be > 1.0 (or -1 for auto) for EM");
    std::unique_ptr<stc_em_group, void (*)(stc_em_group*)> g(new stc_em_group, destroy);
    open_members(*g, device_ids, n_devices);
    const int n = g->n();
    g->row0 = shard_rows(indptr, n_rows, n);
    // explicit zeros are entries but not edges: a shard's first edge is the count of non-zeros before it
    g->edge0.assign((size_t)n + 1, 0);
    for (int i = 0; i < n; ++i) {
      int64_t e = 0;
      for (int64_t p = indptr[g->row0[(size_t)i]]; p < indptr[g->row0[(size_t)i + 1]]; ++p) e += values[p] != 0.0;
      g->edge0[(size_t)i + 1] = g->edge0[(size_t)i] + e;
    }
    g->em.assign((size_t)n, nullptr);
    for_members(*g, [&](int i) {
      stc_ctx* c = g->ctx[(size_t)i];
      stc_dcsr* d = upload_rows(c, g->row0[(size_t)i], g->row0[(size_t)i + 1], n_cols, indptr, indices, values, STC_F64);
      struct Free {
        stc_dcsr* d;
        ~Free() { (void)stc_dcsr_free(d); }
      } free_shard{d};  // the member copies what it needs
      g->em[(size_t)i] =
          em::member_create(*c, *d, k, doc_concentration, topic_concentration, state_dtype, g->edge0[(size_t)i]);
    });
    g->k = k;
    g->D = n_rows;
    g->V = n_cols;
    member_ok(stc_em_get_state(g->em[0], nullptr, nullptr, nullptr, &g->alpha, &g->eta));
    *out = g.release();
  });
}

int stc_em_group_create(const int* device_ids, int n_devices, int64_t n_rows, int64_t n_cols, const int64_t* indptr,
                        const int32_t* indices, const double* values, int32_t k, double doc_concentration,
                        double topic_concentration, stc_em_group** out) {
  return stc_em_group_create_as(device_ids, n_devices, n_rows, n_cols, indptr, indices, values, k, doc_concentration,
                                topic_concentration, STC_F64, out);
}

int stc_em_group_destroy(stc_em_group* g) {
  return guard([&] { destroy(g); });
}

int stc_em_group_size(const stc_em_group* g, int* n_out) {
  return guard([&] {
    STC_REQUIRE(g && n_out, "em group/n_out");
    *n_out = g->n();
  });
}

int stc_em_group_transport(const stc_em_group* g, int* transport_out) {
  return guard([&] {
    STC_REQUIRE(g && transport_out, "em group/transport_out");
    *transport_out = g->transport;
  });
}

int stc_em_group_shape(const stc_em_group* g, int32_t* k, int64_t* n_docs, int64_t* vocab, int64_t* n_edges) {
  return guard([&] {
    STC_REQUIRE(g, "em group");
    if (k) *k = g->k;
    if (n_docs) *n_docs = g->D;
    if (vocab) *vocab = g->V;
    if (n_edges) *n_edges = g->edge0.back();
  });
}

int stc_em_group_member(stc_em_group* g, int i, stc_em** em_out, int64_t* row0_out) {
  return guard([&] {
    STC_REQUIRE(g && em_out && i >= 0 && i < g->n(), "em group/member index");
    *em_out = g->em[(size_t)i];
    if (row0_out) *row0_out = g->row0[(size_t)i];
  });
}

int stc_em_group_init_random(stc_em_group* g, uint64_t seed) {
  return guard([&] {
    STC_REQUIRE(g, "em group");
    for_members(*g, [&](int i) { em::member_init_random(*g->em[(size_t)i], seed); });
    g->has_state = true;
  });
}

int stc_em_group_set_state(stc_em_group* g, const double* doc_topics, const double* term_topics) {
  return guard([&] {
    STC_REQUIRE(g, "em group");
    STC_REQUIRE((doc_topics || g->D == 0) && term_topics, "em: doc_topics / term_topics");
    const int64_t kk = g->k, nd = g->D * kk, nw = g->V * kk;
    for (int64_t i = 0; i < nd; ++i) STC_REQUIRE(doc_topics[i] >= 0.0, "em: doc_topics must be non-negative");
    for (int64_t i = 0; i < nw; ++i) STC_REQUIRE(term_topics[i] >= 0.0, "em: term_topics must be non-negative");
    for_members(*g, [&](int i) {
      em::member_set_state(*g->em[(size_t)i], doc_topics ? doc_topics + g->row0[(size_t)i] * kk : nullptr, term_topics);
    });
    g->has_state = true;
  });
}

int stc_em_group_get_state(stc_em_group* g, double* doc_topics, double* term_topics, double* totals, double* alpha_out,
                           double* eta_out) {
  return guard([&] {
    STC_REQUIRE(g, "em group");
    if (alpha_out) *alpha_out = g->alpha;
    if (eta_out) *eta_out = g->eta;
    if (!doc_topics && !term_topics && !totals) return;
    require_usable(*g);
    require_state(*g);
    // copies only, no collective: N_wk and N_k are the same on every member, member 0's are returned
    for (int i = 0; i < g->n(); ++i) {
      g->ctx[(size_t)i]->use();
      double* dt = doc_topics ? doc_topics + g->row0[(size_t)i] * g->k : nullptr;
      member_ok(stc_em_get_state(g->em[(size_t)i], dt, i == 0 ? term_topics : nullptr, i == 0 ? totals : nullptr,
                                 nullptr, nullptr));
    }
  });
}

int stc_em_group_next(stc_em_group* g, int32_t n_iterations) {
  return guard([&] {
    STC_REQUIRE(g, "em group");
    STC_REQUIRE(n_iterations >= 0, "em: n_iterations >= 0");
    require_usable(*g);
    require_state(*g);
    for_members(*g, [&](int i) { em::member_next(*g->em[(size_t)i], n_iterations); });
  });
}

int stc_em_group_synchronize(stc_em_group* g) {
  return guard([&] {
    STC_REQUIRE(g, "em group");
    require_usable(*g);
    for (auto* m : g->em) em::member_wait(*m);
  });
}

int stc_em_group_log_likelihood(stc_em_group* g, double* log_likelihood_out, double* log_prior_out) {
  return guard([&] {
    STC_REQUIRE(g, "em group");
    require_usable(*g);
    require_state(*g);
    const size_t n = (size_t)g->n();
    std::vector<double> ll(n, 0.0), tp(n, 0.0), dp(n, 0.0);
    for_members(*g, [&](int i) {
      em::member_log_likelihood(*g->em[(size_t)i], log_likelihood_out ? &ll[(size_t)i] : nullptr,
                                log_prior_out ? &tp[(size_t)i] : nullptr, log_prior_out ? &dp[(size_t)i] : nullptr);
    });
    // every edge and every document vertex lies on one member: their sums add up, in member order; the
    // term vertices are the same on every member: counted once
    double l = ll[0], d = dp[0];
    for (size_t i = 1; i < n; ++i) l += ll[i], d += dp[i];
    if (log_likelihood_out) *log_likelihood_out = l;
    if (log_prior_out) *log_prior_out = (g->eta - 1.0) * tp[0] + (g->alpha - 1.0) * d;
  });
}

int stc_em_group_topic_assignments(stc_em_group* g, int64_t* indptr_out, int32_t* terms_out, int32_t* topics_out) {
  return guard([&] {
    STC_REQUIRE(g, "em group");
    require_usable(*g);
    require_state(*g);
    std::vector<std::vector<int64_t>> ip((size_t)g->n());
    for_members(*g, [&](int i) {
      const int64_t r0 = g->row0[(size_t)i], rows = g->row0[(size_t)i + 1] - r0, e0 = g->edge0[(size_t)i];
      if (indptr_out) ip[(size_t)i].assign((size_t)rows + 1, 0);
      em::member_topic_assignments(*g->em[(size_t)i], indptr_out ? ip[(size_t)i].data() : nullptr,
                                   terms_out ? terms_out + e0 : nullptr, topics_out ? topics_out + e0 : nullptr);
      // the member's ranges start at 0: shift them behind the earlier members' edges
      if (indptr_out)
        for (int64_t r = 0; r < rows; ++r) indptr_out[r0 + r] = ip[(size_t)i][(size_t)r] + e0;
    });
    if (indptr_out) indptr_out[g->D] = g->edge0.back();
  });
}

// N_wk and N_k are replicated: member 0 answers
int stc_em_group_describe(stc_em_group* g, int32_t max_terms, int32_t* idx_out, double* weight_out) {
  return guard([&] {
    STC_REQUIRE(g, "em group");
    STC_REQUIRE(idx_out && weight_out, "em: idx_out / weight_out");
    STC_REQUIRE(max_terms > 0, "em: max_terms > 0");
    require_usable(*g);
    require_state(*g);
    g->ctx[0]->use();
    em::member_describe(*g->em[0], max_terms, idx_out, weight_out);
  });
}

// every member selects its shard's best rows per topic; the global best N lie in the union of the shards' best
// N, and a weight depends on its own row only: merged by (weight descending, row ascending) the answer is the
// single handle's
int stc_em_group_top_documents(stc_em_group* g, int64_t max_docs, int64_t* n_out, int64_t* row_out, double* weight_out) {
  return guard([&] {
    STC_REQUIRE(g, "em group");
    STC_REQUIRE(n_out && row_out && weight_out, "em: n_out / row_out / weight_out");
    STC_REQUIRE(max_docs > 0, "em: max_docs > 0");
    require_usable(*g);
    require_state(*g);
    const size_t n = (size_t)g->n();
    std::vector<std::vector<int64_t>> rows(n);
    std::vector<std::vector<double>> w(n);
    std::vector<int64_t> ni(n, 0);
    for_members(*g, [&](int i) {
      ni[(size_t)i] = em::member_top_documents(*g->em[(size_t)i], max_docs, g->row0[(size_t)i], rows[(size_t)i], w[(size_t)i]);
    });
    int64_t vertices = 0;
    for (size_t i = 0; i < n; ++i) vertices += ni[i];
    const int64_t N = std::min(max_docs, vertices), cap = std::min(max_docs, g->D);
    std::vector<std::pair<double, int64_t>> all;
    for (int t = 0; t < g->k; ++t) {
      all.clear();
      for (size_t i = 0; i < n; ++i)
        for (int64_t j = 0; j < ni[i]; ++j) all.emplace_back(w[i][(size_t)(t * ni[i] + j)], rows[i][(size_t)(t * ni[i] + j)]);
      std::sort(all.begin(), all.end(), [](const std::pair<double, int64_t>& a, const std::pair<double, int64_t>& b) {
        return a.first > b.first || (a.first == b.first && a.second < b.second);
      });
      for (int64_t j = 0; j < N; ++j) {
        row_out[t * cap + j] = all[(size_t)j].second;
        weight_out[t * cap + j] = all[(size_t)j].first;
      }
    }
    *n_out = N;
  });
}

// every member ranks its own rows; concatenated in row order
int stc_em_group_top_topics(stc_em_group* g, int32_t n_topics, int32_t* idx_out, double* weight_out) {
  return guard([&] {
    STC_REQUIRE(g, "em group");
    STC_REQUIRE((idx_out && weight_out) || g->D == 0, "em: idx_out / weight_out");
    STC_REQUIRE(n_topics > 0, "em: n_topics > 0");
    require_usable(*g);
    require_state(*g);
    const int64_t N = std::min<int64_t>(n_topics, g->k);
    for_members(*g, [&](int i) {
      const int64_t off = g->row0[(size_t)i] * N;
      em::member_top_topics(*g->em[(size_t)i], n_topics, idx_out ? idx_out + off : nullptr,
                            weight_out ? weight_out + off : nullptr);
    });
  });
}

}  // extern "C"
