// lda_em.h — the member side of an stc_em_group (em_group.hip), implemented in lda_em.hip.
//
// A member is an stc_em over a contiguous shard of the documents (all V columns) on a context joined to the
// group's communicator: N_dk is its own, N_wk / N_k / inv are replicated.  Every function below runs on the
// member's host thread with its device set; the ones marked collective make the same collective calls on
// every member.  The public stc_em_* entry points keep refusing a connected context: only stc_em_shape and
// stc_em_get_state serve a member.
#pragma once

#include <vector>

#include "stc_handles.h"

struct stc_em;

namespace stc {
namespace em {

// collective.  pos_base: the number of edges (non-zero entries) in the earlier shards, so that the RNG keys of
// init_random continue the global CSR order.  All-reduces the column degrees: a term vertex exists iff any
// member has an edge of it.  state_dtype (STC_F64 | STC_F32): how the member stores N_dk / N_wk, and the type
// its N_wk' is all-reduced in.
stc_em* member_create(Ctx& c, const DCsr& shard, int32_t k, double doc_concentration, double topic_concentration,
                      int state_dtype, int64_t pos_base);
void member_init_random(stc_em& m, uint64_t seed);  // collective
// doc_topics: the member's own rows; both arrays already checked non-negative by the group
void member_set_state(stc_em& m, const double* doc_topics, const double* term_topics);
void member_next(stc_em& m, int32_t n_iterations);  // collective
// any may be NULL: Σ c ln(φ·θ) over the member's edges, Σ ln φ over the term vertices of the whole graph
// (the same on every member), Σ ln θ over the member's document vertices
void member_log_likelihood(stc_em& m, double* ll, double* term_prior, double* doc_prior);
// the member's rows: indptr_out int64[D_i + 1] from 0, terms_out / topics_out int32[E_i]
void member_topic_assignments(stc_em& m, int64_t* indptr_out, int32_t* terms_out, int32_t* topics_out);
// the ranked queries (stc.h) over the member's rows and its replica of N_wk / N_k; none is collective.
// top_documents: per topic the member's best N_i = min(max_docs, its document vertices) rows, as global rows
// (row0 + local row): rows / weights k×N_i; returns N_i
void member_describe(stc_em& m, int32_t max_terms, int32_t* idx_out, double* weight_out);
int64_t member_top_documents(stc_em& m, int64_t max_docs, int64_t row0, std::vector<int64_t>& rows,
                             std::vector<double>& weights);
void member_top_topics(stc_em& m, int32_t n_topics, int32_t* idx_out, double* weight_out);
void member_wait(stc_em& m);  // until the member's queued iterations have finished

}  // namespace em
}  // namespace stc
