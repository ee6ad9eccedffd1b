// lda_em.h — EMLDAOptimizer / DistributedLDAModel on the device (lda_em.hip): the graph in both
// orientations and the state N_dk, N_wk, N_k.  api.hip checks the ABI's pointers and forwards here.
#pragma once

#include "stc_internal.h"

namespace stc {
namespace em {

stc_em* create(Ctx& c, const DCsr& corpus, int32_t k, double doc_concentration, double topic_concentration);
void destroy(stc_em* m);
void shape(const stc_em& m, int32_t* k, int64_t* n_docs, int64_t* vocab, int64_t* n_edges);
void init_random(stc_em& m, uint64_t seed);
void set_state(stc_em& m, const double* doc_topics, const double* term_topics);
void get_state(stc_em& m, double* doc_topics, double* term_topics, double* totals, double* alpha_out, double* eta_out);
void next(stc_em& m, int32_t n_iterations);
void log_likelihood(stc_em& m, double* log_likelihood_out, double* log_prior_out);

}  // namespace em
}  // namespace stc
