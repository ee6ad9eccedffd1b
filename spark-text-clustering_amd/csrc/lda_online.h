// lda_online.h — what stc_group (group.hip) needs of its members' online-LDA handles beyond the public ABI.
// struct stc_lda itself stays private to the handle's own translation units (lda_handle.h); these are defined in
// lda_train.hip.
#pragma once

#include "stc_internal.h"

namespace stc {

int corpus_dtype(const stc_lda& L);  // the CSR value dtype the handle reads
// force_coll: the sliced M-step and its collectives on a 1-rank communicator too (STC_GROUP_RCCL);
// tail_fault: the tail_fault-th next step fails before its reduce-scatter (STC_GROUP_STEP_FAULT), 0: none
void set_group_knobs(stc_lda& L, bool force_coll, int tail_fault);
const DCsr* corpus(const stc_lda& L);
void forget_corpus(stc_lda& L);  // no corpus, and no draw or row order made from the previous one
void settle_side(stc_lda& L);    // waits for and drops a draw still being sampled on the side stream
hipStream_t side_stream(const stc_lda& L);  // nullptr before the first stc_lda_next
void gather_lambda(stc_lda& L);  // collective: the full λ on every member after sharded M-steps

}  // namespace stc
