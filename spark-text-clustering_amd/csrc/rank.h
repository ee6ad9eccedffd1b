// rank.h — ranked queries over a resident matrix (rank.hip): the N largest entries of every column of a
// row-major R×k matrix (describeTopics, topDocumentsPerTopic, the important terms' S_t) and of every row
// (topTopicsPerDocument).  lda_em.hip drives them from an stc_em's buffers, lda_online.hip from λ, lda_score.hip
// from a score's γ; everything here is enqueued on the given stream.  The device pieces shared with those
// files' own kernels are in rank_key.h.
#pragma once

#include "stc_internal.h"

namespace stc {
namespace rank {

// grow-only device scratch of the column selection, kept by the handle
struct Scratch {
  DevBuf sel;       // Sel[k]: every topic's selected key prefix and counters
  DevBuf hist;      // uint32[k×256]: the current digit's histogram of every topic
  DevBuf cand_key;  // uint64[k×P]: the survivors' value keys (P: the power of two at or above N + kSlack)
  DevBuf cand_row;  // uint32[k×P]: their rows
  DevBuf rowsum;    // double[R]: Σ_j M[r][j], j ascending; −1 marks a row without a vertex
  DevBuf count;     // int64: the rows that have a vertex
  DevBuf out_row;   // int64[k×N] / int32[R×N]
  DevBuf out_w;     // double[k×N] / double[R×N]
};

// rowsum[r] = ((M[r][0] + M[r][1]) + …) + M[r][k−1] in fp64 (the stored values widened), or −1 where ptr is
// given and row r has no edge (ptr[r+1] == ptr[r]).  f32: M holds floats, else doubles.
void row_sums(hipStream_t s, const void* m, bool f32, const int64_t* ptr, int64_t R, int k, double* rowsum);
// *count = the rows r < R with ptr[r+1] > ptr[r]
void count_vertices(hipStream_t s, const int64_t* ptr, int64_t R, int64_t* count);

// For every topic t the N largest values of column t, ordered by (value descending, row ascending):
// out_row[t·N + i] = row0 + row, out_w[t·N + i] = its weight.  1 <= N <= candidates (R, or the rows whose
// rowsum is not −1).  rowsum == nullptr, the raw mode: the value is M[r][t] and the weight value / nk[t]
// (the value where nk is nullptr).  Otherwise the row-normalised mode: value and weight are M[r][t] / rowsum[r]
// (M[r][t] where rowsum[r] is 0), and rows marked −1 are no candidates.
void select_columns(hipStream_t s, Scratch& sc, const void* m, bool f32, int64_t R, int k, int64_t N,
                    const double* rowsum, const double* nk, int64_t row0, int64_t* out_row, double* out_w);

// describeTopics: select_columns in raw mode on c's stream into sc.out_row / sc.out_w, then the k×N lists on the
// host — idx_out[t·N + i] the row as int32 (R < 2^31), weight_out[t·N + i] = M[row][t] / nk[t].  Waits for the stream.
void describe_columns(Ctx& c, Scratch& sc, const void* m, bool f32, int64_t R, int k, int64_t N, const double* nk,
                      int32_t* idx_out, double* weight_out);

// For every row the N <= k largest counts, ordered by (count descending, topic ascending):
// out_idx[r·N + i] = topic, out_w[r·N + i] = count / rowsum[r] (the count where rowsum[r] is 0).
void select_rows(hipStream_t s, const void* m, bool f32, const double* rowsum, int64_t R, int k, int N,
                 int32_t* out_idx, double* out_w);

}  // namespace rank
}  // namespace stc
