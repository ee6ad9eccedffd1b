// coherence_host.h — the host arithmetic of stc_coherence (include/stc.h "Topic coherence"): UMass and document-level
// NPMI from document co-occurrence counts.  Plain C++ with no device or runtime dependency, so the one new piece of
// host code that walks caller-sized arrays also builds into a stand-alone sanitizer program (tools/coherence_host_check.cpp).
#pragma once

#include <cmath>
#include <cstdint>

#include "stc.h"

namespace stc {
namespace coherence {

// nullptr, or the requirement the arguments break (nothing is written then).  df k×n, codf k×n×n; topic_out k and
// pairs_out k may be null.  Per topic the pairs (m, l), 1 <= m < n, 0 <= l < m, in that order, added sequentially.
inline const char* measure_topics(const int64_t* df, const int64_t* codf, int32_t k, int32_t n, int64_t n_docs,
                                  int measure, double eps, double* topic_out, int32_t* pairs_out) {
  if (!df || !codf) return "coherence: df/codf";
  if (k < 1 || n < 1) return "coherence: k >= 1 and n >= 1";
  if (measure != STC_COH_UMASS && measure != STC_COH_NPMI) return "coherence: measure";
  if (n_docs <= 0) return "coherence: n_docs must be > 0";
  if (measure == STC_COH_UMASS && !(eps > 0.0)) return "coherence: eps must be > 0 for UMass";
  const int64_t kn = (int64_t)k * n;
  for (int64_t q = 0; q < kn; ++q)
    if (df[q] < 0) return "coherence: a negative df";
  for (int64_t q = 0; q < kn * n; ++q)
    if (codf[q] < 0) return "coherence: a negative codf";
  const double D = (double)n_docs;
  for (int64_t t = 0; t < k; ++t) {
    const int64_t* d = df + t * n;
    const int64_t* co = codf + t * n * n;
    double sum = 0.0;
    int32_t pairs = 0;
    for (int m = 1; m < n; ++m) {
      for (int l = 0; l < m; ++l) {
        if (d[m] <= 0 || d[l] <= 0) continue;  // an unused slot, or a term the corpus does not hold
        const int64_t c = co[(int64_t)m * n + l];
        double v;
        if (measure == STC_COH_UMASS)
          v = std::log(((double)c + eps) / (double)d[l]);
        else if (c == 0)
          v = -1.0;
        else if (c == n_docs)
          v = 0.0;
        else
          v = std::log(((double)c * D) / ((double)d[m] * (double)d[l])) / -std::log((double)c / D);
        sum += v;
        ++pairs;
      }
    }
    if (topic_out) topic_out[t] = measure == STC_COH_NPMI && pairs > 0 ? sum / (double)pairs : sum;
    if (pairs_out) pairs_out[t] = pairs;
  }
  return nullptr;
}

}  // namespace coherence
}  // namespace stc
