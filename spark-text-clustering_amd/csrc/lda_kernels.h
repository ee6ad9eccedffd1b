// lda_kernels.h — host-side launch API of the online-LDA E-step kernels (lda.hip, lda_grid.hip, lda_rows64.hip,
// lda_wide.hip, lda_team64.hip).  The rest of a step (sstats, M-step, batch kernels): lda_step_kernels.h.
#pragma once

#include <cmath>

#include "stc_internal.h"

namespace stc {
namespace lda {

constexpr int kBlock = 256;           // threads per E-step workgroup (4 waves of 64)
constexpr int kLdsBudget = 80 * 1024; // dynamic LDS per E-step workgroup → 2 workgroups / CU

// An entry's sort value for the term-sorted sstats SpMM: its member slot in the high word and, in
// the low word, r itself for fp32 (so the SpMM reads (slot, r) with the sorted keys instead of
// gathering them per entry) or the entry index for fp64 (r is gathered from r[e]).
template <typename T>
__device__ __forceinline__ uint64_t entry_val(int64_t slot, int64_t e, T r) {
  if constexpr (sizeof(T) == 4)
    return ((uint64_t)(uint32_t)slot << 32) | __builtin_bit_cast(uint32_t, r);
  else
    return ((uint64_t)(uint32_t)slot << 32) | (uint32_t)e;
}

// Everything the E-step kernel reads/writes.  T = the E-step arithmetic type (float/double).
template <typename T>
struct EStepArgs {
  int k = 0, kp = 0, P = 0;            // topics, global row pitch of Bp, LDS row pitch
  int lds_rows = 0;                    // docs with nnz <= lds_rows keep their block in LDS
  const int64_t* indptr = nullptr;     // documents (CSR rows)
  const int32_t* indices = nullptr;
  const T* values = nullptr;
  // A launch covers slots [slot0, slot0 + n).  slot → row via `batch` (nullptr: row = slot);
  // slot → caller's member index via `orig` (nullptr: member = slot) — γ₀, γ, iters, nonempty,
  // bound and the RNG key are per MEMBER; eth / elogth / entry slots are per SLOT.
  const int32_t* batch = nullptr;
  const int32_t* orig = nullptr;
  int64_t slot0 = 0;
  int64_t n = 0;                       // slots in this launch
  const int64_t* bptr = nullptr;       // slot → first entry slot (nullptr: the row's CSR offset)
  // per CSR entry: the in-row position of the row's n-th E-step row (lda_wide.hip: the corpus's
  // rarest terms first, so the register / LDS rows are the cold ones and the streamed rows the hot
  // ones the MALL holds for every CU); nullptr: CSR order
  const int32_t* order = nullptr;
  const T* Bp = nullptr;               // V×kp  row-scaled expElogβ': exp(ψ(λ_vt) − m_v)
  const double* psic = nullptr;        // 2k    ψ(Σ_v λ_vt), then exp(−ψ(Σ_v λ_vt)): eθ' = exp(ψ(γ_t) − ψ(Σγ) − psic_t)
  const double* logscale = nullptr;    // V     m_v (BOUND)
  const double* alpha = nullptr;       // k
  const T* gamma0 = nullptr;           // n×k or nullptr (counter RNG)
  uint64_t seed = 0;
  int64_t iteration = 0;
  int rank = 0;
  int key_mode = 0;                    // 0: train_doc_key(iteration, rank, i); 1: doc_id_base + row
  int64_t doc_id_base = 0;
  double gamma_shape = 100.0;
  int max_iter = 100000;
  // Spark's stop rule Σ|Δγ|/k ≤ 1e-3 as one comparison: the largest double T with fl(T / k) ≤ 1e-3
  // (fl(x / k) is monotone in x, so x ≤ T ⇔ fl(x / k) ≤ 1e-3 exactly; stop_threshold() below)
  double stop_thr = 0.0;
  // outputs
  T* gamma = nullptr;                  // n×k (optional)
  T* eth = nullptr;                    // n×kp scaled exp(E[log θ]) (STATS)
  T* elogth = nullptr;                 // n×k  E[log θ] (STATS: logphat)
  T* r = nullptr;                      // entry slots: cts/φ' (always)
  uint32_t* keys = nullptr;            // entry slots: term id (STATS)
  uint64_t* vals = nullptr;            // entry slots: entry_val(slot, entry, r) (STATS)
  int32_t* iters = nullptr;            // n (optional)
  int32_t* nonempty = nullptr;         // n (optional)
  double* bound = nullptr;             // n (BOUND)
  // fp64 rows / fp32 grid kernels: scratch for the list of this launch's long documents (capacity n
  // slots + one count word), filled on the device before the long-document launch walks it (last, so
  // the other kernels' argument layout is unchanged)
  int32_t* long_list = nullptr;
  // BOUND: λ (V×k) for the log-space token term of a row whose scaled dot product underflowed (lda_wide.hip, lda.hip);
  // nullptr (λ sharded, only this rank's slice current): such a row keeps the floored logarithm
  const double* lam = nullptr;
};

// the largest double x with fl(x / k) ≤ 1e-3 (host; see EStepArgs::stop_thr)
inline double stop_threshold(int k) {
  const double kd = (double)k;
  double x = 1e-3 * kd;
  while (x / kd > 1e-3) x = std::nextafter(x, 0.0);
  while (std::nextafter(x, INFINITY) / kd <= 1e-3) x = std::nextafter(x, INFINITY);
  return x;
}

template <typename T>
size_t estep_lds_bytes(int kp, int lds_rows, int P);
template <typename T>
int estep_lds_rows(int k, int kp, int P);
template <typename T>
void launch_estep(hipStream_t s, const EStepArgs<T>& a, bool stats, bool bound);

// fp32 row-lane × topic-group grid E-step (lda_grid.hip): k <= 128, nnz <= grid_row_cap(k) (0 if n/a)
int grid_row_cap(int k);
// documents past grid_onchip_rows(k) run in a second, resident launch (`long_docs`; a.long_list set)
int grid_onchip_rows(int k);
void launch_estep_grid(hipStream_t s, const EStepArgs<float>& a, bool stats, bool bound, bool long_docs);
// fp64 rows-split E-step (lda_rows64.hip): k <= 104, nnz <= rows64_row_cap(k) (0 if n/a); documents
// past rows64_onchip_rows(k) run in a second launch (`long_docs`)
int rows64_row_cap(int k);
int rows64_onchip_rows(int k);
void launch_estep_rows64(hipStream_t s, const EStepArgs<double>& a, bool stats, bool bound, bool long_docs);
// many-topic E-step (lda_wide.hip): topics across a 512-thread workgroup, k <= 2048, nnz <= wide_row_cap(k)
int wide_row_cap(int k);
// a team of P CUs per document for the many-topic E-step (lda_wide.hip k_estep_wide_mc)
struct WideTeam {
  int P = 1;                 // workgroups (CUs) per document
  int blocks = 0;            // persistent grid: a multiple of 8·P, ≤ the CU count
  unsigned* tmo = nullptr;   // timeout word (zeroed before each launch)
  void* xbuf = nullptr;      // [teams][2][P][xstride] 16-byte {epoch, value} granules (zeroed before each launch)
  int64_t xstride = 0;       // granules per member: rows split kp + 1 (s partials, Σ r·φ); topics split
                             // 512 + 2 (φ partials, Σ|Δγ|, Σγ)
  unsigned spin_limit = 1u << 22;  // polls before a member gives up (a few seconds)
  int fault_member = -1;     // debug (STC_TEAM_FAULT): this member of team 0 never publishes
  int max_row = -1;          // the launch's longest document (< 0: unknown) — k_estep_wide_tc sizes its
                             // per-row LDS arrays by it, so the rest of the CU's LDS holds block rows
  int xrows = 0;             // (set by the tc launcher) rows of those arrays
};
// after the E-step's logphat: a timed-out team poisons the non-empty count (small[k] = −1e300, negative
// after any all-reduce over ranks), which gates the λ / colsum / expElogβ' / α updates off
template <typename T>
int wide_resident_rows(int k);
// false: the grid could not be resident at once (nothing launched; the caller runs the one-CU kernel)
template <typename T>
bool launch_estep_wide_mc(hipStream_t s, const EStepArgs<T>& a, bool stats, const WideTeam& wt);
// the same with the TOPICS split over the team (k > 512; lda_wide.hip k_estep_wide_tc)
template <typename T>
bool launch_estep_wide_tc(hipStream_t s, const EStepArgs<T>& a, bool stats, const WideTeam& wt);
template <typename T>
void launch_estep_wide(hipStream_t s, const EStepArgs<T>& a, bool stats, bool bound);
// fp64 many-topic team E-step with the TOPICS split over P = tgrid64_members(kp) CUs and the rows64 grid
// inside a member (lda_team64.hip k_estep_tgrid64): nnz ≤ tgrid64_row_cap(); wt.xstride ≥ tgrid64_xstride();
// false: the grid could not be resident at once (nothing launched)
int tgrid64_row_cap();
int tgrid64_members(int kp);
int64_t tgrid64_xstride();
bool launch_estep_tgrid64(hipStream_t s, const EStepArgs<double>& a, bool stats, const WideTeam& wt);

}  // namespace lda
}  // namespace stc
