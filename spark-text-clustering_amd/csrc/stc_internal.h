// stc_internal.h — internals shared by the libstc.so translation units (gfx950 / HIP only).
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "stc.h"

namespace stc {

// device UTF-8 token blobs are allocated this many bytes past their end: hashing_tf.hip reads each
// token as a 32-byte window of whole aligned dwords from its aligned start
constexpr int64_t kHashPad = 64;

// ---------------------------------------------------------------------------------------
// Errors: every entry point runs inside guard(); failures throw stc::Error and come back to
// the caller as a status code + thread-local message (stc_last_error).  Never abort().
// ---------------------------------------------------------------------------------------
struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

void set_last_error(const std::string& msg);

template <typename F>
int guard(F&& f) {
  try {
    f();
    return STC_OK;
  } catch (const Error& e) {
    set_last_error(e.what());
    return e.code;
  } catch (const std::bad_alloc&) {
    set_last_error("host out of memory");
    return STC_ERR_OOM;
  } catch (const std::exception& e) {
    set_last_error(e.what());
    return STC_ERR_STATE;
  }
}

#define STC_REQUIRE(cond, msg)                                                          \
  do {                                                                                  \
    if (!(cond)) throw ::stc::Error(STC_ERR_INVALID_ARG, std::string("requirement failed: ") + (msg)); \
  } while (0)

#define HIP_CHECK(expr)                                                                 \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess) {                                                             \
      int c_ = (e_ == hipErrorOutOfMemory) ? STC_ERR_OOM : STC_ERR_HIP;                 \
      throw ::stc::Error(c_, std::string(#expr) + ": " + hipGetErrorString(e_) + " @" + \
                                 __FILE__ + ":" + std::to_string(__LINE__));            \
    }                                                                                   \
  } while (0)

#define RCCL_CHECK(expr)                                                                \
  do {                                                                                  \
    ncclResult_t r_ = (expr);                                                           \
    if (r_ != ncclSuccess)                                                              \
      throw ::stc::Error(STC_ERR_RCCL, std::string(#expr) + ": " + ncclGetErrorString(r_)); \
  } while (0)

#define KERNEL_CHECK() HIP_CHECK(hipGetLastError())

// ---------------------------------------------------------------------------------------
// Device buffer (grow-only scratch).  Allocation happens only outside the launch sequence.
// ---------------------------------------------------------------------------------------
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  void reserve(size_t n) {
    if (n <= bytes) return;
    release();
    size_t want = n < 256 ? 256 : n;
    HIP_CHECK(hipMalloc(&p, want));
    bytes = want;
  }
  template <typename T>
  T* as() const { return static_cast<T*>(p); }
};

// Device allocations a freed stc_dcsr handed back to the context that made it, so the next output of a
// similar size (HashingTF, upload) takes one instead of calling hipMalloc (tens of µs for GB-sized
// buffers, inside every call).  At most kMax are kept; the context frees them when it is destroyed.
struct Recycler {
  static constexpr size_t kMax = 6;
  static constexpr size_t kMin = size_t(1) << 20;  // smaller buffers are freed, not kept
  std::mutex mu;
  std::vector<std::pair<void*, size_t>> bufs;
  void put(DevBuf& b) {  // takes b's allocation (b is empty afterwards)
    if (!b.p || b.bytes < kMin) return;
    std::lock_guard<std::mutex> lk(mu);
    if (bufs.size() >= kMax) {  // drop the smallest kept one (or this one)
      size_t sm = 0;
      for (size_t i = 1; i < bufs.size(); ++i)
        if (bufs[i].second < bufs[sm].second) sm = i;
      if (bufs[sm].second >= b.bytes) return;
      (void)hipFree(bufs[sm].first);
      bufs.erase(bufs.begin() + (std::ptrdiff_t)sm);
    }
    bufs.emplace_back(b.p, b.bytes);
    b.p = nullptr;
    b.bytes = 0;
  }
  void take(DevBuf& b, size_t n) {  // b.reserve(n), from a kept allocation of n…2n bytes when one exists
    if (n <= b.bytes) return;
    {
      std::lock_guard<std::mutex> lk(mu);
      size_t best = bufs.size();
      for (size_t i = 0; i < bufs.size(); ++i)
        if (bufs[i].second >= n && bufs[i].second <= 2 * n && (best == bufs.size() || bufs[i].second < bufs[best].second))
          best = i;
      if (best < bufs.size()) {
        b.release();
        b.p = bufs[best].first;
        b.bytes = bufs[best].second;
        bufs.erase(bufs.begin() + (std::ptrdiff_t)best);
        return;
      }
    }
    b.reserve(n);
  }
  ~Recycler() {
    for (auto& x : bufs) (void)hipFree(x.first);
  }
};

// ---------------------------------------------------------------------------------------
// Context: one device, one stream, optional RCCL communicator.
// ---------------------------------------------------------------------------------------
struct LocalColl;  // in-process collectives of the stc_group members that share one device (collectives.h)
struct Ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  ncclComm_t comm = nullptr;
  LocalColl* local = nullptr;  // set instead of comm for same-device group members (owned by the group)
  int n_ranks = 1;
  int rank = 0;
  int cus = 256;          // compute units (the df count sizes its grid to one workgroup per CU)
  // hashing_tf.hip build_csr when every document fits the fused register sort: hash + sort + emit in one
  // look-back pass (STC_TF_MODE=0: false, the passes hash + sort → sorted keys, scan, runs — which longer
  // documents and a timed-out look-back take anyway)
  bool tf_single_pass = true;
  bool tf_force_fault = false;  // test knob (STC_TF_FAULT=1): every look-back gives up at once
  int64_t tf_fallbacks = 0;     // single passes that fell back to the sorted-key passes
  bool idf_cache = true;  // idf.hip: the device IDF model's hot-idf LDS table (STC_IDF_NO_CACHE=1: off)
  Recycler recycle;    // freed stc_dcsr allocations for the next outputs (stc_dcsr_free)
  DevBuf scratch[12];  // grow-only scratch of the featurisation kernels (hashing_tf.hip, idf.hip, features_api.hip IDF)
  DevBuf coll_tmp;    // the in-process all-reduce's staging buffer
  // RCCL failure handling (collectives.hip wait_stream / wait_event): with a communicator, every wait on work that
  // may hold a collective polls with a deadline instead of blocking in the runtime
  const std::atomic<bool>* abort_flag = nullptr;  // the group's: set once any of its members has failed
  std::atomic<bool> comm_aborted{false};          // comm was aborted (ncclCommAbort): never used again
  int64_t coll_timeout_ms = 120000;               // STC_COLL_TIMEOUT_MS (read at stc_init)
  bool in_group = false;                          // between ncclGroupStart and ncclGroupEnd
  bool coll_enqueued = false;                     // a collective was ever enqueued (waits poll from then on)
  void use() const { HIP_CHECK(hipSetDevice(device)); }
  bool coll() const { return comm != nullptr || local != nullptr; }
};

struct DCsr {
  Ctx* ctx = nullptr;  // the context that made it; only it may read the buffers (checked at the ABI)
  int device = -1;     // for stc_dcsr_free, which may run after that context is gone
  int64_t rows = 0, cols = 0, nnz = 0;
  int64_t max_row = -1;  // longest row's nnz when known (host uploads), −1 otherwise
  int dtype = STC_F64;
  // every value is > 0 (a HashingTF output: counts / binary 1; kept by a floored IDF transform), so a
  // df count needs only the indices (cleared by anything that may write a value ≤ 0)
  bool positive = false;
  // every row holds an id at most once (a HashingTF output; kept by the transform): idf.hip may count df
  // in u16 per group of ≤ 65535 rows
  bool unique_ids = false;
  DevBuf indptr;   // int64[rows+1]
  DevBuf indices;  // int32[nnz]
  DevBuf values;   // float/double[nnz]
};

// ---------------------------------------------------------------------------------------
// Counter-based RNG shared bit-for-bit with oracle/oracle.py (splitmix64 streams, uniform
// in (0,1) from the top 53 bits, Box–Muller normal, Marsaglia–Tsang Gamma(shape, 1/shape)).
// ---------------------------------------------------------------------------------------
__host__ __device__ inline uint64_t splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__host__ __device__ inline uint64_t doc_stream(uint64_t seed, uint64_t key) {
  return splitmix64(seed ^ splitmix64(key));
}
__host__ __device__ inline double rng_uniform(uint64_t stream, uint64_t ctr) {
  uint64_t x = splitmix64(stream + ctr * 0xD1B54A32D192ED03ull);
  return ((double)(x >> 11) + 0.5) * (1.0 / 9007199254740992.0);
}
__host__ __device__ inline double gamma_sample(uint64_t stream, int topic, double shape) {
  const double d = shape - 1.0 / 3.0;
  const double c = 1.0 / sqrt(9.0 * d);
  double v = 1.0;
  for (int attempt = 0; attempt < 64; ++attempt) {
    const uint64_t base = ((uint64_t)topic << 8) + 3u * (uint64_t)attempt;
    const double u1 = rng_uniform(stream, base);
    const double u2 = rng_uniform(stream, base + 1);
    const double x = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
    v = 1.0 + c * x;
    if (v <= 0.0) continue;
    v = v * v * v;
    const double u = rng_uniform(stream, base + 2);
    if (u < 1.0 - 0.0331 * (x * x) * (x * x)) break;
    if (log(u) < 0.5 * x * x + d * (1.0 - v + log(v))) break;
  }
  return d * v / shape;
}
// γ₀ key of a training minibatch member (mirrors oracle.train_doc_key)
__host__ __device__ inline uint64_t train_doc_key(int64_t iteration, int rank, int64_t pos) {
  return (((uint64_t)iteration & 0xFFFFFFull) << 40) | (((uint64_t)rank & 0xFFull) << 32) |
         ((uint64_t)pos & 0xFFFFFFFFull);
}

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// kernels-side entry points (implemented in the .hip files)
namespace hashing {
void hash_tokens(Ctx& c, const uint8_t* d_utf8, const int64_t* d_tok_off, int64_t n_tok,
                 int32_t num_features, int variant, int32_t* d_idx);
void row_order_by_df(Ctx& c, const DCsr& m, const int64_t* d_df, int32_t* d_order);
// the documents listed in d_large (n_large of them, each past the register sort's 1024 keys): d_sorted = d_keys
// sorted inside each listed document's [doc_off[d], doc_off[d+1]) (hipcub's segmented radix sort over the bits of
// max_key, the largest key); d_is_large[d] = 1 for each when given.  seg and tmp are the caller's scratch.
void sort_long_docs(Ctx& c, const int32_t* d_keys, int32_t* d_sorted, int64_t n_tok, const int32_t* d_large,
                    int32_t n_large, const int64_t* d_doc_off, int64_t max_key, DevBuf& seg, DevBuf& tmp,
                    uint8_t* d_is_large = nullptr);
// token offsets as int64 (d_tok_off64) or, when d_tok_off32 is given, u32 (a resident upload's narrowed copy)
void build_csr(Ctx& c, const uint8_t* d_utf8, const int64_t* d_tok_off64, const uint32_t* d_tok_off32, int64_t n_tok,
               const int64_t* d_doc_off, int64_t n_docs, int32_t num_features, int binary,
               int variant, int value_dtype, int64_t max_doc /* longest document's tokens, −1 unknown */,
               DCsr& out);
void narrow_offsets(Ctx& c, const int64_t* d_src, int64_t n, uint32_t* d_dst);
}  // namespace hashing
namespace tokenizer {
// Spark ML Tokenizer on device: d_text/d_text_off (n_docs+1) in; lower-cased, separator-free blob,
// token offsets (n_tok+1) and per-document token offsets (n_docs+1) out (the blob may be up to half
// as long again as the input: Java 8 lower-cases a few 2-byte characters to 3 bytes).
void tokenize(Ctx& c, const uint8_t* d_text, const int64_t* d_text_off, int64_t n_docs,
              DevBuf& out_utf8, DevBuf& out_tok_off, DevBuf& out_doc_off, int64_t& n_tok,
              int64_t& n_out_bytes);
}  // namespace tokenizer
namespace idf {
// idf finalised inside the df reduction when the caller already knows m (no collective in between)
struct IdfFinal {
  double m;
  int64_t min_df;
  double* idf;
};
// df (cols); with fin, also idf when the path allows — returns true then (else call finalize)
bool doc_freq(Ctx& c, const DCsr& m, int64_t* d_df /* cols */, const IdfFinal* fin = nullptr);
void finalize(Ctx& c, const int64_t* d_df, int64_t cols, int64_t m, int64_t min_df, double* d_idf);
// cache: the hot-idf table build_cache made for this idf (nullptr: plain gathers)
void transform(Ctx& c, DCsr& m, const double* d_idf, double zero_floor, const DevBuf* cache = nullptr);
// the device IDF model's hot-idf table (false, cache untouched: vocabulary too large or disabled)
bool build_cache(Ctx& c, const int64_t* d_df, const double* d_idf, int64_t cols, DevBuf& cache);
}  // namespace idf

}  // namespace stc
