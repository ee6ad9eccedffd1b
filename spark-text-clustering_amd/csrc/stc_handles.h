// stc_handles.h — what the translation units behind the C ABI share beyond stc_internal.h: the opaque handles
// that more than one of them fills in, and the host-side helpers of their entry points
#pragma once

#include <algorithm>
#include <cstdlib>
#include <initializer_list>
#include <memory>
#include <utility>

#include "stc_internal.h"

struct stc_ctx : stc::Ctx {};
struct stc_dcsr : stc::DCsr {};
struct stc_dtok {
  stc::Ctx* ctx = nullptr;  // the context it was uploaded on / made by; only it may read the buffers
  int device = -1;          // for stc_tokens_free, which may run after that context is gone
  stc::DevBuf utf8, tok_off, doc_off;
  int64_t n_bytes = 0, n_tok = 0, n_docs = 0;
  int64_t max_doc = -1;  // the longest document's token count (from the upload's offsets)
  bool off32 = false;    // tok_off holds u32 offsets (blob + padding < 4 GiB), else int64
};

namespace stc {

template <typename H>
std::unique_ptr<H> new_handle(Ctx& c) {  // an ABI handle made by, and readable only on, context c
  auto h = std::make_unique<H>();
  h->ctx = &c;
  h->device = c.device;
  return h;
}

struct TokenUpload {  // host tokens copied to the device for one call (features_api.hip)
  DevBuf utf8, tok_off, doc_off;
  int64_t max_doc = -1;  // the longest document's token count (doc_off given), −1 unknown
};
void upload_tokens(Ctx& c, TokenUpload& u, const uint8_t* utf8, int64_t n_bytes, const int64_t* tok_off,
                   int64_t n_tok, const int64_t* doc_off, int64_t n_docs);
namespace stages {
// the longest document's token count from device document offsets (token_stages.hip); waits for the stream
int64_t longest_doc(Ctx& c, const int64_t* d_doc_off, int64_t n_docs);
}  // namespace stages
inline void swap(DevBuf& a, DevBuf& b) {
  std::swap(a.p, b.p);
  std::swap(a.bytes, b.bytes);
}

// The hipcub / rocprim two-call idiom: f(nullptr, bytes) asks for the temporary storage's size, tmp grows
// to it, f(tmp.p, bytes) runs (unless run is false).  f: (void*, size_t&) -> hipError_t.
template <typename F>
void with_temp(DevBuf& tmp, F&& f, bool run = true) {
  size_t bytes = 0;
  HIP_CHECK(f(nullptr, bytes));
  tmp.reserve(bytes);
  if (run) HIP_CHECK(f(tmp.p, bytes));
}

// Owners of the HIP objects a handle keeps: get() makes the object on first use, the destructor releases it;
// the member itself is null until then (a handle asks "is there a side stream yet" that way).
struct NoCopy {
  NoCopy() = default;
  NoCopy(const NoCopy&) = delete;
  NoCopy& operator=(const NoCopy&) = delete;
};
struct Event : NoCopy {
  hipEvent_t e = nullptr;
  ~Event() {
    if (e) (void)hipEventDestroy(e);
  }
  hipEvent_t get(unsigned flags = hipEventDisableTiming) {
    if (!e) HIP_CHECK(hipEventCreateWithFlags(&e, flags));
    return e;
  }
};
struct Stream : NoCopy {
  hipStream_t s = nullptr;
  ~Stream() {
    if (s) (void)hipStreamDestroy(s);
  }
  hipStream_t get(unsigned flags = hipStreamNonBlocking, bool lowest_priority = false) {
    if (!s && lowest_priority) {
      int least = 0, greatest = 0;
      HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
      HIP_CHECK(hipStreamCreateWithPriority(&s, flags, least));
    }
    if (!s) HIP_CHECK(hipStreamCreateWithFlags(&s, flags));
    return s;
  }
};
template <typename T, size_t N = 1>
struct Pinned : NoCopy {  // N host words the device copies into; zero when made
  T* p = nullptr;
  ~Pinned() {
    if (p) (void)hipHostFree(p);
  }
  T* get() {
    if (!p) {
      HIP_CHECK(hipHostMalloc((void**)&p, N * sizeof(T), hipHostMallocDefault));
      std::fill(p, p + N, T{});
    }
    return p;
  }
};

// Launch geometry.  blocks_for: a grid of blocks of `per` elements over n of them, one block at the least.
// pow2_at_least: the power of two at or above k, 2 at the least — the lanes a row of k topics takes.
inline unsigned blocks_for(int64_t n, int64_t per = 256) { return (unsigned)std::max<int64_t>(1, ceil_div(n, per)); }
inline int pow2_at_least(int k) {
  int p = 2;
  while (p < k) p <<= 1;
  return p;
}

// Environment switches.  env_int: an integer clamped to [lo, hi], dflt when unset.  env_flag: by the value's
// first character — a switch that is on by default is off only at '0', one that is off by default is on only at '1'.
inline int env_int(const char* name, int dflt, int lo, int hi) {
  const char* e = std::getenv(name);
  return e ? std::max(lo, std::min(hi, std::atoi(e))) : dflt;
}
inline char env_first(const char* name) {  // the value's first character, 0 when unset or empty
  const char* e = std::getenv(name);
  return e ? e[0] : '\0';
}
inline bool env_flag(const char* name, bool dflt) { return dflt ? env_first(name) != '0' : env_first(name) == '1'; }

// api.hip: off[0 .. n] of the host array `name` starts at 0, is non-decreasing and ends at `total` (spans) or
// at most there; a host CSR's arrays (both return the largest gap: the longest document or row); and bufs'
// allocations back to the recycler of the context that made them, if that context still exists on `device`
int64_t check_offsets(const char* name, const int64_t* off, int64_t n, int64_t total, const char* total_name,
                      bool spans);
int64_t check_host_csr(int64_t rows, int64_t cols, const int64_t* indptr, const int32_t* indices, const double* values);
void recycle_to(Ctx* ctx, int device, std::initializer_list<DevBuf*> bufs);

}  // namespace stc
