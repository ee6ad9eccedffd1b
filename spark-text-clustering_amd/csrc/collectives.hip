// collectives.hip — RCCL or in-process collectives of a context, and its polling waits (collectives.h)
#include "collectives.h"

#include <algorithm>
#include <chrono>
#include <thread>

namespace stc {

// ---------------------------------------------------------------------------------------
// Waiting on work that may hold RCCL collectives.  A collective whose peer never arrives (a member
// thread or a rank that failed before enqueuing its side) never completes, and hipStreamSynchronize
// would block for ever behind it.  So on a context with a communicator every wait polls — the stream or
// event, the group's abort flag, ncclCommGetAsyncError — against a deadline (STC_COLL_TIMEOUT_MS,
// default 120 s).  A timeout or an asynchronous RCCL error aborts this context's communicator
// (ncclCommAbort releases its queued kernels) and throws STC_ERR_RCCL; a failed peer throws STC_ERR_STATE
// (stc_group's for_members then aborts every member's communicator).  Without a communicator: plain
// blocking waits, as before.
// ---------------------------------------------------------------------------------------
void abort_comm(Ctx& c) {
  if (!c.comm || c.comm_aborted.exchange(true)) return;
  (void)ncclCommAbort(c.comm);  // (c.comm stays set: the context keeps counting as collective, and refuses)
}

namespace {

struct MemberPtrs {
  const void* p[kMaxMembers];
};
template <typename T>
__global__ void k_sum_members(T* __restrict__ out, MemberPtrs src, int n, int64_t off, int64_t count) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
    T acc = static_cast<const T*>(src.p[0])[off + i];
    for (int m = 1; m < n; ++m) acc += static_cast<const T*>(src.p[m])[off + i];
    out[i] = acc;
  }
}
size_t dt_size(ncclDataType_t t) { return t == ncclFloat32 ? 4 : 8; }
void launch_sum_members(hipStream_t s, ncclDataType_t t, void* out, const MemberPtrs& src, int n, int64_t off,
                        int64_t count) {
  if (count == 0) return;
  const int grid = (int)std::min<int64_t>(ceil_div(count, 256), 4096);
  if (t == ncclFloat64) k_sum_members<double><<<grid, 256, 0, s>>>(static_cast<double*>(out), src, n, off, count);
  else if (t == ncclFloat32) k_sum_members<float><<<grid, 256, 0, s>>>(static_cast<float*>(out), src, n, off, count);
  else if (t == ncclInt64) k_sum_members<int64_t><<<grid, 256, 0, s>>>(static_cast<int64_t*>(out), src, n, off, count);
  else throw Error(STC_ERR_STATE, "in-process collective: unsupported type");
  KERNEL_CHECK();
}
MemberPtrs published(const LocalColl& L) {
  MemberPtrs p{};
  for (int m = 0; m < L.n; ++m) p.p[m] = L.ptr[(size_t)m];
  return p;
}

void check_comm(const Ctx& c) {
  if (c.comm_aborted.load())
    throw Error(STC_ERR_STATE, "the RCCL communicator was aborted after a failure: destroy this context / group");
  if (c.abort_flag && c.abort_flag->load())
    throw Error(STC_ERR_STATE, "another member of the group failed; its collectives were abandoned");
}
template <class Query, class Block>
void poll_wait(Ctx& c, Query query, Block block, const char* what) {
  if (!c.comm || !c.coll_enqueued) {  // nothing can be stuck behind a collective (e.g. the corpus upload)
    HIP_CHECK(block());
    return;
  }
  check_comm(c);
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    const hipError_t e = query();
    if (e == hipSuccess) return;
    if (e != hipErrorNotReady) HIP_CHECK(e);
    check_comm(c);
    ncclResult_t ae = ncclSuccess;
    if (ncclCommGetAsyncError(c.comm, &ae) == ncclSuccess && ae != ncclSuccess && ae != ncclInProgress) {
      abort_comm(c);
      throw Error(STC_ERR_RCCL, std::string("RCCL asynchronous error while waiting for ") + what + ": " +
                                    ncclGetErrorString(ae) + " (communicator aborted)");
    }
    const int64_t ms = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count();
    if (ms > c.coll_timeout_ms) {
      abort_comm(c);
      throw Error(STC_ERR_RCCL, std::string("waiting for ") + what + ": not complete after " + std::to_string(ms) +
                                    " ms (STC_COLL_TIMEOUT_MS = " + std::to_string(c.coll_timeout_ms) +
                                    "): a collective's peer never arrived; communicator aborted");
    }
    // yield for the first 20 ms (a step's wait is milliseconds, and a sleep costs its timer slack — ≈ 50 µs
    // on Linux — per wait), then sleep in 100 µs steps
    if (ms < 20) std::this_thread::yield();
    else std::this_thread::sleep_for(std::chrono::microseconds(100));
  }
}
}  // namespace
void wait_stream(Ctx& c, hipStream_t s) {
  poll_wait(c, [&] { return hipStreamQuery(s); }, [&] { return hipStreamSynchronize(s); }, "a stream");
}
void wait_event(Ctx& c, hipEvent_t e) {
  poll_wait(c, [&] { return hipEventQuery(e); }, [&] { return hipEventSynchronize(e); }, "an event");
}

void coll_group_start(Ctx& c) {
  if (!c.comm) return;
  check_comm(c);
  RCCL_CHECK(ncclGroupStart());
  c.in_group = true;
  c.coll_enqueued = true;
}
void coll_group_end(Ctx& c) {
  if (!c.comm) return;
  c.in_group = false;
  RCCL_CHECK(ncclGroupEnd());
}
// in place: buf ← Σ over members
void coll_all_reduce(Ctx& c, void* buf, size_t count, ncclDataType_t t, hipStream_t s) {
  if (c.comm) {
    if (!c.in_group) check_comm(c);
    c.coll_enqueued = true;
    RCCL_CHECK(ncclAllReduce(buf, buf, count, t, ncclSum, c.comm, s));
    return;
  }
  LocalColl& L = *c.local;
  HIP_CHECK(hipStreamSynchronize(s));
  L.ptr[(size_t)c.rank] = buf;
  L.barrier();
  c.coll_tmp.reserve(dt_size(t) * std::max<size_t>(count, 1));
  launch_sum_members(s, t, c.coll_tmp.p, published(L), L.n, 0, (int64_t)count);
  HIP_CHECK(hipStreamSynchronize(s));
  L.barrier();  // every member has read every buffer
  HIP_CHECK(hipMemcpyAsync(buf, c.coll_tmp.p, dt_size(t) * count, hipMemcpyDeviceToDevice, s));
  HIP_CHECK(hipStreamSynchronize(s));
}
// recv (recvcount elements) ← Σ over members of their send[rank·recvcount, +recvcount); recv may be
// the member's own slice of send
void coll_reduce_scatter(Ctx& c, const void* send, void* recv, size_t recvcount, ncclDataType_t t, hipStream_t s) {
  if (c.comm) {
    if (!c.in_group) check_comm(c);
    c.coll_enqueued = true;
    RCCL_CHECK(ncclReduceScatter(send, recv, recvcount, t, ncclSum, c.comm, s));
    return;
  }
  LocalColl& L = *c.local;
  HIP_CHECK(hipStreamSynchronize(s));
  L.ptr[(size_t)c.rank] = const_cast<void*>(send);
  L.barrier();
  launch_sum_members(s, t, recv, published(L), L.n, (int64_t)(c.rank * recvcount), (int64_t)recvcount);
  HIP_CHECK(hipStreamSynchronize(s));
  L.barrier();
}
// recv[q·sendcount, +sendcount) ← member q's send, on every member (send may be its own slice of recv)
void coll_all_gather(Ctx& c, const void* send, void* recv, size_t sendcount, ncclDataType_t t, hipStream_t s) {
  if (c.comm) {
    if (!c.in_group) check_comm(c);
    c.coll_enqueued = true;
    RCCL_CHECK(ncclAllGather(send, recv, sendcount, t, c.comm, s));
    return;
  }
  LocalColl& L = *c.local;
  const size_t bytes = dt_size(t) * sendcount;
  HIP_CHECK(hipStreamSynchronize(s));
  L.ptr[(size_t)c.rank] = recv;
  L.barrier();
  for (int q = 0; q < L.n; ++q) {
    char* dst = static_cast<char*>(L.ptr[(size_t)q]) + (size_t)c.rank * bytes;
    if (dst != send && bytes) HIP_CHECK(hipMemcpyAsync(dst, send, bytes, hipMemcpyDeviceToDevice, s));
  }
  HIP_CHECK(hipStreamSynchronize(s));
  L.barrier();
}

void allreduce_host(Ctx& c, double* x, int64_t n) {
  if (!c.coll() || n == 0) return;
  DevBuf d;
  d.reserve(sizeof(double) * n);
  HIP_CHECK(hipMemcpyAsync(d.p, x, sizeof(double) * n, hipMemcpyHostToDevice, c.stream));
  coll_all_reduce(c, d.p, (size_t)n, ncclFloat64, c.stream);
  HIP_CHECK(hipMemcpyAsync(x, d.p, sizeof(double) * n, hipMemcpyDeviceToHost, c.stream));
  wait_stream(c, c.stream);
}

}  // namespace stc
