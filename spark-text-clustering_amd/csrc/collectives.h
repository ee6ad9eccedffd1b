// collectives.h — the collectives of a context and the waits on work that may hold one (collectives.hip).
//
// RCCL over the context's communicator — or, for the members of one stc_group that share a device (a group
// of N handles on one GPU: the multi-GPU decomposition exercised on one device), an in-process transport:
// every member runs on its own host thread, the members exchange device pointers under a barrier and sum /
// copy with a kernel, in member order (so every member's result is bit-identical).  Same call sequence on
// every member, as with RCCL.
#pragma once

#include <condition_variable>

#include "stc_internal.h"

namespace stc {

constexpr int kMaxMembers = 16;
struct LocalColl {
  int n = 0;
  std::mutex m;
  std::condition_variable cv;
  int arrived = 0;
  uint64_t gen = 0;
  bool broken = false;
  std::vector<void*> ptr;
  explicit LocalColl(int members) : n(members), ptr((size_t)members, nullptr) {}
  void barrier() {
    std::unique_lock<std::mutex> lk(m);
    if (broken) throw Error(STC_ERR_STATE, "another member of the group failed");
    const uint64_t g = gen;
    if (++arrived == n) {
      arrived = 0;
      ++gen;
      cv.notify_all();
      return;
    }
    cv.wait(lk, [&] { return gen != g || broken; });
    if (broken && gen == g) throw Error(STC_ERR_STATE, "another member of the group failed");
  }
  void fail() {
    std::lock_guard<std::mutex> lk(m);
    broken = true;
    cv.notify_all();
  }
};

// the waits poll against STC_COLL_TIMEOUT_MS on a context with a communicator, and abort it on a timeout
void abort_comm(Ctx& c);
void wait_stream(Ctx& c, hipStream_t s);
void wait_event(Ctx& c, hipEvent_t e);
void coll_group_start(Ctx& c);
void coll_group_end(Ctx& c);
void coll_all_reduce(Ctx& c, void* buf, size_t count, ncclDataType_t t, hipStream_t s);
void coll_reduce_scatter(Ctx& c, const void* send, void* recv, size_t recvcount, ncclDataType_t t, hipStream_t s);
void coll_all_gather(Ctx& c, const void* send, void* recv, size_t sendcount, ncclDataType_t t, hipStream_t s);
void allreduce_host(Ctx& c, double* x, int64_t n);  // in place, a host array

}  // namespace stc
