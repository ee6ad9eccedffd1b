// group_common.h — what the one-process, N-device handles share (stc_group in group.hip, stc_em_group in
// em_group.hip): N contexts joined by one communicator (ncclCommInitAll over distinct devices; the in-process
// transport of collectives.h when every member shares one device), every call run on one host thread per member,
// the failure handling of those threads, and the sharding of a host CSR by contiguous row ranges.
#pragma once

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <exception>
#include <memory>
#include <thread>

#include "collectives.h"
#include "stc_handles.h"

namespace stc {

struct GroupBase {
  std::vector<stc_ctx*> ctx;
  std::unique_ptr<LocalColl> local;
  int transport = STC_TRANSPORT_NONE;  // how the members' collectives travel (stc_group_transport)
  bool threaded = false;               // run even a one-member call on its own host thread (STC_GROUP_RCCL)
  // RCCL fault handling: a member's failure sets `abort` (every member's waits then throw instead of waiting
  // on collectives the failed member never joins) and, after the call, aborts every member's communicator;
  // the group is then `broken`: every later call but destroy fails with STC_ERR_STATE
  std::atomic<bool> abort{false};
  bool broken = false;
  std::string broken_why;
  int n() const { return (int)ctx.size(); }
};

inline void member_ok(int rc) {
  if (rc != STC_OK) throw Error(rc, stc_last_error());
}
inline void require_usable(const GroupBase& g) {
  if (g.broken) throw Error(STC_ERR_STATE, "the group's RCCL communicator was aborted after a member failed (" +
                                               g.broken_why + "): destroy the group and create a new one");
}
// f(i) for every member on its own thread (device set); the first failure is rethrown here.
// In-process transport: a failure releases the members waiting in its barrier, and the group stays usable.
// RCCL: a failure sets the group's abort flag, so every member's next wait throws instead of waiting for a
// collective the failed member never enqueued; a member still blocked inside the runtime after a grace
// period (a copy queued behind such a collective) has its communicator aborted by this thread, which
// releases the collective's kernels; after the join every member's communicator is aborted and the group
// is broken (STC_ERR_STATE from then on; the group's destroy returns).
template <typename F>
void for_members(GroupBase& g, F f) {
  require_usable(g);
  const int n = g.n();
  const bool rccl = g.transport == STC_TRANSPORT_RCCL;
  std::vector<std::exception_ptr> err((size_t)n);
  std::mutex fm;
  std::condition_variable fcv;
  int first = -1;  // the member that failed first (the others may only report "another member failed")
  int running = n;
  auto run = [&](int i) {
    try {
      g.ctx[(size_t)i]->use();
      f(i);
    } catch (...) {
      err[(size_t)i] = std::current_exception();
      {
        std::lock_guard<std::mutex> lk(fm);
        if (first < 0) first = i;
      }
      if (g.local) g.local->fail();  // release the members waiting in a barrier
      if (rccl) g.abort.store(true);
    }
    std::lock_guard<std::mutex> lk(fm);
    --running;
    fcv.notify_all();
  };
  if (n == 1 && !g.threaded) {
    run(0);
  } else {
    std::vector<std::thread> th;
    th.reserve((size_t)n);
    for (int i = 0; i < n; ++i) th.emplace_back(run, i);
    if (rccl) {
      std::unique_lock<std::mutex> lk(fm);
      fcv.wait(lk, [&] { return running == 0 || first >= 0; });
      if (running > 0 && !fcv.wait_for(lk, std::chrono::seconds(5), [&] { return running == 0; }))
        for (auto* c : g.ctx) abort_comm(*c);  // members still blocked behind the failed member's collectives
    }
    for (auto& t : th) t.join();
  }
  if (g.local) {  // a failed call leaves the transport usable for the next one
    std::lock_guard<std::mutex> lk(g.local->m);
    g.local->broken = false;
    g.local->arrived = 0;
  }
  if (first >= 0) {
    if (rccl) {
      for (auto* c : g.ctx) {
        c->use();
        abort_comm(*c);
      }
      g.broken = true;
      try {
        std::rethrow_exception(err[(size_t)first]);
      } catch (const std::exception& e) {
        g.broken_why = "member " + std::to_string(first) + ": " + e.what();
      } catch (...) {
        g.broken_why = "member " + std::to_string(first);
      }
    }
    std::rethrow_exception(err[(size_t)first]);
  }
}

// One context per entry of device_ids, joined by the group's communicator.  Device rules: all distinct (RCCL)
// or all the same device (in-process).  Debug knob STC_GROUP_RCCL=1: a group of distinct devices — one device
// included — builds its RCCL communicator with ncclCommInitAll and drives every member from its own host
// thread: the one-JVM, N-GPU drop-in path (LDATraining.scala:7) exercised end to end on a one-GPU box, where
// no two-device communicator exists.  Returns whether that knob applies.  On a failure the contexts made so
// far stay in g.ctx for the caller to destroy.
inline bool open_members(GroupBase& g, const int* device_ids, int n_devices) {
  STC_REQUIRE(n_devices >= 1 && n_devices <= kMaxMembers, "1 <= n_devices <= 16");
  int nd = 0;
  HIP_CHECK(hipGetDeviceCount(&nd));
  bool same = true, distinct = true;
  for (int i = 0; i < n_devices; ++i) {
    STC_REQUIRE(device_ids[i] >= 0 && device_ids[i] < nd, "device index out of range");
    same &= device_ids[i] == device_ids[0];
    for (int j = 0; j < i; ++j) distinct &= device_ids[i] != device_ids[j];
  }
  STC_REQUIRE(same || distinct, "device_ids: all distinct (RCCL) or all the same device (in-process)");
  for (int i = 0; i < n_devices; ++i) {
    stc_ctx* c = nullptr;
    member_ok(stc_init(device_ids[i], &c));
    g.ctx.push_back(c);
  }
  const char* gr = getenv("STC_GROUP_RCCL");
  const bool rccl1 = gr && gr[0] == '1' && distinct;
  if (n_devices > 1 && same) {
    g.local = std::make_unique<LocalColl>(n_devices);
    g.transport = STC_TRANSPORT_IN_PROCESS;
  }
  if (n_devices > 1 || rccl1) {
    std::vector<ncclComm_t> comms((size_t)n_devices, nullptr);
    if (!g.local) {
      RCCL_CHECK(ncclCommInitAll(comms.data(), n_devices, device_ids));
      g.transport = STC_TRANSPORT_RCCL;
    }
    g.threaded = rccl1;
    for (int i = 0; i < n_devices; ++i) {
      g.ctx[(size_t)i]->comm = comms[(size_t)i];
      g.ctx[(size_t)i]->local = g.local.get();
      g.ctx[(size_t)i]->n_ranks = n_devices;
      g.ctx[(size_t)i]->rank = i;
    }
  }
  for (auto* c : g.ctx) c->abort_flag = &g.abort;
  return rccl1;
}
inline void close_members(GroupBase& g) {
  for (auto* c : g.ctx) {
    c->local = nullptr;
    (void)stc_destroy(c);
  }
  g.ctx.clear();
}

// contiguous row ranges of a host CSR, one per member, balanced by entries
inline std::vector<int64_t> shard_rows(const int64_t* indptr, int64_t rows, int n) {
  std::vector<int64_t> r0((size_t)n + 1, rows);
  r0[0] = 0;
  const int64_t nnz = indptr[rows];
  int64_t r = 0;
  for (int q = 1; q < n; ++q) {
    const int64_t target = (nnz * q + n - 1) / n;
    while (r < rows && indptr[r] < target) ++r;
    r0[(size_t)q] = std::max(r, r0[(size_t)q - 1]);
  }
  return r0;
}
// member i's rows [r0[i], r0[i+1]) of a host CSR uploaded to its device (indptr rebased)
inline stc_dcsr* upload_rows(stc_ctx* ctx, int64_t lo, int64_t hi, int64_t cols, const int64_t* indptr,
                             const int32_t* indices, const double* values, int dtype) {
  std::vector<int64_t> ip((size_t)(hi - lo + 1));
  for (int64_t r = lo; r <= hi; ++r) ip[(size_t)(r - lo)] = indptr[r] - indptr[lo];
  stc_dcsr* d = nullptr;
  member_ok(stc_dcsr_upload(ctx, hi - lo, cols, ip.data(), indices ? indices + indptr[lo] : nullptr,
                            values ? values + indptr[lo] : nullptr, dtype, &d));
  return d;
}

}  // namespace stc
