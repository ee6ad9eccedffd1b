// api.hip — the core of the C ABI of libstc.so (include/stc.h): the last error, contexts and their communicator,
// device CSR matrices, and the host-side checks every entry point shares (stc_handles.h).  The rest of the ABI lives
// with its subsystem: features_api.hip, lda_online.hip, lda_em.hip, count_vectorizer.hip, text_prep.hip, group.hip.
#include <algorithm>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <unordered_set>

#include "collectives.h"
#include "stc_handles.h"

using namespace stc;

static thread_local std::string g_last_error;
void stc::set_last_error(const std::string& msg) { g_last_error = msg; }

int64_t stc::check_offsets(const char* name, const int64_t* off, int64_t n, int64_t total, const char* total_name,
                           bool spans) {
  const std::string nm(name);
  if (spans) STC_REQUIRE(off[0] == 0 && off[n] == total, nm + " must span [0, " + total_name + "]");
  else STC_REQUIRE(off[0] == 0 && off[n] <= total, nm + " must start at 0 and stay within " + total_name);
  int64_t gap = 0;
  for (int64_t i = 0; i < n; ++i) {
    STC_REQUIRE(off[i + 1] >= off[i], nm + " must be non-decreasing");
    gap = std::max(gap, off[i + 1] - off[i]);
  }
  return gap;
}

int64_t stc::check_host_csr(int64_t rows, int64_t cols, const int64_t* indptr, const int32_t* indices,
                            const double* values) {
  STC_REQUIRE(indptr && rows >= 0, "indptr / rows");
  STC_REQUIRE(indptr[rows] == 0 || (indices && values), "indices / values");
  STC_REQUIRE(rows >= 0 && cols > 0, "csr: rows >= 0 and cols > 0");
  STC_REQUIRE(cols <= (int64_t(1) << 31), "csr: at most 2^31 columns");
  STC_REQUIRE(indptr[0] == 0, "csr: indptr[0] must be 0");
  const int64_t nnz = indptr[rows];
  const int64_t max_row = check_offsets("csr: indptr", indptr, rows, nnz, "nnz", true);
  for (int64_t e = 0; e < nnz; ++e)
    STC_REQUIRE(indices[e] >= 0 && (int64_t)indices[e] < cols, "csr: column index out of range");
  return max_row;
}

// the contexts that exist (a freed matrix or model hands its buffers back only to a live one)
static std::mutex g_live_mu;
static std::unordered_set<stc_ctx*> g_live;

void stc::recycle_to(Ctx* ctx, int device, std::initializer_list<DevBuf*> bufs) {
  if (device >= 0) (void)hipSetDevice(device);
  // every queued reader first — the context's stream and any other (an LDA handle's side stream sampling
  // from this corpus): a recycled buffer is rewritten by the next taker, so the implicit device
  // synchronisation hipFree gives is kept — outside the process-wide lock, so frees and
  // creates in other threads (a group's members, other devices) do not queue behind this drain
  if (device >= 0) (void)hipDeviceSynchronize();
  std::lock_guard<std::mutex> lk(g_live_mu);
  if (!ctx || !g_live.count(static_cast<stc_ctx*>(ctx)) || ctx->device != device) return;
  for (DevBuf* b : bufs) ctx->recycle.put(*b);
}

extern "C" {

const char* stc_last_error(void) { return g_last_error.c_str(); }
int stc_abi_version(void) { return STC_ABI_VERSION; }

int stc_device_count(int* n_out) {
  return guard([&] {
    STC_REQUIRE(n_out, "n_out");
    int n = 0;
    HIP_CHECK(hipGetDeviceCount(&n));
    *n_out = n;
  });
}

int stc_init(int device, stc_ctx** out) {
  return guard([&] {
    STC_REQUIRE(out, "out");
    int n = 0;
    HIP_CHECK(hipGetDeviceCount(&n));
    STC_REQUIRE(device >= 0 && device < n, "device index out of range");
    auto c = std::make_unique<stc_ctx>();
    c->device = device;
    HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIP_CHECK(hipDeviceGetAttribute(&c->cus, hipDeviceAttributeMultiprocessorCount, device));
    {
      std::lock_guard<std::mutex> lk(g_live_mu);
      g_live.insert(c.get());
    }
    const char* tm = std::getenv("STC_TF_MODE");  // A/B knob: "0" HashingTF's sorted-key passes (stc_internal.h Ctx)
    c->tf_single_pass = !(tm && tm[0] == '0' && tm[1] == 0);
    const char* tf = std::getenv("STC_TF_FAULT");  // test knob
    c->tf_force_fault = tf && tf[0] == '1';
    const char* ct = std::getenv("STC_COLL_TIMEOUT_MS");  // the deadline of a wait behind RCCL collectives
    if (ct && std::atoll(ct) > 0) c->coll_timeout_ms = std::atoll(ct);
    const char* nc = std::getenv("STC_IDF_NO_CACHE");  // A/B knob: plain idf gathers in the transform
    c->idf_cache = !(nc && nc[0] == '1');
    *out = c.release();
  });
}

int stc_destroy(stc_ctx* ctx) {
  return guard([&] {
    if (!ctx) return;
    {
      std::lock_guard<std::mutex> lk(g_live_mu);
      g_live.erase(ctx);
    }
    (void)hipSetDevice(ctx->device);
    // an aborted communicator is already freed; a live one is destroyed (a group's members first settle
    // their streams in stc_group_destroy, so nothing of it is still queued)
    if (ctx->comm && !ctx->comm_aborted.load()) (void)ncclCommDestroy(ctx->comm);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
  });
}

int stc_synchronize(stc_ctx* ctx) {
  return guard([&] {
    STC_REQUIRE(ctx, "ctx");
    ctx->use();
    wait_stream(*ctx, ctx->stream);
  });
}

int stc_comm_unique_id(uint8_t id_out[128]) {
  return guard([&] {
    STC_REQUIRE(id_out, "id_out");
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    ncclUniqueId id;
    RCCL_CHECK(ncclGetUniqueId(&id));
    std::memcpy(id_out, &id, 128);
  });
}

int stc_comm_init(stc_ctx* ctx, const uint8_t id[128], int n_ranks, int rank) {
  return guard([&] {
    STC_REQUIRE(ctx && id, "ctx/id");
    STC_REQUIRE(n_ranks >= 1 && rank >= 0 && rank < n_ranks, "rank / n_ranks");
    STC_REQUIRE(!ctx->comm, "communicator already initialised");
    ctx->use();
    ncclUniqueId uid;
    std::memcpy(&uid, id, 128);
    RCCL_CHECK(ncclCommInitRank(&ctx->comm, n_ranks, uid, rank));
    ctx->n_ranks = n_ranks;
    ctx->rank = rank;
  });
}

int stc_comm_allreduce_f64(stc_ctx* ctx, double* host_inout, int64_t n) {
  return guard([&] {
    STC_REQUIRE(ctx && (host_inout || n == 0), "ctx/host_inout");
    ctx->use();
    allreduce_host(*ctx, host_inout, n);
  });
}

int stc_dcsr_upload(stc_ctx* ctx, int64_t n_rows, int64_t n_cols, const int64_t* indptr,
                    const int32_t* indices, const double* values, int value_dtype, stc_dcsr** out) {
  return guard([&] {
    STC_REQUIRE(ctx && indptr && out, "ctx/indptr/out");
    STC_REQUIRE(value_dtype == STC_F32 || value_dtype == STC_F64, "value_dtype");
    const int64_t nnz = indptr[n_rows];
    STC_REQUIRE(nnz == 0 || (indices && values), "indices/values");
    const int64_t max_row = check_host_csr(n_rows, n_cols, indptr, indices, values);
    ctx->use();
    auto m = new_handle<stc_dcsr>(*ctx);
    m->rows = n_rows;
    m->cols = n_cols;
    m->nnz = nnz;
    m->dtype = value_dtype;
    m->max_row = max_row;
    ctx->recycle.take(m->indptr, 8 * (n_rows + 1));
    ctx->recycle.take(m->indices, 4 * std::max<int64_t>(nnz, 1));
    ctx->recycle.take(m->values, (value_dtype == STC_F32 ? 4 : 8) * std::max<int64_t>(nnz, 1));
    HIP_CHECK(hipMemcpyAsync(m->indptr.p, indptr, 8 * (n_rows + 1), hipMemcpyHostToDevice, ctx->stream));
    if (nnz > 0) {
      HIP_CHECK(hipMemcpyAsync(m->indices.p, indices, 4 * nnz, hipMemcpyHostToDevice, ctx->stream));
      if (value_dtype == STC_F64) {
        HIP_CHECK(hipMemcpyAsync(m->values.p, values, 8 * nnz, hipMemcpyHostToDevice, ctx->stream));
        wait_stream(*ctx, ctx->stream);
      } else {
        std::vector<float> f((size_t)nnz);
        for (int64_t e = 0; e < nnz; ++e) f[(size_t)e] = (float)values[e];
        HIP_CHECK(hipMemcpyAsync(m->values.p, f.data(), 4 * nnz, hipMemcpyHostToDevice, ctx->stream));
        wait_stream(*ctx, ctx->stream);
      }
    }
    wait_stream(*ctx, ctx->stream);
    *out = m.release();
  });
}

int stc_dcsr_shape(const stc_dcsr* m, int64_t* n_rows, int64_t* n_cols, int64_t* nnz) {
  return guard([&] {
    STC_REQUIRE(m, "m");
    if (n_rows) *n_rows = m->rows;
    if (n_cols) *n_cols = m->cols;
    if (nnz) *nnz = m->nnz;
  });
}

int stc_dcsr_download(stc_ctx* ctx, const stc_dcsr* m, int64_t* indptr, int32_t* indices, double* values) {
  return guard([&] {
    STC_REQUIRE(ctx && m, "ctx/m");
    STC_REQUIRE(m->ctx == ctx, "the matrix belongs to another stc_ctx");
    ctx->use();
    hipStream_t s = ctx->stream;
    if (indptr) HIP_CHECK(hipMemcpyAsync(indptr, m->indptr.p, 8 * (m->rows + 1), hipMemcpyDeviceToHost, s));
    if (indices && m->nnz) HIP_CHECK(hipMemcpyAsync(indices, m->indices.p, 4 * m->nnz, hipMemcpyDeviceToHost, s));
    if (values && m->nnz) {
      if (m->dtype == STC_F64) {
        HIP_CHECK(hipMemcpyAsync(values, m->values.p, 8 * m->nnz, hipMemcpyDeviceToHost, s));
      } else {
        std::vector<float> f((size_t)m->nnz);
        HIP_CHECK(hipMemcpyAsync(f.data(), m->values.p, 4 * m->nnz, hipMemcpyDeviceToHost, s));
        wait_stream(*ctx, s);
        for (int64_t e = 0; e < m->nnz; ++e) values[e] = f[(size_t)e];
      }
    }
    wait_stream(*ctx, s);
  });
}

int stc_dcsr_free(stc_dcsr* m) {
  return guard([&] {
    if (!m) return;
    recycle_to(m->ctx, m->device, {&m->indices, &m->values, &m->indptr});
    delete m;
  });
}

}  // extern "C"
