// features_api.hip — the featurisation entry points of the C ABI (include/stc.h): token upload, HashingTF,
// Tokenizer and IDF.  They check the caller's arrays, move them to the device and run the kernels of
// hashing_tf.hip, tokenizer.hip and idf.hip.
#include <algorithm>

#include "collectives.h"
#include "stc_handles.h"

using namespace stc;

// ---- HashingTF ------------------------------------------------------------------------
void stc::upload_tokens(Ctx& c, TokenUpload& u, const uint8_t* utf8, int64_t n_bytes, const int64_t* tok_off,
                        int64_t n_tok, const int64_t* doc_off, int64_t n_docs) {
  STC_REQUIRE(n_bytes >= 0 && n_tok >= 0 && n_docs >= 0, "sizes must be >= 0");
  STC_REQUIRE(tok_off && (n_bytes == 0 || utf8), "utf8/tok_off");
  check_offsets("tok_off", tok_off, n_tok, n_bytes, "n_bytes", false);
  if (doc_off) u.max_doc = check_offsets("doc_off", doc_off, n_docs, n_tok, "n_tok", true);
  u.utf8.reserve(n_bytes + kHashPad);  // the hash reads 32-byte windows of whole aligned dwords
  u.tok_off.reserve(8 * (n_tok + 1));
  if (n_bytes) HIP_CHECK(hipMemcpyAsync(u.utf8.p, utf8, n_bytes, hipMemcpyHostToDevice, c.stream));
  HIP_CHECK(hipMemcpyAsync(u.tok_off.p, tok_off, 8 * (n_tok + 1), hipMemcpyHostToDevice, c.stream));
  if (doc_off) {
    u.doc_off.reserve(8 * (n_docs + 1));
    HIP_CHECK(hipMemcpyAsync(u.doc_off.p, doc_off, 8 * (n_docs + 1), hipMemcpyHostToDevice, c.stream));
  }
}

struct stc_didf {
  Ctx* ctx = nullptr;
  int device = -1;
  int64_t cols = 0, m = 0;
  DevBuf idf, df;
  DevBuf cache;  // the hot-idf table of idf.hip k_transform_cached (empty: not used)
};

namespace {
// IDF.fit on the device: df (all ranks' when connected), m, idf into the given buffers
void idf_fit_impl(Ctx& c, const DCsr& tf, int64_t min_doc_freq, DevBuf& df, DevBuf& idf, int64_t& m) {
  hipStream_t s = c.stream;
  c.recycle.take(df, 8 * tf.cols);
  c.recycle.take(idf, 8 * tf.cols);
  m = tf.rows;
  if (!c.coll()) {  // m known: idf written by the df reduction itself
    const idf::IdfFinal fin{(double)m, min_doc_freq, idf.as<double>()};
    if (idf::doc_freq(c, tf, df.as<int64_t>(), &fin)) return;
    idf::finalize(c, df.as<int64_t>(), tf.cols, m, min_doc_freq, idf.as<double>());
    return;
  }
  idf::doc_freq(c, tf, df.as<int64_t>());
  {  // DocumentFrequencyAggregator.merge over ranks
    DevBuf mm;
    mm.reserve(8);
    HIP_CHECK(hipMemcpyAsync(mm.p, &m, 8, hipMemcpyHostToDevice, s));
    coll_group_start(c);
    coll_all_reduce(c, df.p, (size_t)tf.cols, ncclInt64, s);
    coll_all_reduce(c, mm.p, 1, ncclInt64, s);
    coll_group_end(c);
    HIP_CHECK(hipMemcpyAsync(&m, mm.p, 8, hipMemcpyDeviceToHost, s));
    wait_stream(c, s);
  }
  idf::finalize(c, df.as<int64_t>(), tf.cols, m, min_doc_freq, idf.as<double>());
}
}  // namespace

extern "C" {

int stc_tokens_upload(stc_ctx* ctx, const uint8_t* utf8, int64_t n_bytes, const int64_t* tok_off,
                      int64_t n_tok, const int64_t* doc_off, int64_t n_docs, stc_dtok** out) {
  return guard([&] {
    STC_REQUIRE(ctx && doc_off && out, "ctx/doc_off/out");
    ctx->use();
    auto t = new_handle<stc_dtok>(*ctx);
    TokenUpload u;
    upload_tokens(*ctx, u, utf8, n_bytes, tok_off, n_tok, doc_off, n_docs);
    wait_stream(*ctx, ctx->stream);
    swap(t->utf8, u.utf8);
    if (n_bytes + kHashPad <= (int64_t(1) << 32)) {  // u32 offsets: half the bytes HashingTF reads for them
      t->tok_off.reserve(4 * (n_tok + 1));
      hashing::narrow_offsets(*ctx, u.tok_off.as<int64_t>(), n_tok + 1, t->tok_off.as<uint32_t>());
      wait_stream(*ctx, ctx->stream);
      t->off32 = true;
    } else {
      swap(t->tok_off, u.tok_off);
    }
    swap(t->doc_off, u.doc_off);
    t->n_bytes = n_bytes;
    t->n_tok = n_tok;
    t->n_docs = n_docs;
    t->max_doc = u.max_doc;
    *out = t.release();
  });
}

int stc_tokens_free(stc_dtok* t) {
  return guard([&] {
    if (!t) return;
    if (t->device >= 0) (void)hipSetDevice(t->device);
    delete t;
  });
}

int stc_hashing_tf_tokens(stc_ctx* ctx, const stc_dtok* tokens, int32_t num_features, int binary,
                          int hash_variant, int value_dtype, stc_dcsr** out) {
  return guard([&] {
    STC_REQUIRE(ctx && tokens && out, "ctx/tokens/out");
    STC_REQUIRE(tokens->ctx == ctx, "tokens were uploaded on another stc_ctx");
    STC_REQUIRE(num_features > 0, "numFeatures must be > 0");
    STC_REQUIRE(hash_variant == STC_HASH_STANDARD || hash_variant == STC_HASH_SPARK24, "hash_variant");
    STC_REQUIRE(value_dtype == STC_F32 || value_dtype == STC_F64, "value_dtype");
    ctx->use();
    auto m = new_handle<stc_dcsr>(*ctx);
    hashing::build_csr(*ctx, tokens->utf8.as<uint8_t>(), tokens->off32 ? nullptr : tokens->tok_off.as<int64_t>(),
                       tokens->off32 ? tokens->tok_off.as<uint32_t>() : nullptr, tokens->n_tok,
                       tokens->doc_off.as<int64_t>(), tokens->n_docs, num_features, binary, hash_variant,
                       value_dtype, tokens->max_doc, *m);
    *out = m.release();
  });
}

int stc_hash_tokens(stc_ctx* ctx, const uint8_t* utf8, int64_t n_bytes, const int64_t* tok_off,
                    int64_t n_tok, int32_t num_features, int hash_variant, int32_t* idx_out) {
  return guard([&] {
    STC_REQUIRE(ctx && (idx_out || n_tok == 0), "ctx/idx_out");
    STC_REQUIRE(num_features > 0, "numFeatures must be > 0");
    STC_REQUIRE(hash_variant == STC_HASH_STANDARD || hash_variant == STC_HASH_SPARK24, "hash_variant");
    ctx->use();
    TokenUpload u;
    upload_tokens(*ctx, u, utf8, n_bytes, tok_off, n_tok, nullptr, 0);
    DevBuf out;
    out.reserve(4 * std::max<int64_t>(n_tok, 1));
    hashing::hash_tokens(*ctx, u.utf8.as<uint8_t>(), u.tok_off.as<int64_t>(), n_tok, num_features,
                         hash_variant, out.as<int32_t>());
    if (n_tok) HIP_CHECK(hipMemcpyAsync(idx_out, out.p, 4 * n_tok, hipMemcpyDeviceToHost, ctx->stream));
    wait_stream(*ctx, ctx->stream);
  });
}

int stc_hashing_tf_dev(stc_ctx* ctx, const uint8_t* utf8, int64_t n_bytes, const int64_t* tok_off,
                       int64_t n_tok, const int64_t* doc_off, int64_t n_docs, int32_t num_features,
                       int binary, int hash_variant, int value_dtype, stc_dcsr** out) {
  return guard([&] {
    STC_REQUIRE(ctx && doc_off && out, "ctx/doc_off/out");
    STC_REQUIRE(num_features > 0, "numFeatures must be > 0");
    STC_REQUIRE(hash_variant == STC_HASH_STANDARD || hash_variant == STC_HASH_SPARK24, "hash_variant");
    STC_REQUIRE(value_dtype == STC_F32 || value_dtype == STC_F64, "value_dtype");
    ctx->use();
    TokenUpload u;
    upload_tokens(*ctx, u, utf8, n_bytes, tok_off, n_tok, doc_off, n_docs);
    auto m = new_handle<stc_dcsr>(*ctx);
    hashing::build_csr(*ctx, u.utf8.as<uint8_t>(), u.tok_off.as<int64_t>(), nullptr, n_tok, u.doc_off.as<int64_t>(),
                       n_docs, num_features, binary, hash_variant, value_dtype, u.max_doc, *m);
    *out = m.release();
  });
}

int stc_hashing_tf(stc_ctx* ctx, const uint8_t* utf8, int64_t n_bytes, const int64_t* tok_off,
                   int64_t n_tok, const int64_t* doc_off, int64_t n_docs, int32_t num_features,
                   int binary, int hash_variant, int64_t* indptr_out, int32_t* indices_out,
                   double* values_out) {
  stc_dcsr* m = nullptr;
  int rc = stc_hashing_tf_dev(ctx, utf8, n_bytes, tok_off, n_tok, doc_off, n_docs, num_features,
                              binary, hash_variant, STC_F64, &m);
  if (rc != STC_OK) return rc;
  rc = stc_dcsr_download(ctx, m, indptr_out, indices_out, values_out);
  stc_dcsr_free(m);
  return rc;
}

// ---- Tokenizer (K0) ---------------------------------------------------------------------
namespace {
struct Tokens {
  DevBuf utf8, tok_off, doc_off;
  int64_t n_tok = 0, n_bytes = 0;
};
void run_tokenizer(Ctx& c, Tokens& t, const uint8_t* text, int64_t n_bytes, const int64_t* text_off,
                   int64_t n_docs) {
  STC_REQUIRE(n_bytes >= 0 && n_docs >= 0, "sizes must be >= 0");
  STC_REQUIRE(n_docs < (int64_t(1) << 31) - 1, "at most 2^31-2 documents per call");
  STC_REQUIRE(text_off && (n_bytes == 0 || text), "text/text_off");
  check_offsets("text_off", text_off, n_docs, n_bytes, "n_bytes", true);
  DevBuf d_text, d_off;
  d_text.reserve(n_bytes + 64);  // k_count reads whole aligned dwords past the last byte
  d_off.reserve(8 * (n_docs + 1));
  if (n_bytes) HIP_CHECK(hipMemcpyAsync(d_text.p, text, n_bytes, hipMemcpyHostToDevice, c.stream));
  HIP_CHECK(hipMemcpyAsync(d_off.p, text_off, 8 * (n_docs + 1), hipMemcpyHostToDevice, c.stream));
  tokenizer::tokenize(c, d_text.as<uint8_t>(), d_off.as<int64_t>(), n_docs, t.utf8, t.tok_off, t.doc_off,
                      t.n_tok, t.n_bytes);
}
}  // namespace

int stc_tokenize(stc_ctx* ctx, const uint8_t* text, int64_t n_bytes, const int64_t* text_off,
                 int64_t n_docs, uint8_t* utf8_out, int64_t utf8_cap, int64_t* n_out_bytes,
                 int64_t* tok_off_out, int64_t* n_tok_out, int64_t* doc_off_out) {
  return guard([&] {
    STC_REQUIRE(ctx && n_out_bytes, "ctx/n_out_bytes");
    STC_REQUIRE(utf8_cap >= 0, "utf8_cap must be >= 0");
    const bool query = utf8_out == nullptr;  // the size query: *n_out_bytes (and *n_tok_out) only
    STC_REQUIRE(query ? utf8_cap == 0 : (n_tok_out && tok_off_out && doc_off_out), "outputs");
    ctx->use();
    Tokens t;
    run_tokenizer(*ctx, t, text, n_bytes, text_off, n_docs);
    if (query) {
      *n_out_bytes = t.n_bytes;
      if (n_tok_out) *n_tok_out = t.n_tok;
      return;
    }
    // the lower-cased blob can outgrow the input (İ → i̇, Ⱥ → ⱥ: 2 → 3 bytes); its size is known from the
    // count pass, so a short buffer is refused before anything is copied (*n_out_bytes = the size needed)
    *n_out_bytes = t.n_bytes;
    if (t.n_bytes > utf8_cap)
      throw Error(STC_ERR_INVALID_ARG, "utf8_out holds " + std::to_string(utf8_cap) + " bytes, the lower-cased text needs " +
                                           std::to_string(t.n_bytes));
    hipStream_t s = ctx->stream;
    if (t.n_bytes) HIP_CHECK(hipMemcpyAsync(utf8_out, t.utf8.p, t.n_bytes, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(tok_off_out, t.tok_off.p, 8 * (t.n_tok + 1), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(doc_off_out, t.doc_off.p, 8 * (n_docs + 1), hipMemcpyDeviceToHost, s));
    wait_stream(*ctx, s);
    *n_out_bytes = t.n_bytes;
    *n_tok_out = t.n_tok;
  });
}

// the tokenizer's result turned into device tokens with the invariants of stc_tokens_upload
int stc_tokenize_tokens(stc_ctx* ctx, const uint8_t* text, int64_t n_bytes, const int64_t* text_off, int64_t n_docs,
                        stc_dtok** out) {
  return guard([&] {
    STC_REQUIRE(ctx && out, "ctx/out");
    if (ctx->coll()) throw Error(STC_ERR_STATE, "token stages: the context is connected to other ranks (the token stages are single-device)");
    ctx->use();
    hipStream_t s = ctx->stream;
    Tokens t;
    run_tokenizer(*ctx, t, text, n_bytes, text_off, n_docs);
    auto d = new_handle<stc_dtok>(*ctx);
    HIP_CHECK(hipMemsetAsync(t.utf8.as<uint8_t>() + t.n_bytes, 0, kHashPad, s));  // (reserved by the tokenizer)
    if (t.n_bytes + kHashPad <= (int64_t(1) << 32)) {
      d->tok_off.reserve(4 * (t.n_tok + 1));
      hashing::narrow_offsets(*ctx, t.tok_off.as<int64_t>(), t.n_tok + 1, d->tok_off.as<uint32_t>());
      d->off32 = true;
    } else {
      swap(d->tok_off, t.tok_off);
    }
    d->max_doc = stages::longest_doc(*ctx, t.doc_off.as<int64_t>(), n_docs);  // (waits for the stream)
    swap(d->utf8, t.utf8);
    swap(d->doc_off, t.doc_off);
    d->n_bytes = t.n_bytes;
    d->n_tok = t.n_tok;
    d->n_docs = n_docs;
    *out = d.release();
  });
}

int stc_tokenize_hashing_tf_dev(stc_ctx* ctx, const uint8_t* text, int64_t n_bytes,
                                const int64_t* text_off, int64_t n_docs, int32_t num_features,
                                int binary, int hash_variant, int value_dtype, stc_dcsr** out) {
  return guard([&] {
    STC_REQUIRE(ctx && out, "ctx/out");
    STC_REQUIRE(num_features > 0, "numFeatures must be > 0");
    STC_REQUIRE(hash_variant == STC_HASH_STANDARD || hash_variant == STC_HASH_SPARK24, "hash_variant");
    STC_REQUIRE(value_dtype == STC_F32 || value_dtype == STC_F64, "value_dtype");
    ctx->use();
    Tokens t;
    run_tokenizer(*ctx, t, text, n_bytes, text_off, n_docs);
    auto m = new_handle<stc_dcsr>(*ctx);
    hashing::build_csr(*ctx, t.utf8.as<uint8_t>(), t.tok_off.as<int64_t>(), nullptr, t.n_tok, t.doc_off.as<int64_t>(),
                       n_docs, num_features, binary, hash_variant, value_dtype, -1, *m);
    *out = m.release();
  });
}

// ---- IDF --------------------------------------------------------------------------------
int stc_idf_fit(stc_ctx* ctx, const stc_dcsr* tf, int64_t min_doc_freq, double* idf_out,
                int64_t* df_out, int64_t* m_out) {
  return guard([&] {
    STC_REQUIRE(ctx && tf && idf_out, "ctx/tf/idf_out");
    STC_REQUIRE(tf->ctx == ctx, "the matrix belongs to another stc_ctx");
    STC_REQUIRE(min_doc_freq >= 0, "minDocFreq must be >= 0");
    ctx->use();
    hipStream_t s = ctx->stream;
    DevBuf& df = ctx->scratch[9];  // grow-only on the context: no per-call allocation
    DevBuf& idf = ctx->scratch[10];
    int64_t m = 0;
    idf_fit_impl(*ctx, *tf, min_doc_freq, df, idf, m);
    HIP_CHECK(hipMemcpyAsync(idf_out, idf.p, 8 * tf->cols, hipMemcpyDeviceToHost, s));
    if (df_out) HIP_CHECK(hipMemcpyAsync(df_out, df.p, 8 * tf->cols, hipMemcpyDeviceToHost, s));
    wait_stream(*ctx, s);
    if (m_out) *m_out = m;
  });
}

int stc_idf_fit_dev(stc_ctx* ctx, const stc_dcsr* tf, int64_t min_doc_freq, stc_didf** out) {
  return guard([&] {
    STC_REQUIRE(ctx && tf && out, "ctx/tf/out");
    STC_REQUIRE(tf->ctx == ctx, "the matrix belongs to another stc_ctx");
    STC_REQUIRE(min_doc_freq >= 0, "minDocFreq must be >= 0");
    ctx->use();
    auto md = new_handle<stc_didf>(*ctx);
    md->cols = tf->cols;
    idf_fit_impl(*ctx, *tf, min_doc_freq, md->df, md->idf, md->m);
    idf::build_cache(*ctx, md->df.as<int64_t>(), md->idf.as<double>(), md->cols, md->cache);
    *out = md.release();  // (the stream orders every later use of the model after the fit)
  });
}

int stc_idf_get(stc_ctx* ctx, const stc_didf* md, double* idf_out, int64_t* df_out, int64_t* m_out) {
  return guard([&] {
    STC_REQUIRE(ctx && md, "ctx/model");
    STC_REQUIRE(md->ctx == ctx, "the model belongs to another stc_ctx");
    ctx->use();
    hipStream_t s = ctx->stream;
    if (idf_out) HIP_CHECK(hipMemcpyAsync(idf_out, md->idf.p, 8 * md->cols, hipMemcpyDeviceToHost, s));
    if (df_out) HIP_CHECK(hipMemcpyAsync(df_out, md->df.p, 8 * md->cols, hipMemcpyDeviceToHost, s));
    wait_stream(*ctx, s);
    if (m_out) *m_out = md->m;
  });
}

int stc_didf_shape(const stc_didf* md, int64_t* cols_out, int64_t* m_out) {
  return guard([&] {
    STC_REQUIRE(md, "model");
    if (cols_out) *cols_out = md->cols;
    if (m_out) *m_out = md->m;
  });
}

int stc_idf_transform_dev(stc_ctx* ctx, stc_dcsr* tf, const stc_didf* md, double zero_floor) {
  return guard([&] {
    STC_REQUIRE(ctx && tf && md, "ctx/tf/model");
    STC_REQUIRE(tf->ctx == ctx && md->ctx == ctx, "the matrix or model belongs to another stc_ctx");
    STC_REQUIRE(tf->cols == md->cols, "vector size does not match the IDF size");
    STC_REQUIRE(zero_floor >= 0.0, "zero_floor must be >= 0");
    ctx->use();
    idf::transform(*ctx, *tf, md->idf.as<double>(), zero_floor, &md->cache);
    wait_stream(*ctx, ctx->stream);
  });
}

int stc_didf_free(stc_didf* md) {
  return guard([&] {
    if (!md) return;
    recycle_to(md->ctx, md->device, {&md->idf, &md->df});
    delete md;
  });
}

int stc_idf_transform(stc_ctx* ctx, stc_dcsr* tf, const double* idf, double zero_floor) {
  return guard([&] {
    STC_REQUIRE(ctx && tf && idf, "ctx/tf/idf");
    STC_REQUIRE(tf->ctx == ctx, "the matrix belongs to another stc_ctx");
    STC_REQUIRE(zero_floor >= 0.0, "zero_floor must be >= 0");
    ctx->use();
    DevBuf& d = ctx->scratch[11];
    d.reserve(8 * tf->cols);
    HIP_CHECK(hipMemcpyAsync(d.p, idf, 8 * tf->cols, hipMemcpyHostToDevice, ctx->stream));
    idf::transform(*ctx, *tf, d.as<double>(), zero_floor);
    wait_stream(*ctx, ctx->stream);
  });
}

}  // extern "C"
