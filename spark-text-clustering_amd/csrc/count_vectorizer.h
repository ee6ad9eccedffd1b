// count_vectorizer.h — CountVectorizer / CountVectorizerModel on the device (count_vectorizer.hip): the
// vocabulary blob, its per-term counts and the hash table that maps a token to its index.  api.hip checks
// the ABI's pointers, uploads host tokens (padded as stc_tokens_upload does) and forwards here.
#pragma once

#include "stc_internal.h"

// CountVectorizerModel: term j is blob[term_off[j] .. term_off[j+1]), index = position
struct stc_cvm {
  stc::Ctx* ctx = nullptr;  // the context that made it; only it may read the buffers (checked at the ABI)
  int device = -1;          // for stc_cv_free, which may run after that context is gone
  int64_t n_terms = 0, n_bytes = 0;
  int hash_bits = 64;       // STC_CV_HASH_BITS at construction: the hash is masked to its low bits everywhere
  bool has_counts = false;  // fitted (count / df hold the corpus statistics) or made from a list (zeros)
  uint64_t table_mask = 0;  // table slots − 1 (a power of two ≥ 2 · n_terms: load ≤ 0.5)
  stc::DevBuf blob;         // uint8[n_bytes + kHashPad]
  stc::DevBuf term_off;     // int64[n_terms + 1]
  stc::DevBuf count, df;    // int64[n_terms]
  stc::DevBuf table;        // Slot[table_mask + 1]: term index (−1 = empty), length, first 16 bytes, blob offset
};

namespace stc {
namespace cv {

// tokens on the device: token t is utf8[off[t] .. off[t+1]) with off = off32 when given, else off64; the
// blob carries kHashPad bytes of padding; document d owns tokens [doc_off[d], doc_off[d+1])
struct TokView {
  const uint8_t* utf8 = nullptr;
  const int64_t* off64 = nullptr;
  const uint32_t* off32 = nullptr;
  int64_t n_tok = 0;
  const int64_t* doc_off = nullptr;  // nullptr for index_of
  int64_t n_docs = 0;
  int64_t max_doc = -1;  // the longest document's token count when the upload knows it, −1 otherwise
};

stc_cvm* fit(Ctx& c, const TokView& tk, int64_t vocab_size, double min_df, double max_df);
// host arrays in (the list is checked for duplicates on the device)
stc_cvm* from_vocabulary(Ctx& c, const uint8_t* utf8, int64_t n_bytes, const int64_t* term_off, int64_t n_terms);
void get(Ctx& c, const stc_cvm& m, uint8_t* utf8_out, int64_t* term_off_out, int64_t* count_out, int64_t* df_out);
void index_of(Ctx& c, const stc_cvm& m, const TokView& tk, int32_t* idx_out /* host, n_tok */);
void transform(Ctx& c, const stc_cvm& m, const TokView& tk, double min_tf, int binary, int value_dtype, DCsr& out);
void destroy(stc_cvm* m);

}  // namespace cv
}  // namespace stc
