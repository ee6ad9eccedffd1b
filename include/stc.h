/*
 * stc.h — the C ABI of libstc.so, the MI355X-native text-clustering hot path.
 *
 * This is the drop-in boundary: the entry points a JNI shim binds so that
 * the reference's Spark pipeline can route its hot path to HIP kernels on gfx950.  Plain C
 * types only (pointers + sizes); no torch, no C++ in the signatures.
 *
 * Which reference interface each entry point replaces ([U] = upstream spark-mllib 2.4.3,
 * TextClustering/build.sbt:10; paths relative to /root/reference/TextClustering/src/main/scala):
 *
 *   stc_tokenize[_hashing_tf_dev] [U] ml.feature.Tokenizer (toLowerCase.split("\\s")), the step in
 *                               front of HashingTF (the reference's own
 *                               CoreNLP lemmatiser at LDAClustering.scala:116-120 is out of scope)
 *   stc_prep_*                  the reference's own steps behind that lemmatiser: LDAUtil.filterSpecialCharacters,
 *                               OpenNLP SimpleTokenizer, the stop-word filter and OpenNLP PorterStemmer —
 *                               LDAClustering.scala:121-139 (training), :221-238 (scoring)
 *   stc_swr_*, stc_ngram_tokens [U] ml.feature.StopWordsRemover and ml.feature.NGram, the stages a Spark pipeline puts
 *                               between its tokenizer and its vectorizer (device tokens in and out);
 *                               stc_tokenize_tokens is the Tokenizer feeding them
 *   stc_hashing_tf[_dev]        [U] mllib.feature.HashingTF.transform / murmur3Hash — the slot of
 *                               the vocab-indexed counting at LDAClustering.scala:154-167
 *   stc_cv_*                    [U] ml.feature.CountVectorizer / CountVectorizerModel — the vocabulary-indexed
 *                               counting itself: fit at LDAClustering.scala:143-171, the saved vocabulary's
 *                               lookup + counts at LDALoader.scala:83-105
 *   stc_idf_fit                 IDF(minDocFreq).fit(tf).idf — LDAClustering.scala:177
 *   stc_idf_transform           tf × idf (+ the 0 → 1e-4 floor) — LDAClustering.scala:180-192
 *   stc_lda_create / set_corpus new LDA().setOptimizer(online)...setK... — LDAClustering.scala:37-54
 *                               ([U] OnlineLDAOptimizer.initialize)
 *   stc_lda_next / stc_lda_step one OnlineLDAOptimizer.next() / submitMiniBatch inside
 *                               lda.run(corpus) — LDAClustering.scala:61
 *   stc_lda_get_topics          [U] LocalLDAModel.topicsMatrix (getLDAModel)
 *   stc_lda_describe            ldaModel.describeTopics(maxTermsPerTopic) — LDAClustering.scala:81,
 *                               LDALoader.scala:66
 *   stc_lda_topic_distribution  toLocal.topicDistribution(tf) — LDALoader.scala:108
 *   stc_lda_score, stc_score_*  the report LDALoader writes from those proportions: the main topic —
 *                               LDALoader.scala:131-140, the books of each topic — :142-149, and the
 *                               ranked lists a report adds (topTopicsPerDocument / topDocumentsPerTopic)
 *   stc_lda_important_terms     "Book most important words" — LDALoader.scala:86-94 (the book's tokens by
 *                               count), :154-163 (the first 100 ∩ the main topic's 300 terms, the first 10)
 *   stc_term_cooccurrence,      the number behind the reference's one quality check, a person reading each topic's
 *   stc_coherence               top terms — LDALoader.scala:66-69, 177-187: UMass / NPMI topic coherence
 *   stc_lda_bound               [U] LocalLDAModel.logLikelihood / logPerplexity
 *   stc_em_*                    [U] EMLDAOptimizer, the reference's default optimizer ("em", Params.scala:9) —
 *                               LDAClustering.scala:41; stc_em_log_likelihood is
 *                               DistributedLDAModel.logLikelihood / logPrior — LDAClustering.scala:75
 *   stc_em_topic_assignments    [U] DistributedLDAModel.topicAssignments (the model LDALoader.scala:37 loads)
 *   stc_em_group_*              the same optimizer over the node's GPUs from one process: documents sharded
 *                               as Spark partitions them, the term side summed (its aggregateMessages)
 *   stc_comm_*                  the role of Spark's broadcast + treeReduce inside lda.run
 *                               (per minibatch: RCCL reduce-scatter of the k×V sstats over
 *                               vocabulary slices, the slice's λ update, all-gather of expElogβ)
 *
 * Conventions
 *   - Every function returns STC_OK (0) or an STC_ERR_* code; the message of the last failure on
 *     the calling thread is returned by stc_last_error().  The library never aborts.
 *   - The caller owns every host array; output arrays are caller-allocated with the sizes given
 *     in each comment.  The library owns all device memory behind the opaque handles.
 *   - A handle is not thread-safe: serialise calls per handle.  One stc_ctx = one GPU.  Several
 *     GPUs are driven either from ONE process through an stc_group (one handle, N devices, one
 *     host thread per member inside each group call — the JVM drop-in's form, Spark local[*]), or
 *     by one process per GPU whose contexts are connected with stc_comm_init.
 *   - Matrices are row-major.  The topics matrix crosses the boundary as V×k (Spark's
 *     topicsMatrix orientation, element (v, t) at [v*k + t]) unless a KV layout flag is given.
 */
#ifndef STC_H_
#define STC_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STC_ABI_VERSION 2  /* 2: stc_lda_config.mixed_resolve_iters, STC_MIXED */

enum stc_status {
  STC_OK = 0,
  STC_ERR_INVALID_ARG = 1, /* maps to IllegalArgumentException on the JVM side */
  STC_ERR_HIP = 2,         /* HIP runtime error (IllegalStateException) */
  STC_ERR_RCCL = 3,        /* RCCL error */
  STC_ERR_OOM = 4,         /* device allocation failed */
  STC_ERR_STATE = 5        /* call not valid in the handle's current state */
};

/* The reference pins spark-mllib 2.4.3 (TextClustering/build.sbt:10), whose HashingTF hashes with the
 * legacy tail: callers reproducing the reference's pipeline pass STC_HASH_SPARK24 (the Python mirror's
 * default, stc.HashingTF(hashAlgorithm="murmur3-spark24")).  The two agree iff len % 4 == 0. */
enum stc_hash_variant {
  STC_HASH_STANDARD = 0, /* MurmurHash3_x86_32 (Spark 3.x hashUnsafeBytes2) */
  STC_HASH_SPARK24 = 1   /* Spark 2.4.x hashUnsafeBytes: per-byte sign-extended tail */
};

enum stc_dtype {
  STC_F32 = 0,
  STC_F64 = 1,
  /* an LDA dtype only (stc_lda_config.dtype; the corpus CSR is STC_F64): the fp32 E-step for every document,
   * then the documents whose fp32 fixed point took more than mixed_resolve_iters iterations — the slowly
   * contracting ones, where fp32 rounding moves the stopping iterate — re-solved from the same γ₀ in fp64
   * (expElogβ' kept in both precisions); sstats, stat and the expElogβ' the E-step reads in fp32, λ / α /
   * colsum / the bound in fp64.  Inference (bound, topicDistribution) runs in fp64. */
  STC_MIXED = 2
};

enum stc_layout {
  STC_LAYOUT_VK = 0, /* V×k row-major: topicsMatrix(v, t) at [v*k + t] */
  STC_LAYOUT_KV = 1  /* k×V row-major: Spark's internal λ / a column-major topicsMatrix */
};

typedef struct stc_ctx stc_ctx;   /* one device (+ optional RCCL communicator) */
typedef struct stc_dcsr stc_dcsr; /* device-resident CSR matrix (rows = documents) */
typedef struct stc_lda stc_lda;   /* online-LDA optimizer state / LocalLDAModel */

/* ---- library / device ------------------------------------------------------------------ */
const char* stc_last_error(void);
int stc_abi_version(void);
int stc_device_count(int* n_out);
int stc_init(int device, stc_ctx** out);
int stc_destroy(stc_ctx* ctx);
int stc_synchronize(stc_ctx* ctx);

/* ---- RCCL: one process per GPU ---------------------------------------------------------
 * Rank 0 calls stc_comm_unique_id and ships the 128 bytes to the other ranks out of band
 * (the Spark driver broadcast, or torch.distributed's store); every rank then calls
 * stc_comm_init.  Once connected, stc_idf_fit, stc_lda_step/next and stc_lda_bound reduce
 * their partial results over all ranks (RCCL over xGMI), and the M-step is sharded: each rank
 * updates λ on its vocabulary slice, so the λ readers stc_lda_get_topics / stc_lda_describe
 * become collective too (every rank calls them; the first after a step all-gathers λ).
 * Connect before stc_lda_create (a later connect re-lays the model out before the next step). */
int stc_comm_unique_id(uint8_t id_out[128]);
int stc_comm_init(stc_ctx* ctx, const uint8_t id[128], int n_ranks, int rank);
int stc_comm_allreduce_f64(stc_ctx* ctx, double* host_inout, int64_t n); /* host scalars */

/* ---- device CSR ------------------------------------------------------------------------- */
/* values are stored on device as `value_dtype` (STC_F32 or STC_F64).  A device object (stc_dcsr,
 * stc_dtok) belongs to the stc_ctx that made it: every call that reads it requires that same ctx (or an
 * LDA handle created on it) and returns STC_ERR_INVALID_ARG otherwise.  The *_free calls remember the
 * device, not the ctx, so they remain valid after stc_destroy of the owning context. */
int stc_dcsr_upload(stc_ctx* ctx, int64_t n_rows, int64_t n_cols, const int64_t* indptr,
                    const int32_t* indices, const double* values, int value_dtype,
                    stc_dcsr** out);
int stc_dcsr_shape(const stc_dcsr* m, int64_t* n_rows, int64_t* n_cols, int64_t* nnz);
/* indptr[n_rows+1], indices[nnz], values[nnz] (any may be NULL to skip) */
int stc_dcsr_download(stc_ctx* ctx, const stc_dcsr* m, int64_t* indptr, int32_t* indices,
                      double* values);
/* Waits for the device to finish queued work, then hands the buffers back to the owning context for
 * reuse.  Detach a training corpus from every stc_lda (stc_lda_set_corpus with another matrix, or
 * stc_lda_destroy) before freeing it: the handle keeps a reference. */
int stc_dcsr_free(stc_dcsr* m);

/* ---- HashingTF (K1 murmur3 + nonNegativeMod, K2 per-doc count → sorted CSR) -----------
 * Tokens are given as one UTF-8 byte blob: token t is utf8[tok_off[t] .. tok_off[t+1]),
 * document d owns tokens [doc_off[d], doc_off[d+1]).  Output row d holds the sorted distinct
 * bucket indices nonNegativeMod(murmur3_x86_32(token, seed 42), num_features) and their
 * counts (1.0 when binary).  Bit-exact with [U] HashingTF.transform.                      */
int stc_hashing_tf_dev(stc_ctx* ctx, const uint8_t* utf8, int64_t n_bytes,
                       const int64_t* tok_off /* n_tok+1 */, int64_t n_tok,
                       const int64_t* doc_off /* n_docs+1 */, int64_t n_docs,
                       int32_t num_features, int binary, int hash_variant, int value_dtype,
                       stc_dcsr** out);
/* host-in/host-out convenience: indices_out/values_out need capacity n_tok */
int stc_hashing_tf(stc_ctx* ctx, const uint8_t* utf8, int64_t n_bytes, const int64_t* tok_off,
                   int64_t n_tok, const int64_t* doc_off, int64_t n_docs, int32_t num_features,
                   int binary, int hash_variant, int64_t* indptr_out /* n_docs+1 */,
                   int32_t* indices_out, double* values_out);
/* device-resident token input: the same (utf8, tok_off, doc_off) triple uploaded once, for callers that
 * keep the corpus on the GPU between calls (and for timing the kernels without the PCIe upload) */
typedef struct stc_dtok stc_dtok;
int stc_tokens_upload(stc_ctx* ctx, const uint8_t* utf8, int64_t n_bytes, const int64_t* tok_off,
                      int64_t n_tok, const int64_t* doc_off, int64_t n_docs, stc_dtok** out);
int stc_tokens_free(stc_dtok* t);
int stc_hashing_tf_tokens(stc_ctx* ctx, const stc_dtok* tokens, int32_t num_features, int binary,
                          int hash_variant, int value_dtype, stc_dcsr** out);
/* raw per-token bucket indices (test hook for K1): idx_out[n_tok] */
int stc_hash_tokens(stc_ctx* ctx, const uint8_t* utf8, int64_t n_bytes, const int64_t* tok_off,
                    int64_t n_tok, int32_t num_features, int hash_variant, int32_t* idx_out);

/* ---- CountVectorizer ([U] ml.feature.CountVectorizer → CountVectorizerModel) -----------------
 * Tokens in HashingTF's layout (utf8, tok_off, doc_off).  Two tokens are the same term iff their bytes are
 * equal; the empty string is a term like any other.
 * fit: for every distinct term, count = its occurrences and df = the documents holding it (n_docs counts
 * empty documents).  With minDf = min_df >= 1 ? min_df : min_df * n_docs and maxDf likewise (fp64, as Spark),
 * the terms with minDf <= df <= maxDf are ordered by count descending, then by their UTF-8 bytes ascending
 * (unsigned, a proper prefix first: Spark leaves ties to the partitioning, this fixes them so the vocabulary
 * does not depend on document order), and the first min(vocab_size, #terms) are kept.  Spark's defaults:
 * vocab_size 2^18, min_df 1.0, max_df 2^63-1.  STC_ERR_INVALID_ARG: vocab_size <= 0, a negative threshold,
 * maxDf < minDf, or nothing kept ("The vocabulary size should be > 0. Lower minDF as necessary.").
 * transform: row d holds, ascending, the indices of the vocabulary terms whose count c in document d is
 * >= (min_tf >= 1 ? min_tf : tokenCount_d * min_tf), tokenCount_d counting every token of the document, those
 * outside the vocabulary too; the value is c (1.0 when binary).  The matrix has n_terms columns and the
 * guarantees of a HashingTF output.  Spark's defaults: min_tf 1.0, binary 0.
 * At most 2^31-1 tokens per call.  Bitwise reproducible.  Single device: every call on a context connected
 * to other ranks returns STC_ERR_STATE.  Test knob: STC_CV_HASH_BITS=n (1..64, read when a model is made and
 * kept in it) masks the internal 64-bit term hash to its low n bits; no result depends on it. */
typedef struct stc_cvm stc_cvm; /* CountVectorizerModel on the device; belongs to its stc_ctx as an stc_dcsr does */
int stc_cv_fit(stc_ctx* ctx, const uint8_t* utf8, int64_t n_bytes, const int64_t* tok_off /* n_tok+1 */,
               int64_t n_tok, const int64_t* doc_off /* n_docs+1 */, int64_t n_docs, int64_t vocab_size,
               double min_df, double max_df, stc_cvm** out);
int stc_cv_fit_tokens(stc_ctx* ctx, const stc_dtok* tokens, int64_t vocab_size, double min_df, double max_df,
                      stc_cvm** out);
/* a model from a list of terms, index = position; a term given twice: STC_ERR_INVALID_ARG naming it */
int stc_cv_from_vocabulary(stc_ctx* ctx, const uint8_t* utf8, int64_t n_bytes,
                           const int64_t* term_off /* n_terms+1 */, int64_t n_terms, stc_cvm** out);
int stc_cv_shape(const stc_cvm* model, int64_t* n_terms_out, int64_t* n_bytes_out);
/* utf8_out[n_bytes], term_off_out[n_terms+1], count_out[n_terms], df_out[n_terms]; any may be NULL; count and
 * df are 0 for a model made from a list */
int stc_cv_get(stc_ctx* ctx, const stc_cvm* model, uint8_t* utf8_out, int64_t* term_off_out,
               int64_t* count_out, int64_t* df_out);
/* idx_out[n_tok]: each token's vocabulary index, -1 when it is not in the vocabulary */
int stc_cv_index_of(stc_ctx* ctx, const stc_cvm* model, const uint8_t* utf8, int64_t n_bytes,
                    const int64_t* tok_off, int64_t n_tok, int32_t* idx_out);
int stc_cv_transform_dev(stc_ctx* ctx, const stc_cvm* model, const uint8_t* utf8, int64_t n_bytes,
                         const int64_t* tok_off, int64_t n_tok, const int64_t* doc_off, int64_t n_docs,
                         double min_tf, int binary, int value_dtype, stc_dcsr** out);
int stc_cv_transform_tokens(stc_ctx* ctx, const stc_cvm* model, const stc_dtok* tokens, double min_tf,
                            int binary, int value_dtype, stc_dcsr** out);
/* waits for queued work, then frees the device memory (valid after stc_destroy of the context) */
int stc_cv_free(stc_cvm* model);

/* ---- Tokenizer (K0) ----------------------------------------------------------------------
 * Document d is the UTF-8 string text[text_off[d] .. text_off[d+1]).  Output: Spark's
 * Tokenizer result — lower-case, split on each Java \\s character ([ \t\n\x0B\f\r]), interior empty
 * tokens kept, trailing empty tokens dropped, a separator-free string is one token ("" → [""]) —
 * laid out as stc_hashing_tf's input: the separator-free lower-cased blob utf8_out (utf8_cap bytes;
 * n_bytes + n_bytes / 2 always suffices: lower-casing can grow a 2-byte character to 3 bytes — when the
 * text needs more than utf8_cap the call fails with STC_ERR_INVALID_ARG before writing any output and
 * *n_out_bytes holds the size needed), tok_off_out (capacity n_bytes + n_docs + 1) and doc_off_out[n_docs+1].
 * Size query: utf8_out = NULL with utf8_cap = 0 returns STC_OK with only *n_out_bytes (and *n_tok_out when
 * given) set; tok_off_out and doc_off_out may then be NULL.
 * Lower-casing is Java 8's String.toLowerCase (root locale, Unicode 6.2) for every code point: the BMP
 * through a generated table, Deseret inline, characters Java 8 does not case passed through, and the 18
 * code points whose mapping is not a same-length 1:1 map by rule: U+0130 İ → "i̇" (2 → 3 bytes), U+03A3 Σ
 * → ς / σ by its Final_Sigma context, and the capitals whose lower case changes UTF-8 length (U+023A,
 * U+023E, U+1E9E, U+2126, U+212A, U+212B, U+2C62, U+2C64, U+2C6D–U+2C70, U+2C7E, U+2C7F, U+A78D, U+A7AA). */
int stc_tokenize(stc_ctx* ctx, const uint8_t* text, int64_t n_bytes, const int64_t* text_off,
                 int64_t n_docs, uint8_t* utf8_out, int64_t utf8_cap, int64_t* n_out_bytes,
                 int64_t* tok_off_out, int64_t* n_tok_out, int64_t* doc_off_out);
/* Tokenizer → HashingTF fused on device (no host round trip between the two stages) */
int stc_tokenize_hashing_tf_dev(stc_ctx* ctx, const uint8_t* text, int64_t n_bytes,
                                const int64_t* text_off, int64_t n_docs, int32_t num_features,
                                int binary, int hash_variant, int value_dtype, stc_dcsr** out);

/* ---- Text preprocessing (the reference's own front end behind its lemmatiser) ---------------
 * filterSpecialCharacters → OpenNLP SimpleTokenizer → drop stop words → OpenNLP PorterStemmer, what the reference
 * runs on every book between CoreNLP's lemmatiser and the vocabulary (LDAClustering.scala:121-139, :221-238).  A
 * document is a UTF-8 string; a "char" is a Java char (a UTF-16 code unit; every BMP code point is one char).
 * 1. Strip.  A set of BMP code points counts as white space (the reference replaces each by one space, which
 *    yields the same tokens).  Default (strip_cp NULL, n_strip -1): what the regex class of
 *    LDAClustering.scala:283-284 denotes under java.util.regex — U+0020–U+002D (its trailing "' ' '-' '-'" is that
 *    range), . : ; ? @ ^ _ `, U+00AB, U+00BB, U+2019, U+201D, U+2212.  (U+201C, U+2018 and / are not in it.)
 * 2. SimpleTokenizer (OpenNLP 1.6.0 tokenizePos).  A char is WHITESPACE (Character.isWhitespace or category Zs; the
 *    stripped chars too), ALPHABETIC (Character.isLetter, category L*), NUMERIC (Character.isDigit, category Nd) or
 *    OTHER.  A token is a maximal run of non-WHITESPACE chars of one class; an OTHER run also ends where the char
 *    changes ("--" is one token, "-/" two).  No lower-casing.  A document is tokenised on its own.  The classes come
 *    from a generated table of the BMP (csrc/class_table.h: Java 8 is Unicode 6.2; code points assigned later are
 *    classed by the generator's newer database — parity unpinned).  The one departure: a code point >= U+10000 is
 *    always one OTHER token of its own (Java sees two unpaired-looking surrogate chars, which UTF-8 cannot carry).
 * 3. Stop words.  A token whose bytes equal a listed word is dropped: exact, case-sensitive, before stemming (so
 *    "being" → "be" survives although "be" is listed).  An empty list drops nothing.
 * 4. Porter stemmer (opennlp.tools.stemmer.PorterStemmer.stem(String), 1.6.0, Lucene's): tokens of <= 2 chars
 *    unchanged; only a e i o u are vowels, y after a consonant too, every other char (capitals, digits, non-ASCII)
 *    is a consonant; Lucene's step1–step6 with its tables (bli → ble and logi → log present, ion only after s or
 *    t, each switch case of steps 3–5 done after its first matching suffix whether replaced or not); doublec and
 *    cvc compare chars, not bytes.  The stem is never longer than the token and never empty.
 * 5. Every input document yields a row of the result, possibly without tokens.  (The reference drops the empty
 *    documents and renumbers the rest: the caller's job.)
 * The result is an stc_dtok like an upload's (stc_cv_fit_tokens, stc_cv_transform_tokens and stc_hashing_tf_tokens
 * take it).  Bitwise reproducible.  STC_ERR_INVALID_ARG: malformed UTF-8 in the text or the stop words (the message
 * names the byte offset), a strip code point >= U+10000 or a surrogate, more than 2^31-1 tokens.  Single device:
 * every call on a context connected to other ranks returns STC_ERR_STATE. */
typedef struct stc_prep stc_prep; /* strip set + stop words + stemmer switch on the device; belongs to its stc_ctx */
int stc_prep_create(stc_ctx* ctx, const uint32_t* strip_cp, int64_t n_strip /* NULL, -1: the reference's set */,
                    const uint8_t* stop_utf8, int64_t n_bytes, const int64_t* stop_off /* n_stop+1 */,
                    int64_t n_stop, int stem /* 0 none, 1 Porter */, stc_prep** out);
int stc_prep_free(stc_prep* prep); /* valid after stc_destroy of the context */
int stc_prep_tokens(stc_ctx* ctx, const stc_prep* prep, const uint8_t* text, int64_t n_bytes,
                    const int64_t* text_off /* n_docs+1 */, int64_t n_docs, stc_dtok** out);
/* sizes of device tokens (any may be NULL), and their copy to the host: utf8_out[n_bytes], tok_off_out[n_tok+1],
 * doc_off_out[n_docs+1] (any may be NULL) */
int stc_tokens_shape(const stc_dtok* tokens, int64_t* n_bytes, int64_t* n_tok, int64_t* n_docs);
/* the longest document's token count the device tokens carry (the vectorizers choose their kernel path from it):
 * exact for an upload and for every result of the library */
int stc_tokens_max_doc(const stc_dtok* tokens, int64_t* max_doc_out);
int stc_tokens_download(stc_ctx* ctx, const stc_dtok* tokens, uint8_t* utf8_out, int64_t* tok_off_out,
                        int64_t* doc_off_out);
/* the stemmer alone, each token on its own (test hook): utf8_out[n_bytes], tok_off_out[n_tok+1] */
int stc_stem_tokens(stc_ctx* ctx, const uint8_t* utf8, int64_t n_bytes, const int64_t* tok_off, int64_t n_tok,
                    uint8_t* utf8_out, int64_t* tok_off_out);

/* ---- Token stages (device tokens in, device tokens out) --------------------------------------
 * What sits between a tokenizer and a vectorizer in a Spark ML pipeline, without leaving the device: either front end
 * (stc_tokenize_tokens, stc_prep_tokens, or an upload) feeds either vectorizer (stc_hashing_tf_tokens, stc_cv_*_tokens)
 * through any chain of these stages.  Every result is an stc_dtok with the invariants of stc_tokens_upload (zero
 * padding behind the blob, u32 offsets when blob + padding fit in 4 GiB, the longest document's token count), freed
 * with stc_tokens_free; the input is left as it is.  Every input document keeps its row, possibly empty.
 * stc_tokenize_tokens: exactly stc_tokenize's tokens (the same lower-casing, the same errors), left on the device.
 * StopWordsRemover ([U] ml.feature.StopWordsRemover.transform).  Kept tokens keep their order and their original
 *   bytes.  The list is the caller's (Spark's bundled language lists are not part of this library); duplicates are
 *   fine, n_stop = 0 keeps everything, and the empty word is legal and drops empty tokens (the Tokenizer makes them).
 *   Stop words must be well-formed UTF-8 in both modes.
 *   case_sensitive = 1: a token is dropped iff its bytes equal a stop word's bytes; tokens are not validated.
 *   case_sensitive = 0 (Spark's default): a token is dropped iff toLowerCase(token) equals toLowerCase(w) for some
 *   stop word w, toLowerCase being the Tokenizer block's Java 8 root-locale lower-casing applied to the token (or the
 *   word) as a string of its own: the Final_Sigma context is the token, İ → "i̇" changes the length.  Tokens and stop
 *   words go through the same device routine, so the two sides cannot drift.  That routine's Final_Sigma rule is the
 *   Unicode one, not the JVM's BreakIterator-word scan: the two differ when a digit stands between Σ and a cased
 *   letter ("Α1Σ": Java ς, here σ; parity unpinned, as for stc_tokenize).  Spark lower-cases with a locale parameter
 *   (the JVM default); this is the root locale, which differs from tr, az and lt only.  In this mode every token must
 *   be well-formed UTF-8: STC_ERR_INVALID_ARG naming the byte offset in the blob otherwise.
 * NGram ([U] ml.feature.NGram: sliding(n).withPartial(false).map(_.mkString(" "))).  n >= 1, else
 *   STC_ERR_INVALID_ARG.  A document of T tokens yields max(T - n + 1, 0) tokens; output token i is input tokens
 *   i .. i+n-1 joined by one U+0020; empty tokens join as they are (["a", "", "b"], n = 2 → ["a ", " b"]); n = 1 is a
 *   copy.
 * At most 2^31-1 input tokens per call.  Bitwise reproducible.  A handle made by another context is
 * STC_ERR_INVALID_ARG.  Single device: every call on a context connected to other ranks returns STC_ERR_STATE. */
int stc_tokenize_tokens(stc_ctx* ctx, const uint8_t* text, int64_t n_bytes, const int64_t* text_off /* n_docs+1 */,
                        int64_t n_docs, stc_dtok** out);
typedef struct stc_swr stc_swr; /* the stop words' table on the device; belongs to its stc_ctx as an stc_prep does */
int stc_swr_create(stc_ctx* ctx, const uint8_t* stop_utf8, int64_t n_bytes, const int64_t* stop_off /* n_stop+1 */,
                   int64_t n_stop, int case_sensitive, stc_swr** out);
int stc_swr_free(stc_swr* swr); /* valid after stc_destroy of the context */
int stc_swr_tokens(stc_ctx* ctx, const stc_swr* swr, const stc_dtok* in, stc_dtok** out);
int stc_ngram_tokens(stc_ctx* ctx, const stc_dtok* in, int32_t n, stc_dtok** out);

/* ---- IDF (K3 df count, K4 idf, K5 transform) ---------------------------------------------
 * df_j = #rows with value_j > 0, m = #rows (summed over all ranks when connected);
 * idf_j = df_j >= min_doc_freq ? ln((m+1)/(df_j+1)) : 0.                                  */
int stc_idf_fit(stc_ctx* ctx, const stc_dcsr* tf, int64_t min_doc_freq,
                double* idf_out /* n_cols */, int64_t* df_out /* n_cols, may be NULL */,
                int64_t* m_out /* may be NULL */);
/* values[e] *= idf[indices[e]]; when zero_floor > 0 an idf of exactly 0 is replaced by
 * zero_floor (the reference's LDAClustering.scala:184-187 quirk; 0 = stock Spark)          */
int stc_idf_transform(stc_ctx* ctx, stc_dcsr* tf, const double* idf /* n_cols */,
                      double zero_floor);
/* The same IDFModel kept on the device (the GPU-resident HashingTF → IDF → LDA pipeline: the idf
 * vector need not cross PCIe between fit and transform); stc_idf_get copies it out (any may be NULL). */
typedef struct stc_didf stc_didf;
int stc_idf_fit_dev(stc_ctx* ctx, const stc_dcsr* tf, int64_t min_doc_freq, stc_didf** out);
int stc_idf_get(stc_ctx* ctx, const stc_didf* model, double* idf_out /* n_cols */,
                int64_t* df_out /* n_cols */, int64_t* m_out);
int stc_idf_transform_dev(stc_ctx* ctx, stc_dcsr* tf, const stc_didf* model, double zero_floor);
/* the model's vector size (numFeatures: stc_idf_get writes n_cols values to each output) and m */
int stc_didf_shape(const stc_didf* model, int64_t* n_cols_out, int64_t* m_out);
int stc_didf_free(stc_didf* model);

/* ---- online LDA ----------------------------------------------------------------------- */
typedef struct stc_lda_config {
  int32_t k;                     /* number of topics */
  int64_t vocab_size;            /* V (= numFeatures) */
  const double* doc_concentration; /* α: 1 value (−1 ⇒ 1/k) or k values */
  int32_t doc_concentration_len;
  double topic_concentration;    /* η (−1 ⇒ 1/k) */
  double tau0;                   /* learningOffset, default 1024 */
  double kappa;                  /* learningDecay, default 0.51 */
  double mini_batch_fraction;    /* subsamplingRate, default 0.05 */
  double gamma_shape;            /* default 100 */
  int32_t optimize_doc_concentration; /* ml.LDA default 1, mllib default 0 */
  int32_t sample_with_replacement;    /* mllib default 1 */
  uint64_t seed;                 /* λ₀ / membership / γ₀ counter-RNG seed */
  int32_t dtype;                 /* STC_F64 (default: Spark's Double E-step), STC_F32 or STC_MIXED */
  int32_t max_inner_iter;        /* E-step safety cap (upstream has none); 0 ⇒ 100000 */
  int32_t mixed_resolve_iters;   /* STC_MIXED: re-solve in fp64 the documents past this many fp32 iterations
                                    (0 ⇒ 500) */
} stc_lda_config;

/* fills the upstream defaults (ml.clustering.LDA) */
void stc_lda_config_default(stc_lda_config* cfg);

typedef struct stc_step_stats {
  int64_t batch_docs;        /* docs in the minibatch on this rank */
  int64_t nonempty_docs;     /* all ranks */
  int64_t batch_entries;     /* (doc, term) entries on this rank */
  int64_t inner_iters;       /* Σ E-step iterations on this rank */
  int32_t inner_iters_max;
  int32_t cap_hits;          /* docs stopped by max_inner_iter */
  double rho;                /* learning rate used */
} stc_step_stats;

int stc_lda_create(stc_ctx* ctx, const stc_lda_config* cfg, stc_lda** out);
int stc_lda_destroy(stc_lda* lda);
/* the documents of THIS rank; corpus_size_total = Σ over ranks (Spark's corpusSize).
 * The CSR values are read in the LDA's dtype; the handle keeps a reference to `corpus`.    */
int stc_lda_set_corpus(stc_lda* lda, const stc_dcsr* corpus, int64_t corpus_size_total);
/* λ₀ ~ Gamma(gamma_shape, 1/gamma_shape) i.i.d. from the counter RNG (seed) — identical on
 * every rank, so no broadcast is needed                                                    */
int stc_lda_init_random(stc_lda* lda, uint64_t seed);
int stc_lda_set_topics(stc_lda* lda, const double* topics, int layout);
int stc_lda_get_topics(stc_lda* lda, double* topics_out, int layout);
int stc_lda_set_alpha(stc_lda* lda, const double* alpha /* k */);
int stc_lda_get_alpha(stc_lda* lda, double* alpha_out /* k */);
int stc_lda_get_eta(stc_lda* lda, double* eta_out);
int stc_lda_get_iteration(stc_lda* lda, int64_t* iteration_out);
/* k and V of the handle (the JNI shim sizes and checks its Java arrays with them) */
int stc_lda_shape(const stc_lda* lda, int32_t* k_out, int64_t* vocab_out);

/* One submitMiniBatch over an injected membership: batch_doc_ids are row indices of this
 * rank's corpus (duplicates allowed = sampling with replacement).  gamma0 (n×k, may be NULL)
 * injects γ₀; otherwise γ₀ comes from the counter RNG keyed (seed, iteration, rank, pos).
 * stats may be NULL (then the call does not wait for the GPU).                              */
int stc_lda_step(stc_lda* lda, const int64_t* batch_doc_ids, int64_t n, const double* gamma0,
                 stc_step_stats* stats);
/* One OnlineLDAOptimizer.next(): device-side Poisson/Bernoulli membership sampling with
 * fraction mini_batch_fraction, then the same step.  Every call draws a new sample (an empty
 * GLOBAL sample returns without an iteration, as Spark's `if (batch.isEmpty()) return this`);
 * the next draw is sampled during this step, so consecutive calls do not drain the stream.  */
int stc_lda_next(stc_lda* lda, stc_step_stats* stats);
/* E-step only (no model update), for tests: gamma_out n×k; stat_out (k×V as V×k layout,
 * may be NULL) receives the summed sufficient statistics Σ_d eθ_d ⊗ (cts/φ) scattered to
 * their terms (Spark's `stat` before ⊙ expElogβ); iters_out n (may be NULL).              */
int stc_lda_estep(stc_lda* lda, const int64_t* batch_doc_ids, int64_t n, const double* gamma0,
                  double* gamma_out, double* stat_out, int32_t* iters_out);

/* LocalLDAModel.logLikelihood over `docs` (any CSR with V columns, this rank's part):
 * bound = corpusPart (Σ over all ranks) + topicsPart.  γ₀ per doc: gamma0 (rows×k) if given,
 * else counter RNG keyed (gamma_seed, doc_id_base + row).  token_count = Σ values.          */
int stc_lda_bound(stc_lda* lda, const stc_dcsr* docs, uint64_t gamma_seed, int64_t doc_id_base,
                  const double* gamma0, double* bound_out, double* corpus_part_out,
                  double* topics_part_out, double* token_count_out);
/* LocalLDAModel.topicDistribution for every row of `docs`: out rows×k (zeros for empty rows) */
int stc_lda_topic_distribution(stc_lda* lda, const stc_dcsr* docs, uint64_t gamma_seed,
                               int64_t doc_id_base, const double* gamma0, double* out);
/* LocalLDAModel.describeTopics(max_terms): idx_out k×N, weight_out k×N (N = min(max,V)) */
int stc_lda_describe(stc_lda* lda, int32_t max_terms, int32_t* idx_out, double* weight_out);

/* Average device time (ms, HIP events) of the last step's phases, for the bench:
 * [0] sample+scan, [1] E-step kernel, [2] sstats (sort + segmented SpMM), [3] all-reduce,
 * [4] M-step (λ update + expElogβ).  Requires stc_lda_enable_timing(lda, 1) beforehand.    */
int stc_lda_enable_timing(stc_lda* lda, int on);
/* cumulative since creation: [0] batch docs, [1] batch entries, [2] Σ inner E-step iterations,
 * [3] docs stopped by max_inner_iter                                                         */
int stc_lda_counters(stc_lda* lda, int64_t out[4]);
int stc_lda_phase_times(stc_lda* lda, double* ms_out /* 5 */, int64_t* steps_out);
/* E-step launches per kernel family, cumulative since creation (training and inference): what actually
 * ran, so a caller can name the kernel it timed (a team launch that timed out and was re-run on the
 * one-CU kernel counts under its family, under STC_KC_WIDE and under STC_KC_TEAM_FALLBACK) */
enum stc_kernel_count {
  STC_KC_ROWS64 = 0,        /* k_estep_rows64[_pers]: fp64, k <= 104 */
  STC_KC_ROWS64_LONG = 1,   /* k_estep_rows64_long: the pass over 7-8-row-set documents (may find none) */
  STC_KC_GRID = 2,          /* k_estep_grid[_pers] (+ its long-document pass): fp32, k <= 128 */
  STC_KC_WIDE = 3,          /* k_estep_wide: many topics, one CU per document */
  STC_KC_WIDE_MC = 4,       /* k_estep_wide_mc: many topics, the rows split over a team of CUs */
  STC_KC_WIDE_TC = 5,       /* k_estep_wide_tc: many topics, the topics split over a team */
  STC_KC_TGRID64 = 6,       /* k_estep_tgrid64: fp64, the topics split, the rows64 grid in each member */
  STC_KC_TEAM_FALLBACK = 7, /* team launches re-run on k_estep_wide after a co-residency timeout */
  STC_KC_WORKGROUP = 8,     /* k_estep: documents past the fast kernels' row capacity */
  STC_KC_MIXED_RESOLVES = 9, /* STC_MIXED: fp64 re-solve passes launched (documents past the threshold) */
  STC_KC_MIXED_DOCS = 10,   /* STC_MIXED: documents re-solved in fp64 */
  STC_KC_N = 12
};
int stc_lda_kernel_counts(stc_lda* lda, int64_t out[12]);

/* ---- EM LDA ([U] EMLDAOptimizer → DistributedLDAModel) ------------------------------------
 * The corpus is a bipartite graph: every CSR entry (document d, term w, value c != 0) is an edge; entries
 * whose value is exactly 0 are not edges, and a document or term without an edge has no vertex (its row of
 * the state is 0).  State, fp64 (stored as fp32 by stc_em_create_as, below): doc_topics N_dk (D×k), term_topics N_wk (V×k, the model's unnormalised
 * topicsMatrix), totals N_k = Σ_w N_wk.  One iteration: along every edge the message c·γ with
 *   γ_j ∝ (N_wk[w][j] + η−1)(N_dk[d][j] + α−1) / (N_k[j] + V(η−1)),  Σ_j γ_j = 1,
 * all reads from the old state; a vertex's new counts are the sum of the messages of its edges.
 * α (symmetric) and η: −1 picks Spark's EM defaults 50/k + 1 and 1.1; anything else must be > 1.
 * 2 <= k <= 1024.  The results are bitwise reproducible (no float atomics; fixed summation orders).
 * Single device: every call on a context connected to other ranks returns STC_ERR_STATE (several devices:
 * stc_em_group, below).                                                                          */
typedef struct stc_em stc_em;
/* builds the graph on the device (the filtered CSR and its transpose) from an STC_F64 `corpus` of ctx (an
 * STC_F32 one: STC_ERR_INVALID_ARG).  The handle copies what it needs and keeps no reference to `corpus`. */
int stc_em_create(stc_ctx* ctx, const stc_dcsr* corpus, int32_t k, double doc_concentration,
                  double topic_concentration, stc_em** out);
/* waits for queued iterations, then frees the device memory (valid after stc_destroy of the context) */
int stc_em_destroy(stc_em* em);
/* any may be NULL; n_edges counts the non-zero entries */
int stc_em_shape(const stc_em* em, int32_t* k, int64_t* n_docs, int64_t* vocab, int64_t* n_edges);
/* every edge draws k uniforms in (0,1) from the counter RNG keyed (seed, the edge's position among the
 * edges in CSR order, topic) and normalises them to sum 1: N_dk[d] += c·γ_e, N_wk[w] += c·γ_e */
int stc_em_init_random(stc_em* em, uint64_t seed);
/* state injection: doc_topics D×k, term_topics V×k (non-negative); rows of documents / terms without an
 * edge are stored as 0, N_k is derived */
int stc_em_set_state(stc_em* em, const double* doc_topics, const double* term_topics);
/* doc_topics D×k, term_topics V×k, totals k, the resolved α and η; any may be NULL.  Waits for queued
 * iterations.  The three arrays need a state (STC_ERR_STATE before init_random / set_state). */
int stc_em_get_state(stc_em* em, double* doc_topics, double* term_topics, double* totals, double* alpha_out,
                     double* eta_out);
/* n_iterations × EMLDAOptimizer.next(); enqueues on the context's stream and does not wait
 * (stc_synchronize, or any call that copies results out, does).  STC_ERR_STATE without a state. */
int stc_em_next(stc_em* em, int32_t n_iterations);
/* DistributedLDAModel.logLikelihood = Σ_edges c·ln(φ_w · θ_d), φ_w[j] = (N_wk[w][j] + η−1) / (N_k[j] + V(η−1)),
 * θ_d = (N_dk[d] + α−1) normalised; logPrior = (η−1) Σ_terms Σ_j ln φ_w[j] + (α−1) Σ_docs Σ_j ln θ_d[j] over
 * the vertices that exist.  Either may be NULL.  STC_ERR_STATE without a state. */
int stc_em_log_likelihood(stc_em* em, double* log_likelihood_out, double* log_prior_out);
/* DistributedLDAModel.topicAssignments under the current state: for every edge, in the filtered graph's CSR
 * order, the topic j maximising (N_wk[w][j] + η−1)(N_dk[d][j] + α−1) / (N_k[j] + V(η−1)), formed as
 * stc_em_next forms it; ties go to the smallest j.  indptr_out int64[D+1] (a document without an edge has an
 * empty range), terms_out int32[E] (ascending inside a document), topics_out int32[E]; E from stc_em_shape;
 * any may be NULL.  Waits for queued iterations (with all three NULL the pass is only enqueued, as an
 * iteration is: nothing is copied, so there is nothing to wait for).  STC_ERR_STATE without a state. */
int stc_em_topic_assignments(stc_em* em, int64_t* indptr_out, int32_t* terms_out, int32_t* topics_out);

/* ---- one process, N devices ---------------------------------------------------------------
 * The reference trains in ONE JVM (Spark local[*], LDATraining.scala:7), so its drop-in drives every GPU
 * of the node from one handle ("single-process multi-device").  stc_group_create makes
 * one context and one LDA handle per device (distinct devices: one RCCL communicator, ncclCommInitAll;
 * the same device repeated: an in-process transport, the multi-GPU decomposition on one GPU), and every
 * group call runs the per-device call on one host thread per member.  The corpus is given once, on the
 * host, and sharded by contiguous document ranges balanced by entries (document ids stay global).  Each
 * group call = the same stc_lda_* call on every member (the collectives pair up by construction). */
typedef struct stc_group stc_group;
int stc_group_create(const int* device_ids, int n_devices, const stc_lda_config* cfg, stc_group** out);
int stc_group_destroy(stc_group* g);
int stc_group_size(const stc_group* g, int* n_out);
/* How the members' collectives travel.  Debug knob: with STC_GROUP_RCCL=1 in the environment at
 * stc_group_create, a group of distinct devices of any size (one included) builds its communicator with
 * ncclCommInitAll, runs the sharded M-step's collectives over it and drives every member from its own
 * host thread — the multi-GPU drop-in path on a one-GPU machine. */
enum stc_transport {
  STC_TRANSPORT_NONE = 0,       /* one member, no collectives */
  STC_TRANSPORT_IN_PROCESS = 1, /* one device repeated: device pointers exchanged between member threads */
  STC_TRANSPORT_RCCL = 2        /* an RCCL communicator over the members' devices (ncclCommInitAll) */
};
int stc_group_transport(const stc_group* g, int* transport_out);
/* member i's handle (counters, timing); do not call its collective entry points directly */
int stc_group_member(stc_group* g, int i, stc_lda** lda_out);
/* the training corpus (rows = documents, values in the group's dtype on device) */
int stc_group_set_corpus(stc_group* g, int64_t n_rows, int64_t n_cols, const int64_t* indptr,
                         const int32_t* indices, const double* values);
/* frees the training corpus shards (inference — describe, bound, topicDistribution — needs none;
 * next / step fail with STC_ERR_STATE until a new stc_group_set_corpus) */
int stc_group_release_corpus(stc_group* g);
int stc_group_init_random(stc_group* g, uint64_t seed);
int stc_group_set_topics(stc_group* g, const double* topics, int layout);
int stc_group_get_topics(stc_group* g, double* topics_out, int layout);
int stc_group_get_alpha(stc_group* g, double* alpha_out /* k */);
int stc_group_get_iteration(stc_group* g, int64_t* iteration_out);
/* waits until every member's queued work (the last next / step included) has finished */
int stc_group_synchronize(stc_group* g);
/* OnlineLDAOptimizer.next() over every member's documents; stats summed over the members */
int stc_group_next(stc_group* g, stc_step_stats* stats);
/* submitMiniBatch over injected GLOBAL document ids (gamma0 n×k in the same order, may be NULL) */
int stc_group_step(stc_group* g, const int64_t* batch_doc_ids, int64_t n, const double* gamma0,
                   stc_step_stats* stats);
int stc_group_describe(stc_group* g, int32_t max_terms, int32_t* idx_out, double* weight_out);
/* logLikelihood / topicDistribution of host documents, sharded over the members; γ₀ keys are
 * doc_id_base + global row, so the results equal a single handle's over the same rows */
int stc_group_bound(stc_group* g, int64_t n_rows, int64_t n_cols, const int64_t* indptr,
                    const int32_t* indices, const double* values, uint64_t gamma_seed, int64_t doc_id_base,
                    const double* gamma0, double* bound_out, double* corpus_part_out,
                    double* topics_part_out, double* token_count_out);
int stc_group_topic_distribution(stc_group* g, int64_t n_rows, int64_t n_cols, const int64_t* indptr,
                                 const int32_t* indices, const double* values, uint64_t gamma_seed,
                                 int64_t doc_id_base, const double* gamma0, double* out /* rows×k */);

/* ---- EM LDA, one process, N devices -------------------------------------------------------
 * The EM optimizer of stc_em_* over the devices of an stc_group (the same device rules, transports,
 * STC_GROUP_RCCL knob, member threads and failure handling; at most 16 members).  The corpus is given once,
 * on the host, and sharded as stc_group_set_corpus shards it: contiguous document ranges balanced by entries.
 * Member i holds an stc_em over its documents with all V columns.  N_dk stays on the member; N_wk, N_k are
 * replicated.  One iteration on every member: the row pass over its documents (exact, local), the column pass
 * over its own edges (a term without a local edge: a 0 row), one all-reduce of N_wk' (V×k fp64), then N_k'.
 * What is global: the RNG keys of init_random are the edges' positions in the whole corpus's CSR order, and a
 * term has a vertex iff any member has an edge of it.  Document ids, rows of doc_topics and the order of
 * topicAssignments are the whole corpus's.
 * Against a single stc_em only the summation order of N_wk differs (per member, then over the members): N_dk'
 * of one step from an injected state is bitwise the single handle's, a one-member group is bitwise an stc_em.
 * With the in-process transport the members' sum runs in member order, so the replicas are bitwise equal and a
 * run is bitwise reproducible for a given member count.
 * Argument checks and error codes are stc_em_create's; a member with no documents or no edges is valid. */
typedef struct stc_em_group stc_em_group;
/* the host CSR (values double; entries of value 0 are not edges) is copied: nothing of it is kept */
int stc_em_group_create(const int* device_ids, int n_devices, int64_t n_rows, int64_t n_cols, const int64_t* indptr,
                        const int32_t* indices, const double* values, int32_t k, double doc_concentration,
                        double topic_concentration, stc_em_group** out);
int stc_em_group_destroy(stc_em_group* g);
int stc_em_group_size(const stc_em_group* g, int* n_out);
int stc_em_group_transport(const stc_em_group* g, int* transport_out); /* enum stc_transport */
/* of the whole corpus; any may be NULL */
int stc_em_group_shape(const stc_em_group* g, int32_t* k, int64_t* n_docs, int64_t* vocab, int64_t* n_edges);
/* member i's handle and its first corpus row (may be NULL), for reading only: stc_em_shape and stc_em_get_state
 * (the member's own N_dk rows, its replica of N_wk and N_k).  Every other stc_em_* call on a member of a group
 * with a communicator returns STC_ERR_STATE. */
int stc_em_group_member(stc_em_group* g, int i, stc_em** em_out, int64_t* row0_out);
int stc_em_group_init_random(stc_em_group* g, uint64_t seed);
/* doc_topics D×k (rows of the whole corpus), term_topics V×k */
int stc_em_group_set_state(stc_em_group* g, const double* doc_topics, const double* term_topics);
/* doc_topics D×k gathered from the members, term_topics V×k and totals k from member 0; any may be NULL */
int stc_em_group_get_state(stc_em_group* g, double* doc_topics, double* term_topics, double* totals,
                           double* alpha_out, double* eta_out);
/* enqueues on every member; with an RCCL communicator it does not wait (stc_em_group_synchronize does), the
 * in-process transport synchronises the host inside every all-reduce */
int stc_em_group_next(stc_em_group* g, int32_t n_iterations);
int stc_em_group_synchronize(stc_em_group* g);
/* the members' edge and document sums added in member order, the term vertices counted once */
int stc_em_group_log_likelihood(stc_em_group* g, double* log_likelihood_out, double* log_prior_out);
/* as stc_em_topic_assignments, in the whole corpus's filtered CSR order: indptr_out int64[D+1] */
int stc_em_group_topic_assignments(stc_em_group* g, int64_t* indptr_out, int32_t* terms_out, int32_t* topics_out);

/* ---- EM LDA, fp32 state storage -----------------------------------------------------------
 * state_dtype STC_F64 is stc_em_create / stc_em_group_create (bitwise); STC_F32 stores N_dk and N_wk as fp32;
 * anything else: STC_ERR_INVALID_ARG.  The contract of an STC_F32 handle: it runs exactly the fp64 handle's
 * iteration on the values it stores, and rounds each new N_dk / N_wk element to the nearest fp32 once, when it
 * is stored.  Everything else stays fp64, in the fp64 handle's order: the edge counts, α, η, N_k (the fixed-shape
 * column sum of the stored, rounded N_wk), γ, every accumulator and partial sum, logLikelihood, logPrior and the
 * argmax of topicAssignments.  So on one device every result of an STC_F32 handle is bitwise that of an STC_F64
 * handle given the same fp32-valued state, rounded.  Elements below fp32's normal range (2^-126) are unpinned.
 * The corpus stays STC_F64 (counts and TF·IDF weights are not rounded; an STC_F32 corpus is still refused).
 * stc_em_set_state takes doubles and stores them rounded to nearest, after the vertex mask; stc_em_get_state
 * returns the stored values widened to doubles, which is exact.  init_random rounds its sums the same way.
 * A group of STC_F32 members: each member's partial N_wk' row is rounded when stored and the members' partials
 * are added in fp32 (the all-reduce carries fp32: half the bytes; the in-process transport adds in member
 * order); N_dk' is the single handle's.
 * (Declared as a block of their own; the arguments before state_dtype are stc_em_create's and
 * stc_em_group_create's.) */
  int stc_em_create_as(stc_ctx* ctx, const stc_dcsr* corpus, int32_t k, double doc_concentration,
                       double topic_concentration, int state_dtype /* STC_F64 | STC_F32 */, stc_em** out);
  /* STC_F64 or STC_F32; serves a member of a group too */
  int stc_em_state_dtype(const stc_em* em, int* dtype_out);
  int stc_em_group_create_as(const int* device_ids, int n_devices, int64_t n_rows, int64_t n_cols,
                             const int64_t* indptr, const int32_t* indices, const double* values, int32_t k,
                             double doc_concentration, double topic_concentration, int state_dtype,
                             stc_em_group** out);

/* ---- EM LDA, ranked queries ([U] DistributedLDAModel.describeTopics / topDocumentsPerTopic /
 * topTopicsPerDocument) -----------------------------------------------------------------------
 * Selections over the resident state (no copy of it, no full sort), of an STC_F64 or STC_F32 handle (the stored
 * values widened; all arithmetic fp64).  Exact and bitwise reproducible: a result depends on the state alone.
 * Tie rule: equal values rank by ascending index (term, document row, topic), whatever their number and
 * wherever they lie.  Row sums Σ_j N_dk[d][j] are added sequentially in ascending j.
 *   describe       per topic t the N = min(max_terms, V) terms with the largest N_wk[w][t] (ranked by the stored
 *                  count, then normalised): idx_out int32[k×N], weight_out double[k×N] = N_wk[w][t] / N_k[t].
 *                  Terms without a vertex (count 0) follow the others in ascending index.
 *   top_documents  per topic t the documents with the largest N_dk[d][t] / Σ_j N_dk[d][j] (the count itself
 *                  where the sum is 0), among the documents that have a vertex (at least one edge) only.
 *                  cap = min(max_docs, D) is the stride of the outputs: row_out int64[k×cap] (corpus rows),
 *                  weight_out double[k×cap]; *n_out = N = min(max_docs, document vertices), the first N of each
 *                  topic's cap entries are written.
 *   top_topics     per document the N = min(n_topics, k) topics with the largest N_dk[d][j]: idx_out int32[D×N],
 *                  weight_out double[D×N] = N_dk[d][j] / Σ_j N_dk[d][j] (the count where the sum is 0: a document
 *                  without a vertex yields topics 0 … N−1 with weight 0).
 * The semantics are recalled from spark-mllib 2.4.3; Spark's own order among equal weights comes out of a
 * BoundedPriorityQueue and argtopk and is not pinned by anything in the reference.
 * Every call waits for queued iterations.  STC_ERR_INVALID_ARG: a NULL argument, a count <= 0; STC_ERR_STATE:
 * no state yet, or (stc_em_*) a context connected to other ranks.
 * Groups: describe runs on member 0 (N_wk, N_k are replicated); top_topics on every member over its rows;
 * top_documents selects per member and merges the members' lists on the host by (weight descending, row
 * ascending) — a weight depends on its own row only, so all three are bitwise the single handle's on the same
 * state. */
  int stc_em_describe(stc_em* em, int32_t max_terms, int32_t* idx_out, double* weight_out);
  int stc_em_top_documents(stc_em* em, int64_t max_docs, int64_t* n_out, int64_t* row_out, double* weight_out);
  int stc_em_top_topics(stc_em* em, int32_t n_topics, int32_t* idx_out, double* weight_out);
  int stc_em_group_describe(stc_em_group* g, int32_t max_terms, int32_t* idx_out, double* weight_out);
  int stc_em_group_top_documents(stc_em_group* g, int64_t max_docs, int64_t* n_out, int64_t* row_out,
                                 double* weight_out);
  int stc_em_group_top_topics(stc_em_group* g, int32_t n_topics, int32_t* idx_out, double* weight_out);

/* ---- Document scores (the clustering report of LDALoader.scala:86-94, 131-163) ------------------
 * A set of documents is scored once; the score stays on the device and answers what a clustering report
 * asks — each document's main topic, the documents of each topic, ranked lists, the words that tie a document
 * to its topic — without γ crossing to the host.
 * An stc_dscore holds γ (rows×k, fp64; a row marked empty is stored as 0) and per row
 *   rowsum[r] = ((|γ[r][0]| + |γ[r][1]|) + …) + |γ[r][k−1]|, added sequentially in ascending j, −1 for an empty row;
 * θ[r][j] = γ[r][j] / rowsum[r] (γ[r][j] itself where the sum is 0, so an empty row's θ is 0).
 *   stc_lda_score         exactly the E-step of stc_lda_topic_distribution (same arguments, same γ₀ keys, an
 *                         STC_MIXED handle infers in fp64) with γ widened to fp64 and kept; a row is empty iff it
 *                         has no entries.  Keeps no reference to `docs`.
 *   stc_score_from_gamma  the same object from a host matrix (the EM model's doc_topics, planted values): gamma
 *                         rows×k, every entry finite and >= 0 (else STC_ERR_INVALID_ARG); empty[r] != 0 marks row r
 *                         empty (NULL: none is).  2 <= k <= 4096.
 *   topic_distribution    out rows×k = θ: bitwise what stc_lda_topic_distribution writes for the same call.
 *   main_topics           the topic with the largest θ, among equal maxima the LARGEST index (LDALoader.scala:136
 *                         updates on `mainTopicWeight <= weight`); weight_out = that θ (bitwise γ / rowsum).  An
 *                         empty row: topic −1, weight 0 (the reference drops empty documents).  count_out[t] = the
 *                         rows whose main topic is t.  Any k the online handle accepts (<= 4096).
 *   members               the non-empty rows grouped by main topic, ascending inside a topic: indptr_out int64[k+1]
 *                         (indptr_out[t+1] − indptr_out[t] = count[t]), rows_out int64[nonempty] (stc_score_shape).
 *                         Integer counters and a stable integer sort only.
 *   top_topics            stc_em_top_topics' contract over (γ, rowsum): idx_out int32[rows×N], weight_out
 *                         double[rows×N], N = min(n_topics, k), ties by ascending topic, an empty row yields topics
 *                         0 … N−1 with weight 0.  k <= 1024 (above: STC_ERR_INVALID_ARG).
 *   top_documents         stc_em_top_documents' contract: per topic the non-empty rows with the largest θ, ties by
 *                         ascending row; cap = min(max_docs, rows) is the outputs' stride, row_out int64[k×cap],
 *                         weight_out double[k×cap], *n_out = N = min(max_docs, nonempty).
 *   stc_lda_important_terms  per row d of `docs` (the matrix that was scored: the same rows, V columns):
 *                         t_d = row d's main topic (topic_of == NULL) or topic_of[d] (−1: the row yields nothing; any
 *                         other value outside 0 … k−1: STC_ERR_INVALID_ARG);
 *                         L_d = the first min(doc_terms, nnz_d) entries of the row by (value descending, term index
 *                         ascending) — values widened to fp64, −0 read as 0, negative values below positive ones,
 *                         NaN unpinned; ties rank by term index whatever the order of the row's entries;
 *                         S_t = the min(topic_terms, V) terms with the largest λ[w][t], ties by ascending term
 *                         (stc_lda_describe's order; no V·k < 2^31 limit here);
 *                         the result = the first max_out entries of L_d whose term is in S_{t_d}, in L_d's order
 *                         (Scala's slice(0, 100).intersect(topicVocab).slice(0, 10); LDALoader's numbers are
 *                         doc_terms 100, topic_terms 300, max_out 10).  idx_out int32[rows×max_out] and value_out
 *                         double[rows×max_out] (unused slots: −1 and 0), n_out int32[rows].  All three counts >= 1,
 *                         doc_terms <= 1024.
 * Any output pointer may be NULL.  A score belongs to its stc_ctx as an stc_dcsr does: a handle of another
 * context returns STC_ERR_INVALID_ARG.  Single device: a context connected to other ranks returns STC_ERR_STATE,
 * as does an LDA handle without topics.  Every call waits for queued work.  Results are bitwise reproducible: a
 * result depends on the scores (and for the terms on `docs` and λ) alone; no float atomics anywhere. */
typedef struct stc_dscore stc_dscore;
  int stc_lda_score(stc_lda* lda, const stc_dcsr* docs, uint64_t gamma_seed, int64_t doc_id_base,
                    const double* gamma0, stc_dscore** out);
  int stc_score_from_gamma(stc_ctx* ctx, const double* gamma, const uint8_t* empty, int64_t rows, int32_t k,
                           stc_dscore** out);
  /* frees the device memory (valid after stc_destroy of the context) */
  int stc_score_free(stc_dscore* score);
  int stc_score_shape(const stc_dscore* score, int64_t* rows, int32_t* k, int64_t* nonempty);
  int stc_score_topic_distribution(stc_ctx* ctx, const stc_dscore* score, double* out /* rows×k */);
  int stc_score_main_topics(stc_ctx* ctx, const stc_dscore* score, int32_t* topic_out /* rows */,
                            double* weight_out /* rows */, int64_t* count_out /* k */);
  int stc_score_members(stc_ctx* ctx, const stc_dscore* score, int64_t* indptr_out /* k+1 */,
                        int64_t* rows_out /* nonempty */);
  int stc_score_top_topics(stc_ctx* ctx, const stc_dscore* score, int32_t n_topics, int32_t* idx_out,
                           double* weight_out);
  int stc_score_top_documents(stc_ctx* ctx, const stc_dscore* score, int64_t max_docs, int64_t* n_out,
                              int64_t* row_out, double* weight_out);
  int stc_lda_important_terms(stc_lda* lda, const stc_dcsr* docs, const stc_dscore* score, const int32_t* topic_of,
                              int32_t doc_terms, int32_t topic_terms, int32_t max_out, int32_t* idx_out,
                              double* value_out, int32_t* n_out);

/* ---- Topic coherence (UMass, Mimno et al. 2011; document-level NPMI) -----------------------------
 * A number for what LDALoader.scala:66-69, 177-187 leaves to the reader's eye: do a topic's top terms occur in the
 * same documents.  Both measures are functions of document co-occurrence counts of the top terms, so the device
 * counts (one integer pass over a resident matrix) and the host does the arithmetic.
 *   stc_term_cooccurrence  terms int32[k×n] on the host: terms[t·n + i] is the term in slot i of topic t's list, best
 *                         first; −1 marks an unused slot (all its counts are 0); any other value outside
 *                         0 … n_cols−1: STC_ERR_INVALID_ARG.  A term may sit in several lists and more than once in
 *                         one list: every slot counts on its own.  A document contains term w iff its row has an
 *                         entry with index w and value > 0 (stc_idf_fit's rule: explicit zeros, negatives and NaN do
 *                         not count); a row that lists w twice contains it once; rows need not be sorted; the matrix
 *                         may be STC_F32 or STC_F64.
 *                         df_out int64[k×n]: the documents that contain slot i's term; codf_out int64[k×n×n]: the
 *                         documents that contain both slots' terms (symmetric, codf[t][i][i] = df[t][i]);
 *                         *n_docs_out = the matrix's rows, empty ones included (IDF's m).  1 <= n <= 64,
 *                         1 <= k <= 4096, fewer than 2^32 rows.  Any output pointer may be NULL.
 *   stc_coherence         host only: no context, callable without a GPU.  For topic t the pairs (m, l), 1 <= m < n,
 *                         0 <= l < m, m ascending and l ascending inside m; a pair with df[t][m] <= 0 or
 *                         df[t][l] <= 0 (an unused slot, a term the corpus does not hold) is skipped; pairs_out[t]
 *                         = the pairs that were not; the pair values are added sequentially in that order in fp64.
 *                         STC_COH_UMASS: pair value ln((codf[t][m][l] + eps) / df[t][l]), topic_out[t] = the sum
 *                         (0 without pairs); eps > 0 (Mimno et al.: 1).  STC_COH_NPMI, D = n_docs, c = codf[t][m][l]:
 *                         −1 when c = 0, 0 when c = D, else ln(c·D / (df[t][m]·df[t][l])) / −ln(c / D); topic_out[t] =
 *                         the mean over the counted pairs (0 without any); eps is ignored.  topic_out double[k],
 *                         pairs_out int32[k], either may be NULL.  STC_ERR_INVALID_ARG: df or codf NULL, an unknown
 *                         measure, n_docs <= 0, k or n < 1, a negative count.
 * The matrix belongs to its stc_ctx: a handle of another context returns STC_ERR_INVALID_ARG.  Single device: a
 * context connected to other ranks returns STC_ERR_STATE.  The count waits for queued work.  Its results are exact
 * and bitwise reproducible: integer adds only on the device, no floating-point arithmetic and no float atomics. */
enum stc_coherence_measure { STC_COH_UMASS = 0, STC_COH_NPMI = 1 };
  int stc_term_cooccurrence(stc_ctx* ctx, const stc_dcsr* docs, const int32_t* terms /* k×n, host */, int32_t k,
                            int32_t n, int64_t* df_out /* k×n */, int64_t* codf_out /* k×n×n */, int64_t* n_docs_out);
  int stc_coherence(const int64_t* df, const int64_t* codf, int32_t k, int32_t n, int64_t n_docs, int measure,
                    double eps, double* topic_out /* k */, int32_t* pairs_out /* k */);

#ifdef __cplusplus
}
#endif
#endif /* STC_H_ */
