package org.apache.spark.mllib.clustering;

/**
 * JNI declarations of libstc.so (include/stc.h) — one native method per C entry point, implemented
 * by jni/stcjni.c (libstcjni.so, which links libstc.so).  Handles (stc_ctx*, stc_dcsr*, stc_lda*) are
 * longs; a non-zero status surfaces as IllegalArgumentException (STC_ERR_INVALID_ARG) or
 * IllegalStateException with the library's message.  Callers: HipOnlineLDAOptimizer (the
 * LDAClustering.scala:40-46 optimizer switch), mllib.feature.HipIDF (LDAClustering.scala:177), and
 * the Spark-ML wrappers HipHashingTF / HipLDA.
 */
public final class StcNative {
  static {
    System.loadLibrary("stcjni");
  }

  private StcNative() {}

  public static final int F32 = 0, F64 = 1;
  /** LDA dtype only: the fp32 E-step with the documents past 500 fp32 iterations re-solved in fp64 (stc.h STC_MIXED) */
  public static final int MIXED = 2;
  public static final int HASH_STANDARD = 0, HASH_SPARK24 = 1;
  public static final int LAYOUT_VK = 0, LAYOUT_KV = 1;

  // ---- library / device
  public static native String lastError();
  public static native int abiVersion();
  public static native int deviceCount();
  public static native long init(int device);
  public static native void destroy(long ctx);
  public static native void synchronize(long ctx);

  // ---- RCCL (one process per GPU: rank 0's id is broadcast by the driver)
  public static native byte[] commUniqueId();
  public static native void commInit(long ctx, byte[] id, int nRanks, int rank);
  public static native void commAllreduceF64(long ctx, double[] inout);

  // ---- device CSR (rows = documents)
  public static native long dcsrUpload(long ctx, long rows, long cols, long[] indptr, int[] indices,
                                       double[] values, int valueDtype);
  /** {rows, cols, nnz} */
  public static native long[] dcsrShape(long dcsr);
  public static native void dcsrDownload(long ctx, long dcsr, long[] indptr, int[] indices, double[] values);
  public static native void dcsrFree(long dcsr);

  // ---- HashingTF: token t = utf8[tokOff[t], tokOff[t+1]), doc d = tokens [docOff[d], docOff[d+1])
  public static native long hashingTfDev(long ctx, byte[] utf8, long[] tokOff, long[] docOff, int numFeatures,
                                         boolean binary, int hashVariant, int valueDtype);
  public static native void hashingTf(long ctx, byte[] utf8, long[] tokOff, long[] docOff, int numFeatures,
                                      boolean binary, int hashVariant, long[] indptrOut, int[] indicesOut,
                                      double[] valuesOut);
  public static native void hashTokens(long ctx, byte[] utf8, long[] tokOff, int numFeatures, int hashVariant,
                                       int[] idxOut);
  /** tokens kept on the GPU between calls (stc_tokens_upload / stc_hashing_tf_tokens) */
  public static native long tokensUpload(long ctx, byte[] utf8, long[] tokOff, long[] docOff);
  public static native void tokensFree(long tokens);
  public static native long hashingTfTokens(long ctx, long tokens, int numFeatures, boolean binary, int hashVariant,
                                            int valueDtype);

  // ---- Tokenizer (ml.feature.Tokenizer: toLowerCase.split("\\s")); returns {nOutBytes, nTok}.
  // utf8Out holds text.length * 3 / 2 bytes (Java lower-cases a few 2-byte characters to 3 bytes)
  public static native long[] tokenize(long ctx, byte[] text, long[] textOff, byte[] utf8Out, long[] tokOffOut,
                                       long[] docOffOut);
  public static native long tokenizeHashingTfDev(long ctx, byte[] text, long[] textOff, int numFeatures,
                                                 boolean binary, int hashVariant, int valueDtype);

  // ---- IDF: returns m (documents, summed over ranks)
  public static native long idfFit(long ctx, long dcsr, long minDocFreq, double[] idfOut, long[] dfOut);
  public static native void idfTransform(long ctx, long dcsr, double[] idf, double zeroFloor);
  // the IDF model kept on the device (a handle); idfGet copies idf / df out (either may be null), returns m
  public static native long idfFitDev(long ctx, long dcsr, long minDocFreq);
  public static native long idfGet(long ctx, long model, long cols, double[] idfOut, long[] dfOut);
  public static native void idfTransformDev(long ctx, long dcsr, long model, double zeroFloor);
  // {numFeatures, m} of a device IDF model (idfGet's cols must equal numFeatures)
  public static native long[] didfShape(long model);
  public static native void didfFree(long model);

  // ---- online LDA (alpha null ⇒ −1 ⇒ 1/k; eta −1 ⇒ 1/k)
  public static native long ldaCreate(long ctx, int k, long vocabSize, double[] alpha, double eta, double tau0,
                                      double kappa, double miniBatchFraction, double gammaShape,
                                      boolean optimizeDocConcentration, boolean sampleWithReplacement, long seed,
                                      int dtype, int maxInnerIter);
  public static native void ldaDestroy(long lda);
  public static native void ldaSetCorpus(long lda, long dcsr, long corpusSizeTotal);
  public static native void ldaInitRandom(long lda, long seed);
  public static native void ldaSetTopics(long lda, double[] topics, int layout);
  public static native void ldaGetTopics(long lda, double[] out, int layout);
  public static native void ldaSetAlpha(long lda, double[] alpha);
  public static native void ldaGetAlpha(long lda, double[] out);
  public static native double ldaGetEta(long lda);
  public static native long ldaGetIteration(long lda);
  /** {k, vocabSize} of the handle */
  public static native long[] ldaShape(long lda);
  /** stats (nullable, 7): batchDocs, nonemptyDocs, batchEntries, innerIters, innerItersMax, capHits, rho */
  public static native void ldaStep(long lda, long[] batchDocIds, double[] gamma0, double[] stats);
  public static native void ldaNext(long lda, double[] stats);
  public static native void ldaEstep(long lda, long[] batchDocIds, double[] gamma0, double[] gammaOut,
                                     double[] statOut, int[] itersOut);
  /** {bound, corpusPart, topicsPart, tokenCount} */
  public static native double[] ldaBound(long lda, long dcsr, long gammaSeed, long docIdBase, double[] gamma0);
  public static native void ldaTopicDistribution(long lda, long dcsr, long gammaSeed, long docIdBase,
                                                 double[] gamma0, double[] out);
  public static native void ldaDescribe(long lda, int maxTerms, int[] idxOut, double[] weightOut);
  public static native void ldaEnableTiming(long lda, boolean on);
  public static native void ldaCounters(long lda, long[] out4);
  public static native long ldaPhaseTimes(long lda, double[] msOut5);
  /** E-step launches per kernel family (stc.h enum stc_kernel_count), 12 words */
  public static native void ldaKernelCounts(long lda, long[] out12);

  // ---- EM LDA (stc_em_*: EMLDAOptimizer / DistributedLDAModel; docConcentration / topicConcentration −1 = auto)
  public static native long emCreate(long ctx, long dcsr, int k, double docConcentration, double topicConcentration);
  /** stateDtype: STC_F64 = 1 (emCreate) or STC_F32 = 0: N_dk / N_wk stored as fp32, all arithmetic in fp64 */
  public static native long emCreateAs(long ctx, long dcsr, int k, double docConcentration, double topicConcentration,
                                       int stateDtype);
  /** STC_F64 = 1 or STC_F32 = 0; serves a group member's handle too */
  public static native int emStateDtype(long em);
  public static native void emDestroy(long em);
  /** {k, nDocs, vocabSize, nEdges} of the handle */
  public static native long[] emShape(long em);
  public static native void emInitRandom(long em, long seed);
  /** docTopics nDocs×k, termTopics vocabSize×k (row-major) */
  public static native void emSetState(long em, double[] docTopics, double[] termTopics);
  /** every array nullable: docTopics nDocs×k, termTopics vocabSize×k, totals k, alphaEta 2 */
  public static native void emGetState(long em, double[] docTopics, double[] termTopics, double[] totals,
                                       double[] alphaEta);
  /** enqueues nIterations EM iterations (does not wait) */
  public static native void emNext(long em, int nIterations);
  /** {logLikelihood, logPrior} */
  public static native double[] emLogLikelihood(long em);
  /** DistributedLDAModel.topicAssignments: per edge in CSR order the first topic with the largest factor; every
   *  array nullable: indptr nDocs + 1, terms nEdges (ascending per document), topics nEdges */
  public static native void emTopicAssignments(long em, long[] indptr, int[] terms, int[] topics);
  /** DistributedLDAModel.describeTopics on the device: idx / weight k × min(maxTerms, vocabSize), per topic the
   *  terms by (N_wk descending, term ascending), weight N_wk / N_k */
  public static native void emDescribe(long em, int maxTerms, int[] idx, double[] weight);
  /** topDocumentsPerTopic: rows / weight k × min(maxDocs, nDocs); returns N = min(maxDocs, document vertices), the
   *  valid entries at the head of each topic's range, by (N_dk / row sum descending, row ascending) */
  public static native long emTopDocuments(long em, long maxDocs, long[] rows, double[] weight);
  /** topTopicsPerDocument: idx / weight nDocs × min(nTopics, k), by (N_dk descending, topic ascending) */
  public static native void emTopTopics(long em, int nTopics, int[] idx, double[] weight);

  // ---- CountVectorizer (stc_cv_*: ml.feature.CountVectorizer / CountVectorizerModel; tokens as for HashingTF)
  /** fit: the vocabSize most frequent terms with minDf <= df <= maxDf (ties by the terms' UTF-8 bytes) */
  public static native long cvFit(long ctx, byte[] utf8, long[] tokOff, long[] docOff, long vocabSize, double minDf,
                                  double maxDf);
  public static native long cvFitTokens(long ctx, long tokens, long vocabSize, double minDf, double maxDf);
  /** term j = utf8[termOff[j], termOff[j+1]), index = position; a term given twice: IllegalArgumentException */
  public static native long cvFromVocabulary(long ctx, byte[] utf8, long[] termOff);
  /** {nTerms, nBytes} of the model */
  public static native long[] cvShape(long model);
  /** every array nullable: utf8Out nBytes, termOffOut nTerms + 1, countOut nTerms, dfOut nTerms */
  public static native void cvGet(long ctx, long model, byte[] utf8Out, long[] termOffOut, long[] countOut,
                                  long[] dfOut);
  /** idxOut[nTok]: each token's vocabulary index, −1 outside the vocabulary */
  public static native void cvIndexOf(long ctx, long model, byte[] utf8, long[] tokOff, int[] idxOut);
  public static native long cvTransformDev(long ctx, long model, byte[] utf8, long[] tokOff, long[] docOff,
                                           double minTf, boolean binary, int valueDtype);
  public static native long cvTransformTokens(long ctx, long model, long tokens, double minTf, boolean binary,
                                              int valueDtype);
  public static native void cvFree(long model);

  /** the reference's text preprocessing behind its lemmatiser (stc_prep_*: strip, SimpleTokenizer, stop words,
   *  Porter stemmer); stripCp null = the reference's set, stop word j = stopUtf8[stopOff[j], stopOff[j+1]) */
  public static native long prepCreate(long ctx, int[] stripCp, byte[] stopUtf8, long[] stopOff, boolean stem);
  public static native void prepFree(long prep);
  /** document d = text[textOff[d], textOff[d+1]); the result is device tokens (tokensFree) */
  public static native long prepTokens(long ctx, long prep, byte[] text, long[] textOff);
  /** token stages (stc_tokenize_tokens, stc_swr_*, stc_ngram_tokens): device tokens in, new device tokens out
   *  (tokensFree each; the input stays valid).  tokenizeTokens: ml.feature.Tokenizer's result left on the device */
  public static native long tokenizeTokens(long ctx, byte[] text, long[] textOff);
  /** ml.feature.StopWordsRemover: stop word j = stopUtf8[stopOff[j], stopOff[j+1]); caseSensitive false compares
   *  Java 8 root-locale lower cases */
  public static native long swrCreate(long ctx, byte[] stopUtf8, long[] stopOff, boolean caseSensitive);
  public static native void swrFree(long swr);
  public static native long swrTokens(long ctx, long swr, long tokens);
  /** ml.feature.NGram: every run of n consecutive tokens of a document joined by one space */
  public static native long ngramTokens(long ctx, long tokens, int n);
  /** {nBytes, nTok, nDocs} of device tokens */
  public static native long[] tokensShape(long tokens);
  /** the longest document's token count of device tokens */
  public static native long tokensMaxDoc(long tokens);
  /** every array nullable: utf8Out nBytes, tokOffOut nTok + 1, docOffOut nDocs + 1 */
  public static native void tokensDownload(long ctx, long tokens, byte[] utf8Out, long[] tokOffOut, long[] docOffOut);
  /** the stemmer alone, each token on its own: utf8Out utf8.length, tokOffOut tokOff.length */
  public static native void stemTokens(long ctx, byte[] utf8, long[] tokOff, byte[] utf8Out, long[] tokOffOut);

  // ---- host helpers (pure Java): Spark vectors → CSR arrays
  /** CSR of sparse or dense rows: {indptr long[n+1], indices int[nnz], values double[nnz]} */
  public static Object[] toCsr(org.apache.spark.mllib.linalg.Vector[] rows) {
    org.apache.spark.mllib.linalg.SparseVector[] sp = new org.apache.spark.mllib.linalg.SparseVector[rows.length];
    long[] indptr = new long[rows.length + 1];
    int nnz = 0;
    for (int i = 0; i < rows.length; ++i) {
      sp[i] = rows[i].toSparse();  // sorted indices, explicit zeros dropped
      nnz += sp[i].indices().length;
      indptr[i + 1] = nnz;
    }
    int[] indices = new int[nnz];
    double[] values = new double[nnz];
    int p = 0;
    for (org.apache.spark.mllib.linalg.SparseVector s : sp) {
      System.arraycopy(s.indices(), 0, indices, p, s.indices().length);
      System.arraycopy(s.values(), 0, values, p, s.values().length);
      p += s.indices().length;
    }
    return new Object[] {indptr, indices, values};
  }

  // ---- one process, N devices (stc_group): the multi-GPU form of the drop-in inside one JVM ----------
  public static native long groupCreate(int[] deviceIds, int k, long vocabSize, double[] alpha, double eta,
                                        double tau0, double kappa, double miniBatchFraction, double gammaShape,
                                        boolean optimizeAlpha, boolean withReplacement, long seed, int dtype,
                                        int maxInnerIter);
  public static native void groupDestroy(long group);
  public static native int groupSize(long group);
  // how the group's collectives travel: 0 none (one member), 1 in-process (one device repeated), 2 RCCL
  public static native int groupTransport(long group);
  public static native long groupMember(long group, int i);
  public static native void groupSetCorpus(long group, long rows, long cols, long[] indptr, int[] indices,
                                           double[] values);
  public static native void groupReleaseCorpus(long group);
  public static native void groupInitRandom(long group, long seed);
  public static native void groupSynchronize(long group);
  public static native void groupSetTopics(long group, double[] topics, int layout);
  public static native void groupGetTopics(long group, double[] out, int layout);
  public static native void groupGetAlpha(long group, double[] out);
  public static native long groupGetIteration(long group);
  public static native void groupNext(long group, double[] stats);
  public static native void groupStep(long group, long[] batchDocIds, double[] gamma0, double[] stats);
  public static native void groupDescribe(long group, int maxTerms, int[] idxOut, double[] weightOut);
  /** {bound, corpusPart, topicsPart, tokenCount} */
  public static native double[] groupBound(long group, long rows, long cols, long[] indptr, int[] indices,
                                           double[] values, long gammaSeed, long docIdBase, double[] gamma0);
  public static native void groupTopicDistribution(long group, long rows, long cols, long[] indptr, int[] indices,
                                                   double[] values, long gammaSeed, long docIdBase,
                                                   double[] gamma0, double[] out);

  // ---- EM LDA over N devices from one JVM (stc_em_group): documents sharded, the term side all-reduced ----
  /** the host CSR is copied; docConcentration / topicConcentration −1 = auto; device rules as groupCreate */
  public static native long emGroupCreate(int[] deviceIds, long rows, long cols, long[] indptr, int[] indices,
                                          double[] values, int k, double docConcentration,
                                          double topicConcentration);
  public static native long emGroupCreateAs(int[] deviceIds, long rows, long cols, long[] indptr, int[] indices,
                                            double[] values, int k, double docConcentration,
                                            double topicConcentration, int stateDtype);
  public static native void emGroupDestroy(long emGroup);
  public static native int emGroupSize(long emGroup);
  public static native int emGroupTransport(long emGroup);
  /** {k, nDocs, vocabSize, nEdges} of the whole corpus */
  public static native long[] emGroupShape(long emGroup);
  /** {member i's em handle (emShape / emGetState only), its first corpus row} */
  public static native long[] emGroupMember(long emGroup, int i);
  public static native void emGroupInitRandom(long emGroup, long seed);
  public static native void emGroupSetState(long emGroup, double[] docTopics, double[] termTopics);
  /** every array nullable: docTopics nDocs×k, termTopics vocabSize×k, totals k, alphaEta 2 */
  public static native void emGroupGetState(long emGroup, double[] docTopics, double[] termTopics, double[] totals,
                                            double[] alphaEta);
  public static native void emGroupNext(long emGroup, int nIterations);
  public static native void emGroupSynchronize(long emGroup);
  /** {logLikelihood, logPrior} */
  public static native double[] emGroupLogLikelihood(long emGroup);
  /** every array nullable: indptr nDocs + 1, terms nEdges, topics nEdges, in the whole corpus's CSR order */
  public static native void emGroupTopicAssignments(long emGroup, long[] indptr, int[] terms, int[] topics);
  /** emDescribe / emTopDocuments / emTopTopics over the whole corpus: bitwise a single handle's on the same state */
  public static native void emGroupDescribe(long emGroup, int maxTerms, int[] idx, double[] weight);
  public static native long emGroupTopDocuments(long emGroup, long maxDocs, long[] rows, double[] weight);
  public static native void emGroupTopTopics(long emGroup, int nTopics, int[] idx, double[] weight);

  // ---- document scores (stc_lda_score / stc_score_*: the report of LDALoader.scala:86-94, 131-163)
  /** ldaTopicDistribution's E-step with γ kept on the GPU; the score belongs to the LDA handle's context */
  public static native long ldaScore(long lda, long dcsr, long gammaSeed, long docIdBase, double[] gamma0);
  /** the same object from a host matrix rows×k (finite, >= 0); empty[r] != 0 marks row r empty (nullable) */
  public static native long scoreFromGamma(long ctx, double[] gamma, byte[] empty, long rows, int k);
  public static native void scoreFree(long score);
  /** {rows, k, nonEmpty} */
  public static native long[] scoreShape(long score);
  /** out rows×k: bitwise ldaTopicDistribution's of the same call */
  public static native void scoreTopicDistribution(long ctx, long score, double[] out);
  /** topic[rows] (the largest θ, among equal maxima the largest index; −1 for an empty row), weight[rows], count[k];
   *  every array nullable */
  public static native void scoreMainTopics(long ctx, long score, int[] topic, double[] weight, long[] count);
  /** the non-empty rows grouped by main topic, ascending inside a topic: indptr[k + 1], rows[nonEmpty] */
  public static native void scoreMembers(long ctx, long score, long[] indptr, long[] rows);
  /** emTopTopics' contract over the score: idx / weight rows × min(nTopics, k); k <= 1024 */
  public static native void scoreTopTopics(long ctx, long score, int nTopics, int[] idx, double[] weight);
  /** emTopDocuments' contract: rows / weight k × min(maxDocs, rows); returns N = min(maxDocs, nonEmpty) */
  public static native long scoreTopDocuments(long ctx, long score, long maxDocs, long[] rows, double[] weight);
  /** "Book most important words": per row of dcsr (the matrix that was scored) the first maxOut of its docTerms
   *  largest entries (value descending, term ascending) whose term is among the topicTerms heaviest terms of the
   *  row's main topic (topicOf[rows], nullable: of that topic; −1 skips the row).  idx / value rows × maxOut
   *  (unused slots −1 / 0), nOut[rows].  LDALoader's numbers: 100, 300, 10 */
  public static native void ldaImportantTerms(long lda, long dcsr, long score, int[] topicOf, int docTerms,
                                              int topicTerms, int maxOut, int[] idx, double[] value, int[] nOut);

  // ---- topic coherence (stc_term_cooccurrence / stc_coherence: the number behind LDALoader.scala:66-69, 177-187)
  /** document co-occurrence counts of k term lists of n slots (terms k × n, best first, −1 = unused) over a resident
   *  matrix: df[k × n], codf[k × n × n] (nullable); a document contains a term iff its row has an entry of it with
   *  value > 0.  Exact.  n <= 64, k <= 4096.  Returns the matrix's rows (IDF's m) */
  public static native long termCooccurrence(long ctx, long dcsr, int[] terms, int k, int n, long[] df, long[] codf);
  /** host only: per topic the UMass sum (measure 0, eps > 0) or the NPMI mean (measure 1) over the pairs whose two
   *  terms occur in the corpus; topic[k], pairs[k] (nullable) */
  public static native void coherence(long[] df, long[] codf, int k, int n, long nDocs, int measure, double eps,
                                      double[] topic, int[] pairs);
}
