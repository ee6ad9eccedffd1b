"""LDA with the Spark ML / mllib surface, backed by libstc: online variational Bayes (K6–K12) and EM.

* ``LDA`` / ``LDAModel`` mirror ``org.apache.spark.ml.clustering.{LDA, LocalLDAModel}``
  ([U] spark 2.4.3): k=10, maxIter=20, optimizer="online", learningOffset=1024,
  learningDecay=0.51, subsamplingRate=0.05, optimizeDocConcentration=true, seed = the class-name
  hash; model methods topicsMatrix, describeTopics, logLikelihood, logPerplexity, transform.
* ``OnlineLDAOptimizer`` + ``MllibLDA`` mirror the RDD API the reference drives at
  LDAClustering.scala:37-61 (``new LDA().setOptimizer(new OnlineLDAOptimizer()
  .setMiniBatchFraction(0.05 + 1.0 / N)).setK(..).setMaxIterations(..)...run(corpus)``).

* ``EMLDAOptimizer`` + ``MllibLDA.setOptimizer("em")`` is the reference's default branch (Params.scala:9,
  LDAClustering.scala:40-41): ``run`` trains on the GPU through an ``EmHandle`` (stc_em_*: the corpus as a
  bipartite graph, N_dk / N_wk / N_k in fp64) and returns a ``DistributedLDAModel`` with logLikelihood,
  logPrior, topicDistributions, topTopicsPerDocument, topDocumentsPerTopic and save.  With ``devices`` set
  (``MllibLDA(devices=[0, 1])`` / ``setDevices``) the same run goes through an ``EmGroup`` (stc_em_group_*: the
  documents sharded over the devices, N_wk all-reduced once per iteration).

The ml estimator ``LDA`` stays online-only (the reference selects EM on the mllib class); an optimizer
other than "em" / "online" raises as in LDAClustering.scala:44-45.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib as L
from .coherence import check_top_n, topic_coherence
from .core import Context, CsrMatrix, DeviceCsr


def _java_string_hash(s: str) -> int:
    h = 0
    for ch in s:
        h = (31 * h + ord(ch)) & 0xFFFFFFFF
    return h - (1 << 32) if h >= (1 << 31) else h


ML_LDA_DEFAULT_SEED = _java_string_hash("org.apache.spark.ml.clustering.LDA")
_DTYPES = {"f32": L.STC_F32, "float32": L.STC_F32, "f64": L.STC_F64, "float64": L.STC_F64, "mixed": L.STC_MIXED}


def _lda_config(lib, k, vocab_size, doc_concentration, topic_concentration, tau0, kappa, mini_batch_fraction,
                gamma_shape, optimize_doc_concentration, sample_with_replacement, seed, dtype, max_inner_iter,
                mixed_resolve_iters=0):
    """stc_lda_config from the Spark-ML parameters (returns the config and the α buffer it points to)."""
    cfg = L.LdaConfig()
    lib.stc_lda_config_default(C.byref(cfg))
    cfg.k = int(k)
    cfg.vocab_size = int(vocab_size)
    alpha_buf = None
    if doc_concentration is not None:
        alpha_buf = L.as_f64(np.atleast_1d(doc_concentration))
        cfg.doc_concentration = L.ptr(alpha_buf, C.c_double)
        cfg.doc_concentration_len = alpha_buf.size
    cfg.topic_concentration = float(-1.0 if topic_concentration is None else topic_concentration)
    cfg.tau0 = float(tau0)
    cfg.kappa = float(kappa)
    cfg.mini_batch_fraction = float(mini_batch_fraction)
    cfg.gamma_shape = float(gamma_shape)
    cfg.optimize_doc_concentration = int(bool(optimize_doc_concentration))
    cfg.sample_with_replacement = int(bool(sample_with_replacement))
    cfg.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    cfg.dtype = _DTYPES[dtype] if isinstance(dtype, str) else int(dtype)
    cfg.max_inner_iter = int(max_inner_iter)
    cfg.mixed_resolve_iters = int(mixed_resolve_iters)  # dtype "mixed": the fp64 re-solve threshold (0: 500)
    return cfg, alpha_buf


def _phase_times(lib, h):
    """stc_lda_phase_times of one handle: mean device ms per step of each phase"""
    ms = np.zeros(5, np.float64)
    steps = C.c_int64()
    L.check(lib.stc_lda_phase_times(h, L.ptr(ms, C.c_double), C.byref(steps)))
    return {"sample": ms[0], "estep": ms[1], "sstats": ms[2], "allreduce": ms[3], "mstep": ms[4],
            "steps": steps.value}


# stc.h enum stc_kernel_count: the E-step kernel families stc_lda_kernel_counts counts launches of
KERNEL_FAMILIES = ("k_estep_rows64", "k_estep_rows64_long", "k_estep_grid", "k_estep_wide", "k_estep_wide_mc",
                   "k_estep_wide_tc", "k_estep_tgrid64", "team_fallback", "k_estep", "mixed_resolves", "mixed_docs")


def _counters(lib, h):
    """stc_lda_counters + stc_lda_kernel_counts of one handle (cumulative since creation)"""
    out = np.zeros(4, np.int64)
    L.check(lib.stc_lda_counters(h, L.ptr(out, C.c_int64)))
    kc = np.zeros(12, np.int64)
    L.check(lib.stc_lda_kernel_counts(h, L.ptr(kc, C.c_int64)))
    return {"docs": int(out[0]), "entries": int(out[1]), "inner_iters": int(out[2]), "cap_hits": int(out[3]),
            "kernels": {f: int(kc[i]) for i, f in enumerate(KERNEL_FAMILIES)}}


class DocumentScores:
    """Owns one stc_dscore: a set of documents scored once, γ and its row sums kept on the GPU (include/stc.h,
    "Document scores").  Made by ``LdaHandle.score`` / ``LDAModel.score`` or ``DocumentScores.from_gamma``; every
    method is a device query, none copies γ to the host."""

    def __init__(self, ctx: Context, handle, lda: "LdaHandle | None" = None):
        self.ctx, self.handle, self._lda = ctx, handle, lda
        rows, k, nonempty = C.c_int64(), C.c_int32(), C.c_int64()
        L.check(ctx.lib.stc_score_shape(handle, C.byref(rows), C.byref(k), C.byref(nonempty)))
        self.num_rows, self.k, self.nonempty = rows.value, k.value, nonempty.value

    @staticmethod
    def from_gamma(ctx: Context, gamma, empty=None) -> "DocumentScores":
        """the scores of a host matrix (rows×k, finite and >= 0; ``empty[r]`` marks row r as an empty document): the
        EM model's doc_topics, or planted values"""
        g = L.as_f64(gamma)
        if g.ndim != 2:
            raise ValueError("gamma must be rows×k")
        e = None if empty is None else np.ascontiguousarray(empty, dtype=np.uint8)
        if e is not None and e.shape != (g.shape[0],):
            raise ValueError("empty must have one entry per row")
        h = C.c_void_p()
        L.check(ctx.lib.stc_score_from_gamma(ctx.handle, L.ptr(g, C.c_double), L.ptr(e, C.c_uint8), g.shape[0],
                                             g.shape[1], C.byref(h)))
        return DocumentScores(ctx, h)

    def topicDistribution(self):
        """θ rows×k = γ / Σ_j γ_j, zeros for empty rows: bitwise ``LdaHandle.topic_distribution`` of the same call"""
        out = np.zeros((self.num_rows, self.k), np.float64)
        L.check(self.ctx.lib.stc_score_topic_distribution(self.ctx.handle, self.handle, L.ptr(out, C.c_double)))
        return out

    def mainTopics(self):
        """(topic int32[rows], weight float64[rows], counts int64[k]): the topic with the largest θ — among equal
        maxima the largest index, as LDALoader.scala:136 — and that θ; an empty row: −1 and 0"""
        topic = np.zeros(self.num_rows, np.int32)
        weight = np.zeros(self.num_rows, np.float64)
        counts = np.zeros(self.k, np.int64)
        L.check(self.ctx.lib.stc_score_main_topics(self.ctx.handle, self.handle, L.ptr(topic, C.c_int32),
                                                   L.ptr(weight, C.c_double), L.ptr(counts, C.c_int64)))
        return topic, weight, counts

    def members(self):
        """(indptr int64[k+1], rows int64[nonempty]): the non-empty rows grouped by main topic, ascending inside one"""
        indptr = np.zeros(self.k + 1, np.int64)
        rows = np.zeros(self.nonempty, np.int64)
        L.check(self.ctx.lib.stc_score_members(self.ctx.handle, self.handle, L.ptr(indptr, C.c_int64),
                                               L.ptr(rows, C.c_int64)))
        return indptr, rows

    def topTopics(self, n):
        """(topics int32[rows×N], weights float64[rows×N]), N = min(n, k): ``EmHandle.top_topics``' contract"""
        m = max(0, min(int(n), self.k))
        idx = np.zeros((self.num_rows, m), np.int32)
        w = np.zeros((self.num_rows, m), np.float64)
        L.check(self.ctx.lib.stc_score_top_topics(self.ctx.handle, self.handle, int(n), L.ptr(idx, C.c_int32),
                                                  L.ptr(w, C.c_double)))
        return idx, w

    def topDocuments(self, n):
        """(rows int64[k×N], weights float64[k×N]), N = min(n, non-empty rows): ``EmHandle.top_documents``' contract"""
        cap = max(0, min(int(n), self.num_rows))
        rows = np.zeros((self.k, cap), np.int64)
        w = np.zeros((self.k, cap), np.float64)
        got = C.c_int64()
        L.check(self.ctx.lib.stc_score_top_documents(self.ctx.handle, self.handle, int(n), C.byref(got),
                                                     L.ptr(rows, C.c_int64), L.ptr(w, C.c_double)))
        return rows[:, :got.value].copy(), w[:, :got.value].copy()

    def importantTerms(self, dataset, docTerms=100, topicTerms=300, n=10, topics=None):
        """(terms int32[rows×n] padded with −1, values float64[rows×n] padded with 0, counts int32[rows]): per row
        of ``dataset`` — the matrix that was scored — the first n of its docTerms largest entries (value descending,
        term ascending) whose term is among the topicTerms heaviest terms of the row's main topic (``topics``: of
        that topic instead; −1 skips the row).  LDALoader.scala:154-163 with its 100 / 300 / 10."""
        if self._lda is None:
            raise ValueError("importantTerms needs the scores of an LDA model (LdaHandle.score)")
        h = self._lda
        d, own = _as_device(self.ctx, dataset, h.dtype)
        try:
            width = max(0, int(n))
            idx = np.zeros((self.num_rows, width), np.int32)
            val = np.zeros((self.num_rows, width), np.float64)
            cnt = np.zeros(self.num_rows, np.int32)
            t = None if topics is None else L.as_i32(topics)
            if t is not None and t.shape != (self.num_rows,):
                raise ValueError("topics must have one entry per row")
            L.check(self.ctx.lib.stc_lda_important_terms(h.handle, d.handle, self.handle, L.ptr(t, C.c_int32),
                                                         int(docTerms), int(topicTerms), int(n), L.ptr(idx, C.c_int32),
                                                         L.ptr(val, C.c_double), L.ptr(cnt, C.c_int32)))
            return idx, val, cnt
        finally:
            if own:
                d.free()

    def close(self):
        if self.handle:
            self.ctx.lib.stc_score_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LdaHandle:
    """Owns one stc_lda (optimizer state + LocalLDAModel parameters on the GPU)."""

    def __init__(self, ctx: Context, k, vocab_size, doc_concentration=None, topic_concentration=-1.0,
                 tau0=1024.0, kappa=0.51, mini_batch_fraction=0.05, gamma_shape=100.0,
                 optimize_doc_concentration=True, sample_with_replacement=True, seed=0,
                 dtype="f64", max_inner_iter=0, mixed_resolve_iters=0):
        self.ctx = ctx
        cfg, self._alpha_buf = _lda_config(ctx.lib, k, vocab_size, doc_concentration, topic_concentration, tau0,
                                           kappa, mini_batch_fraction, gamma_shape, optimize_doc_concentration,
                                           sample_with_replacement, seed, dtype, max_inner_iter, mixed_resolve_iters)
        h = C.c_void_p()
        L.check(ctx.lib.stc_lda_create(ctx.handle, C.byref(cfg), C.byref(h)))
        self.handle = h
        self.k, self.vocab_size, self.dtype = cfg.k, cfg.vocab_size, cfg.dtype
        self.seed = cfg.seed
        self.gamma_shape = cfg.gamma_shape
        self._corpus = None

    # ---- state
    def set_corpus(self, corpus: DeviceCsr, corpus_size_total=None):
        total = corpus.num_rows if corpus_size_total is None else int(corpus_size_total)
        L.check(self.ctx.lib.stc_lda_set_corpus(self.handle, corpus.handle, total))
        self._corpus = corpus  # keep alive

    def init_random(self, seed):
        L.check(self.ctx.lib.stc_lda_init_random(self.handle, int(seed) & 0xFFFFFFFFFFFFFFFF))

    def set_topics(self, topics, layout=L.STC_LAYOUT_VK):
        t = L.as_f64(topics)
        L.check(self.ctx.lib.stc_lda_set_topics(self.handle, L.ptr(t, C.c_double), layout))

    def topics(self, layout=L.STC_LAYOUT_VK):
        shape = (self.vocab_size, self.k) if layout == L.STC_LAYOUT_VK else (self.k, self.vocab_size)
        out = np.zeros(shape, np.float64)
        L.check(self.ctx.lib.stc_lda_get_topics(self.handle, L.ptr(out, C.c_double), layout))
        return out

    def alpha(self):
        out = np.zeros(self.k, np.float64)
        L.check(self.ctx.lib.stc_lda_get_alpha(self.handle, L.ptr(out, C.c_double)))
        return out

    def set_alpha(self, a):
        a = L.as_f64(np.broadcast_to(np.asarray(a, np.float64), (self.k,)))
        L.check(self.ctx.lib.stc_lda_set_alpha(self.handle, L.ptr(a, C.c_double)))

    def eta(self):
        x = C.c_double()
        L.check(self.ctx.lib.stc_lda_get_eta(self.handle, C.byref(x)))
        return x.value

    def iteration(self):
        x = C.c_int64()
        L.check(self.ctx.lib.stc_lda_get_iteration(self.handle, C.byref(x)))
        return x.value

    # ---- optimizer
    def step(self, batch_ids, gamma0=None, stats=True):
        ids = L.as_i64(batch_ids)
        g0 = None if gamma0 is None else L.as_f64(gamma0)
        st = L.StepStats() if stats else None
        L.check(self.ctx.lib.stc_lda_step(self.handle, L.ptr(ids, C.c_int64), ids.size,
                                          L.ptr(g0, C.c_double), C.byref(st) if stats else None))
        return st.as_dict() if stats else None

    def next(self, stats=True):
        st = L.StepStats() if stats else None
        L.check(self.ctx.lib.stc_lda_next(self.handle, C.byref(st) if stats else None))
        return st.as_dict() if stats else None

    def estep(self, batch_ids, gamma0=None, want_stat=False):
        ids = L.as_i64(batch_ids)
        g0 = None if gamma0 is None else L.as_f64(gamma0)
        gamma = np.zeros((ids.size, self.k), np.float64)
        iters = np.zeros(ids.size, np.int32)
        stat = np.zeros((self.vocab_size, self.k), np.float64) if want_stat else None
        L.check(self.ctx.lib.stc_lda_estep(self.handle, L.ptr(ids, C.c_int64), ids.size, L.ptr(g0, C.c_double),
                                           L.ptr(gamma, C.c_double), L.ptr(stat, C.c_double),
                                           L.ptr(iters, C.c_int32)))
        return gamma, stat, iters

    # ---- LocalLDAModel
    def bound(self, docs: DeviceCsr, gamma_seed=0, doc_id_base=0, gamma0=None):
        g0 = None if gamma0 is None else L.as_f64(gamma0)
        b, cp, tp, tok = C.c_double(), C.c_double(), C.c_double(), C.c_double()
        L.check(self.ctx.lib.stc_lda_bound(self.handle, docs.handle, int(gamma_seed) & 0xFFFFFFFFFFFFFFFF,
                                           int(doc_id_base), L.ptr(g0, C.c_double), C.byref(b), C.byref(cp),
                                           C.byref(tp), C.byref(tok)))
        return {"bound": b.value, "corpus_part": cp.value, "topics_part": tp.value, "token_count": tok.value}

    def topic_distribution(self, docs: DeviceCsr, gamma_seed=0, doc_id_base=0, gamma0=None):
        g0 = None if gamma0 is None else L.as_f64(gamma0)
        out = np.zeros((docs.num_rows, self.k), np.float64)
        L.check(self.ctx.lib.stc_lda_topic_distribution(self.handle, docs.handle,
                                                        int(gamma_seed) & 0xFFFFFFFFFFFFFFFF, int(doc_id_base),
                                                        L.ptr(g0, C.c_double), L.ptr(out, C.c_double)))
        return out

    def score(self, docs: DeviceCsr, gamma_seed=0, doc_id_base=0, gamma0=None) -> DocumentScores:
        """the E-step of ``topic_distribution`` with γ kept on the GPU (stc_lda_score)"""
        g0 = None if gamma0 is None else L.as_f64(gamma0)
        h = C.c_void_p()
        L.check(self.ctx.lib.stc_lda_score(self.handle, docs.handle, int(gamma_seed) & 0xFFFFFFFFFFFFFFFF,
                                           int(doc_id_base), L.ptr(g0, C.c_double), C.byref(h)))
        return DocumentScores(self.ctx, h, self)

    def describe(self, max_terms=10):
        n = min(int(max_terms), self.vocab_size)
        idx = np.zeros((self.k, n), np.int32)
        w = np.zeros((self.k, n), np.float64)
        L.check(self.ctx.lib.stc_lda_describe(self.handle, int(max_terms), L.ptr(idx, C.c_int32),
                                              L.ptr(w, C.c_double)))
        return idx, w

    # ---- instrumentation
    def enable_timing(self, on=True):
        L.check(self.ctx.lib.stc_lda_enable_timing(self.handle, int(bool(on))))

    def phase_times(self):
        return _phase_times(self.ctx.lib, self.handle)

    def counters(self):
        return _counters(self.ctx.lib, self.handle)

    def close(self):
        if self.handle:
            self.ctx.lib.stc_lda_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LdaGroup:
    """Owns one stc_group: the LDA over several devices from ONE process (stc_group_create; the JVM
    drop-in's multi-GPU form).  The corpus is given on the host and sharded by the library; document ids
    are global.  ``devices`` repeating one device runs the multi-GPU decomposition on that device."""

    def __init__(self, devices, k, vocab_size, doc_concentration=None, topic_concentration=-1.0, tau0=1024.0,
                 kappa=0.51, mini_batch_fraction=0.05, gamma_shape=100.0, optimize_doc_concentration=True,
                 sample_with_replacement=True, seed=0, dtype="f64", max_inner_iter=0, mixed_resolve_iters=0):
        self.lib = L.load()
        cfg, self._alpha_buf = _lda_config(self.lib, k, vocab_size, doc_concentration, topic_concentration, tau0,
                                           kappa, mini_batch_fraction, gamma_shape, optimize_doc_concentration,
                                           sample_with_replacement, seed, dtype, max_inner_iter, mixed_resolve_iters)
        devs = np.ascontiguousarray(np.asarray(devices, np.int32))
        h = C.c_void_p()
        L.check(self.lib.stc_group_create(L.ptr(devs, C.c_int32), devs.size, C.byref(cfg), C.byref(h)))
        self.handle = h
        self.devices = devs.tolist()
        self.k, self.vocab_size = cfg.k, cfg.vocab_size

    @staticmethod
    def _csr(m: CsrMatrix):
        return (L.as_i64(m.indptr), np.ascontiguousarray(m.indices, np.int32), L.as_f64(m.values))

    def set_corpus(self, corpus: CsrMatrix):
        ip, ix, v = self._csr(corpus)
        L.check(self.lib.stc_group_set_corpus(self.handle, corpus.num_rows, corpus.num_cols, L.ptr(ip, C.c_int64),
                                              L.ptr(ix, C.c_int32), L.ptr(v, C.c_double)))

    def init_random(self, seed):
        L.check(self.lib.stc_group_init_random(self.handle, int(seed) & 0xFFFFFFFFFFFFFFFF))

    def set_topics(self, topics, layout=L.STC_LAYOUT_VK):
        t = L.as_f64(topics)
        L.check(self.lib.stc_group_set_topics(self.handle, L.ptr(t, C.c_double), layout))

    def topics(self, layout=L.STC_LAYOUT_VK):
        shape = (self.vocab_size, self.k) if layout == L.STC_LAYOUT_VK else (self.k, self.vocab_size)
        out = np.zeros(shape, np.float64)
        L.check(self.lib.stc_group_get_topics(self.handle, L.ptr(out, C.c_double), layout))
        return out

    def alpha(self):
        out = np.zeros(self.k, np.float64)
        L.check(self.lib.stc_group_get_alpha(self.handle, L.ptr(out, C.c_double)))
        return out

    def iteration(self):
        x = C.c_int64()
        L.check(self.lib.stc_group_get_iteration(self.handle, C.byref(x)))
        return x.value

    def release_corpus(self):
        """frees the training corpus shards (inference needs none; stc_group_release_corpus)"""
        L.check(self.lib.stc_group_release_corpus(self.handle))

    def synchronize(self):
        """waits for every member's queued work (stc_group_synchronize)"""
        L.check(self.lib.stc_group_synchronize(self.handle))

    def members(self):
        """the member stc_lda handles, for counters and timing only (stc_group_member)"""
        out = []
        for i in range(len(self.devices)):
            h = C.c_void_p()
            L.check(self.lib.stc_group_member(self.handle, i, C.byref(h)))
            out.append(h)
        return out

    def enable_timing(self, on=True):
        for h in self.members():
            L.check(self.lib.stc_lda_enable_timing(h, int(bool(on))))

    def phase_times(self):
        """per member: mean device ms per step of each phase"""
        return [_phase_times(self.lib, h) for h in self.members()]

    def counters(self):
        """per member: cumulative docs / entries / inner iterations / cap hits"""
        return [_counters(self.lib, h) for h in self.members()]

    def transport(self):
        """how the members' collectives travel: "none" (one member), "in-process" (one device repeated) or
        "rccl" (ncclCommInitAll over distinct devices — one included under STC_GROUP_RCCL=1)"""
        t = C.c_int32()
        L.check(self.lib.stc_group_transport(self.handle, C.byref(t)))
        return {L.STC_TRANSPORT_NONE: "none", L.STC_TRANSPORT_IN_PROCESS: "in-process",
                L.STC_TRANSPORT_RCCL: "rccl"}[t.value]

    def step(self, batch_ids, gamma0=None, stats=True):
        ids = L.as_i64(batch_ids)
        g0 = None if gamma0 is None else L.as_f64(gamma0)
        st = L.StepStats() if stats else None
        L.check(self.lib.stc_group_step(self.handle, L.ptr(ids, C.c_int64), ids.size, L.ptr(g0, C.c_double),
                                        C.byref(st) if stats else None))
        return st.as_dict() if stats else None

    def next(self, stats=True):
        st = L.StepStats() if stats else None
        L.check(self.lib.stc_group_next(self.handle, C.byref(st) if stats else None))
        return st.as_dict() if stats else None

    def describe(self, max_terms=10):
        n = min(int(max_terms), self.vocab_size)
        idx = np.zeros((self.k, n), np.int32)
        w = np.zeros((self.k, n), np.float64)
        L.check(self.lib.stc_group_describe(self.handle, int(max_terms), L.ptr(idx, C.c_int32), L.ptr(w, C.c_double)))
        return idx, w

    def bound(self, docs: CsrMatrix, gamma_seed=0, doc_id_base=0, gamma0=None):
        ip, ix, v = self._csr(docs)
        g0 = None if gamma0 is None else L.as_f64(gamma0)
        b, cp, tp, tok = C.c_double(), C.c_double(), C.c_double(), C.c_double()
        L.check(self.lib.stc_group_bound(self.handle, docs.num_rows, docs.num_cols, L.ptr(ip, C.c_int64),
                                         L.ptr(ix, C.c_int32), L.ptr(v, C.c_double),
                                         int(gamma_seed) & 0xFFFFFFFFFFFFFFFF, int(doc_id_base),
                                         L.ptr(g0, C.c_double), C.byref(b), C.byref(cp), C.byref(tp), C.byref(tok)))
        return {"bound": b.value, "corpus_part": cp.value, "topics_part": tp.value, "token_count": tok.value}

    def topic_distribution(self, docs: CsrMatrix, gamma_seed=0, doc_id_base=0, gamma0=None):
        ip, ix, v = self._csr(docs)
        g0 = None if gamma0 is None else L.as_f64(gamma0)
        out = np.zeros((docs.num_rows, self.k), np.float64)
        L.check(self.lib.stc_group_topic_distribution(self.handle, docs.num_rows, docs.num_cols, L.ptr(ip, C.c_int64),
                                                      L.ptr(ix, C.c_int32), L.ptr(v, C.c_double),
                                                      int(gamma_seed) & 0xFFFFFFFFFFFFFFFF, int(doc_id_base),
                                                      L.ptr(g0, C.c_double), L.ptr(out, C.c_double)))
        return out

    def close(self):
        if self.handle:
            self.lib.stc_group_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


_EM_DTYPES = {"f64": L.STC_F64, "float64": L.STC_F64, "f32": L.STC_F32, "float32": L.STC_F32}


def _em_dtype(dtype):
    """the state dtype code of an EM handle: "f64" or "f32" (EM has no mixed mode)"""
    if dtype not in _EM_DTYPES:
        raise ValueError(f"EM state dtype must be 'f64' or 'f32', but was {dtype!r}")
    return _EM_DTYPES[dtype]


def _em_state_dtype(lib, em_handle):
    """an stc_em's (a group member's) state dtype, read back from the library"""
    t = C.c_int32()
    L.check(lib.stc_em_state_dtype(em_handle, C.byref(t)))
    return {L.STC_F64: "f64", L.STC_F32: "f32"}[t.value]


class _EmRanked:
    """The ranked queries of an ``EmHandle`` (``_rank = "stc_em_"``) or ``EmGroup`` (``"stc_em_group_"``): device
    selections over the resident state, ties by ascending index (include/stc.h, "EM LDA, ranked queries")."""

    def _rank_call(self, name):
        return getattr(self._rank_lib(), self._rank + name)

    def describe(self, max_terms=10):
        """(terms int32[k×N], weights float64[k×N]), N = min(max_terms, V): per topic the terms with the largest
        N_wk[w][t], (count descending, term ascending), weights N_wk[w][t] / N_k[t]"""
        n = max(0, min(int(max_terms), self.vocab_size))
        idx = np.zeros((self.k, n), np.int32)
        w = np.zeros((self.k, n), np.float64)
        L.check(self._rank_call("describe")(self.handle, int(max_terms), L.ptr(idx, C.c_int32), L.ptr(w, C.c_double)))
        return idx, w

    def top_documents(self, max_docs):
        """(rows int64[k×N], weights float64[k×N]), N = min(max_docs, documents with an edge): per topic the corpus
        rows with the largest N_dk[d][t] / Σ_j N_dk[d][j], (weight descending, row ascending)"""
        cap = max(0, min(int(max_docs), self.num_docs))
        rows = np.zeros((self.k, cap), np.int64)
        w = np.zeros((self.k, cap), np.float64)
        n = C.c_int64()
        L.check(self._rank_call("top_documents")(self.handle, int(max_docs), C.byref(n), L.ptr(rows, C.c_int64),
                                                 L.ptr(w, C.c_double)))
        return rows[:, :n.value].copy(), w[:, :n.value].copy()

    def top_topics(self, n_topics):
        """(topics int32[D×N], weights float64[D×N]), N = min(n_topics, k): per document the topics with the largest
        N_dk[d][j], (count descending, topic ascending), weights N_dk[d][j] / Σ_j N_dk[d][j]; a document without an
        edge: topics 0 … N−1 with weight 0"""
        n = max(0, min(int(n_topics), self.k))
        idx = np.zeros((self.num_docs, n), np.int32)
        w = np.zeros((self.num_docs, n), np.float64)
        L.check(self._rank_call("top_topics")(self.handle, int(n_topics), L.ptr(idx, C.c_int32), L.ptr(w, C.c_double)))
        return idx, w


class EmHandle(_EmRanked):
    """Owns one stc_em: the EM optimizer's bipartite graph (built once from ``corpus``, which may be freed
    afterwards) and its state N_dk (D×k), N_wk (V×k), N_k on the GPU.  ``doc_concentration`` /
    ``topic_concentration``: −1 picks Spark's EM defaults 50/k + 1 and 1.1, anything else must be > 1.
    ``dtype``: "f64", or "f32" — N_dk and N_wk stored as fp32 (every new element rounded once, when stored),
    all arithmetic, N_k and the scores in fp64; the corpus stays STC_F64 and the state travels as float64."""

    _rank = "stc_em_"

    def _rank_lib(self):
        return self.ctx.lib

    def __init__(self, ctx: Context, corpus: DeviceCsr, k, doc_concentration=-1.0, topic_concentration=-1.0,
                 dtype="f64"):
        self.ctx = ctx
        self.handle = None
        code = _em_dtype(dtype)
        h = C.c_void_p()
        L.check(ctx.lib.stc_em_create_as(ctx.handle, corpus.handle, int(k), float(doc_concentration),
                                         float(topic_concentration), code, C.byref(h)))
        self.handle = h
        kk, d, v, e = C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()
        L.check(ctx.lib.stc_em_shape(h, C.byref(kk), C.byref(d), C.byref(v), C.byref(e)))
        self.k, self.num_docs, self.vocab_size, self.num_edges = kk.value, d.value, v.value, e.value
        self.dtype = _em_state_dtype(ctx.lib, h)

    def init_random(self, seed):
        L.check(self.ctx.lib.stc_em_init_random(self.handle, int(seed) & 0xFFFFFFFFFFFFFFFF))

    def set_state(self, doc_topics, term_topics):
        dt, tt = L.as_f64(doc_topics), L.as_f64(term_topics)
        if dt.shape != (self.num_docs, self.k) or tt.shape != (self.vocab_size, self.k):
            raise ValueError(f"state shapes {dt.shape}, {tt.shape}: expected ({self.num_docs}, {self.k}) and "
                             f"({self.vocab_size}, {self.k})")
        L.check(self.ctx.lib.stc_em_set_state(self.handle, L.ptr(dt, C.c_double), L.ptr(tt, C.c_double)))

    def state(self):
        """(N_dk D×k, N_wk V×k, N_k k); waits for queued iterations"""
        dt = np.zeros((self.num_docs, self.k), np.float64)
        tt = np.zeros((self.vocab_size, self.k), np.float64)
        nk = np.zeros(self.k, np.float64)
        L.check(self.ctx.lib.stc_em_get_state(self.handle, L.ptr(dt, C.c_double), L.ptr(tt, C.c_double),
                                              L.ptr(nk, C.c_double), None, None))
        return dt, tt, nk

    def concentrations(self):
        """the resolved (docConcentration α, topicConcentration η)"""
        a, e = C.c_double(), C.c_double()
        L.check(self.ctx.lib.stc_em_get_state(self.handle, None, None, None, C.byref(a), C.byref(e)))
        return a.value, e.value

    def next(self, n_iterations=1):
        """enqueues n EM iterations (does not wait for the GPU)"""
        L.check(self.ctx.lib.stc_em_next(self.handle, int(n_iterations)))

    def log_likelihood(self):
        """(logLikelihood, logPrior) of the current state"""
        ll, lp = C.c_double(), C.c_double()
        L.check(self.ctx.lib.stc_em_log_likelihood(self.handle, C.byref(ll), C.byref(lp)))
        return ll.value, lp.value

    def topic_assignments(self):
        """(indptr int64[D+1], terms int32[E], topics int32[E]): per edge of the filtered graph, in CSR order,
        the first topic with the largest factor under the current state; waits for queued iterations"""
        indptr = np.zeros(self.num_docs + 1, np.int64)
        terms = np.zeros(self.num_edges, np.int32)
        topics = np.zeros(self.num_edges, np.int32)
        L.check(self.ctx.lib.stc_em_topic_assignments(self.handle, L.ptr(indptr, C.c_int64), L.ptr(terms, C.c_int32),
                                                      L.ptr(topics, C.c_int32)))
        return indptr, terms, topics

    def close(self):
        if self.handle:
            self.ctx.lib.stc_em_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EmGroup(_EmRanked):
    """Owns one stc_em_group: the EM optimizer over several devices from ONE process.  The host ``corpus`` is
    sharded by the library (contiguous document ranges balanced by entries; document ids stay global); N_dk is
    kept by the member that owns the document, N_wk and N_k are replicated and all-reduced once per iteration.
    ``devices`` repeating one device runs that decomposition on the one device.  ``EmHandle``'s methods and
    attributes, over the whole corpus.  ``dtype`` "f32": every member stores its state as fp32 (``EmHandle``) and
    N_wk' is all-reduced as fp32."""

    _rank = "stc_em_group_"

    def _rank_lib(self):
        return self.lib

    def __init__(self, devices, corpus: CsrMatrix, k, doc_concentration=-1.0, topic_concentration=-1.0, dtype="f64"):
        self.handle = None
        code = _em_dtype(dtype)
        self.lib = L.load()
        devs = np.ascontiguousarray(np.asarray(devices, np.int32))
        ip, ix, v = L.as_i64(corpus.indptr), np.ascontiguousarray(corpus.indices, np.int32), L.as_f64(corpus.values)
        h = C.c_void_p()
        L.check(self.lib.stc_em_group_create_as(L.ptr(devs, C.c_int32), devs.size, corpus.num_rows, corpus.num_cols,
                                                L.ptr(ip, C.c_int64), L.ptr(ix, C.c_int32), L.ptr(v, C.c_double),
                                                int(k), float(doc_concentration), float(topic_concentration), code,
                                                C.byref(h)))
        self.handle = h
        self.devices = devs.tolist()
        kk, d, vv, e = C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()
        L.check(self.lib.stc_em_group_shape(h, C.byref(kk), C.byref(d), C.byref(vv), C.byref(e)))
        self.k, self.num_docs, self.vocab_size, self.num_edges = kk.value, d.value, vv.value, e.value
        self.dtype = _em_state_dtype(self.lib, self.members()[0][0])

    def members(self):
        """[(member stc_em handle, its first corpus row)], for reading only: stc_em_shape, stc_em_get_state"""
        out = []
        for i in range(len(self.devices)):
            h, r0 = C.c_void_p(), C.c_int64()
            L.check(self.lib.stc_em_group_member(self.handle, i, C.byref(h), C.byref(r0)))
            out.append((h, r0.value))
        return out

    def transport(self):
        """ "none" (one member), "in-process" (one device repeated) or "rccl" """
        t = C.c_int32()
        L.check(self.lib.stc_em_group_transport(self.handle, C.byref(t)))
        return {L.STC_TRANSPORT_NONE: "none", L.STC_TRANSPORT_IN_PROCESS: "in-process",
                L.STC_TRANSPORT_RCCL: "rccl"}[t.value]

    def synchronize(self):
        """waits for every member's queued iterations"""
        L.check(self.lib.stc_em_group_synchronize(self.handle))

    def init_random(self, seed):
        L.check(self.lib.stc_em_group_init_random(self.handle, int(seed) & 0xFFFFFFFFFFFFFFFF))

    def set_state(self, doc_topics, term_topics):
        dt, tt = L.as_f64(doc_topics), L.as_f64(term_topics)
        if dt.shape != (self.num_docs, self.k) or tt.shape != (self.vocab_size, self.k):
            raise ValueError(f"state shapes {dt.shape}, {tt.shape}: expected ({self.num_docs}, {self.k}) and "
                             f"({self.vocab_size}, {self.k})")
        L.check(self.lib.stc_em_group_set_state(self.handle, L.ptr(dt, C.c_double), L.ptr(tt, C.c_double)))

    def state(self):
        """(N_dk D×k gathered from the members, N_wk V×k and N_k k of member 0); waits for queued iterations"""
        dt = np.zeros((self.num_docs, self.k), np.float64)
        tt = np.zeros((self.vocab_size, self.k), np.float64)
        nk = np.zeros(self.k, np.float64)
        L.check(self.lib.stc_em_group_get_state(self.handle, L.ptr(dt, C.c_double), L.ptr(tt, C.c_double),
                                                L.ptr(nk, C.c_double), None, None))
        return dt, tt, nk

    def concentrations(self):
        """the resolved (docConcentration α, topicConcentration η)"""
        a, e = C.c_double(), C.c_double()
        L.check(self.lib.stc_em_group_get_state(self.handle, None, None, None, C.byref(a), C.byref(e)))
        return a.value, e.value

    def next(self, n_iterations=1):
        L.check(self.lib.stc_em_group_next(self.handle, int(n_iterations)))

    def log_likelihood(self):
        """(logLikelihood, logPrior) of the current state"""
        ll, lp = C.c_double(), C.c_double()
        L.check(self.lib.stc_em_group_log_likelihood(self.handle, C.byref(ll), C.byref(lp)))
        return ll.value, lp.value

    def topic_assignments(self):
        """(indptr int64[D+1], terms int32[E], topics int32[E]) in the whole corpus's filtered CSR order"""
        indptr = np.zeros(self.num_docs + 1, np.int64)
        terms = np.zeros(self.num_edges, np.int32)
        topics = np.zeros(self.num_edges, np.int32)
        L.check(self.lib.stc_em_group_topic_assignments(self.handle, L.ptr(indptr, C.c_int64), L.ptr(terms, C.c_int32),
                                                        L.ptr(topics, C.c_int32)))
        return indptr, terms, topics

    def close(self):
        if self.handle:
            self.lib.stc_em_group_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _as_device(ctx, data, dtype):
    if isinstance(data, DeviceCsr):
        return data, False
    return DeviceCsr.upload(ctx, data, L.corpus_dtype(dtype)), True


class LDAModel:
    """LocalLDAModel: topicsMatrix (V×k = λᵀ), docConcentration α, topicConcentration η."""

    def __init__(self, handle: LdaHandle, gamma_seed=None):
        self._h = handle
        self.k = handle.k
        self.vocabSize = handle.vocab_size
        self.gammaSeed = handle.seed if gamma_seed is None else gamma_seed

    @staticmethod
    def from_topics(topics_matrix, doc_concentration, topic_concentration, gamma_shape=100.0,
                    seed=0, dtype="f64", ctx: Context | None = None):
        """Build a LocalLDAModel from an existing V×k topicsMatrix (e.g. DistributedLDAModel.toLocal)."""
        tm = np.asarray(topics_matrix, np.float64)
        ctx = ctx or Context.get()
        h = LdaHandle(ctx, tm.shape[1], tm.shape[0], doc_concentration=doc_concentration,
                      topic_concentration=topic_concentration, gamma_shape=gamma_shape, seed=seed,
                      dtype=dtype)
        h.set_topics(tm)
        return LDAModel(h)

    def isDistributed(self):
        return False

    def topicsMatrix(self):
        return self._h.topics(L.STC_LAYOUT_VK)

    def estimatedDocConcentration(self):
        return self._h.alpha()

    def getTopicConcentration(self):
        return self._h.eta()

    def describeTopics(self, maxTermsPerTopic=10):
        """[(topic, termIndices, termWeights)] like the ml DataFrame rows."""
        idx, w = self._h.describe(maxTermsPerTopic)
        return [(t, idx[t].astype(np.int64), w[t]) for t in range(self.k)]

    def logLikelihood(self, dataset, gamma0=None):
        d, own = _as_device(self._h.ctx, dataset, self._h.dtype)
        try:
            return self._h.bound(d, self.gammaSeed, 0, gamma0)["bound"]
        finally:
            if own:
                d.free()

    def logPerplexity(self, dataset, gamma0=None):
        d, own = _as_device(self._h.ctx, dataset, self._h.dtype)
        try:
            b = self._h.bound(d, self.gammaSeed, 0, gamma0)
            return -b["bound"] / b["token_count"]
        finally:
            if own:
                d.free()

    def transform(self, dataset, gamma0=None):
        """topicDistribution of every row (LDALoader.scala:108); zeros for empty rows."""
        d, own = _as_device(self._h.ctx, dataset, self._h.dtype)
        try:
            return self._h.topic_distribution(d, self.gammaSeed, 0, gamma0)
        finally:
            if own:
                d.free()

    topicDistribution = transform

    def score(self, dataset, gamma0=None) -> DocumentScores:
        """``transform``'s E-step with the result kept on the GPU: main topics, members, ranked lists and important
        terms are device queries of the returned ``DocumentScores``"""
        d, own = _as_device(self._h.ctx, dataset, self._h.dtype)
        try:
            return self._h.score(d, self.gammaSeed, 0, gamma0)
        finally:
            if own:
                d.free()

    def report(self, dataset, vocabulary=None, docTerms=100, topicTerms=300, n=10, gamma0=None):
        """LDALoader's report (LDALoader.scala:108-163, :171-199) as plain data, written nowhere:
        ``{"documents": [{"row", "topicDistribution", "mainTopic", "mainTopicWeight", "importantTerms",
        "importantTermValues"}], "topics": [{"topic", "count", "rows"}]}``.  importantTerms holds strings when a
        vocabulary (term index → string) is given, else term indices; an empty row has mainTopic −1 and no terms."""
        d, own = _as_device(self._h.ctx, dataset, self._h.dtype)
        try:
            s = self._h.score(d, self.gammaSeed, 0, gamma0)
            try:
                theta = s.topicDistribution()
                topic, weight, counts = s.mainTopics()
                indptr, rows = s.members()
                idx, val, cnt = s.importantTerms(d, docTerms, topicTerms, n)
            finally:
                s.close()
        finally:
            if own:
                d.free()
        name = (lambda i: int(i)) if vocabulary is None else (lambda i: vocabulary[int(i)])
        docs = [{"row": r, "topicDistribution": theta[r], "mainTopic": int(topic[r]), "mainTopicWeight": float(weight[r]),
                 "importantTerms": [name(i) for i in idx[r, :cnt[r]]], "importantTermValues": val[r, :cnt[r]].copy()}
                for r in range(theta.shape[0])]
        topics = [{"topic": t, "count": int(counts[t]), "rows": rows[indptr[t]:indptr[t + 1]].copy()}
                  for t in range(self.k)]
        return {"documents": docs, "topics": topics}

    def topicCoherence(self, dataset, topN=10, measure="umass", eps=1.0):
        """float64[k]: the UMass ("umass") or document-level NPMI ("npmi") coherence of each topic's ``topN`` terms
        (``describeTopics``' lists) over ``dataset``, counted on the GPU (``stc.term_cooccurrence``)"""
        topN = check_top_n(topN)
        return topic_coherence(self.describeTopics(topN), dataset, measure, eps, self._h.ctx)

    # ---- persistence: [U] LocalLDAModel.save / LocalLDAModel.load (SaveLoadV1_0 layout, stc.io)
    def save(self, path, overwrite=False):
        """Write this model as a Spark mllib LocalLDAModel directory (stock Spark can load it)."""
        from . import io

        io.save_local(path, self.topicsMatrix(), self.estimatedDocConcentration(), self.getTopicConcentration(),
                      self._h.gamma_shape, overwrite=overwrite)

    @staticmethod
    def load(path, dtype="f64", seed=0, ctx: Context | None = None) -> "LDAModel":
        """Read a Spark mllib LocalLDAModel directory onto the GPU."""
        from . import io

        m = io.load_local(path)
        return LDAModel.from_topics(m["topics"], m["alpha"], m["eta"], gamma_shape=m["gamma_shape"], seed=seed,
                                    dtype=dtype, ctx=ctx)


class DistributedLDAModel:
    """[U] DistributedLDAModel as the reference loads it (LDALoader.scala:37): the saved EM graph, read
    from its parquet layout (stc.io).  What the reference then asks of it — describeTopics
    (LDALoader.scala:66) and toLocal.topicDistribution (:108) — runs on the GPU through ``toLocal``
    (topicsMatrix = the term vertices' counts n_wk).

    It is also what ``MllibLDA.run`` returns under the EM optimizer (LDAClustering.scala:41, :61-63): the
    trained graph's state read back from its ``EmHandle``.  ``logLikelihood`` / ``logPrior``
    (LDAClustering.scala:75) and ``topicAssignments`` run on the GPU; a loaded model builds its ``EmHandle`` from the stored edges
    and state on first use, so the reference's own saved models can be scored."""

    def __init__(self, data, em: "EmHandle | EmGroup | None" = None):
        self._d = data
        self.k, self.vocabSize = data["k"], data["vocab_size"]
        self.docConcentration = data["alpha"]
        self.topicConcentration = data["eta"]
        self.gammaShape = data["gamma_shape"]
        self.iterationTimes = data["iteration_times"]
        self._local = {}
        self._em = em
        self._em_rows_are_ids = em is not None  # the trainer's graph: row = document id; a rebuilt one: its rank

    @staticmethod
    def _from_em(em: "EmHandle | EmGroup", corpus: CsrMatrix, iteration_times,
                 gamma_shape=100.0) -> "DistributedLDAModel":
        """the model of a trained EmHandle or EmGroup over the host copy of its corpus (vertex id = row index)"""
        ndk, nwk, nk = em.state()
        alpha, eta = em.concentrations()
        keep = corpus.values != 0.0
        src = np.repeat(np.arange(corpus.num_rows, dtype=np.int64), np.diff(corpus.indptr))[keep]
        doc_ids = np.unique(src)
        return DistributedLDAModel({
            "topics": nwk, "global_topic_totals": nk, "doc_ids": doc_ids, "doc_topics": ndk[doc_ids],
            "edges": (src, corpus.indices[keep].astype(np.int64), corpus.values[keep]),
            "alpha": np.full(em.k, alpha), "eta": eta, "gamma_shape": float(gamma_shape),
            "iteration_times": np.asarray(iteration_times, np.float64), "k": em.k, "vocab_size": em.vocab_size}, em=em)

    def _edge_rows(self) -> CsrMatrix:
        """the stored edges as rows, one per document vertex in ``doc_ids``' order (the training corpus)"""
        d = self._d
        src, term, cnt = d["edges"]
        row = np.searchsorted(d["doc_ids"], src)
        if row.size and (row.max() >= d["doc_ids"].size or np.any(d["doc_ids"][row] != src)):
            raise ValueError("an edge names a document that has no vertex")
        order = np.argsort(row, kind="stable")
        indptr = np.zeros(d["doc_ids"].size + 1, np.int64)
        np.cumsum(np.bincount(row, minlength=d["doc_ids"].size), out=indptr[1:])
        return CsrMatrix(indptr, term[order], cnt[order], self.vocabSize)

    def _em_handle(self, ctx: Context | None = None) -> "EmHandle | EmGroup":
        """the GPU graph of this model: the trainer's, or one built from the stored edges and state"""
        if self._em is None:
            d = self._d
            alpha = np.asarray(d["alpha"], np.float64)
            if np.any(alpha != alpha[0]):
                raise ValueError("an EM model has a symmetric docConcentration")
            rows = self._edge_rows()
            ctx = ctx or Context.get()
            dev = DeviceCsr.upload(ctx, rows, L.STC_F64)
            try:
                em = EmHandle(ctx, dev, self.k, float(alpha[0]), float(d["eta"]))
            finally:
                dev.free()
            em.set_state(d["doc_topics"], d["topics"])
            self._em = em
        return self._em

    def logLikelihood(self, ctx: Context | None = None):
        """[U] DistributedLDAModel.logLikelihood: Σ_edges c · ln(φ_w · θ_d) of the training corpus"""
        return self._em_handle(ctx).log_likelihood()[0]

    def logPrior(self, ctx: Context | None = None):
        """[U] DistributedLDAModel.logPrior: ln P(topics, topic distributions | α, η) up to its constant"""
        return self._em_handle(ctx).log_likelihood()[1]

    def topicAssignments(self, ctx: Context | None = None):
        """[U] DistributedLDAModel.topicAssignments: [(document id, terms int32[], topics int32[])], one entry
        per document vertex in ``topicDistributions``' order; per (document, term) edge, terms ascending, the
        first topic with the largest (N_wk[w][j] + η−1)(N_dk[d][j] + α−1) / (N_k[j] + V(η−1)), on the GPU"""
        indptr, terms, topics = self._em_handle(ctx).topic_assignments()
        ids = self._d["doc_ids"]
        rows = ids if self._em_rows_are_ids else np.arange(ids.size)
        return [(int(d), terms[indptr[r]:indptr[r + 1]].copy(), topics[indptr[r]:indptr[r + 1]].copy())
                for d, r in zip(ids, rows)]

    javaTopicAssignments = topicAssignments

    def topicDistributions(self):
        """(document ids, D'×k matrix): N_dk[d] / Σ_j N_dk[d][j] for every document vertex"""
        dt = self._d["doc_topics"]
        return self._d["doc_ids"].copy(), dt / dt.sum(axis=1, keepdims=True)

    def topTopicsPerDocument(self, k, device=False, ctx: Context | None = None):
        """[(document id, topic indices, topic weights)], each document's top k topics by weight descending.
        ``device=True``: a selection on the model's EM graph on the GPU (``EmHandle.top_topics``: ranked by the
        count, ties to the smaller topic) instead of a sort of the host copy"""
        if device:
            idx, w = self._em_handle(ctx).top_topics(k)
            ids = self._d["doc_ids"]
            rows = ids if self._em_rows_are_ids else np.arange(ids.size)
            return [(int(d), idx[r].astype(np.int64), w[r]) for d, r in zip(ids, rows)]
        ids, td = self.topicDistributions()
        n = min(int(k), self.k)
        top = np.argsort(-td, axis=1, kind="stable")[:, :n]
        return [(int(ids[i]), top[i], td[i, top[i]]) for i in range(ids.size)]

    def topDocumentsPerTopic(self, maxDocumentsPerTopic, device=False, ctx: Context | None = None):
        """[(document ids, weights)] per topic: the documents with the largest weight of it, descending.
        ``device=True``: a selection on the model's EM graph on the GPU (``EmHandle.top_documents``: ties to the
        smaller row, which is the smaller document id) instead of k sorts of the host copy"""
        if device:
            rows, w = self._em_handle(ctx).top_documents(maxDocumentsPerTopic)
            ids = rows if self._em_rows_are_ids else self._d["doc_ids"][rows]
            return [(ids[t].astype(self._d["doc_ids"].dtype), w[t]) for t in range(self.k)]
        ids, td = self.topicDistributions()
        n = min(int(maxDocumentsPerTopic), ids.size)
        out = []
        for t in range(self.k):
            top = np.argsort(-td[:, t], kind="stable")[:n]
            out.append((ids[top], td[top, t]))
        return out

    def save(self, path, overwrite=False):
        """Write this model as a Spark mllib DistributedLDAModel directory (stc.io.save_distributed)."""
        from . import io

        d = self._d
        io.save_distributed(path, d["doc_ids"], d["doc_topics"], d["topics"], d["edges"], d["alpha"], d["eta"],
                            gamma_shape=d["gamma_shape"], iteration_times=d["iteration_times"], overwrite=overwrite)

    @staticmethod
    def load(path) -> "DistributedLDAModel":
        from . import io

        return DistributedLDAModel(io.load_distributed(path))

    def isDistributed(self):
        return True

    def topicsMatrix(self):
        return self._d["topics"].copy()

    def globalTopicTotals(self):
        return self._d["global_topic_totals"].copy()

    def toLocal(self, dtype="f64", seed=0, ctx: Context | None = None) -> LDAModel:
        key = (dtype, seed, id(ctx))
        if key not in self._local:
            self._local[key] = LDAModel.from_topics(self._d["topics"], self.docConcentration, self.topicConcentration,
                                                    gamma_shape=self.gammaShape, seed=seed, dtype=dtype, ctx=ctx)
        return self._local[key]

    def describeTopics(self, maxTermsPerTopic=10, ctx: Context | None = None, device=False):
        """Top terms per topic by n_wk / Σ_w n_wk (the EM model's column totals), on the GPU.
        ``device=True``: a selection over the N_wk of the model's EM graph (``EmHandle.describe``) instead of an
        upload into a local model and its full sort"""
        if device:
            idx, w = self._em_handle(ctx).describe(maxTermsPerTopic)
            return [(t, idx[t].astype(np.int64), w[t]) for t in range(self.k)]
        return self.toLocal(ctx=ctx).describeTopics(maxTermsPerTopic)

    def topicCoherence(self, dataset=None, topN=10, measure="umass", eps=1.0, ctx: Context | None = None):
        """float64[k]: ``LDAModel.topicCoherence`` for the terms of ``describeTopics(topN, device=True)``;
        ``dataset=None`` counts over the model's own stored edges, the corpus it was trained on"""
        topN = check_top_n(topN)
        described = self.describeTopics(topN, ctx=ctx, device=True)
        return topic_coherence(described, self._edge_rows() if dataset is None else dataset, measure, eps, ctx)


class LDA:
    """ml.clustering.LDA estimator (optimizer="online" only)."""

    def __init__(self, k=10, maxIter=20, optimizer="online", learningOffset=1024.0, learningDecay=0.51,
                 subsamplingRate=0.05, optimizeDocConcentration=True, docConcentration=None,
                 topicConcentration=None, seed=ML_LDA_DEFAULT_SEED, featuresCol="features",
                 topicDistributionCol="topicDistribution", dtype="f64", maxInnerIter=0,
                 ctx: Context | None = None):
        self.setK(k).setMaxIter(maxIter).setOptimizer(optimizer).setLearningOffset(learningOffset)
        self.setLearningDecay(learningDecay).setSubsamplingRate(subsamplingRate)
        self.optimizeDocConcentration = bool(optimizeDocConcentration)
        self.docConcentration = docConcentration
        self.topicConcentration = topicConcentration
        self.seed = int(seed)
        self.featuresCol, self.topicDistributionCol = featuresCol, topicDistributionCol
        self.dtype = dtype
        self.maxInnerIter = int(maxInnerIter)
        self._ctx = ctx
        self.iterationTimes = []

    def setK(self, k):
        if int(k) <= 1:
            raise ValueError(f"LDA k (number of clusters) must be > 1, but was set to {k}")
        self.k = int(k)
        return self

    def setMaxIter(self, n):
        if int(n) < 0:
            raise ValueError(f"maxIter must be >= 0 but got {n}")
        self.maxIter = int(n)
        return self

    def setOptimizer(self, o):
        if str(o).lower() != "online":
            raise ValueError(f"Only online is supported by this build but got {o}.")
        self.optimizer = "online"
        return self

    def setLearningOffset(self, v):
        if float(v) <= 0:
            raise ValueError(f"learningOffset must be > 0 but got {v}")
        self.learningOffset = float(v)
        return self

    def setLearningDecay(self, v):
        if float(v) <= 0:
            raise ValueError(f"learningDecay must be > 0 but got {v}")
        self.learningDecay = float(v)
        return self

    def setSubsamplingRate(self, v):
        if not (0.0 < float(v) <= 1.0):
            raise ValueError(f"subsamplingRate must be in range (0, 1] but got {v}")
        self.subsamplingRate = float(v)
        return self

    def setSeed(self, s):
        self.seed = int(s)
        return self

    def fit(self, dataset, corpus_size_total=None) -> LDAModel:
        ctx = self._ctx or Context.get()
        d, _ = _as_device(ctx, dataset, _DTYPES[self.dtype])
        total = d.num_rows
        if corpus_size_total is None and ctx.n_ranks > 1:
            total = int(ctx.allreduce([float(d.num_rows)])[0])
        elif corpus_size_total is not None:
            total = int(corpus_size_total)
        h = LdaHandle(ctx, self.k, d.num_cols, doc_concentration=self.docConcentration,
                      topic_concentration=self.topicConcentration, tau0=self.learningOffset,
                      kappa=self.learningDecay, mini_batch_fraction=self.subsamplingRate,
                      optimize_doc_concentration=self.optimizeDocConcentration, seed=self.seed,
                      dtype=self.dtype, max_inner_iter=self.maxInnerIter)
        h.set_corpus(d, total)
        h.init_random(self.seed)
        import time
        self.iterationTimes = []
        for _ in range(self.maxIter):
            t0 = time.perf_counter()
            h.next(stats=False)
            ctx.synchronize()
            self.iterationTimes.append(time.perf_counter() - t0)
        return LDAModel(h)


class OnlineLDAOptimizer:
    """mllib OnlineLDAOptimizer setters (defaults: tau0 1024, kappa 0.51, fraction 0.05,
    optimizeDocConcentration false, gammaShape 100, sampleWithReplacement true)."""

    def __init__(self):
        self.tau0, self.kappa, self.miniBatchFraction = 1024.0, 0.51, 0.05
        self.optimizeDocConcentration, self.gammaShape, self.sampleWithReplacement = False, 100.0, True

    def setTau0(self, v):
        if v <= 0:
            raise ValueError(f"LDA tau0 must be positive, but was set to {v}")
        self.tau0 = float(v)
        return self

    def setKappa(self, v):
        if v < 0:
            raise ValueError(f"Online LDA kappa must be nonnegative, but was set to {v}")
        self.kappa = float(v)
        return self

    def setMiniBatchFraction(self, v):
        if not (0.0 < v <= 1.0):
            raise ValueError(f"Online LDA miniBatchFraction must be in range (0,1], but was set to {v}")
        self.miniBatchFraction = float(v)
        return self

    def setOptimizeDocConcentration(self, b):
        self.optimizeDocConcentration = bool(b)
        return self

    def setGammaShape(self, v):
        self.gammaShape = float(v)
        return self

    def setSampleWithReplacement(self, b):
        self.sampleWithReplacement = bool(b)
        return self


class EMLDAOptimizer:
    """mllib EMLDAOptimizer (``new EMLDAOptimizer``, LDAClustering.scala:41).  keepLastCheckpoint concerns
    Spark's RDD lineage only: accepted and inert here."""

    def __init__(self):
        self.keepLastCheckpoint = True

    def getKeepLastCheckpoint(self):
        return self.keepLastCheckpoint

    def setKeepLastCheckpoint(self, b):
        self.keepLastCheckpoint = bool(b)
        return self


def em_concentrations(k, docConcentration=-1.0, topicConcentration=-1.0):
    """[U] EMLDAOptimizer.initialize's parameter rules → (α, η): a symmetric docConcentration (a scalar or k
    equal values; −1 ⇒ 50/k + 1) and a topicConcentration (−1 ⇒ 1.1), both > 1 otherwise."""
    a = np.atleast_1d(np.asarray(-1.0 if docConcentration is None else docConcentration, np.float64))
    if a.size not in (1, int(k)):
        raise ValueError(f"docConcentration must have 1 or k = {k} values but has {a.size}")
    if np.any(a != a[0]):
        raise ValueError("EMLDAOptimizer currently only supports symmetric document-topic priors")
    alpha = float(a[0])
    eta = float(-1.0 if topicConcentration is None else topicConcentration)
    if alpha == -1.0:
        alpha = 50.0 / int(k) + 1.0
    elif not alpha > 1.0:
        raise ValueError(f"For EM optimizer, docConcentration must be > 1.0 (or -1 for auto) but was set to {alpha}")
    if eta == -1.0:
        eta = 1.1
    elif not eta > 1.0:
        raise ValueError(f"For EM optimizer, topicConcentration must be > 1.0 (or -1 for auto) but was set to {eta}")
    return alpha, eta


class MllibLDA:
    """mllib.clustering.LDA as driven at LDAClustering.scala:37-61: the optimizer switch of :40-46 takes
    ``"em"`` / ``EMLDAOptimizer`` (the reference's default) or ``"online"`` / ``OnlineLDAOptimizer``.
    ``devices`` (or ``setDevices``): the EM optimizer trains over those devices through an ``EmGroup``."""

    def __init__(self, ctx: Context | None = None, devices=None):
        self.k, self.maxIterations, self.docConcentration, self.topicConcentration = 10, 20, -1.0, -1.0
        self.seed = _java_string_hash("org.apache.spark.mllib.clustering.LDA")
        self.optimizer = OnlineLDAOptimizer()
        self.checkpointInterval = 10
        self.dtype = "f64"
        self._ctx = ctx
        self.devices = None if devices is None else [int(d) for d in devices]

    def setDevices(self, devices):
        """the devices the EM optimizer trains over (one repeated: the same decomposition on that device);
        None: the context's device alone"""
        self.devices = None if devices is None else [int(d) for d in devices]
        return self

    def setOptimizer(self, opt):
        if isinstance(opt, str):
            if opt.lower() not in ("em", "online"):
                raise ValueError(f"Only em, online are supported but got {opt}.")
            opt = EMLDAOptimizer() if opt.lower() == "em" else OnlineLDAOptimizer()
        self.optimizer = opt
        return self

    def setK(self, k):
        if int(k) <= 1:
            raise ValueError(f"LDA k (number of clusters) must be > 1, but was set to {k}")
        self.k = int(k)
        return self

    def setMaxIterations(self, n):
        if int(n) < 0:
            raise ValueError(f"Maximum of iterations must be nonnegative, but was set to {n}")
        self.maxIterations = int(n)
        return self

    def setDocConcentration(self, a):
        self.docConcentration = a
        return self

    def setTopicConcentration(self, e):
        self.topicConcentration = float(e)
        return self

    def setCheckpointInterval(self, n):
        self.checkpointInterval = int(n)  # EM-only in Spark; accepted and ignored here
        return self

    def setSeed(self, s):
        self.seed = int(s)
        return self

    def _run_em(self, corpus) -> DistributedLDAModel:
        """EMLDAOptimizer.initialize, maxIterations × next, getLDAModel (a DistributedLDAModel)"""
        import time

        _em_dtype(self.dtype)  # "mixed" is the online optimizer's: EM has no mixed mode
        alpha, eta = em_concentrations(self.k, self.docConcentration, self.topicConcentration)
        if self.devices is not None:
            host = corpus.download() if isinstance(corpus, DeviceCsr) else corpus
            em = EmGroup(self.devices, host, self.k, alpha, eta, dtype=self.dtype)
            em.init_random(self.seed)
            em.synchronize()
            self.iterationTimes = []
            for _ in range(self.maxIterations):
                t0 = time.perf_counter()
                em.next(1)
                em.synchronize()
                self.iterationTimes.append(time.perf_counter() - t0)
            return DistributedLDAModel._from_em(em, host, self.iterationTimes)
        ctx = self._ctx or Context.get()
        if isinstance(corpus, DeviceCsr):
            dev, host = corpus, corpus.download()
        else:
            dev, host = DeviceCsr.upload(ctx, corpus, L.STC_F64), corpus
        try:
            em = EmHandle(ctx, dev, self.k, alpha, eta, dtype=self.dtype)
        finally:
            if dev is not corpus:
                dev.free()
        em.init_random(self.seed)
        ctx.synchronize()
        self.iterationTimes = []
        for _ in range(self.maxIterations):
            t0 = time.perf_counter()
            em.next(1)
            ctx.synchronize()
            self.iterationTimes.append(time.perf_counter() - t0)
        return DistributedLDAModel._from_em(em, host, self.iterationTimes)

    def run(self, corpus):
        """lda.run(corpus): a ``DistributedLDAModel`` under the EM optimizer, an ``LDAModel`` under the online one"""
        o = self.optimizer
        if isinstance(o, EMLDAOptimizer):
            return self._run_em(corpus)
        ctx = self._ctx or Context.get()
        d, _ = _as_device(ctx, corpus, _DTYPES[self.dtype])
        total = int(ctx.allreduce([float(d.num_rows)])[0]) if ctx.n_ranks > 1 else d.num_rows
        h = LdaHandle(ctx, self.k, d.num_cols, doc_concentration=self.docConcentration,
                      topic_concentration=self.topicConcentration, tau0=o.tau0, kappa=o.kappa,
                      mini_batch_fraction=o.miniBatchFraction, gamma_shape=o.gammaShape,
                      optimize_doc_concentration=o.optimizeDocConcentration,
                      sample_with_replacement=o.sampleWithReplacement, seed=self.seed, dtype=self.dtype)
        h.set_corpus(d, total)
        h.init_random(self.seed)
        for _ in range(self.maxIterations):
            h.next(stats=False)
        return LDAModel(h)


def reference_mini_batch_fraction(corpus_size):
    """LDAClustering.scala:43: 0.05 + 1.0 / actualCorpusSize."""
    return 0.05 + 1.0 / float(corpus_size)


def rho(tau0, kappa, iteration):
    return math.pow(tau0 + iteration, -kappa)
