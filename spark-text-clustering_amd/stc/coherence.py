"""Topic coherence: do a topic's top terms occur in the same documents (include/stc.h "Topic coherence").

The reference judges a trained model by eye, from each topic's ten top-weighted terms (LDALoader.scala:66-69,
177-187).  UMass (Mimno et al. 2011) and document-level NPMI are the standard numbers for that reading; both are
functions of document co-occurrence counts of the top terms.  ``term_cooccurrence`` counts on the GPU over a resident
corpus (integers, exact); ``coherence`` is host arithmetic and needs no GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .core import Context, CsrMatrix, DeviceCsr

STC_COH_UMASS, STC_COH_NPMI = 0, 1
MEASURES = {"umass": STC_COH_UMASS, "npmi": STC_COH_NPMI}
MAX_TERMS = 64  # one 64-bit mask per topic on the device


def term_cooccurrence(docs, terms, ctx: Context | None = None):
    """(df int64[k, n], codf int64[k, n, n], n_docs) of the term lists ``terms`` (int32[k, n], −1 = unused slot) over
    ``docs``: a ``DeviceCsr``, or a ``CsrMatrix`` that is uploaded for the call and freed.  A document contains a
    term iff its row has an entry of it with value > 0."""
    t = L.as_i32(terms)
    if t.ndim != 2:
        raise ValueError("terms must be a k×n matrix")
    k, n = t.shape
    own = not isinstance(docs, DeviceCsr)
    if own:
        ctx = ctx or Context.get()
        docs = DeviceCsr.upload(ctx, docs, L.STC_F64)
    else:
        ctx = ctx or docs.ctx
    try:
        df = np.zeros((k, n), np.int64)
        codf = np.zeros((k, n, n), np.int64)
        m = C.c_int64()
        L.check(ctx.lib.stc_term_cooccurrence(ctx.handle, docs.handle, L.ptr(t, C.c_int32), k, n, L.ptr(df, C.c_int64),
                                              L.ptr(codf, C.c_int64), C.byref(m)))
    finally:
        if own:
            docs.free()
    return df, codf, m.value


def coherence(df, codf, n_docs, measure="umass", eps=1.0):
    """(float64[k], pairs int32[k]): per topic the UMass sum Σ ln((codf[m][l] + eps) / df[l]) or the NPMI mean over
    the pairs l < m whose two terms both occur in the corpus; ``pairs`` counts them.  Host only."""
    if measure not in MEASURES:
        raise ValueError(f"measure must be one of {sorted(MEASURES)}")
    df = L.as_i64(df)
    codf = L.as_i64(codf)
    if df.ndim != 2 or codf.shape != df.shape + (df.shape[1],):
        raise ValueError("df must be k×n and codf k×n×n")
    k, n = df.shape
    out = np.zeros(k, np.float64)
    pairs = np.zeros(k, np.int32)
    L.check(L.load().stc_coherence(L.ptr(df, C.c_int64), L.ptr(codf, C.c_int64), k, n, int(n_docs), MEASURES[measure],
                                   float(eps), L.ptr(out, C.c_double), L.ptr(pairs, C.c_int32)))
    return out, pairs


def check_top_n(topN):
    """the topN a model's topicCoherence accepts: a pair at the least, the device mask's 64 bits at the most"""
    topN = int(topN)
    if topN < 2 or topN > MAX_TERMS:
        raise ValueError(f"topN must be in 2 … {MAX_TERMS}")
    return topN


def topic_coherence(described, docs, measure, eps, ctx: Context | None = None):
    """float64[k] from a model's describeTopics rows [(topic, termIndices, termWeights)] counted over ``docs``"""
    if measure not in MEASURES:
        raise ValueError(f"measure must be one of {sorted(MEASURES)}")
    terms = np.stack([np.asarray(idx, np.int32) for _, idx, _ in described])
    df, codf, n_docs = term_cooccurrence(docs, terms, ctx)
    return coherence(df, codf, n_docs, measure, eps)[0]
