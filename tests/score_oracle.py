"""NumPy restatement of the document scores (include/stc.h, "Document scores"; csrc/lda_score.hip).

A score is (γ, rowsum): γ rows×k fp64 with the rows marked empty stored as 0, rowsum[r] = ((|γ₀|+|γ₁|)+…) added
sequentially in ascending j (``np.cumsum``), −1 for an empty row.  θ = γ / rowsum (γ itself where the sum is 0).

* main topic: the largest θ, among equal maxima the largest index (LDALoader.scala:133-139, ``<=``); an empty
  row: topic −1, weight 0.
* members: the non-empty rows grouped by main topic, ascending inside a topic.
* top topics / top documents: tests/em_rank_oracle.py on (γ, rowsum != −1).
* important terms: L_d = the first doc_terms entries of the row by (value descending, term ascending); S_t = the
  topic_terms terms with the largest λ[w][t] (ties by ascending term); the first max_out entries of L_d whose term
  is in S_t, in L_d's order (Scala's ``slice(0, 100).intersect(topicVocab).slice(0, 10)``).
"""
import numpy as np

import em_rank_oracle as R


def build(gamma, empty=None):
    """(γ with the empty rows zeroed, rowsum)"""
    g = np.array(gamma, np.float64, ndmin=2)
    rows = g.shape[0]
    e = np.zeros(rows, bool) if empty is None else np.asarray(empty).astype(bool)
    g[e] = 0.0
    s = np.cumsum(np.abs(g), axis=1)[:, -1] if rows else np.zeros(0)
    s = np.where(e, -1.0, s)
    return g, s


def theta(g, s):
    return np.where(s[:, None] > 0.0, g / np.where(s > 0.0, s, 1.0)[:, None], g)


def main_topics(g, s):
    """(topic int32[rows], weight[rows], counts int64[k])"""
    rows, k = g.shape
    th = theta(g, s)
    topic = (k - 1 - np.argmax(th[:, ::-1], axis=1)).astype(np.int32) if rows else np.zeros(0, np.int32)
    weight = th[np.arange(rows), topic] if rows else np.zeros(0)
    empty = s < 0.0
    topic = np.where(empty, -1, topic).astype(np.int32)
    weight = np.where(empty, 0.0, weight)
    counts = np.bincount(topic[~empty], minlength=k).astype(np.int64)
    return topic, weight, counts


def members(topic, k):
    """(indptr int64[k+1], rows int64[nonempty])"""
    keep = np.flatnonzero(topic >= 0)
    order = keep[np.argsort(topic[keep], kind="stable")]
    indptr = np.zeros(k + 1, np.int64)
    np.cumsum(np.bincount(topic[keep], minlength=k), out=indptr[1:])
    return indptr, order.astype(np.int64)


def top_topics(g, s, n_topics):
    return R.top_topics(g, n_topics)


def top_documents(g, s, max_docs):
    """(N, rows int64[k×N], weights[k×N])"""
    cand = np.flatnonzero(s >= 0.0)  # R.top_documents without its pair-by-pair gap report: both sums are sequential
    n = min(int(max_docs), cand.size)
    w = R.doc_weights(g)
    rows = np.zeros((g.shape[1], n), np.int64)
    for t in range(g.shape[1]):
        rows[t] = cand[R.ranked(w[cand, t], n)]
    return n, rows, np.stack([w[rows[t], t] for t in range(g.shape[1])])


def doc_order(idx, val, doc_terms):
    """positions of L_d inside the row"""
    val = np.asarray(val, np.float64) + 0.0  # −0 → +0
    return np.lexsort((np.asarray(idx), -val))[:int(doc_terms)]


def topic_sets(lam, topic_terms):
    """bool[k×V]: S_t"""
    V, k = lam.shape
    n = min(int(topic_terms), V)
    out = np.zeros((k, V), bool)
    for t in range(k):
        out[t, R.ranked(lam[:, t], n)] = True
    return out


def important_terms(indptr, indices, values, topic_of, sets, doc_terms, max_out):
    """(idx int32[rows×max_out] padded −1, value[rows×max_out] padded 0, n int32[rows])"""
    rows = len(indptr) - 1
    idx = np.full((rows, max_out), -1, np.int32)
    val = np.zeros((rows, max_out))
    n = np.zeros(rows, np.int32)
    for d in range(rows):
        t = int(topic_of[d])
        if t < 0:
            continue
        i = np.asarray(indices[indptr[d]:indptr[d + 1]])
        v = np.asarray(values[indptr[d]:indptr[d + 1]], np.float64) + 0.0
        o = doc_order(i, v, doc_terms)
        o = o[sets[t, i[o]]][:max_out]
        n[d] = o.size
        idx[d, :o.size] = i[o]
        val[d, :o.size] = v[o]
    return idx, val, n
