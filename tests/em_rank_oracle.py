"""NumPy restatement of the EM model's ranked queries (include/stc.h, "EM LDA, ranked queries"; csrc/rank.hip).

Order: (value descending, index ascending) — ``np.lexsort((index, -value))``.  Row sums are sequential in
ascending j (``np.cumsum(x, axis=1)[:, -1]``), the device's documented order, so the normalised weights are
expected bitwise.

Comparison rule.  In the raw modes (describe, top topics) the ranking is over stored numbers: indices must equal
the oracle's exactly.  In the row-normalised mode (top documents) a pair of ranked neighbours — the N-th and
(N+1)-th included — is *decided* if its relative gap exceeds B = (2k+2)·2^-53 (the most that two summation
orders of k positive terms plus one division can differ by), or if the two rows are bitwise equal (their weights
then are, whatever the order).  A test asserts that all its pairs are decided, then demands exact indices."""
import numpy as np


def bound(k):
    return (2 * k + 2) * 2.0 ** -53


def row_sums(m):
    m = np.asarray(m, np.float64)
    return np.cumsum(m, axis=1)[:, -1] if m.shape[0] else np.zeros(0)


def ranked(values, n):
    """the first n indices by (value descending, index ascending)"""
    values = np.asarray(values, np.float64) + 0.0  # −0 → +0
    return np.lexsort((np.arange(values.size), -values))[:n]


def describe(nwk, nk, max_terms):
    """(terms int64[k×N], weights [k×N]): ranked by the stored count, then N_wk[w][t] / N_k[t]"""
    V, k = nwk.shape
    n = min(int(max_terms), V)
    idx = np.stack([ranked(nwk[:, t], n) for t in range(k)])
    w = np.stack([nwk[idx[t], t] / nk[t] for t in range(k)])
    return idx, w


def doc_weights(ndk):
    """N_dk[d][t] / Σ_j N_dk[d][j], the count itself where the sum is 0"""
    s = row_sums(ndk)
    return np.where(s[:, None] > 0.0, ndk / np.where(s > 0.0, s, 1.0)[:, None], ndk)


def top_documents(ndk, has_vertex, max_docs):
    """(rows int64[k×N], weights [k×N], undecided pairs, smallest decided-by-gap relative gap); candidates are the
    rows with a vertex, N = min(max_docs, their number)"""
    D, k = ndk.shape
    cand = np.flatnonzero(has_vertex)
    n = min(int(max_docs), cand.size)
    w = doc_weights(ndk)
    rows = np.zeros((k, n), np.int64)
    out = np.zeros((k, n))
    undecided, min_gap = 0, np.inf
    for t in range(k):
        order = cand[ranked(w[cand, t], n + 1)]  # one more: the neighbour across the cut
        rows[t], out[t] = order[:n], w[order[:n], t]
        for a, b in zip(order[:-1], order[1:]):
            if np.array_equal(ndk[a], ndk[b]):
                continue
            gap = (w[a, t] - w[b, t]) / w[a, t] if w[a, t] > 0.0 else 0.0
            if gap > bound(k):
                min_gap = min(min_gap, gap)
            else:
                undecided += 1
    return rows, out, undecided, min_gap


def top_topics(ndk, n_topics):
    """(topics int64[D×N], weights [D×N]): ranked by the stored count, weights count / row sum (the count where the
    sum is 0)"""
    D, k = ndk.shape
    n = min(int(n_topics), k)
    w = doc_weights(ndk)
    idx = np.stack([ranked(ndk[d], n) for d in range(D)]) if D else np.zeros((0, n), np.int64)
    return idx, np.take_along_axis(w, idx, axis=1)
