"""Topic coherence restated in NumPy / SciPy from its definitions (not from the library).

A document contains term w iff its row has an entry with index w and value > 0 (zeros, negatives and NaN do not count;
an index listed twice counts once).  For term lists terms[t][i] (−1 = unused slot):
  df[t][i]      = the documents that contain slot i's term
  codf[t][i][j] = the documents that contain both slots' terms
  n_docs        = the rows of the matrix, empty ones included
UMass (Mimno et al. 2011): Σ over the pairs (m, l), 1 <= m < n, 0 <= l < m, of ln((codf[m][l] + eps) / df[l]).
NPMI: the mean over the same pairs of −1 (c = 0), 0 (c = D), else ln(c·D / (df_m·df_l)) / −ln(c / D), c = codf[m][l].
A pair with df[m] <= 0 or df[l] <= 0 is skipped.
"""
import math

import numpy as np
import scipy.sparse as sp


def contains_matrix(indptr, indices, values, num_cols):
    """boolean rows×cols: (d, w) is set iff row d has an entry of w with value > 0"""
    indptr = np.asarray(indptr, np.int64)
    indices = np.asarray(indices, np.int64)
    values = np.asarray(values)
    rows = indptr.size - 1
    row_of = np.repeat(np.arange(rows, dtype=np.int64), np.diff(indptr))
    with np.errstate(invalid="ignore"):
        keep = values > 0
    m = sp.csr_matrix((np.ones(int(keep.sum()), np.int64), (row_of[keep], indices[keep])), shape=(rows, num_cols))
    m.sum_duplicates()
    m.data[:] = 1  # an index listed twice in a row counts once
    return m


def cooccurrence(csr, terms):
    """(df int64[k, n], codf int64[k, n, n], n_docs) by boolean sub-matrix products; csr = (indptr, indices, values,
    num_cols) or an object with those attributes"""
    if not isinstance(csr, tuple):
        csr = (csr.indptr, csr.indices, csr.values, csr.num_cols)
    b = contains_matrix(*csr).tocsc()
    terms = np.asarray(terms, np.int64)
    k, n = terms.shape
    df = np.zeros((k, n), np.int64)
    codf = np.zeros((k, n, n), np.int64)
    for t in range(k):
        used = np.flatnonzero(terms[t] >= 0)
        if used.size == 0:
            continue
        s = b[:, terms[t][used]]
        g = np.asarray((s.T @ s).todense(), np.int64)
        codf[t][np.ix_(used, used)] = g
        df[t][used] = np.diag(g)
    return df, codf, b.shape[0]


def coherence(df, codf, n_docs, measure, eps=1.0):
    """(value float64[k], pairs int[k], Σ|pair value| float64[k]) as a plain loop in the defining pair order"""
    df = np.asarray(df)
    codf = np.asarray(codf)
    k, n = df.shape
    D = float(n_docs)
    out, pairs, mag = np.zeros(k), np.zeros(k, np.int64), np.zeros(k)
    for t in range(k):
        total, cnt, absum = 0.0, 0, 0.0
        for m in range(1, n):
            for l in range(m):
                dm, dl = int(df[t][m]), int(df[t][l])
                if dm <= 0 or dl <= 0:
                    continue
                c = int(codf[t][m][l])
                if measure == "umass":
                    v = math.log((float(c) + eps) / float(dl))
                elif measure == "npmi":
                    if c == 0:
                        v = -1.0
                    elif c == int(n_docs):
                        v = 0.0
                    else:
                        v = math.log((float(c) * D) / (float(dm) * float(dl))) / -math.log(float(c) / D)
                else:
                    raise ValueError(measure)
                total += v
                absum += abs(v)
                cnt += 1
        out[t] = total / cnt if (measure == "npmi" and cnt) else total
        pairs[t] = cnt
        mag[t] = absum
    return out, pairs, mag


def top_terms(nwk, n):
    """int32[k, n]: per topic the n terms with the largest weight, ties by ascending index (nwk is V×k)"""
    nwk = np.asarray(nwk)
    return np.stack([np.lexsort((np.arange(nwk.shape[0]), -nwk[:, t]))[:n] for t in range(nwk.shape[1])]).astype(np.int32)
