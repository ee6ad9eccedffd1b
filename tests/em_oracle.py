"""NumPy restatement of [U] EMLDAOptimizer / DistributedLDAModel (spark-mllib 2.4.3), the checker of stc_em_*.

The corpus is a bipartite graph: every CSR entry (document d, term w, value c != 0) is an edge.  State:
N_dk (D×k), N_wk (V×k), N_k = Σ_w N_wk.  Plain fp64 NumPy; every per-vertex sum is one ``np.bincount``
per topic (edges in CSR order).
"""
import numpy as np


def resolve(k, doc_concentration=-1.0, topic_concentration=-1.0):
    """(α, η): −1 ⇒ 50/k + 1 and 1.1; anything else must be > 1"""
    alpha = 50.0 / k + 1.0 if doc_concentration == -1.0 else float(doc_concentration)
    eta = 1.1 if topic_concentration == -1.0 else float(topic_concentration)
    assert alpha > 1.0 and eta > 1.0
    return alpha, eta


def edges_of(m):
    """(src, term, count) of a CsrMatrix: the entries whose value is not exactly 0, in CSR order"""
    keep = m.values != 0.0
    src = np.repeat(np.arange(m.num_rows, dtype=np.int64), np.diff(m.indptr))[keep]
    return src, m.indices[keep].astype(np.int64), m.values[keep].astype(np.float64)


def edges_of_model(m):
    """(row, term, count) of a loaded DistributedLDAModel dict (stc.io.load_distributed): document vertex
    ids mapped to their rank among m["doc_ids"] (the row of m["doc_topics"]), edges ordered by row (stable)"""
    src, term, cnt = m["edges"]
    row = np.searchsorted(m["doc_ids"], src)
    assert np.array_equal(m["doc_ids"][row], src)
    order = np.argsort(row, kind="stable")
    return row[order].astype(np.int64), term[order].astype(np.int64), cnt[order].astype(np.float64)


def mask_state(ndk, nwk, src, term):
    """an injected state keeps to the graph's vertices: rows of documents / terms without an edge are 0"""
    ndk, nwk = np.array(ndk, np.float64), np.array(nwk, np.float64)
    has_d = np.zeros(ndk.shape[0], bool)
    has_w = np.zeros(nwk.shape[0], bool)
    has_d[src] = True
    has_w[term] = True
    ndk[~has_d] = 0.0
    nwk[~has_w] = 0.0
    return ndk, nwk


def _scatter(idx, msg, n):
    return np.stack([np.bincount(idx, weights=msg[:, j], minlength=n) for j in range(msg.shape[1])], axis=1)


def edge_factors(ndk, nwk, nk, src, term, alpha, eta):
    """per edge and topic: (N_wk[w][j] + η−1)(N_dk[d][j] + α−1) / (N_k[j] + V(η−1)), unnormalised"""
    V = nwk.shape[0]
    return (nwk[term] + (eta - 1.0)) * (ndk[src] + (alpha - 1.0)) / (nk + V * (eta - 1.0))


def step(ndk, nwk, nk, src, term, cnt, alpha, eta):
    """one EM iteration, all reads from the old state → (N_dk', N_wk', N_k')"""
    msg = edge_factors(ndk, nwk, nk, src, term, alpha, eta)
    msg *= (cnt / msg.sum(axis=1))[:, None]  # c · γ / Σ_j γ_j
    ndk2 = _scatter(src, msg, ndk.shape[0])
    nwk2 = _scatter(term, msg, nwk.shape[0])
    return ndk2, nwk2, nwk2.sum(axis=0)


def iterate(ndk, nwk, src, term, cnt, alpha, eta, n):
    nk = nwk.sum(axis=0)
    for _ in range(n):
        ndk, nwk, nk = step(ndk, nwk, nk, src, term, cnt, alpha, eta)
    return ndk, nwk, nk


def log_likelihood(ndk, nwk, nk, src, term, cnt, alpha, eta):
    """Σ_edges c · ln(φ_w · θ_d)"""
    V = nwk.shape[0]
    phi = (nwk + (eta - 1.0)) / (nk + V * (eta - 1.0))
    theta = ndk + (alpha - 1.0)
    theta = theta / theta.sum(axis=1, keepdims=True)
    return float(np.sum(cnt * np.log(np.sum(phi[term] * theta[src], axis=1))))


def log_prior(ndk, nwk, nk, src, term, alpha, eta):
    """(η−1) Σ_{term vertices} Σ_j ln φ_w[j] + (α−1) Σ_{doc vertices} Σ_j ln θ_d[j]"""
    V = nwk.shape[0]
    ws, ds = np.unique(term), np.unique(src)
    phi = (nwk[ws] + (eta - 1.0)) / (nk + V * (eta - 1.0))
    theta = ndk[ds] + (alpha - 1.0)
    theta = theta / theta.sum(axis=1, keepdims=True)
    return float((eta - 1.0) * np.sum(np.log(phi)) + (alpha - 1.0) * np.sum(np.log(theta)))


def topic_distributions(ndk, src):
    """(doc vertex ids, their N_dk rows normalised to sum 1)"""
    ds = np.unique(src)
    return ds, ndk[ds] / ndk[ds].sum(axis=1, keepdims=True)


def init_gamma(seed, n_edges, k):
    """the library's initial γ_e: k uniforms in (0,1) from the counter RNG keyed (seed, edge position among
    the edges in CSR order, topic), normalised to sum 1"""
    from oracle import oracle as O

    u = np.empty((n_edges, k), np.float64)
    for e in range(n_edges):
        st = O.doc_stream(seed, e)
        for j in range(k):
            u[e, j] = O._uniform(st, j)
    return u / u.sum(axis=1, keepdims=True), u


def init_state(seed, src, term, cnt, D, V, k):
    g, _ = init_gamma(seed, src.size, k)
    msg = cnt[:, None] * g
    nwk = _scatter(term, msg, V)
    return _scatter(src, msg, D), nwk, nwk.sum(axis=0)


def mass_identities(ndk, nwk, nk, src, term, cnt):
    """max relative error of: Σ_j N_dk[d] = the document's edge weights, Σ_j N_wk[w] = the term's edge
    weights, N_k = Σ_w N_wk"""
    dw = np.bincount(src, weights=cnt, minlength=ndk.shape[0])
    tw = np.bincount(term, weights=cnt, minlength=nwk.shape[0])
    ed = np.max(np.abs(ndk.sum(axis=1) - dw) / np.maximum(dw, 1e-300)) if src.size else 0.0
    et = np.max(np.abs(nwk.sum(axis=1) - tw) / np.maximum(tw, 1e-300)) if src.size else 0.0
    col = nwk.sum(axis=0)
    ek = np.max(np.abs(nk - col) / col)
    return float(ed), float(et), float(ek)
