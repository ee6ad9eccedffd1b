"""NumPy restatement of the stc_em_group decomposition (csrc/em_group.hip), built on tests/em_oracle.py.

Documents are sharded by contiguous row ranges balanced by entries (the rule of stc_group_set_corpus); a member
sums the messages of its own edges — N_dk rows of its documents, and a V×k partial of N_wk in which a term
without a local edge is a 0 row —, the partials are added in member order, N_k follows from the sum.  The RNG
keys of the initial state are edge positions in the whole corpus's CSR order: a member's first key is the count
of non-zero entries before its shard (explicit zeros are entries, not edges).
"""
import numpy as np

import em_oracle as E


def shard_rows(indptr, n):
    """r0[0..n]: member q owns rows [r0[q], r0[q+1]); boundary q is the first row whose start reaches
    ceil(nnz·q / n) entries"""
    rows = len(indptr) - 1
    nnz = int(indptr[rows])
    r0 = [0] + [rows] * n
    r = 0
    for q in range(1, n):
        target = (nnz * q + n - 1) // n
        while r < rows and indptr[r] < target:
            r += 1
        r0[q] = max(r, r0[q - 1])
    return r0


def shards(m, n):
    """per member: (row0, row1, pos_base, src (global rows), term, cnt) of its edges"""
    r0 = shard_rows(m.indptr, n)
    src, term, cnt = E.edges_of(m)
    out, base = [], 0
    for q in range(n):
        lo, hi = r0[q], r0[q + 1]
        sel = (src >= lo) & (src < hi)
        nz = int(np.count_nonzero(m.values[m.indptr[lo]:m.indptr[hi]]))
        assert nz == int(sel.sum())
        out.append((lo, hi, base, src[sel], term[sel], cnt[sel]))
        base += nz
    return out


def step(m, n, ndk, nwk, nk, alpha, eta):
    """one iteration the way n members run it → (N_dk', N_wk', N_k')"""
    D, V = ndk.shape[0], nwk.shape[0]
    ndk2 = np.zeros_like(ndk)
    parts = []
    for lo, hi, _, src, term, cnt in shards(m, n):
        msg = E.edge_factors(ndk, nwk, nk, src, term, alpha, eta)
        msg *= (cnt / msg.sum(axis=1))[:, None]
        ndk2[lo:hi] = E._scatter(src - lo, msg, hi - lo) if src.size else 0.0
        parts.append(E._scatter(term, msg, V) if src.size else np.zeros((V, nwk.shape[1])))
    nwk2 = parts[0].copy()
    for p in parts[1:]:  # member order
        nwk2 += p
    return ndk2, nwk2, nwk2.sum(axis=0)


def init_state(seed, m, n, k):
    """the initial state the way n members draw it: member q's edge e has the key pos_base_q + e"""
    from oracle import oracle as O

    D, V = m.shape
    ndk = np.zeros((D, k))
    parts = []
    for lo, hi, base, src, term, cnt in shards(m, n):
        u = np.empty((src.size, k))
        for e in range(src.size):
            st = O.doc_stream(seed, base + e)
            for j in range(k):
                u[e, j] = O._uniform(st, j)
        msg = cnt[:, None] * (u / u.sum(axis=1, keepdims=True))
        ndk[lo:hi] = E._scatter(src - lo, msg, hi - lo) if src.size else 0.0
        parts.append(E._scatter(term, msg, V) if src.size else np.zeros((V, k)))
    nwk = parts[0].copy()
    for p in parts[1:]:
        nwk += p
    return ndk, nwk, nwk.sum(axis=0)
