"""GPU: stc_term_cooccurrence (document co-occurrence counts of the topics' top terms, csrc/coherence.hip) against
tests/coherence_oracle.py, and the models' topicCoherence on the reference's saved EN model.

Counts are integers and are compared with ==.  Coherence values: |got − oracle| <= 1e-12 · max(1, Σ|pair value|)
(both sides add the same pair values in the same order; a log may differ by a few ulp, the sum's own rounding is at
most 2016 · 2^-53 of Σ|pair value|).
"""
import ctypes as C
import os

import numpy as np
import pytest

import coherence_oracle as CO
from helpers import GOLDEN, golden_npz, random_corpus

pytestmark = pytest.mark.gpu

REF_MODEL = os.path.join(GOLDEN, "LdaModel_EN_1591049082850")


def _check(ctx, corpus, terms, dtype=None, dev=None):
    """the device's counts == the oracle's; returns them"""
    import stc

    own = dev is None
    if own:
        dev = stc.DeviceCsr.upload(ctx, corpus, stc.STC_F64 if dtype is None else dtype)
    try:
        df, codf, D = stc.term_cooccurrence(dev, terms)
    finally:
        if own:
            dev.free()
    terms = np.asarray(terms)
    k, n = terms.shape
    assert df.dtype == np.int64 and codf.dtype == np.int64 and df.shape == (k, n) and codf.shape == (k, n, n)
    odf, ocodf, oD = CO.cooccurrence(corpus, terms)
    assert D == oD == corpus.num_rows
    assert np.array_equal(df, odf), np.argwhere(df != odf)[:5]
    assert np.array_equal(codf, ocodf), np.argwhere(codf != ocodf)[:5]
    return df, codf, D


def _idf_df(ctx, dev):
    """the document frequencies the IDF fit counts on the same device matrix"""
    idf = np.zeros(dev.num_cols)
    df = np.zeros(dev.num_cols, np.int64)
    m = C.c_int64()
    rc = ctx.lib.stc_idf_fit(ctx.handle, dev.handle, 0, idf.ctypes.data_as(C.POINTER(C.c_double)),
                             df.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(m))
    assert rc == 0
    return df, m.value


@pytest.fixture(scope="module")
def en():
    import stc

    tf = golden_npz("en_idf.npz")
    nwk = golden_npz("en_topics.npz")["nwk"]
    return stc.CsrMatrix(tf["indptr"], tf["indices"], tf["tfidf"], int(tf["vocab_size"])), nwk


@pytest.fixture(scope="module")
def small():
    """D = 300, V = 97, 0-3 entries per row, every seventh row empty: many documents per ticket"""
    return random_corpus(np.random.default_rng(41), 300, 97, 0, 3, empty_every=7)


def _zipf_flat(rng, D=70001, V=501, s=1.3, max_len=11):
    """(row_of, term) of rows of 0 … max_len Zipf draws over the terms 0 … V−2 (term V−1 is never drawn)"""
    p = 1.0 / np.arange(1, V) ** s
    p /= p.sum()
    lens = rng.integers(0, max_len + 1, D)
    row_of = np.repeat(np.arange(D, dtype=np.int64), lens)
    return row_of, rng.choice(V - 1, size=row_of.size, p=p).astype(np.int32), V


def _csr(row_of, term, val, D, V):
    import stc

    indptr = np.zeros(D + 1, np.int64)
    np.cumsum(np.bincount(row_of, minlength=D), out=indptr[1:])
    return stc.CsrMatrix(indptr, term, val, V)


@pytest.fixture(scope="module")
def zipf():
    """70,001 rows with sorted distinct indices and counts"""
    row_of, term, V = _zipf_flat(np.random.default_rng(42))
    D = 70001
    key, cnt = np.unique(row_of * V + term, return_counts=True)
    return _csr(key // V, (key % V).astype(np.int32), cnt.astype(np.float64), D, V)


ZIPF_TERMS = np.stack([np.arange(33), np.concatenate([np.arange(468, 500), [500]])]).astype(np.int32)


@pytest.mark.parametrize("n", [10, 64])
def test_en_books(ctx, en, n):
    """51 rows of 1,039-12,670 entries (far more than a wave's 64 lanes per step), STC_F64 TF·IDF; n = 64 sets bit 63"""
    import stc

    corpus, nwk = en
    assert np.diff(corpus.indptr).min() >= 1039 and np.diff(corpus.indptr).max() == 12670
    terms = CO.top_terms(nwk, n)
    dev = stc.DeviceCsr.upload(ctx, corpus, stc.STC_F64)
    try:
        df, codf, D = _check(ctx, corpus, terms, dev=dev)
        idf_df, m = _idf_df(ctx, dev)
        assert m == D == 51 and np.array_equal(df, idf_df[terms])
        again = stc.term_cooccurrence(dev, terms)
        assert again[0].tobytes() == df.tobytes() and again[1].tobytes() == codf.tobytes()
    finally:
        dev.free()
    assert codf[:, np.arange(n), np.arange(n)].tolist() == df.tolist()


def test_small_rows_n33(ctx, small):
    """k = 3, n = 33 crosses the mask's 32-bit half; empty rows count in n_docs"""
    import stc

    rng = np.random.default_rng(43)
    terms = np.stack([rng.choice(97, 33, replace=False) for _ in range(3)]).astype(np.int32)
    dev = stc.DeviceCsr.upload(ctx, small, stc.STC_F64)
    try:
        df, _, D = _check(ctx, small, terms, dev=dev)
        idf_df, m = _idf_df(ctx, dev)
    finally:
        dev.free()
    assert D == m == 300 and np.array_equal(df, idf_df[terms]) and df.max() > 0


def test_zipf_counts_past_16_bits(ctx, zipf):
    """70,001 > 65,535 documents and a hottest term in more than 65,535 / 2 of them: 16-bit or per-tile counters
    would overflow; term 500 is in no document (df 0: a skipped slot); then the same with −1 in that slot"""
    import stc

    dev = stc.DeviceCsr.upload(ctx, zipf, stc.STC_F64)
    try:
        df, codf, D = _check(ctx, zipf, ZIPF_TERMS, dev=dev)
        idf_df, _ = _idf_df(ctx, dev)
        assert np.array_equal(df, idf_df[ZIPF_TERMS])
        assert D == 70001 and df[0, 0] > 65535 // 2 and df[1, 32] == 0 and not codf[1, 32].any()
        for name in ("umass", "npmi"):
            got, pairs = stc.coherence(df, codf, D, measure=name)
            exp, opairs, mag = CO.coherence(df, codf, D, name)
            assert pairs.tolist() == opairs.tolist() == [33 * 32 // 2, 32 * 31 // 2]
            assert np.all(np.abs(got - exp) <= 1e-12 * np.maximum(1.0, mag))
        unused = ZIPF_TERMS.copy()
        unused[1, 32] = -1
        df2, codf2, _ = _check(ctx, zipf, unused, dev=dev)
        assert np.array_equal(df2, df) and np.array_equal(codf2, codf)
        again = stc.term_cooccurrence(dev, unused)
        assert again[0].tobytes() == df2.tobytes() and again[1].tobytes() == codf2.tobytes()
    finally:
        dev.free()


def test_value_rule_f32_dirty_rows(ctx):
    """STC_F32 with explicit zeros (10 %), negatives (5 %), a few NaN, indices listed twice and unsorted rows: a
    document contains a term iff one of its entries of it has a value > 0, once"""
    import stc

    rng = np.random.default_rng(44)
    row_of, term, V = _zipf_flat(rng)  # draws with replacement, in draw order: duplicates, unsorted
    val = rng.integers(1, 5, term.size).astype(np.float64)
    u = rng.random(term.size)
    val[u < 0.10] = 0.0
    val[(u >= 0.10) & (u < 0.15)] = -val[(u >= 0.10) & (u < 0.15)]
    val[rng.choice(term.size, 40, replace=False)] = np.nan
    corpus = _csr(row_of, term, val, 70001, V)
    pairs = row_of * V + term
    assert np.unique(pairs).size < pairs.size  # some rows list an index twice
    dev = stc.DeviceCsr.upload(ctx, corpus, stc.STC_F32)
    try:
        df, _, _ = _check(ctx, corpus, ZIPF_TERMS, dev=dev)
    finally:
        dev.free()
    clean = CO.cooccurrence((corpus.indptr, corpus.indices, np.ones(term.size), V), ZIPF_TERMS)[0]
    assert np.all(df <= clean) and np.any(df < clean)  # the values mattered
    _check(ctx, corpus, ZIPF_TERMS, dtype=stc.STC_F64)


@pytest.mark.parametrize("k,n", [(64, 64), (4096, 3)])
def test_counters_past_lds(ctx, small, k, n):
    """the counters in global memory: k = 64, n = 64 needs 520 KB of them, past a CU's 160 KB of LDS; k = 4096, n = 3
    needs 96 KB beside 48 KB of masks and touched list per wave, which leaves room for fewer than four waves"""
    rng = np.random.default_rng(45 + k)
    terms = np.stack([rng.choice(97, n, replace=False) for _ in range(k)]).astype(np.int32)
    lds, counters, per_wave = 160 * 1024, 4 * k * n * (n + 1) // 2, 12 * k + 4
    assert counters + 4 * per_wave > lds
    df, _, _ = _check(ctx, small, terms)
    assert df.max() > 0


def test_slots_are_independent(ctx):
    """one term in all five lists, a list that repeats a term (codf[i][j] = df for its two slots), unsorted rows"""
    import stc

    rng = np.random.default_rng(46)
    rows = []
    for _ in range(500):
        ids = rng.choice(40, size=int(rng.integers(0, 9)), replace=False).astype(np.int32)  # unsorted
        rows.append((ids, np.ones(ids.size)))
    corpus = stc.CsrMatrix.from_rows(rows, 40)
    terms = np.array([[7, 1, 2, 3], [4, 7, 5, 6], [8, 9, 7, 10], [11, 12, 13, 7], [7, 20, 7, 21]], np.int32)
    df, codf, _ = _check(ctx, corpus, terms)
    assert len({int(df[t][list(terms[t]).index(7)]) for t in range(5)}) == 1 and df[0, 0] > 0
    assert codf[4, 0, 2] == codf[4, 2, 0] == df[4, 0] == df[4, 2]
    assert np.array_equal(codf[4, 0], codf[4, 2])


def test_edges(ctx):
    """n = 1, k = 1; a matrix without rows; a matrix without entries"""
    import stc

    one = stc.CsrMatrix.from_rows([([3], [2.0]), ([], []), ([3, 1], [1.0, 1.0])], 5)
    df, codf, D = _check(ctx, one, np.array([[3]], np.int32))
    assert df.tolist() == [[2]] and codf.tolist() == [[[2]]] and D == 3
    terms = np.array([[0, 1, 4], [2, -1, 3]], np.int32)
    for corpus in (stc.CsrMatrix([0], [], [], 5), stc.CsrMatrix([0, 0, 0, 0], [], [], 5)):
        df, codf, D = _check(ctx, corpus, terms)
        assert D == corpus.num_rows and not df.any() and not codf.any()
    df, codf, _ = _check(ctx, one, np.full((2, 3), -1, np.int32))  # nothing but unused slots
    assert not df.any() and not codf.any()


def test_null_outputs(ctx, small):
    import stc

    terms = np.arange(6, dtype=np.int32).reshape(2, 3)
    dev = stc.DeviceCsr.upload(ctx, small, stc.STC_F64)
    try:
        df, codf, D = stc.term_cooccurrence(dev, terms)
        p = terms.ctypes.data_as(C.POINTER(C.c_int32))
        only = np.zeros((2, 3), np.int64)
        assert ctx.lib.stc_term_cooccurrence(ctx.handle, dev.handle, p, 2, 3, only.ctypes.data_as(C.POINTER(C.c_int64)),
                                             None, None) == 0
        assert np.array_equal(only, df)
        m = C.c_int64()
        assert ctx.lib.stc_term_cooccurrence(ctx.handle, dev.handle, p, 2, 3, None, None, C.byref(m)) == 0
        assert m.value == D == 300
    finally:
        dev.free()


def test_error_returns(ctx, small):
    import stc

    lib, inv = ctx.lib, stc.STC_ERR_INVALID_ARG
    dev = stc.DeviceCsr.upload(ctx, small, stc.STC_F64)
    try:
        def call(terms, k, n, c=ctx, d=dev):
            t = np.ascontiguousarray(terms, np.int32)
            df = np.zeros(max(k * n, 1), np.int64)
            codf = np.zeros(max(k * n * n, 1), np.int64)
            return lib.stc_term_cooccurrence(c.handle, d.handle, t.ctypes.data_as(C.POINTER(C.c_int32)), k, n,
                                             df.ctypes.data_as(C.POINTER(C.c_int64)),
                                             codf.ctypes.data_as(C.POINTER(C.c_int64)), None)

        assert call([[0, 1, 2]], 1, 3) == 0
        assert call([[0, 97, 2]], 1, 3) == inv  # a term index >= n_cols
        assert b"97" in lib.stc_last_error()
        assert call([[0, -2, 2]], 1, 3) == inv
        assert call(np.zeros((1, 65)), 1, 65) == inv
        assert call(np.zeros((4097, 1)), 4097, 1) == inv
        assert call([[0]], 1, 0) == inv and call([[0]], 0, 1) == inv
        ctx2 = stc.Context(0)
        try:
            assert call([[0, 1, 2]], 1, 3, c=ctx2) == inv  # a matrix of another context
        finally:
            ctx2.close()
        with pytest.raises(stc.StcIllegalArgument):
            stc.term_cooccurrence(dev, [[0, 1, 200]])
        with pytest.raises(ValueError):
            stc.term_cooccurrence(dev, [0, 1, 2])
    finally:
        dev.free()


def test_model_topic_coherence(ctx, en):
    """LDAModel.topicCoherence over the books and DistributedLDAModel.topicCoherence() over its own stored edges, on
    the reference's saved EN model: the same terms and the same corpus by two routes, both the oracle's values"""
    import stc

    corpus, nwk = en
    model = stc.DistributedLDAModel.load(REF_MODEL)
    local = model.toLocal(ctx=ctx)
    df, codf, D = CO.cooccurrence(corpus, CO.top_terms(nwk, 10))
    for name in ("umass", "npmi"):
        exp, pairs, mag = CO.coherence(df, codf, D, name, 1.0)
        assert pairs.tolist() == [45] * 5
        tol = 1e-12 * np.maximum(1.0, mag)
        a = local.topicCoherence(corpus, topN=10, measure=name)
        b = model.topicCoherence(topN=10, measure=name, ctx=ctx)
        assert a.dtype == np.float64 and a.shape == (5,) and b.shape == (5,)
        print(name, "local − oracle", a - exp, "distributed − oracle", b - exp, "Σ|pair|", mag)
        assert np.all(np.abs(a - exp) <= tol), (name, a - exp)
        assert np.all(np.abs(b - exp) <= tol), (name, b - exp)
        assert np.all(np.abs(a - b) <= tol), (name, a - b)
    assert np.array_equal(local.topicCoherence(corpus), local.topicCoherence(corpus, 10, "umass", 1.0))
    assert np.array_equal(model.topicCoherence(corpus, ctx=ctx), model.topicCoherence(ctx=ctx))  # the books are its edges
    with pytest.raises(ValueError):
        local.topicCoherence(corpus, topN=65)
    with pytest.raises(ValueError):
        local.topicCoherence(corpus, topN=1)
    with pytest.raises(ValueError):
        local.topicCoherence(corpus, measure="c_v")
