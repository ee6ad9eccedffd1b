"""GPU: document scores (stc_lda_score, stc_score_*, stc_lda_important_terms) against tests/score_oracle.py.

Everything is compared exactly: θ and the weights bitwise (the device forms the row sum in the oracle's sequential
order and divides once), indices and counts as integers.
"""
import ctypes as C
import os

import numpy as np
import pytest

import score_oracle as S
from helpers import GOLDEN, golden_json, golden_npz, random_corpus

pytestmark = pytest.mark.gpu

ROWS = [1, 63, 64, 65, 513, 3000]


# ---- θ bitwise against the host path ---------------------------------------------------------------------
@pytest.mark.parametrize("inject", [True, False], ids=["gamma0", "seed"])
@pytest.mark.parametrize("k", [5, 100, 130, 257])
@pytest.mark.parametrize("dtype", ["f64", "f32", "mixed"])
def test_theta_is_bitwise_the_host_path(ctx, dtype, k, inject):
    import stc

    rng = np.random.default_rng(100 + k)
    D, V = 200, 1500
    corpus = random_corpus(rng, D, V, 1, 40, empty_every=7)
    lam = rng.gamma(100.0, 0.01, size=(V, k))
    g0 = rng.gamma(100.0, 0.01, size=(D, k)) if inject else None
    model = stc.LDAModel.from_topics(lam, None, -1.0, seed=11, dtype=dtype, ctx=ctx)
    want = model.transform(corpus, g0)
    s = model.score(corpus, g0)
    got = s.topicDistribution()
    assert np.array_equal(got, want)
    empty = np.diff(corpus.indptr) == 0
    assert (s.num_rows, s.k, s.nonempty) == (D, k, int((~empty).sum()))
    assert not got[empty].any()
    # the queries agree with the oracle on what θ itself decides
    topic, weight, counts = s.mainTopics()
    assert np.array_equal(topic[empty], np.full(empty.sum(), -1)) and not weight[empty].any()
    ne = np.flatnonzero(~empty)
    assert np.array_equal(weight[ne], got[ne].max(axis=1))
    assert np.array_equal(topic[ne], k - 1 - np.argmax(got[ne][:, ::-1], axis=1))
    assert np.array_equal(counts, np.bincount(topic[ne], minlength=k))
    indptr, rows = s.members()
    o_indptr, o_rows = S.members(topic, k)
    assert np.array_equal(indptr, o_indptr) and np.array_equal(rows, o_rows)
    s.close()
    model._h.close()


# ---- planted scores ---------------------------------------------------------------------------------------
def planted_gamma(rows, k, seed):
    """rows by r mod 7: two equal maxima at topics 0 and k−1; three (0, k/2, k−1; two when k = 2); a constant row;
    an all-zero non-empty row; an empty row; small integers (many ties); distinct doubles"""
    rng = np.random.default_rng(seed)
    g = rng.random((rows, k)) + 0.5
    empty = np.zeros(rows, np.uint8)
    for r in range(rows):
        m = r % 7
        if m == 0:
            g[r, [0, k - 1]] = 7.0
        elif m == 1:
            g[r, [0, k // 2, k - 1]] = 9.0
        elif m == 2:
            g[r] = 0.25
        elif m == 3:
            g[r] = 0.0
        elif m == 4:
            empty[r] = 1
        elif m == 5:
            g[r] = rng.integers(0, 4, k)
    return g, empty


@pytest.fixture(scope="module")
def planted():
    cache = {}

    def get(rows, k):
        if (rows, k) not in cache:
            g, empty = planted_gamma(rows, k, 1000 * rows + k)
            og, osum = S.build(g, empty)
            g.setflags(write=False)
            cache[(rows, k)] = (g, empty, og, osum)
        return cache[(rows, k)]

    return get


@pytest.mark.parametrize("k", [2, 5, 64, 65, 100, 257, 1024, 1025, 4096])
@pytest.mark.parametrize("rows", ROWS)
def test_main_topics_and_members(ctx, planted, rows, k):
    import stc

    g, empty, og, osum = planted(rows, k)
    s = stc.DocumentScores.from_gamma(ctx, g, empty)
    assert np.array_equal(s.topicDistribution(), S.theta(og, osum))
    topic, weight, counts = s.mainTopics()
    o_topic, o_weight, o_counts = S.main_topics(og, osum)
    assert np.array_equal(topic, o_topic) and np.array_equal(weight, o_weight) and np.array_equal(counts, o_counts)
    assert topic[0] == k - 1  # row 0: topics 0 and k−1 tie, the largest index wins
    assert counts.sum() == s.nonempty == int((empty == 0).sum())
    indptr, members = s.members()
    o_indptr, o_members = S.members(o_topic, k)
    assert np.array_equal(indptr, o_indptr) and np.array_equal(members, o_members)
    assert indptr[0] == 0 and indptr[-1] == s.nonempty and np.array_equal(np.diff(indptr), counts)
    for t in np.flatnonzero(counts > 1)[:50]:
        assert np.all(np.diff(members[indptr[t]:indptr[t + 1]]) > 0)
    assert np.all(np.diff(indptr)[counts == 0] == 0)
    s.close()


@pytest.mark.parametrize("k", [2, 5, 64, 65, 100, 257, 1024])
@pytest.mark.parametrize("rows", ROWS)
def test_ranked_lists(ctx, planted, rows, k):
    import stc

    g, empty, og, osum = planted(rows, k)
    s = stc.DocumentScores.from_gamma(ctx, g, empty)
    for n in sorted({1, min(k, 3), k if k <= 64 else 6}):
        idx, w = s.topTopics(n)
        o_idx, o_w = S.top_topics(og, osum, n)
        assert np.array_equal(idx, o_idx) and np.array_equal(w, o_w), n
    for n in (5, rows + 10):
        d_rows, d_w = s.topDocuments(n)
        o_n, o_rows, o_w = S.top_documents(og, osum, n)
        assert d_rows.shape == (k, o_n) and np.array_equal(d_rows, o_rows) and np.array_equal(d_w, o_w), n
    s.close()


def test_top_topics_past_1024_topics_is_refused(ctx, planted):
    import stc

    g, empty, _, _ = planted(63, 1025)
    s = stc.DocumentScores.from_gamma(ctx, g, empty)
    with pytest.raises(stc.StcIllegalArgument, match="1024"):
        s.topTopics(3)
    assert s.topDocuments(4)[0].shape == (1025, 4)
    s.close()


# ---- important terms --------------------------------------------------------------------------------------
def term_rows(kind, doc_terms, V, seed, f32):
    """one row per length of the issue's list, the entries in shuffled order"""
    rng = np.random.default_rng(seed)
    lens = sorted({0, 1, max(doc_terms - 1, 0), doc_terms, doc_terms + 1, 63, 64, 65, 255, 256, 257, 1025, 5000})
    idf = np.log((V + 1.0) / (rng.integers(1, V, V) + 1.0))
    rows = []
    for n in lens:
        ids = rng.choice(V, size=n, replace=False).astype(np.int32)
        if kind == "ties":
            v = rng.integers(1, 4, n).astype(np.float64)
        elif kind == "equal":
            v = np.full(n, 2.0)
        elif kind == "distinct":
            v = rng.permutation(n) + 0.5
        else:
            v = rng.integers(1, 30, n) * idf[ids]
        if f32:
            v = v.astype(np.float32).astype(np.float64)
        rows.append((ids, v))
    return rows


@pytest.mark.parametrize("doc_terms", [1, 7, 100, 1024])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kind", ["ties", "equal", "distinct", "tfidf"])
def test_important_terms(ctx, kind, dtype, doc_terms):
    import stc

    V, k = 6000, 4
    rng = np.random.default_rng(7)
    corpus = stc.CsrMatrix.from_rows(term_rows(kind, doc_terms, V, 31 + doc_terms, dtype == "f32"), V)
    R = corpus.num_rows
    lam = rng.integers(1, 40, (V, k)).astype(np.float64)  # ties inside every topic
    h = stc.LdaHandle(ctx, k, V, dtype=dtype)
    h.set_topics(lam)
    dev = stc.DeviceCsr.upload(ctx, corpus, stc.STC_F32 if dtype == "f32" else stc.STC_F64)
    s = h.score(dev, 3)
    topic_of = (np.arange(R) % k).astype(np.int32)
    topic_of[3] = -1
    for topic_terms, n in ((300, 10), (V + 5, 10), (V, doc_terms + 3), (1, 10), (2000, 1)):
        sets = S.topic_sets(lam, topic_terms)
        idx, val, cnt = s.importantTerms(dev, doc_terms, topic_terms, n, topics=topic_of)
        o_idx, o_val, o_cnt = S.important_terms(corpus.indptr, corpus.indices, corpus.values, topic_of, sets, doc_terms, n)
        assert np.array_equal(cnt, o_cnt), (topic_terms, n, cnt, o_cnt)
        assert np.array_equal(idx, o_idx) and np.array_equal(val, o_val), (topic_terms, n)
        assert idx.shape == (R, n) and cnt[3] == 0 and cnt[0] == 0
        for d in range(R):
            assert np.all(idx[d, cnt[d]:] == -1) and not val[d, cnt[d]:].any()
        if topic_terms >= V:  # every term is in the set: the list is L_d's head
            assert np.array_equal(cnt, np.where(topic_of >= 0, np.minimum(np.minimum(np.diff(corpus.indptr), doc_terms), n), 0))
    # the main topic is the default
    topic, _, _ = s.mainTopics()
    idx, val, cnt = s.importantTerms(dev, doc_terms, 300, 10)
    o = S.important_terms(corpus.indptr, corpus.indices, corpus.values, topic, S.topic_sets(lam, 300), doc_terms, 10)
    assert np.array_equal(idx, o[0]) and np.array_equal(val, o[1]) and np.array_equal(cnt, o[2])
    s.close()
    dev.free()
    h.close()


def test_important_terms_zero_and_negative_values(ctx):
    import stc

    V, k = 64, 2
    ids = np.array([9, 2, 7, 4, 0, 5, 11, 3], np.int32)
    v = np.array([2.0, 2.0, -0.0, 3.0, -1.0, 0.0, -np.inf, 1e-300])
    corpus = stc.CsrMatrix.from_rows([(ids, v), (ids[::-1], v[::-1])], V)
    lam = np.random.default_rng(5).random((V, k)) + 0.1
    h = stc.LdaHandle(ctx, k, V, dtype="f64")
    h.set_topics(lam)
    dev = stc.DeviceCsr.upload(ctx, corpus, stc.STC_F64)
    s = stc.DocumentScores.from_gamma(ctx, np.ones((2, k)))
    s._lda = h
    topic_of = np.array([0, 1], np.int32)
    idx, val, cnt = s.importantTerms(dev, 8, V, 8, topics=topic_of)
    assert idx.tolist() == [[4, 2, 9, 3, 5, 7, 0, 11]] * 2 and cnt.tolist() == [8, 8]
    assert val[0].tolist() == [3.0, 2.0, 2.0, 1e-300, 0.0, 0.0, -1.0, -np.inf] and not np.signbit(val[0, 4:6]).any()
    o = S.important_terms(corpus.indptr, corpus.indices, corpus.values, topic_of, S.topic_sets(lam, V), 8, 8)
    assert np.array_equal(idx, o[0]) and np.array_equal(val, o[1])
    s.close()
    dev.free()
    h.close()


# ---- the reference's books --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_reference_books(ctx, dtype):
    """LDALoader's report over its 51 books from the saved model's topicsMatrix (as
    test_topic_distribution_reference_books): main topics and counts as printed, the word lists as the oracle's"""
    import stc

    rep = golden_json("en_report.json")
    meta = golden_json("en_topicdist.json")
    tf = golden_npz("en_idf.npz")
    lam = golden_npz("en_topics.npz")["nwk"]
    with open(os.path.join(GOLDEN, "en_vocab.txt"), encoding="utf-8") as f:
        vocab = f.read().split("\n")[:-1]
    V = int(tf["vocab_size"])
    corpus = stc.CsrMatrix(tf["indptr"], tf["indices"], tf["tf"].astype(np.float64), V)
    model = stc.LDAModel.from_topics(lam, meta["docConcentration"], meta["topicConcentration"],
                                     gamma_shape=meta["gammaShape"], seed=7, dtype=dtype, ctx=ctx)
    want_topic = np.array([b["main_topic"] for b in rep["books"]], np.int32)
    report = model.report(corpus, vocab)
    assert [d["mainTopic"] for d in report["documents"]] == want_topic.tolist()
    assert [t["count"] for t in report["topics"]] == rep["books_per_topic"]
    o_indptr, o_rows = S.members(want_topic, model.k)
    for t, entry in enumerate(report["topics"]):
        assert np.array_equal(entry["rows"], o_rows[o_indptr[t]:o_indptr[t + 1]])
    sets = S.topic_sets(lam, rep["topic_terms"])
    o_idx, o_val, o_cnt = S.important_terms(corpus.indptr, corpus.indices, corpus.values, want_topic, sets,
                                            rep["doc_terms"], rep["n"])
    exact = 0
    for d, doc in enumerate(report["documents"]):
        assert doc["importantTerms"] == [vocab[i] for i in o_idx[d, :o_cnt[d]]], d
        assert np.array_equal(doc["importantTermValues"], o_val[d, :o_cnt[d]])
        assert doc["mainTopicWeight"] == doc["topicDistribution"][doc["mainTopic"]]
        exact += doc["importantTerms"] == rep["books"][d]["words"]
    assert exact == 40  # the recorded lists, term for term (tests/test_score_oracle.py has the tie allowance)
    s = model.score(corpus)
    idx, val, cnt = s.importantTerms(corpus, rep["doc_terms"], rep["topic_terms"], rep["n"])
    assert np.array_equal(idx, o_idx) and np.array_equal(val, o_val) and np.array_equal(cnt, o_cnt)
    s.close()
    model._h.close()


# ---- errors -----------------------------------------------------------------------------------------------
def test_errors(ctx):
    import stc

    rng = np.random.default_rng(3)
    V, k = 200, 3
    corpus = random_corpus(rng, 12, V, 1, 20)
    dev = stc.DeviceCsr.upload(ctx, corpus, stc.STC_F64)
    h = stc.LdaHandle(ctx, k, V, dtype="f64")
    with pytest.raises(stc.StcError) as e:  # no topics yet
        h.score(dev)
    assert e.value.code == stc.STC_ERR_STATE
    ready = stc.LdaHandle(ctx, k, V, dtype="f64")
    ready.set_topics(rng.random((V, k)) + 0.1)
    s = ready.score(dev, 1)
    s_blank = stc.DocumentScores(ctx, s.handle, h)  # the same score asked of the handle without topics
    with pytest.raises(stc.StcError) as e:
        s_blank.importantTerms(dev)
    assert e.value.code == stc.STC_ERR_STATE
    s_blank.handle = None
    for bad in (dict(docTerms=0), dict(topicTerms=0), dict(n=0), dict(docTerms=-3), dict(docTerms=1025)):
        with pytest.raises(stc.StcIllegalArgument):
            s.importantTerms(dev, **bad)
    with pytest.raises(stc.StcIllegalArgument):
        s.importantTerms(dev, topics=np.full(12, k, np.int32))
    other = stc.DeviceCsr.upload(ctx, random_corpus(rng, 11, V, 1, 20), stc.STC_F64)
    with pytest.raises(stc.StcIllegalArgument, match="row count"):
        s.importantTerms(other)
    with pytest.raises(stc.StcIllegalArgument):
        s.topTopics(0)
    with pytest.raises(stc.StcIllegalArgument):
        s.topDocuments(0)
    for g in ([[1.0, -1.0]], [[1.0, np.nan]], [[np.inf, 1.0]]):
        with pytest.raises(stc.StcIllegalArgument):
            stc.DocumentScores.from_gamma(ctx, np.array(g))
    # a score of another context
    ctx2 = stc.Context(0)
    s2 = stc.DocumentScores.from_gamma(ctx2, np.ones((12, k)))
    lib = ctx.lib
    out = np.zeros((12, k))
    assert lib.stc_score_topic_distribution(ctx.handle, s2.handle, out.ctypes.data_as(C.POINTER(C.c_double))) == \
        stc.STC_ERR_INVALID_ARG
    assert lib.stc_score_main_topics(ctx.handle, s2.handle, None, None, None) == stc.STC_ERR_INVALID_ARG
    assert lib.stc_score_members(ctx.handle, s2.handle, None, None) == stc.STC_ERR_INVALID_ARG
    assert lib.stc_score_top_topics(ctx.handle, s2.handle, 1, None, None) == stc.STC_ERR_INVALID_ARG
    assert lib.stc_score_top_documents(ctx.handle, s2.handle, 1, None, None, None) == stc.STC_ERR_INVALID_ARG
    assert lib.stc_lda_important_terms(ready.handle, dev.handle, s2.handle, None, 100, 300, 10, None, None, None) == \
        stc.STC_ERR_INVALID_ARG
    assert s2.mainTopics()[0].tolist() == [k - 1] * 12  # its own context serves it
    ctx2.close()
    s2.close()  # valid after its context is gone
    # every output is optional
    assert lib.stc_score_main_topics(ctx.handle, s.handle, None, None, None) == 0
    assert lib.stc_lda_important_terms(ready.handle, dev.handle, s.handle, None, 100, 300, 10, None, None, None) == 0
    s.close()
    other.free()
    dev.free()
    h.close()
    ready.close()
