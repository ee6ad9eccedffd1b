"""GPU: the EM optimizer (stc_em_*, csrc/lda_em.hip) against its NumPy restatement (tests/em_oracle.py).

Bounds: one step ≤ 1e-12 elementwise relative (two NumPy summation orders differ by 1.5e-14 on the golden
graph at k = 5 and k = 100; every term is positive, so no cancellation), ten steps ≤ 1e-9 (the project's bar
for λ after ten steps; two CPU orders drift 3.8e-12 there)."""
import os

import numpy as np
import pytest

import em_oracle as E
from helpers import GOLDEN, planted_corpus, random_corpus

pytestmark = pytest.mark.gpu

REF_MODEL = os.path.join(GOLDEN, "LdaModel_EN_1591049082850")


def rel_err(got, ref):
    """max elementwise relative error; where the reference is exactly 0 the result must be too"""
    got, ref = np.asarray(got), np.asarray(ref)
    zero = ref == 0.0
    assert np.all(got[zero] == 0.0)
    if zero.all():
        return 0.0
    return float(np.max(np.abs(got[~zero] - ref[~zero]) / np.abs(ref[~zero])))


def make_handle(ctx, corpus, k, alpha=-1.0, eta=-1.0):
    import stc

    dev = stc.DeviceCsr.upload(ctx, corpus, stc.STC_F64)
    try:
        return stc.EmHandle(ctx, dev, k, alpha, eta)  # the handle keeps no reference to the corpus
    finally:
        dev.free()


def random_state(rng, D, V, k):
    return rng.uniform(0.5, 5.0, size=(D, k)), rng.uniform(0.5, 5.0, size=(V, k))


def check_step(ctx, corpus, k, rng, bound=1e-12):
    D, V = corpus.shape
    src, term, cnt = E.edges_of(corpus)
    alpha, eta = E.resolve(k)
    ndk0, nwk0 = random_state(rng, D, V, k)
    h = make_handle(ctx, corpus, k)
    assert (h.k, h.num_docs, h.vocab_size, h.num_edges) == (k, D, V, src.size)
    h.set_state(ndk0, nwk0)
    rd, rw = E.mask_state(ndk0, nwk0, src, term)
    got = h.state()
    assert np.array_equal(got[0], rd) and np.array_equal(got[1], rw)
    assert rel_err(got[2], rw.sum(axis=0)) <= bound
    ref = E.step(rd, rw, rw.sum(axis=0), src, term, cnt, alpha, eta)
    h.next(1)
    got = h.state()
    errs = [rel_err(g, r) for g, r in zip(got, ref)]
    print(f"k={k} D={D} V={V} E={src.size}: rel err N_dk {errs[0]:.2e} N_wk {errs[1]:.2e} N_k {errs[2]:.2e}")
    assert max(errs) <= bound, errs
    h.close()


@pytest.mark.parametrize("k", [2, 5, 64, 65, 100, 257])
def test_one_step_matches_the_restatement(ctx, k):
    rng = np.random.default_rng(100 + k)
    check_step(ctx, random_corpus(rng, 40, 300), k, rng)


def long_vertex_corpus(rng, D=700, V=4000, long_doc=3000, hot=7):
    """document 0 holds 3,000 entries and term `hot` occurs in all 700 documents: with 256-edge chunks the
    document's list is cut into 12 chunks (11 boundaries) and the term's into 3 (2 boundaries), the last
    chunk of each partly filled"""
    import stc

    rows = []
    cold = np.setdiff1d(np.arange(V), [hot])
    for d in range(D):
        n = long_doc - 1 if d == 0 else int(rng.integers(3, 11))
        ids = np.union1d(rng.choice(cold, size=n, replace=False), [hot]).astype(np.int32)
        rows.append((ids, rng.integers(1, 6, ids.size).astype(np.float64)))
    assert rows[0][0].size == long_doc and all(hot in r[0] for r in rows)
    return stc.CsrMatrix.from_rows(rows, V)


@pytest.mark.parametrize("k", [5, 100])
def test_chunk_boundaries(ctx, k):
    rng = np.random.default_rng(200 + k)
    check_step(ctx, long_vertex_corpus(rng), k, rng)


def filtered_corpus():
    """rows 1 and 4 empty, rows 2 and 6 only explicit zeros, zeros inside rows 0 and 5; terms 3, 8 and 10–15
    in no edge (3 and 8 only under explicit zeros)"""
    import stc

    rows = [([0, 1, 3, 5], [2.0, 0.0, 0.0, 1.0]), ([], []), ([3, 8], [0.0, 0.0]), ([1, 2, 9], [1.0, 3.0, 2.0]),
            ([], []), ([0, 4, 8], [1.0, 2.0, 0.0]), ([0], [0.0]), ([6, 7, 9], [4.0, 1.0, 1.0])]
    return stc.CsrMatrix.from_rows(rows, 16)


def test_edge_filtering(ctx):
    import stc

    corpus, k = filtered_corpus(), 5
    D, V = corpus.shape
    src, term, cnt = E.edges_of(corpus)
    no_doc, no_term = [1, 2, 4, 6], [3, 8, 10, 11, 12, 13, 14, 15]
    assert src.size == 10 and sorted(set(range(D)) - set(src)) == no_doc and sorted(set(range(V)) - set(term)) == no_term
    alpha, eta = E.resolve(k)
    rng = np.random.default_rng(3)
    ndk0, nwk0 = random_state(rng, D, V, k)
    h = make_handle(ctx, corpus, k)
    assert h.num_edges == 10
    h.set_state(ndk0, nwk0)
    rd, rw = E.mask_state(ndk0, nwk0, src, term)
    for it in range(2):
        got = h.state()
        assert np.all(got[0][no_doc] == 0.0) and np.all(got[1][no_term] == 0.0)
        ll, lp = h.log_likelihood()
        rk = rw.sum(axis=0)
        assert abs(ll - E.log_likelihood(rd, rw, rk, src, term, cnt, alpha, eta)) <= 1e-12 * abs(ll)
        ref_lp = E.log_prior(rd, rw, rk, src, term, alpha, eta)  # present vertices only
        assert abs(lp - ref_lp) <= 1e-12 * abs(ref_lp), (lp, ref_lp)
        rd, rw, rk = E.step(rd, rw, rk, src, term, cnt, alpha, eta)
        h.next(1)
        got = h.state()
        assert max(rel_err(g, r) for g, r in zip(got, (rd, rw, rk))) <= 1e-12
    h.init_random(9)
    got = h.state()
    assert np.all(got[0][no_doc] == 0.0) and np.all(got[1][no_term] == 0.0)
    assert np.all(got[0][np.unique(src)] > 0.0) and np.all(got[1][np.unique(term)] > 0.0)
    h.close()
    model = stc.MllibLDA(ctx).setOptimizer("em").setK(k).setMaxIterations(2).run(corpus)
    ids, td = model.topicDistributions()
    assert ids.tolist() == [0, 3, 5, 7] and td.shape == (4, k) and np.allclose(td.sum(axis=1), 1.0, atol=1e-14)


@pytest.fixture(scope="module")
def golden():
    import stc

    m = stc.io.load_distributed(REF_MODEL)
    src, term, cnt = E.edges_of_model(m)
    indptr = np.zeros(m["doc_ids"].size + 1, np.int64)
    np.cumsum(np.bincount(src, minlength=m["doc_ids"].size), out=indptr[1:])
    return m, src, term, cnt, stc.CsrMatrix(indptr, term, cnt, m["vocab_size"])


@pytest.mark.parametrize("k", [5, 100])
def test_ten_iterations_on_the_golden_graph(ctx, golden, k):
    m, src, term, cnt, corpus = golden
    rng = np.random.default_rng(400 + k)
    alpha, eta = E.resolve(k)
    ndk0, nwk0 = random_state(rng, corpus.num_rows, corpus.num_cols, k)
    h = make_handle(ctx, corpus, k)
    h.set_state(ndk0, nwk0)
    h.next(10)
    ref = E.iterate(ndk0, nwk0, src, term, cnt, alpha, eta, 10)  # every vertex of the golden graph has an edge
    got = h.state()
    errs = [rel_err(g, r) for g, r in zip(got, ref)]
    print(f"golden graph, k={k}, 10 iterations: rel err N_dk {errs[0]:.2e} N_wk {errs[1]:.2e} N_k {errs[2]:.2e}")
    assert max(errs) <= 1e-9, errs
    h.close()


def test_golden_model_scores_through_load(ctx, golden):
    import stc

    m, src, term, cnt, _ = golden
    model = stc.DistributedLDAModel.load(REF_MODEL)
    alpha, eta = float(m["alpha"][0]), m["eta"]
    ref_ll = E.log_likelihood(m["doc_topics"], m["topics"], m["topics"].sum(axis=0), src, term, cnt, alpha, eta)
    ref_lp = E.log_prior(m["doc_topics"], m["topics"], m["topics"].sum(axis=0), src, term, alpha, eta)
    ll, lp = model.logLikelihood(ctx), model.logPrior(ctx)
    print(f"golden logLikelihood {ll!r} (restated {ref_ll!r}), logPrior {lp!r} (restated {ref_lp!r})")
    assert abs(ll - ref_ll) <= 1e-12 * abs(ref_ll)
    assert abs(lp - ref_lp) <= 1e-12 * abs(ref_lp)
    assert abs(ll - (-6374174.85)) <= 1e-9 * 6374174.85


@pytest.mark.parametrize("k", [5, 100])
def test_init_random(ctx, k):
    rng = np.random.default_rng(600 + k)
    corpus = random_corpus(rng, 40, 300)
    D, V = corpus.shape
    src, term, cnt = E.edges_of(corpus)
    h = make_handle(ctx, corpus, k)
    h.init_random(12345)
    a = h.state()
    assert max(E.mass_identities(*a, src, term, cnt)) <= 1e-12
    h.init_random(12345)
    b = h.state()
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    h.init_random(12346)
    c = h.state()
    assert not np.array_equal(a[0], c[0]) and not np.array_equal(a[1], c[1])
    gamma, u = E.init_gamma(12345, src.size, k)
    assert np.all((u > 0.0) & (u < 1.0)) and np.all((gamma > 0.0) & (gamma < 1.0))
    ref = E.init_state(12345, src, term, cnt, D, V, k)
    assert max(rel_err(g, r) for g, r in zip(a, ref)) <= 1e-12
    # the γ a one-edge document implies is its state row over the edge's count
    single = np.flatnonzero(np.diff(corpus.indptr) == 1)
    for d in single:
        g = a[0][d] / corpus.values[corpus.indptr[d]]
        assert np.all((g > 0.0) & (g < 1.0)) and abs(g.sum() - 1.0) <= 1e-12
    h.close()


@pytest.mark.parametrize("k", [5, 100])
def test_two_handles_are_bitwise_equal(ctx, k):
    rng = np.random.default_rng(700 + k)
    corpus = long_vertex_corpus(rng)
    ndk0, nwk0 = random_state(rng, corpus.num_rows, corpus.num_cols, k)
    out = []
    for _ in range(2):
        h = make_handle(ctx, corpus, k)
        h.set_state(ndk0, nwk0)
        h.next(5)
        out.append(h.state() + h.log_likelihood())
        h.close()
    assert all(np.array_equal(x, y) for x, y in zip(out[0], out[1]))


def test_python_surface_end_to_end(ctx, tmp_path):
    import stc

    rng = np.random.default_rng(7)
    D, V, k = 60, 200, 5
    corpus, _ = planted_corpus(rng, D, V, k)
    src, term, cnt = E.edges_of(corpus)
    lda = stc.MllibLDA(ctx).setOptimizer("em").setK(k).setMaxIterations(5).setSeed(3)
    model = lda.run(corpus)
    assert isinstance(model, stc.DistributedLDAModel) and model.isDistributed()
    assert len(lda.iterationTimes) == 5 and model.iterationTimes.size == 5
    alpha, eta = E.resolve(k)
    assert np.array_equal(model.docConcentration, np.full(k, alpha)) and model.topicConcentration == eta
    ref = E.iterate(*E.init_state(3, src, term, cnt, D, V, k)[:2], src, term, cnt, alpha, eta, 5)
    assert rel_err(model.topicsMatrix(), ref[1]) <= 1e-9 and rel_err(model.globalTopicTotals(), ref[2]) <= 1e-9
    ids, td = model.topicDistributions()
    assert np.array_equal(ids, np.arange(D)) and rel_err(td, ref[0] / ref[0].sum(axis=1, keepdims=True)) <= 1e-9
    top = model.topTopicsPerDocument(2)
    assert len(top) == D and all(w[0] >= w[1] and np.array_equal(w, td[d, t]) for d, t, w in top)
    per_topic = model.topDocumentsPerTopic(3)
    assert len(per_topic) == k
    for t, (docs, w) in enumerate(per_topic):
        assert w[0] >= w[1] >= w[2] and w[0] == td[:, t].max() and np.array_equal(w, td[docs, t])
    path = str(tmp_path / "em_model")
    model.save(path)
    with pytest.raises(FileExistsError):
        model.save(path)
    loaded = stc.DistributedLDAModel.load(path)
    assert np.array_equal(loaded.topicsMatrix(), model.topicsMatrix())
    assert loaded.logLikelihood(ctx) == model.logLikelihood(ctx) and loaded.logPrior(ctx) == model.logPrior(ctx)
    for (t0, i0, w0), (t1, i1, w1) in zip(model.describeTopics(5, ctx=ctx), loaded.describeTopics(5, ctx=ctx)):
        assert t0 == t1 and np.array_equal(i0, i1) and np.array_equal(w0, w1)
    dist = loaded.toLocal(ctx=ctx).topicDistribution(corpus)
    assert dist.shape == (D, k) and np.allclose(dist.sum(axis=1), 1.0, atol=1e-9)
    # logLikelihood over the iterations: the restatement shows it non-decreasing for this input, so must the GPU
    x = E.init_state(3, src, term, cnt, D, V, k)
    ref_ll = []
    for _ in range(6):
        ref_ll.append(E.log_likelihood(*x, src, term, cnt, alpha, eta))
        x = E.step(*x, src, term, cnt, alpha, eta)
    assert np.all(np.diff(ref_ll) >= 0.0), ref_ll
    h = make_handle(ctx, corpus, k)
    h.init_random(3)
    lls = []
    for _ in range(6):
        lls.append(h.log_likelihood()[0])
        h.next(1)
    assert np.all(np.diff(lls) >= 0.0), lls
    assert np.allclose(lls, ref_ll, rtol=1e-9, atol=0.0)
    assert lls[5] == model.logLikelihood(ctx)
    h.close()


def test_error_codes(ctx):
    import stc

    rng = np.random.default_rng(9)
    corpus = random_corpus(rng, 10, 50)

    def code(f):
        with pytest.raises(stc.StcError) as e:
            f()
        return e.value.code

    f32 = stc.DeviceCsr.upload(ctx, corpus, stc.STC_F32)
    assert code(lambda: stc.EmHandle(ctx, f32, 5)) == stc.STC_ERR_INVALID_ARG
    f32.free()
    dev = stc.DeviceCsr.upload(ctx, corpus, stc.STC_F64)
    for k in (1, 1025):
        assert code(lambda: stc.EmHandle(ctx, dev, k)) == stc.STC_ERR_INVALID_ARG
    for alpha, eta in ((1.0, -1.0), (0.5, -1.0), (-1.0, 1.0), (-1.0, -2.0)):
        assert code(lambda: stc.EmHandle(ctx, dev, 5, alpha, eta)) == stc.STC_ERR_INVALID_ARG
    big = stc.EmHandle(ctx, dev, 1024)  # the largest supported k
    assert big.k == 1024
    big.close()
    h = stc.EmHandle(ctx, dev, 5)
    assert h.concentrations() == (11.0, 1.1)  # readable before a state exists
    assert code(lambda: h.next(1)) == stc.STC_ERR_STATE
    assert code(h.log_likelihood) == stc.STC_ERR_STATE
    assert code(h.state) == stc.STC_ERR_STATE
    assert code(lambda: h.next(-1)) == stc.STC_ERR_INVALID_ARG
    lib = ctx.lib
    assert lib.stc_em_next(None, 1) == stc.STC_ERR_INVALID_ARG
    assert lib.stc_em_set_state(h.handle, None, None) == stc.STC_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        h.set_state(np.ones((3, 5)), np.ones((50, 5)))
    h.close()
    # single-device: a context connected to other ranks is refused
    c1 = stc.Context(0)
    c1.comm_init(stc.Context.unique_id(), 1, 0)
    d1 = stc.DeviceCsr.upload(c1, corpus, stc.STC_F64)
    assert code(lambda: stc.EmHandle(c1, d1, 5)) == stc.STC_ERR_STATE
    # a corpus of another context
    assert code(lambda: stc.EmHandle(ctx, d1, 5)) == stc.STC_ERR_INVALID_ARG
    d1.free()
    dev.free()
    c1.close()
