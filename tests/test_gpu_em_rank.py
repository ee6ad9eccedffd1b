"""GPU: the EM model's ranked queries (stc_em_describe / _top_documents / _top_topics, their group forms,
csrc/rank.hip) against the NumPy restatement (tests/em_rank_oracle.py).

The oracle is fed the handle's own state read back (so an fp32 handle is compared on the values it stores).
Comparison rule (em_rank_oracle): describe and top topics rank stored numbers — exact indices, describe's weights
bitwise N_wk[w][t] / N_k[t] with the handle's own N_k; top documents asserts that every pair of ranked neighbours
(the one across the cut included) is decided at B = (2k+2)·2^-53, then demands exact rows, and its weights (and
top topics') are bitwise because the device sums a row in the restated order, j ascending."""
import ctypes as C
import os

import numpy as np
import pytest

import em_oracle as E
import em_rank_oracle as R
from helpers import GOLDEN, golden_json, random_corpus

pytestmark = pytest.mark.gpu

REF_MODEL = os.path.join(GOLDEN, "LdaModel_EN_1591049082850")


def make_handle(ctx, corpus, k, dtype="f64"):
    import stc

    dev = stc.DeviceCsr.upload(ctx, corpus, stc.STC_F64)
    try:
        return stc.EmHandle(ctx, dev, k, dtype=dtype)
    finally:
        dev.free()


def random_state(rng, D, V, k):
    return rng.uniform(0.5, 5.0, size=(D, k)), rng.uniform(0.5, 5.0, size=(V, k))


def has_vertex(corpus):
    src, _, _ = E.edges_of(corpus)
    v = np.zeros(corpus.num_rows, bool)
    v[src] = True
    return v


def check_describe(h, n, label=""):
    _, nwk, nk = h.state()
    idx, w = h.describe(n)
    ref_idx, ref_w = R.describe(nwk, nk, n)
    assert idx.dtype == np.int32 and idx.shape == ref_idx.shape and w.shape == ref_w.shape
    assert np.array_equal(idx, ref_idx), (label, n)
    assert np.array_equal(w, ref_w), (label, n)
    return idx, w


def check_top_documents(h, vertex, n, label=""):
    ndk = h.state()[0]
    rows, w = h.top_documents(n)
    ref_rows, ref_w, undecided, min_gap = R.top_documents(ndk, vertex, n)
    print(f"{label} top_documents({n}): N={ref_rows.shape[1]} undecided {undecided} smallest gap {min_gap:.3g} "
          f"B {R.bound(h.k):.3g}")
    assert undecided == 0
    assert rows.dtype == np.int64 and rows.shape == ref_rows.shape and w.shape == ref_w.shape
    assert np.array_equal(rows, ref_rows), (label, n)
    assert np.array_equal(w, ref_w), (label, n)  # the restated sum order: bitwise (the bound allows B relative)
    return rows, w


def check_top_topics(h, n, label=""):
    ndk = h.state()[0]
    idx, w = h.top_topics(n)
    ref_idx, ref_w = R.top_topics(ndk, n)
    assert idx.dtype == np.int32 and idx.shape == ref_idx.shape and w.shape == ref_w.shape
    assert np.array_equal(idx, ref_idx), (label, n)
    assert np.array_equal(w, ref_w), (label, n)
    return idx, w


@pytest.mark.parametrize("k,dtype", [(2, "f64"), (5, "f64"), (64, "f64"), (65, "f64"), (100, "f64"), (257, "f64"),
                                     (1024, "f64"), (5, "f32"), (100, "f32"), (1024, "f32")])
def test_every_lane_layout(ctx, k, dtype):
    rng = np.random.default_rng(100 + k)
    corpus = random_corpus(rng, 40, 300)
    D, V = corpus.shape
    h = make_handle(ctx, corpus, k, dtype)
    h.set_state(*random_state(rng, D, V, k))
    if dtype == "f32":
        assert all(np.array_equal(a, a.astype(np.float32)) for a in h.state()[:2])
    vertex = has_vertex(corpus)
    for n in (1, 10, V, V + 700):
        check_describe(h, n, f"k={k}")
    for n in (1, 10, D, D + 60):
        check_top_documents(h, vertex, n, f"k={k} {dtype}")
    for n in (1, 10, k, k + 5):
        check_top_topics(h, n, f"k={k}")
    h.close()


@pytest.mark.parametrize("D,V,k", [(5000, 4000, 5), (700, 4000, 100)])
def test_several_tiles_and_ties_across_them(ctx, D, V, k):
    """A block's tile is 512 rows (rank.hip kTileRows): 5000 and 4000 rows are several tiles with a partial last
    one, 700 rows are two.  Rows 3, the middle and R−2 hold the same counts, raised so that they lead topic 0: a
    tie of three across the first, a middle and the last tile."""
    rng = np.random.default_rng(200 + k)
    corpus = random_corpus(rng, D, V, 1, 10)
    ndk0, nwk0 = random_state(rng, D, V, k)
    for x in (ndk0, nwk0):
        R_ = x.shape[0]
        x[3, 0] += 500.0
        x[R_ // 2] = x[3]
        x[R_ - 2] = x[3]
    h = make_handle(ctx, corpus, k)
    h.set_state(ndk0, nwk0)
    vertex = has_vertex(corpus)
    assert vertex[[3, D // 2, D - 2]].all()
    idx, _ = check_describe(h, 300, "tiles")
    nwk = h.state()[1]
    if nwk[3, 0] > 0.0:  # term 3 has a vertex: the equal rows that have one lead topic 0, in ascending order
        terms = np.flatnonzero(np.all(nwk == nwk[3], axis=1))
        assert idx[0][:terms.size].tolist() == terms.tolist()
    rows, _ = check_top_documents(h, vertex, 300, "tiles")
    assert rows[0][:3].tolist() == [3, D // 2, D - 2]
    check_top_documents(h, vertex, 2, "tiles")  # the cut inside the tie
    check_top_topics(h, 1, "tiles")
    check_top_topics(h, k, "tiles")
    h.close()


def test_a_tie_of_forty_rows_through_the_cut(ctx):
    rng = np.random.default_rng(31)
    D, V, k = 100, 300, 5
    corpus = random_corpus(rng, D, V)
    ndk0, nwk0 = random_state(rng, D, V, k)
    ndk0[30:70] = ndk0[30]      # forty bitwise-equal rows …
    ndk0[30:70, 1] += 400.0     # … that lead topic 1 (weight 0.95 … 0.9951) behind five others (>= 0.9995)
    ndk0[[2, 11, 75, 80, 99], 1] += 40000.0
    h = make_handle(ctx, corpus, k)
    h.set_state(ndk0, nwk0)
    rows, w = check_top_documents(h, np.ones(D, bool), 20, "forty")
    assert sorted(rows[1][:5].tolist()) == [2, 11, 75, 80, 99] and rows[1][5:].tolist() == list(range(30, 45))
    assert np.all(w[1][5:] == w[1][5])
    check_top_documents(h, np.ones(D, bool), 45, "forty")
    h.close()


def test_describe_past_the_term_vertices_lists_zero_count_terms_in_ascending_index(ctx):
    rng = np.random.default_rng(32)
    D, V, k = 12, 3000, 5
    corpus = random_corpus(rng, D, V, 1, 20)
    h = make_handle(ctx, corpus, k)
    h.set_state(*random_state(rng, D, V, k))
    used = np.unique(E.edges_of(corpus)[1])
    n = used.size + 1500  # thousands of zero-count terms tie at the cut, across several tiles
    idx, w = check_describe(h, n, "zeros")
    unused = np.setdiff1d(np.arange(V), used)
    for t in range(k):
        assert sorted(idx[t][:used.size].tolist()) == used.tolist()
        assert idx[t][used.size:].tolist() == unused[:1500].tolist() and np.all(w[t][used.size:] == 0.0)
    h.close()


@pytest.mark.parametrize("k,p,q", [(5, 1, 3), (64, 3, 40), (100, 10, 74), (100, 12, 70), (200, 70, 199)])
def test_equal_counts_inside_a_row_rank_by_topic(ctx, k, p, q):
    """test_gpu_em_assignments' placements: columns p < q equal and raised to lead the row — on two lanes of one row
    (k <= 64), in two slices of one lane (10 | 74) and on different lanes and slices; every other row has a third
    column above them, so the tie sits at ranks 0 | 1 and at ranks 1 | 2"""
    rng = np.random.default_rng(300 + k + p)
    corpus = random_corpus(rng, 40, 300)
    ndk0, nwk0 = random_state(rng, *corpus.shape, k)
    ndk0[:, p] += 50.0
    ndk0[:, q] = ndk0[:, p]
    ndk0[0::2, (p + 1) % k] = ndk0[0::2, p] + 1.0
    h = make_handle(ctx, corpus, k)
    h.set_state(ndk0, nwk0)
    for n in (1, 2, 3, k):
        idx, w = check_top_topics(h, n, f"k={k} p={p} q={q}")
    odd = idx[1::2]
    assert np.all(odd[:, 0] == p) and np.all(odd[:, 1] == q) and np.all(w[1::2, 0] == w[1::2, 1])
    even = idx[0::2]
    assert np.all(even[:, 1] == p) and np.all(even[:, 2] == q)
    h.close()


def test_digits(ctx):
    """column 0: every value in [1, 1 + 2^-30) — 3,000 values that differ in their last 8 bits only (256 distinct
    ones, each about 12 times), so a leading-digit selection must reach its last value digit whatever it keeps in
    reserve, and then rank the equal values by row; column 1 spans 1e-30 … 1e30; column 2 holds a subnormal and
    zeros"""
    import stc

    rng = np.random.default_rng(33)
    V, k = 3000, 3
    corpus = stc.CsrMatrix.from_rows([(np.arange(d * 100, (d + 1) * 100, dtype=np.int32), np.ones(100))
                                      for d in range(30)], V)
    nwk0 = np.zeros((V, k))
    nwk0[:, 0] = 1.0 + (rng.permutation(V) % 256) * 2.0 ** -52
    nwk0[:, 1] = 10.0 ** rng.uniform(-30.0, 30.0, V)
    nwk0[417, 2] = 3 * 5e-324
    assert nwk0[:, 0].max() < 1.0 + 2.0 ** -30 and np.unique(nwk0[:, 0]).size == 256
    h = make_handle(ctx, corpus, k)
    h.set_state(rng.uniform(0.5, 5.0, (30, k)), nwk0)
    assert np.array_equal(h.state()[1], nwk0)
    for n in (1, 10, 300, V):
        idx, w = check_describe(h, n, "digits")
        assert idx[2][0] == 417 and idx[2][1:].tolist() == [i for i in range(V) if i != 417][:n - 1]
    assert np.array_equal(idx[0], np.argsort(-nwk0[:, 0], kind="stable"))
    h.close()


def test_documents_without_an_edge(ctx):
    rng = np.random.default_rng(34)
    D, V, k = 60, 300, 5
    corpus = random_corpus(rng, D, V, empty_every=4)
    vertex = has_vertex(corpus)
    assert vertex.sum() == 45
    h = make_handle(ctx, corpus, k)
    h.set_state(*random_state(rng, D, V, k))
    for n in (7, 45, 46, D, D + 1):
        rows, _ = check_top_documents(h, vertex, n, "vertices")
        assert rows.shape == (k, min(n, 45)) and vertex[rows].all()
    for n in (1, 3, k):
        idx, w = check_top_topics(h, n, "vertices")
        assert np.all(idx[~vertex] == np.arange(n)) and np.all(w[~vertex] == 0.0)
    h.close()


def small_corpora():
    """test_gpu_em_group.test_filtering_and_empty_members' corpora: over 3 members "two" leaves member 2 without a
    row and "hollow" gives member 1 one row without an edge"""
    import stc

    filtered = stc.CsrMatrix.from_rows(
        [([0, 1, 3, 5], [2.0, 0.0, 0.0, 1.0]), ([], []), ([3, 8], [0.0, 0.0]), ([1, 2, 9], [1.0, 3.0, 2.0]), ([], []),
         ([0, 4, 8], [1.0, 2.0, 0.0]), ([0], [0.0]), ([6, 7, 9], [4.0, 1.0, 1.0])], 16)
    two = stc.CsrMatrix.from_rows([([0, 3, 5], [2.0, 1.0, 3.0]), ([3, 7], [1.0, 4.0])], 12)
    hollow = stc.CsrMatrix.from_rows([([0, 1, 2], [1.0, 2.0, 1.0]), ([3, 4], [0.0, 0.0]), ([1, 5], [3.0, 1.0])], 8)
    return {"filtered": filtered, "two": two, "hollow": hollow}


@pytest.mark.parametrize("which,n,k,dtype", [("filtered", 2, 5, "f64"), ("filtered", 3, 5, "f64"), ("two", 3, 5, "f64"),
                                             ("hollow", 3, 5, "f64"), ("random", 2, 100, "f64"),
                                             ("random", 3, 100, "f32"), ("random", 3, 5, "f64")])
def test_a_group_answers_as_the_single_handle(ctx, which, n, k, dtype):
    import stc

    rng = np.random.default_rng(500 + n + k)
    corpus = random_corpus(rng, 90, 300, empty_every=7) if which == "random" else small_corpora()[which]
    D, V = corpus.shape
    ndk0, nwk0 = random_state(rng, D, V, k)
    if which == "random":
        ndk0[[5, 40, 85]] = ndk0[5]  # a tie across the members' shards
    h = make_handle(ctx, corpus, k, dtype)
    h.set_state(ndk0, nwk0)
    vertex = has_vertex(corpus)
    with stc.EmGroup([0] * n, corpus, k, dtype=dtype) as g:
        g.set_state(ndk0, nwk0)
        assert all(np.array_equal(a, b) for a, b in zip(g.state(), h.state()))
        for m in (1, 4, V, V + 3):
            assert all(np.array_equal(a, b) for a, b in zip(g.describe(m), check_describe(h, m, which)))
        for m in (1, 2, 4, D, D + 3):
            got, ref = g.top_documents(m), check_top_documents(h, vertex, m, which)
            assert got[0].shape == ref[0].shape and all(np.array_equal(a, b) for a, b in zip(got, ref))
        for m in (1, 3, k + 1):
            assert all(np.array_equal(a, b) for a, b in zip(g.top_topics(m), check_top_topics(h, m, which)))
    h.close()


def test_two_handles_and_repeated_calls_are_bitwise_equal(ctx):
    rng = np.random.default_rng(35)
    D, V, k = 1500, 2000, 100
    corpus = random_corpus(rng, D, V, 1, 10)
    state = random_state(rng, D, V, k)
    outs = []
    for _ in range(2):
        h = make_handle(ctx, corpus, k)
        h.set_state(*state)
        for _ in range(2):
            outs.append(h.describe(300) + h.top_documents(300) + h.top_topics(3))
        h.close()
    for o in outs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(o, outs[0]))


def assert_models_agree(model, k, label):
    """device=True against device=False: the same shapes, ids and indices, weights within B"""
    B = R.bound(k)

    def worst(w0, w1):
        nz = w0 > 0.0
        return float(np.max(np.abs(w0[nz] - w1[nz]) / w0[nz])) if nz.any() else 0.0

    figures = [max(worst(a[2], b[2]) for a, b in zip(model.describeTopics(10 ** 6), model.describeTopics(10 ** 6, device=True))),
               max(worst(a[1], b[1]) for a, b in zip(model.topDocumentsPerTopic(10 ** 6),
                                                     model.topDocumentsPerTopic(10 ** 6, device=True))),
               max(worst(a[2], b[2]) for a, b in zip(model.topTopicsPerDocument(k), model.topTopicsPerDocument(k, device=True)))]
    print(f"{label}: largest relative weight difference, device against host: describe {figures[0]:.3g} "
          f"top documents {figures[1]:.3g} top topics {figures[2]:.3g} (B {B:.3g})")
    for n in (1, 7, 10 ** 6):
        host, dev = model.describeTopics(n), model.describeTopics(n, device=True)
        assert len(host) == len(dev) == k
        for (t0, i0, w0), (t1, i1, w1) in zip(host, dev):
            assert t0 == t1 and i0.dtype == i1.dtype and np.array_equal(i0, i1), (label, n, t0)
            assert np.all(np.abs(w0 - w1) <= B * w0)
        host, dev = model.topDocumentsPerTopic(n), model.topDocumentsPerTopic(n, device=True)
        assert len(host) == len(dev) == k
        for (i0, w0), (i1, w1) in zip(host, dev):
            assert i0.dtype == i1.dtype and np.array_equal(i0, i1), (label, n)
            assert np.all(np.abs(w0 - w1) <= B * w0)
    for n in (1, 3, k + 2):
        host, dev = model.topTopicsPerDocument(n), model.topTopicsPerDocument(n, device=True)
        assert len(host) == len(dev)
        for (d0, i0, w0), (d1, i1, w1) in zip(host, dev):
            assert d0 == d1 and i0.dtype == i1.dtype and np.array_equal(i0, i1), (label, n, d0)
            assert np.all(np.abs(w0 - w1) <= B * w0)


@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_model_surface(ctx, tmp_path, devices):
    import stc

    rng = np.random.default_rng(36)
    k = 5
    corpus = random_corpus(rng, 60, 50, empty_every=5)  # ids are not ranks: 48 document vertices of 60 rows
    assert np.unique(corpus.indices).size == 50  # every term has a vertex: the host path (toLocal) refuses a 0 count
    lda = stc.MllibLDA(ctx, devices=devices).setOptimizer("em").setK(k).setMaxIterations(3).setSeed(11)
    model = lda.run(corpus)
    assert model._em is not None and model._d["doc_ids"].size == 48
    assert_models_agree(model, k, "trained")
    ids = model._d["doc_ids"]
    assert all(set(i.tolist()) <= set(ids.tolist()) for i, _ in model.topDocumentsPerTopic(48, device=True))
    path = str(tmp_path / "m")
    model.save(path)
    loaded = stc.DistributedLDAModel.load(path)
    assert loaded._em is None
    assert_models_agree(loaded, k, "loaded")
    assert loaded._em is not None and loaded._em.num_docs == 48  # the rebuilt handle: rows are ranks, mapped to ids
    for (i0, w0), (i1, w1) in zip(model.topDocumentsPerTopic(9, device=True), loaded.topDocumentsPerTopic(9, device=True)):
        assert np.array_equal(i0, i1) and np.array_equal(w0, w1)
    for a, b in zip(model.topTopicsPerDocument(2, device=True), loaded.topTopicsPerDocument(2, device=True)):
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    if isinstance(model._em, stc.EmGroup):
        model._em.close()


def test_reference_model(ctx, oracle):
    import stc

    model = stc.DistributedLDAModel.load(REF_MODEL)
    meta = golden_json("en_describe.json")
    desc = model.describeTopics(10, device=True, ctx=ctx)
    for run, tops in meta["describe"].items():
        for t, lst in tops.items():
            _, idx, w = desc[int(t)]
            for j, e in enumerate(lst):
                assert idx[j] == e["index"], (run, t, j)
                assert abs(w[j] - float(e["weight"])) / float(e["weight"]) < 1e-12
    ref_idx, _ = oracle.describe_topics(model.topicsMatrix(), 300)
    got = model.describeTopics(300, device=True, ctx=ctx)
    assert np.array_equal(np.stack([g[1] for g in got]), ref_idx)


def test_errors(ctx):
    import stc

    rng = np.random.default_rng(37)
    corpus = random_corpus(rng, 10, 40)
    h = make_handle(ctx, corpus, 5)
    lib = ctx.lib
    i32, i64, dbl, n = (C.c_int32 * 400)(), (C.c_int64 * 400)(), (C.c_double * 400)(), C.c_int64(-1)
    with stc.EmGroup([0, 0], corpus, 5) as g:
        for pre, hd in (("stc_em_", h.handle), ("stc_em_group_", g.handle)):
            describe, top_docs, top_topics = (getattr(lib, pre + s) for s in ("describe", "top_documents", "top_topics"))
            if pre == "stc_em_":  # no state yet
                assert describe(hd, 3, i32, dbl) == stc.STC_ERR_STATE
                assert top_docs(hd, 3, C.byref(n), i64, dbl) == stc.STC_ERR_STATE
                assert top_topics(hd, 3, i32, dbl) == stc.STC_ERR_STATE
                h.set_state(*random_state(rng, 10, 40, 5))
            else:
                assert describe(hd, 3, i32, dbl) == stc.STC_ERR_STATE
                assert top_docs(hd, 3, C.byref(n), i64, dbl) == stc.STC_ERR_STATE
                assert top_topics(hd, 3, i32, dbl) == stc.STC_ERR_STATE
                g.set_state(*random_state(rng, 10, 40, 5))
            for bad in (0, -4):
                assert describe(hd, bad, i32, dbl) == stc.STC_ERR_INVALID_ARG
                assert top_docs(hd, bad, C.byref(n), i64, dbl) == stc.STC_ERR_INVALID_ARG
                assert top_topics(hd, bad, i32, dbl) == stc.STC_ERR_INVALID_ARG
            assert describe(hd, 3, None, dbl) == describe(hd, 3, i32, None) == stc.STC_ERR_INVALID_ARG
            assert top_docs(hd, 3, None, i64, dbl) == top_docs(hd, 3, C.byref(n), None, dbl) == stc.STC_ERR_INVALID_ARG
            assert top_docs(hd, 3, C.byref(n), i64, None) == stc.STC_ERR_INVALID_ARG
            assert top_topics(hd, 3, None, dbl) == top_topics(hd, 3, i32, None) == stc.STC_ERR_INVALID_ARG
            assert n.value == -1
            assert top_docs(hd, 3, C.byref(n), i64, dbl) == 0 and n.value == 3
            n.value = -1
    with pytest.raises(stc.StcIllegalArgument):
        h.describe(0)
    h.close()
