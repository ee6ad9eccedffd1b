"""GPU: DistributedLDAModel.topicAssignments (stc_em_topic_assignments, k_em_pass<kAssign>) against its NumPy
restatement (tests/em_assign_oracle.py).

Comparison rule (em_assign_oracle.compare): the oracle is fed the handle's own state read back, so only the
rounding of one factor separates the sides — the device forms (a·b)·(1/c), NumPy (a·b)/c, each a few units of
2^-53 from the exact value.  An edge whose oracle margin (relative gap between the two largest factors) exceeds
1e-12 must match exactly; on an edge at or below it the device's topic must have a factor within 1e-12 of the
maximum, and such edges may be at most 0.1 % of a case's edges (a cap; on these inputs the oracle leaves none:
minimum margin 1.9e-6 on the random cases, 9.5e-5 on the golden model's stored state)."""
import ctypes
import os

import numpy as np
import pytest

import em_assign_oracle as A
import em_oracle as E
from helpers import GOLDEN, planted_corpus, random_corpus

pytestmark = pytest.mark.gpu

REF_MODEL = os.path.join(GOLDEN, "LdaModel_EN_1591049082850")


def make_handle(ctx, corpus, k, alpha=-1.0, eta=-1.0):
    import stc

    dev = stc.DeviceCsr.upload(ctx, corpus, stc.STC_F64)
    try:
        return stc.EmHandle(ctx, dev, k, alpha, eta)
    finally:
        dev.free()


def random_state(rng, D, V, k):
    return rng.uniform(0.5, 5.0, size=(D, k)), rng.uniform(0.5, 5.0, size=(V, k))


def row_ptr(src, D):
    indptr = np.zeros(D + 1, np.int64)
    np.cumsum(np.bincount(src, minlength=D), out=indptr[1:])
    return indptr


def check_handle(h, src, term, label):
    """indptr / terms equal the filtered graph's, topics obey the comparison rule under the handle's own state"""
    indptr, terms, topics = h.topic_assignments()
    assert indptr.dtype == np.int64 and terms.dtype == np.int32 and topics.dtype == np.int32
    assert np.array_equal(indptr, row_ptr(src, h.num_docs)) and np.array_equal(terms, term)
    alpha, eta = h.concentrations()
    und, mm = A.compare(topics, *h.state(), src, term, alpha, eta)
    print(f"{label}: E={src.size} undecided {und} minimum margin {mm:.3g}")
    assert und <= 0.001 * src.size
    return topics


@pytest.mark.parametrize("k", [2, 5, 64, 65, 100, 257, 1024])
def test_every_lane_layout(ctx, k):
    rng = np.random.default_rng(100 + k)
    corpus = random_corpus(rng, 40, 300)
    src, term, _ = E.edges_of(corpus)
    h = make_handle(ctx, corpus, k)
    h.set_state(*random_state(rng, *corpus.shape, k))
    check_handle(h, src, term, f"k={k}")
    h.close()


def long_vertex_rows(rng, D=700, V=4000, long_doc=3000, hot=7):
    """as test_gpu_em.long_vertex_corpus: document 0 holds 3,000 entries (12 chunks of 256 edges, the last partly
    filled) and term `hot` occurs in all 700 documents"""
    rows = []
    cold = np.setdiff1d(np.arange(V), [hot])
    for d in range(D):
        n = long_doc - 1 if d == 0 else int(rng.integers(3, 11))
        ids = np.union1d(rng.choice(cold, size=n, replace=False), [hot]).astype(np.int32)
        rows.append((ids, rng.integers(1, 6, ids.size).astype(np.float64)))
    assert rows[0][0].size == long_doc and all(hot in r[0] for r in rows)
    return rows


@pytest.mark.parametrize("k", [5, 100])
def test_chunk_boundaries(ctx, k):
    """The second handle moves the long document away from its neighbours and to another chunk position.  Its
    corpus cannot hold that document alone: a term without an edge has no vertex, its injected row is stored
    as 0, and N_k — a factor's denominator — would change with it.  So a filler document that names every term
    of the first graph goes in front (16 chunks), the long document follows as row 1 with its state row, N_wk
    is the same array: N_k is bitwise the same, and so must be every assignment of the long document."""
    import stc

    rng = np.random.default_rng(200 + k)
    V = 4000
    rows = long_vertex_rows(rng, V=V)
    corpus = stc.CsrMatrix.from_rows(rows, V)
    src, term, _ = E.edges_of(corpus)
    ndk0, nwk0 = random_state(rng, *corpus.shape, k)
    h = make_handle(ctx, corpus, k)
    h.set_state(ndk0, nwk0)
    topics = check_handle(h, src, term, f"long vertex, k={k}")
    n_long = rows[0][0].size
    used = np.unique(term).astype(np.int32)
    alone = stc.CsrMatrix.from_rows([(used, np.ones(used.size)), rows[0]], V)
    h2 = make_handle(ctx, alone, k)
    h2.set_state(np.stack([rng.uniform(0.5, 5.0, k), ndk0[0]]), nwk0)
    assert np.array_equal(h2.state()[2], h.state()[2])
    ip2, terms2, topics2 = h2.topic_assignments()
    assert ip2.tolist() == [0, used.size, used.size + n_long] and np.array_equal(terms2[used.size:], rows[0][0])
    assert np.array_equal(topics2[used.size:], topics[:n_long])
    h.close()
    h2.close()


def filtered_corpus():
    """as test_gpu_em.filtered_corpus: rows 1 and 4 empty, rows 2 and 6 only explicit zeros, zeros inside rows
    0 and 5"""
    import stc

    rows = [([0, 1, 3, 5], [2.0, 0.0, 0.0, 1.0]), ([], []), ([3, 8], [0.0, 0.0]), ([1, 2, 9], [1.0, 3.0, 2.0]),
            ([], []), ([0, 4, 8], [1.0, 2.0, 0.0]), ([0], [0.0]), ([6, 7, 9], [4.0, 1.0, 1.0])]
    return stc.CsrMatrix.from_rows(rows, 16)


def test_edge_filtering(ctx):
    corpus, k = filtered_corpus(), 5
    src, term, _ = E.edges_of(corpus)
    rng = np.random.default_rng(3)
    h = make_handle(ctx, corpus, k)
    assert h.num_edges == 10
    h.set_state(*random_state(rng, *corpus.shape, k))
    topics = check_handle(h, src, term, "filtered")
    indptr, terms, _ = h.topic_assignments()
    assert indptr.tolist() == [0, 2, 2, 2, 5, 5, 7, 7, 10]  # documents 1, 2, 4 and 6 have no edge
    assert terms.tolist() == [0, 5, 1, 2, 9, 0, 4, 6, 7, 9] and topics.size == 10  # no explicit zero
    assert all(np.all(np.diff(terms[a:b]) > 0) for a, b in zip(indptr[:-1], indptr[1:]))
    h.close()


@pytest.mark.parametrize("k,p,q", [(5, 1, 3), (64, 3, 40), (100, 10, 74), (100, 12, 70), (200, 70, 199)])
def test_exact_ties_go_to_the_smallest_index(ctx, k, p, q):
    """columns p < q hold the same values in N_dk and N_wk, raised so that the maximum lies among them; the
    derived N_k[p] and N_k[q] are sums of identical values in one fixed order, so the two factors are bitwise
    equal on every edge and the answer is p, never q"""
    rng = np.random.default_rng(300 + k + p)
    corpus = random_corpus(rng, 40, 300)
    src, term, _ = E.edges_of(corpus)
    ndk0, nwk0 = random_state(rng, *corpus.shape, k)
    for x in (ndk0, nwk0):
        x[:, p] += 50.0
        x[:, q] = x[:, p]
    h = make_handle(ctx, corpus, k)
    h.set_state(ndk0, nwk0)
    ndk, nwk, nk = h.state()
    assert np.array_equal(ndk[:, p], ndk[:, q]) and np.array_equal(nwk[:, p], nwk[:, q]) and nk[p] == nk[q]
    alpha, eta = h.concentrations()
    f = E.edge_factors(ndk, nwk, nk, src, term, alpha, eta)
    assert np.all(np.argmax(f, axis=1) == p) and np.array_equal(f[:, p], f[:, q])
    topics = h.topic_assignments()[2]
    assert topics.size == src.size and np.all(topics == p), np.unique(topics, return_counts=True)
    h.close()


@pytest.mark.parametrize("k", [5, 64, 100, 257])
def test_a_state_constant_across_topics_assigns_topic_0(ctx, k):
    rng = np.random.default_rng(350 + k)
    corpus = random_corpus(rng, 40, 300)
    D, V = corpus.shape
    h = make_handle(ctx, corpus, k)
    h.set_state(np.repeat(rng.uniform(0.5, 5.0, (D, 1)), k, axis=1), np.repeat(rng.uniform(0.5, 5.0, (V, 1)), k, axis=1))
    nk = h.state()[2]
    assert np.all(nk == nk[0])
    topics = h.topic_assignments()[2]
    assert topics.size == h.num_edges and np.all(topics == 0), np.unique(topics, return_counts=True)
    h.close()


def test_trained_state_and_surface(ctx, tmp_path):
    import stc

    rng = np.random.default_rng(7)
    D, V, k = 60, 400, 5
    corpus, _ = planted_corpus(rng, D, V, k)
    src, term, cnt = E.edges_of(corpus)
    alpha, eta = E.resolve(k)
    # the margin after training, confirmed on the CPU restatement first
    ref = E.iterate(*E.init_state(3, src, term, cnt, D, V, k)[:2], src, term, cnt, alpha, eta, 3)
    ref_margin = A.assignments(*ref, src, term, alpha, eta)[1]
    print(f"trained state (restatement): minimum margin {ref_margin.min():.3g}")
    assert ref_margin.min() > 1e-9
    model = stc.MllibLDA(ctx).setOptimizer("em").setK(k).setMaxIterations(3).setSeed(3).run(corpus)
    out = model.topicAssignments()
    ids, _ = model.topicDistributions()
    assert [d for d, _, _ in out] == ids.tolist() == list(range(D))
    for d, terms, topics in out:
        assert terms.dtype == np.int32 and topics.dtype == np.int32 and terms.shape == topics.shape
        row_ids, row_vals = corpus.row(d)
        assert np.array_equal(terms, np.asarray(row_ids)[np.asarray(row_vals) != 0.0])
    got = np.concatenate([t for _, _, t in out])
    ndk = np.zeros((D, k))
    ndk[ids] = model._d["doc_topics"]
    und, mm = A.compare(got, ndk, model.topicsMatrix(), model.globalTopicTotals(), src, term, alpha, eta)
    print(f"trained state: E={src.size} undecided {und} minimum margin {mm:.3g}")
    assert und <= 0.001 * src.size
    assert model.javaTopicAssignments is not None
    # a loaded model builds its own graph (rows = ranks among the document ids)
    path = str(tmp_path / "em_model")
    model.save(path)
    loaded = stc.DistributedLDAModel.load(path)
    again = loaded.topicAssignments(ctx)
    assert len(again) == len(out)
    for (d0, t0, z0), (d1, t1, z1) in zip(out, again):
        assert d0 == d1 and np.array_equal(t0, t1) and np.array_equal(z0, z1)
    # two handles from the same corpus and seed
    res = []
    for _ in range(2):
        h = make_handle(ctx, corpus, k)
        h.init_random(3)
        h.next(3)
        res.append(h.topic_assignments())
        h.close()
    assert all(np.array_equal(x, y) for x, y in zip(res[0], res[1]))
    assert np.array_equal(res[0][2], got)


def test_the_references_own_model(ctx):
    import stc

    m = stc.io.load_distributed(REF_MODEL)
    row, term, _ = E.edges_of_model(m)
    assert (m["k"], float(m["alpha"][0]), m["eta"]) == (5, 11.0, 1.1)
    model = stc.DistributedLDAModel.load(REF_MODEL)
    out = model.topicAssignments(ctx)
    assert len(out) == 51 and [d for d, _, _ in out] == m["doc_ids"].tolist()
    assert sum(t.size for _, t, _ in out) == 253368 == row.size
    indptr = row_ptr(row, 51)
    for i, (_, terms, topics) in enumerate(out):
        assert np.array_equal(terms, term[indptr[i]:indptr[i + 1]]) and topics.shape == terms.shape
    got = np.concatenate([z for _, _, z in out])
    nk = m["topics"].sum(axis=0)
    ref, _ = A.assignments(m["doc_topics"], m["topics"], nk, row, term, 11.0, 1.1)
    assert np.bincount(ref, minlength=5).tolist() == [54048, 63774, 38890, 49938, 46718]
    # the handle derives N_k itself; the comparison uses what it derived
    und, mm = A.compare(got, *model._em_handle(ctx).state(), row, term, 11.0, 1.1)
    print(f"golden model: topics per edge {np.bincount(got, minlength=5).tolist()} undecided {und} "
          f"minimum margin {mm:.3g}")
    assert und <= 0.001 * row.size


def test_errors(ctx):
    import stc

    rng = np.random.default_rng(9)
    corpus = random_corpus(rng, 10, 50)
    lib = ctx.lib

    def code(f):
        with pytest.raises(stc.StcError) as e:
            f()
        return e.value.code

    h = make_handle(ctx, corpus, 5)
    assert code(h.topic_assignments) == stc.STC_ERR_STATE  # before init_random / set_state
    assert lib.stc_em_topic_assignments(h.handle, None, None, None) == stc.STC_ERR_STATE
    assert lib.stc_em_topic_assignments(None, None, None, None) == stc.STC_ERR_INVALID_ARG
    h.init_random(4)
    assert lib.stc_em_topic_assignments(h.handle, None, None, None) == stc._lib.STC_OK  # every output may be NULL
    topics = np.full(h.num_edges, -1, np.int32)
    p_topics = topics.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    assert lib.stc_em_topic_assignments(h.handle, None, None, p_topics) == stc._lib.STC_OK
    assert np.array_equal(topics, h.topic_assignments()[2])
    # behind queued iterations the call waits for them
    h.next(7)
    a = h.topic_assignments()
    ctx.synchronize()
    b = h.topic_assignments()
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    h2 = make_handle(ctx, corpus, 5)
    h2.init_random(4)
    h2.next(7)
    ctx.synchronize()
    assert np.array_equal(h2.topic_assignments()[2], a[2])
    h.close()
    h2.close()
    # single-device: refused once the context is connected to other ranks
    c1 = stc.Context(0)
    h3 = make_handle(c1, corpus, 5)
    h3.init_random(4)
    c1.comm_init(stc.Context.unique_id(), 1, 0)
    assert code(h3.topic_assignments) == stc.STC_ERR_STATE
    h3.close()
    c1.close()
