"""GPU: the EM optimizer over several devices (stc_em_group_*, csrc/em_group.hip, the member side of lda_em.hip)
against the NumPy restatement (tests/em_oracle.py), a single EmHandle, and its own replicas.

Members share device 0 (the in-process transport: the multi-GPU decomposition on one GPU) unless a test says
otherwise.  Bounds are the single handle's (tests/test_gpu_em.py): one step ≤ 1e-12 elementwise relative (two
summation orders of positive terms differ by ≈ 1.5e-14), ten steps ≤ 1e-9.  What must be bitwise: N_dk' of one
step and of the initial state (a document lies in one shard, with the same chunks, and the injected / derived
inputs are the same numbers), the members' replicas, two groups of one member count, a one-member group and an
EmHandle."""
import ctypes as C
import os

import numpy as np
import pytest

import em_assign_oracle as A
import em_group_oracle as G
import em_oracle as E
from helpers import GOLDEN, planted_corpus

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
        return stc.EmHandle(ctx, dev, k, alpha, eta)
    finally:
        dev.free()


def make_group(n, corpus, k, alpha=-1.0, eta=-1.0):
    import stc

    return stc.EmGroup([0] * n, corpus, k, alpha, eta)


def random_state(rng, D, V, k):
    return rng.uniform(0.5, 5.0, size=(D, k)), rng.uniform(0.5, 5.0, size=(V, k))


def long_vertex_corpus(rng, D=700, V=4000, long_doc=3000, hot=7):
    """as test_gpu_em.long_vertex_corpus: document 0 holds 3,000 entries (12 chunks), term `hot` occurs in all
    700 documents (3 chunks on a single handle); shards balanced by entries are very unequal in rows"""
    import stc

    rows = []
    cold = np.setdiff1d(np.arange(V), [hot])
    for d in range(D):
        n = long_doc - 1 if d == 0 else int(rng.integers(3, 11))
        ids = np.union1d(rng.choice(cold, size=n, replace=False), [hot]).astype(np.int32)
        rows.append((ids, rng.integers(1, 6, ids.size).astype(np.float64)))
    assert rows[0][0].size == long_doc and all(hot in r[0] for r in rows)
    return stc.CsrMatrix.from_rows(rows, V)


def filtered_corpus():
    """as test_gpu_em.filtered_corpus: rows 1 and 4 empty, rows 2 and 6 only explicit zeros, zeros inside rows 0
    and 5; terms 3, 8 and 10–15 in no edge (3 and 8 only under explicit zeros)"""
    import stc

    rows = [([0, 1, 3, 5], [2.0, 0.0, 0.0, 1.0]), ([], []), ([3, 8], [0.0, 0.0]), ([1, 2, 9], [1.0, 3.0, 2.0]),
            ([], []), ([0, 4, 8], [1.0, 2.0, 0.0]), ([0], [0.0]), ([6, 7, 9], [4.0, 1.0, 1.0])]
    return stc.CsrMatrix.from_rows(rows, 16)


def member_shape(g, i):
    """(rows, edges) of member i's shard (stc_em_group_member + stc_em_shape)"""
    h, _ = g.members()[i]
    kk, d, v, e = C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()
    assert g.lib.stc_em_shape(h, C.byref(kk), C.byref(d), C.byref(v), C.byref(e)) == 0
    assert (kk.value, v.value) == (g.k, g.vocab_size)
    return d.value, e.value


def member_replica(g, i):
    """(rows, row0, N_wk, N_k) of member i, read through stc_em_group_member + the public stc_em_* readers"""
    h, r0 = g.members()[i]
    d = C.c_int64(member_shape(g, i)[0])
    tt = np.zeros((g.vocab_size, g.k))
    nk = np.zeros(g.k)
    assert g.lib.stc_em_get_state(h, None, tt.ctypes.data_as(C.POINTER(C.c_double)),
                                  nk.ctypes.data_as(C.POINTER(C.c_double)), None, None) == 0
    return d.value, r0, tt, nk


@pytest.mark.parametrize("k", [5, 100])
@pytest.mark.parametrize("n", [2, 3])
def test_one_step_matches_the_restatement(ctx, n, k):
    rng = np.random.default_rng(200 + k)
    corpus = long_vertex_corpus(rng)
    D, V = corpus.shape
    src, term, cnt = E.edges_of(corpus)
    sh = G.shards(corpus, n)
    assert sh[0][1] - sh[0][0] < 0.3 * (sh[-1][1] - sh[-1][0])  # very unequal in rows (n = 3: one row against 371)
    assert all(7 in s[4] for s in sh)  # the hot term is in every shard
    in_shards = sum(np.bincount(np.unique(s[4]), minlength=V) for s in sh)
    assert np.count_nonzero(in_shards == 1) > 1000  # 1,400 to 1,800 of the 3,600 terms lie in one shard only
    alpha, eta = E.resolve(k)
    ndk0, nwk0 = random_state(rng, D, V, k)
    with make_group(n, corpus, k) as g:
        assert (g.k, g.num_docs, g.vocab_size, g.num_edges) == (k, D, V, src.size)
        assert g.transport() == "in-process" and len(g.members()) == n
        assert [r0 for _, r0 in g.members()] == [s[0] for s in sh]
        g.set_state(ndk0, nwk0)
        rd, rw = E.mask_state(ndk0, nwk0, src, term)
        got = g.state()
        # a term whose edges all lie in another member's shard keeps its row on every member
        assert np.array_equal(got[0], rd) and np.array_equal(got[1], rw)
        for i in range(n):
            assert np.array_equal(member_replica(g, i)[2], rw)
        assert rel_err(got[2], rw.sum(axis=0)) <= 1e-12
        ref = E.step(rd, rw, rw.sum(axis=0), src, term, cnt, alpha, eta)
        g.next(1)
        got = g.state()
    errs = [rel_err(a, r) for a, r in zip(got, ref)]
    print(f"{n} members, k={k}: rel err N_dk {errs[0]:.2e} N_wk {errs[1]:.2e} N_k {errs[2]:.2e}")
    assert max(errs) <= 1e-12, errs
    h = make_handle(ctx, corpus, k)
    h.set_state(ndk0, nwk0)
    h.next(1)
    single = h.state()
    h.close()
    assert np.array_equal(got[0], single[0])
    assert max(rel_err(a, b) for a, b in zip(got[1:], single[1:])) <= 1e-12


@pytest.mark.parametrize("which,n", [("filtered", 2), ("long", 3)])
def test_init_random_uses_global_edge_positions(ctx, which, n):
    k, seed = 5, 12345
    corpus = filtered_corpus() if which == "filtered" else long_vertex_corpus(np.random.default_rng(31))
    D, V = corpus.shape
    src, term, cnt = E.edges_of(corpus)
    sh = G.shards(corpus, n)
    if which == "filtered":  # member 0: rows 0–3, 9 entries, 5 edges: member 1's first key is 5, not 9
        assert [(lo, hi, base) for lo, hi, base, *_ in sh] == [(0, 4, 0), (4, 8, 5)] and corpus.indptr[4] == 9
    with make_group(n, corpus, k) as g:
        g.init_random(seed)
        got = g.state()
        g.init_random(seed)
        again = g.state()
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    h = make_handle(ctx, corpus, k)
    h.init_random(seed)
    single = h.state()
    h.close()
    ref = E.init_state(seed, src, term, cnt, D, V, k)
    assert np.array_equal(got[0], single[0])
    for other in (single, ref):
        errs = [rel_err(a, b) for a, b in zip(got, other)]
        assert max(errs) <= 1e-12, errs
    assert max(E.mass_identities(*got, src, term, cnt)) <= 1e-12


def small_corpora():
    import stc

    two = stc.CsrMatrix.from_rows([([0, 3, 5], [2.0, 1.0, 3.0]), ([3, 7], [1.0, 4.0])], 12)
    # member 1 of 3 owns document 1 alone: two entries, no edge
    hollow = stc.CsrMatrix.from_rows([([0, 1, 2], [1.0, 2.0, 1.0]), ([3, 4], [0.0, 0.0]), ([1, 5], [3.0, 1.0])], 8)
    return {"filtered": (filtered_corpus(), 4), "two": (two, 3), "hollow": (hollow, 3)}


@pytest.mark.parametrize("which", ["filtered", "two", "hollow"])
def test_filtering_and_empty_members(ctx, which):
    corpus, n = small_corpora()[which]
    k = 5
    D, V = corpus.shape
    src, term, cnt = E.edges_of(corpus)
    sh = G.shards(corpus, n)
    if which == "two":
        assert [(s[0], s[1]) for s in sh] == [(0, 1), (1, 2), (2, 2)]  # member 2 has no row
    if which == "hollow":
        assert (sh[1][0], sh[1][1], sh[1][3].size) == (1, 2, 0)  # a row, no edge
    no_doc = sorted(set(range(D)) - set(src.tolist()))
    no_term = sorted(set(range(V)) - set(term.tolist()))
    alpha, eta = E.resolve(k)
    rng = np.random.default_rng(3)
    ndk0, nwk0 = random_state(rng, D, V, k)
    with make_group(n, corpus, k) as g:
        assert g.num_edges == src.size
        assert [member_shape(g, i) for i in range(n)] == [(s[1] - s[0], s[3].size) for s in sh]
        g.set_state(ndk0, nwk0)
        rd, rw = E.mask_state(ndk0, nwk0, src, term)
        rk = rw.sum(axis=0)
        for it in range(3):
            got = g.state()
            assert np.all(got[0][no_doc] == 0.0) and np.all(got[1][no_term] == 0.0)
            assert max(rel_err(a, r) for a, r in zip(got, (rd, rw, rk))) <= 1e-12
            ll, lp = g.log_likelihood()
            ref_ll = E.log_likelihood(rd, rw, rk, src, term, cnt, alpha, eta)
            ref_lp = E.log_prior(rd, rw, rk, src, term, alpha, eta)  # present vertices, once each
            print(f"{which} it {it}: ll {ll!r} ({ref_ll!r}) lp {lp!r} ({ref_lp!r})")
            assert abs(ll - ref_ll) <= 1e-12 * abs(ref_ll) and abs(lp - ref_lp) <= 1e-12 * abs(ref_lp)
            if it < 2:
                rd, rw, rk = E.step(rd, rw, rk, src, term, cnt, alpha, eta)
                g.next(1)
        g.init_random(9)
        got = g.state()
        assert np.all(got[0][no_doc] == 0.0) and np.all(got[1][no_term] == 0.0)
        assert np.all(got[0][np.unique(src)] > 0.0) and np.all(got[1][np.unique(term)] > 0.0)


@pytest.fixture(scope="module")
def golden():
    import stc

    m = stc.io.load_distributed(REF_MODEL)
    src, term, cnt = E.edges_of_model(m)
    indptr = np.zeros(m["doc_ids"].size + 1, np.int64)
    np.cumsum(np.bincount(src, minlength=m["doc_ids"].size), out=indptr[1:])
    corpus = stc.CsrMatrix(indptr, term, cnt, m["vocab_size"])
    k = 5
    rng = np.random.default_rng(400 + k)
    ndk0, nwk0 = random_state(rng, corpus.num_rows, corpus.num_cols, k)
    ref = E.iterate(ndk0, nwk0, src, term, cnt, *E.resolve(k), 10)  # every vertex of the golden graph has an edge
    return corpus, k, ndk0, nwk0, ref


def check_ten_golden_iterations(ctx, golden, devices):
    import stc

    corpus, k, ndk0, nwk0, ref = golden
    with stc.EmGroup(devices, corpus, k) as g:
        g.set_state(ndk0, nwk0)
        g.next(10)
        got = g.state()
        transport = g.transport()
    h = make_handle(ctx, corpus, k)
    h.set_state(ndk0, nwk0)
    h.next(10)
    single = h.state()
    h.close()
    e_ref = [rel_err(a, r) for a, r in zip(got, ref)]
    e_one = [rel_err(a, r) for a, r in zip(got, single)]
    print(f"golden graph, devices {devices} ({transport}), k={k}, 10 iterations: against the restatement "
          f"{max(e_ref):.2e}, against a single handle {max(e_one):.2e}")
    assert max(e_ref) <= 1e-9 and max(e_one) <= 1e-9, (e_ref, e_one)


def test_ten_iterations_on_the_golden_graph(ctx, golden):
    check_ten_golden_iterations(ctx, golden, [0, 0, 0])


def test_two_real_devices(ctx, golden):
    import stc

    if stc.Context.device_count() < 2:
        pytest.skip("needs two devices")
    check_ten_golden_iterations(ctx, golden, [0, 1])


@pytest.mark.parametrize("k", [5, 100])
def test_replicas_and_reproducibility(ctx, k):
    rng = np.random.default_rng(700 + k)
    corpus = long_vertex_corpus(rng)
    ndk0, nwk0 = random_state(rng, corpus.num_rows, corpus.num_cols, k)
    runs = []
    for _ in range(2):
        with make_group(3, corpus, k) as g:
            g.set_state(ndk0, nwk0)
            g.next(5)
            reps = [member_replica(g, i) for i in range(3)]
            for r in reps[1:]:
                assert np.array_equal(r[2], reps[0][2]) and np.array_equal(r[3], reps[0][3])
            st = g.state()
            assert np.array_equal(st[1], reps[0][2]) and np.array_equal(st[2], reps[0][3])
            runs.append(st + g.log_likelihood() + g.topic_assignments())
    assert all(np.array_equal(x, y) for x, y in zip(runs[0], runs[1]))
    # one member: no collective, the single handle's numbers
    with make_group(1, corpus, k) as g:
        assert g.transport() == "none"
        g.set_state(ndk0, nwk0)
        g.next(5)
        one = g.state() + g.log_likelihood() + g.topic_assignments()
    h = make_handle(ctx, corpus, k)
    h.set_state(ndk0, nwk0)
    h.next(5)
    single = h.state() + h.log_likelihood() + h.topic_assignments()
    h.close()
    assert all(np.array_equal(x, y) for x, y in zip(one, single))


def test_rccl_path_on_one_gpu(ctx, monkeypatch):
    """STC_GROUP_RCCL=1: a one-member group with a real communicator (ncclCommInitAll), its member driven from
    its own host thread, the all-reduce of N_wk' a one-rank RCCL all-reduce: bitwise the plain EmHandle"""
    import stc

    monkeypatch.setenv("STC_GROUP_RCCL", "1")
    k = 5
    rng = np.random.default_rng(55)
    corpus = long_vertex_corpus(rng)
    try:
        g = stc.EmGroup([0], corpus, k)
    except stc.StcError as e:
        if e.code != stc.STC_ERR_RCCL:
            raise
        pytest.skip(f"RCCL communicator on one device refused: {e}")
    with g:
        assert g.transport() == "rccl"
        g.init_random(8)
        g.next(5)
        g.synchronize()
        got = g.state() + g.log_likelihood() + g.topic_assignments()
    monkeypatch.delenv("STC_GROUP_RCCL")
    h = make_handle(ctx, corpus, k)
    h.init_random(8)
    h.next(5)
    single = h.state() + h.log_likelihood() + h.topic_assignments()
    h.close()
    assert all(np.array_equal(x, y) for x, y in zip(got, single))


def row_ptr(src, D):
    indptr = np.zeros(D + 1, np.int64)
    np.cumsum(np.bincount(src, minlength=D), out=indptr[1:])
    return indptr


@pytest.mark.parametrize("k", [5, 100])
def test_topic_assignments(ctx, k):
    rng = np.random.default_rng(900 + k)
    corpus = long_vertex_corpus(rng)
    D, V = corpus.shape
    src, term, cnt = E.edges_of(corpus)
    alpha, eta = E.resolve(k)
    ndk0, nwk0 = random_state(rng, D, V, k)
    # the condition of the exact comparison, on the CPU first: under this seed the restatement leaves no edge
    # undecided, with room for the rounding of the device's own N_k
    rd, rw = E.mask_state(ndk0, nwk0, src, term)
    margin = A.assignments(rd, rw, rw.sum(axis=0), src, term, alpha, eta)[1]
    print(f"k={k}: restatement's minimum margin {margin.min():.3g}")
    assert margin.min() > 1e-9
    with make_group(3, corpus, k) as g:
        g.set_state(ndk0, nwk0)
        indptr, terms, topics = g.topic_assignments()
        state = g.state()
        assert (alpha, eta) == g.concentrations()
    assert indptr.dtype == np.int64 and terms.dtype == np.int32 and topics.dtype == np.int32
    assert np.array_equal(indptr, row_ptr(src, D)) and np.array_equal(terms, term)
    und, mm = A.compare(topics, *state, src, term, alpha, eta)
    print(f"k={k}: E={src.size} undecided {und} minimum margin {mm:.3g}")
    assert und == 0
    assert np.array_equal(topics, A.assignments(*state, src, term, alpha, eta)[0])


def test_topic_assignments_skip_documents_without_an_edge(ctx):
    corpus, k = filtered_corpus(), 5
    rng = np.random.default_rng(3)
    with make_group(3, corpus, k) as g:
        g.set_state(*random_state(rng, *corpus.shape, k))
        indptr, terms, topics = g.topic_assignments()
    assert indptr.tolist() == [0, 2, 2, 2, 5, 5, 7, 7, 10]
    assert terms.tolist() == [0, 5, 1, 2, 9, 0, 4, 6, 7, 9] and topics.size == 10


def test_python_surface(ctx, tmp_path):
    import stc

    rng = np.random.default_rng(7)
    D, V, k = 60, 200, 5
    planted, _ = planted_corpus(rng, D, V, k)
    rows = [planted.row(d) for d in range(D)]
    rows.insert(9, (np.zeros(0, np.int32), np.zeros(0)))  # document 9 has no vertex: ids are not ranks
    corpus = stc.CsrMatrix.from_rows(rows, V)
    lda = stc.MllibLDA(devices=[0, 0]).setOptimizer("em").setK(k).setMaxIterations(5).setSeed(3)
    model = lda.run(corpus)
    assert isinstance(model, stc.DistributedLDAModel) and len(lda.iterationTimes) == 5
    one = stc.MllibLDA(ctx).setOptimizer("em").setK(k).setMaxIterations(5).setSeed(3).run(corpus)
    ll, ll1 = model.logLikelihood(), one.logLikelihood(ctx)
    assert abs(ll - ll1) <= 1e-9 * abs(ll1)
    assert abs(model.logPrior() - one.logPrior(ctx)) <= 1e-9 * abs(one.logPrior(ctx))
    ids, td = model.topicDistributions()
    ids1, td1 = one.topicDistributions()
    assert np.array_equal(ids, ids1) and ids.tolist() == [d for d in range(D + 1) if d != 9]
    assert rel_err(td, td1) <= 1e-9 and rel_err(model.topicsMatrix(), one.topicsMatrix()) <= 1e-9
    out = model.topicAssignments()
    assert [d for d, _, _ in out] == ids.tolist()
    for d, terms, topics in out:
        assert np.array_equal(terms, corpus.row(d)[0]) and topics.shape == terms.shape
    path = str(tmp_path / "em_group_model")
    model.save(path)
    loaded = stc.DistributedLDAModel.load(path)
    assert np.array_equal(loaded.topicsMatrix(), model.topicsMatrix())
    assert abs(loaded.logLikelihood(ctx) - ll) <= 1e-12 * abs(ll)  # a single graph rebuilt from the saved edges
    # setDevices after construction, and none: the single-device path as before
    again = stc.MllibLDA(ctx).setDevices([0, 0]).setOptimizer("em").setK(k).setMaxIterations(5).setSeed(3).run(corpus)
    assert np.array_equal(again.topicsMatrix(), model.topicsMatrix())


def test_errors(ctx):
    import stc

    corpus = filtered_corpus()

    def code(f):
        with pytest.raises(stc.StcError) as e:
            f()
        return e.value.code

    assert code(lambda: stc.EmGroup([0, 1, 0], corpus, 5)) == stc.STC_ERR_INVALID_ARG  # neither distinct nor the same
    assert code(lambda: stc.EmGroup([0] * 17, corpus, 5)) == stc.STC_ERR_INVALID_ARG
    for k in (1, 1025):
        assert code(lambda: stc.EmGroup([0, 0], corpus, k)) == stc.STC_ERR_INVALID_ARG
    for alpha, eta in ((1.0, -1.0), (-1.0, 1.0)):
        assert code(lambda: stc.EmGroup([0, 0], corpus, 5, alpha, eta)) == stc.STC_ERR_INVALID_ARG
    with make_group(2, corpus, 5) as g:
        assert g.concentrations() == (11.0, 1.1)  # readable before a state exists
        assert code(lambda: g.next(1)) == stc.STC_ERR_STATE
        assert code(g.log_likelihood) == stc.STC_ERR_STATE
        assert code(g.topic_assignments) == stc.STC_ERR_STATE
        assert code(g.state) == stc.STC_ERR_STATE
        D, V = corpus.shape
        bad = np.ones((D, 5))
        bad[7, 2] = -1.0
        assert code(lambda: g.set_state(bad, np.ones((V, 5)))) == stc.STC_ERR_INVALID_ARG
        bad_t = np.ones((V, 5))
        bad_t[0, 0] = -0.5
        assert code(lambda: g.set_state(np.ones((D, 5)), bad_t)) == stc.STC_ERR_INVALID_ARG
        with pytest.raises(ValueError):
            g.set_state(np.ones((3, 5)), np.ones((V, 5)))
        g.init_random(1)
        assert code(lambda: g.next(-1)) == stc.STC_ERR_INVALID_ARG
        g.next(1)  # the failed calls left the group usable
        # a member is driven by its group alone
        member, _ = g.members()[1]
        assert g.lib.stc_em_next(member, 1) == stc.STC_ERR_STATE
        assert g.lib.stc_em_init_random(member, 1) == stc.STC_ERR_STATE
        assert g.lib.stc_em_log_likelihood(member, None, None) == stc.STC_ERR_STATE
        assert np.all(np.isfinite(g.state()[1]))
    lib = stc.load()
    assert lib.stc_em_group_next(None, 1) == stc.STC_ERR_INVALID_ARG
    assert lib.stc_em_group_destroy(None) == 0
