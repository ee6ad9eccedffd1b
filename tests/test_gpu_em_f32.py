"""GPU: the EM optimizer with fp32 state storage (stc_em_create_as / stc_em_group_create_as with STC_F32,
csrc/lda_em.hip) against the fp64 handle, bitwise, and against the NumPy restatements (tests/em_oracle.py,
tests/em_f32_oracle.py, tests/em_group_oracle.py).

The contract: an fp32-state handle runs exactly the fp64 handle's iteration on the values it stores and rounds
each new N_dk / N_wk element to the nearest fp32 once, when it is stored.  So on one device, from an fp32-valued
state S, everything an fp32 handle returns is r32 of what the fp64 handle returns — array_equal, no tolerance.

Bounds that are not equalities:
  one step against NumPy      2^-24 + 1e-12: one round-to-nearest on top of the fp64 kernel's own bar
                              (tests/test_gpu_em.py).  Equality with r32(NumPy) is not asked: an element within
                              1e-12 of a rounding midpoint may round the other way under another summation order.
  ten golden iterations       1e-6 against chain32.  A chain32 whose every step is perturbed by 1e-13 relative
                              moves by at most 1.5e-7 after ten iterations (k = 100), and the fp64 kernel sits
                              7e-15 from NumPy per step; fp32 storage itself separates chain32 from the fp64
                              chain by 5.5e-6, so a kernel that also computed in fp32 would not pass.
  a group's N_wk' (M members) (1 + 2^-24)^M − 1 + 1e-12: one rounding per member partial and one per fp32
                              addition, all terms positive.
  a group, ten iterations     4 × the distance of chain32 from the fp64 chain, computed by the test: three
                              members round an N_wk element up to three times where chain32 rounds once.
"""
import ctypes as C
import os

import numpy as np
import pytest

import em_f32_oracle as F
import em_group_oracle as G
import em_oracle as E
from helpers import GOLDEN, planted_corpus, random_corpus

pytestmark = pytest.mark.gpu

REF_MODEL = os.path.join(GOLDEN, "LdaModel_EN_1591049082850")
EPS32 = 2.0 ** -24


def rel_err(got, ref):
    """max elementwise relative error; where the reference is exactly 0 the result must be too"""
    got, ref = np.asarray(got), np.asarray(ref)
    zero = ref == 0.0
    assert np.all(got[zero] == 0.0)
    if zero.all():
        return 0.0
    return float(np.max(np.abs(got[~zero] - ref[~zero]) / np.abs(ref[~zero])))


def make_handle(ctx, corpus, k, dtype):
    import stc

    dev = stc.DeviceCsr.upload(ctx, corpus, stc.STC_F64)
    try:
        return stc.EmHandle(ctx, dev, k, dtype=dtype)  # the handle keeps no reference to the corpus
    finally:
        dev.free()


def random_state(rng, D, V, k):
    return rng.uniform(0.5, 5.0, size=(D, k)), rng.uniform(0.5, 5.0, size=(V, k))


def long_vertex_corpus(rng, D=700, V=4000, long_doc=3000, hot=7):
    """as test_gpu_em.long_vertex_corpus: document 0 holds 3,000 entries (12 chunks of 256 edges), term `hot`
    occurs in all 700 documents (3 chunks), the last chunk of each partly filled"""
    import stc

    rows = []
    cold = np.setdiff1d(np.arange(V), [hot])
    for d in range(D):
        n = long_doc - 1 if d == 0 else int(rng.integers(3, 11))
        ids = np.union1d(rng.choice(cold, size=n, replace=False), [hot]).astype(np.int32)
        rows.append((ids, rng.integers(1, 6, ids.size).astype(np.float64)))
    assert rows[0][0].size == long_doc and all(hot in r[0] for r in rows)
    return stc.CsrMatrix.from_rows(rows, V)


CASES = [("random", k) for k in (2, 5, 64, 65, 100, 257, 1024)] + [("long", k) for k in (5, 100)]
_steps = {}


def one_step(ctx, which, k):
    """one case, computed once and shared by the tests below (nothing in it is modified afterwards): the corpus,
    the injected states, and what an fp64 and an fp32 handle return after set_state and after next(1)"""
    if (which, k) in _steps:
        return _steps[which, k]
    rng = np.random.default_rng((100 if which == "random" else 200) + k)
    corpus = random_corpus(rng, 40, 300) if which == "random" else long_vertex_corpus(rng)
    D, V = corpus.shape
    raw = random_state(rng, D, V, k)
    S = (F.r32(raw[0]), F.r32(raw[1]))
    out = {"corpus": corpus, "raw": raw, "S": S}
    for dtype in ("f64", "f32"):
        h = make_handle(ctx, corpus, k, dtype)
        assert h.dtype == dtype
        h.set_state(*raw)
        out[dtype, "raw"] = h.state()
        h.set_state(*S)
        out[dtype, "set"] = h.state()
        h.next(1)
        out[dtype, "next"] = h.state()
        h.close()
    _steps[which, k] = out
    return out


@pytest.mark.parametrize("which,k", CASES)
def test_one_step_is_the_rounded_fp64_step_bitwise(ctx, which, k):
    c = one_step(ctx, which, k)
    src, term, _ = E.edges_of(c["corpus"])
    # injection: the mask, then one rounding; an fp32-valued state is stored as it is
    masked = E.mask_state(*c["raw"], src, term)
    assert np.array_equal(c["f32", "raw"][0], F.r32(masked[0])) and np.array_equal(c["f32", "raw"][1], F.r32(masked[1]))
    assert np.array_equal(c["f64", "raw"][0], masked[0]) and np.array_equal(c["f64", "raw"][1], masked[1])
    assert not np.array_equal(masked[1], F.r32(masked[1]))  # the raw state was not fp32-valued
    ms = E.mask_state(*c["S"], src, term)
    for dtype in ("f64", "f32"):
        got = c[dtype, "set"]
        assert np.array_equal(got[0], ms[0]) and np.array_equal(got[1], ms[1])
    assert np.array_equal(c["f32", "set"][2], c["f64", "set"][2])  # the same fp64 column sum of the same values
    a, b = c["f64", "next"], c["f32", "next"]
    assert np.array_equal(b[0], F.r32(a[0]))
    assert np.array_equal(b[1], F.r32(a[1]))
    assert not np.array_equal(a[1], F.r32(a[1]))  # the fp64 step's result is not fp32-valued: the rounding happened
    for st in (c["f32", "raw"], c["f32", "set"], b):
        assert np.array_equal(st[0], F.r32(st[0])) and np.array_equal(st[1], F.r32(st[1]))
        assert rel_err(st[2], st[1].sum(axis=0)) <= 1e-12  # N_k over the stored values


@pytest.mark.parametrize("which,k", CASES)
def test_one_step_against_the_restatement(ctx, which, k):
    c = one_step(ctx, which, k)
    src, term, cnt = E.edges_of(c["corpus"])
    alpha, eta = E.resolve(k)
    rd, rw = E.mask_state(*c["S"], src, term)
    ref = E.step(rd, rw, rw.sum(axis=0), src, term, cnt, alpha, eta)
    errs = [rel_err(g, r) for g, r in zip(c["f32", "next"], ref)]
    print(f"{which} k={k}: fp32 state against the fp64 restatement N_dk {errs[0]:.3g} N_wk {errs[1]:.3g} N_k {errs[2]:.3g}")
    assert max(errs) <= EPS32 + 1e-12, errs


@pytest.fixture(scope="module")
def golden():
    import stc

    m = stc.io.load_distributed(REF_MODEL)
    src, term, cnt = E.edges_of_model(m)
    indptr = np.zeros(m["doc_ids"].size + 1, np.int64)
    np.cumsum(np.bincount(src, minlength=m["doc_ids"].size), out=indptr[1:])
    return src, term, cnt, stc.CsrMatrix(indptr, term, cnt, m["vocab_size"])


@pytest.mark.parametrize("k", [5, 100])
def test_ten_iterations_on_the_golden_graph(ctx, golden, k):
    src, term, cnt, corpus = golden
    rng = np.random.default_rng(400 + k)
    alpha, eta = E.resolve(k)
    ndk0, nwk0 = random_state(rng, corpus.num_rows, corpus.num_cols, k)
    h = make_handle(ctx, corpus, k, "f32")
    h.set_state(ndk0, nwk0)
    h.next(10)
    got = h.state()
    h.close()
    ref32 = F.chain32(ndk0, nwk0, src, term, cnt, alpha, eta, 10)  # every vertex of the golden graph has an edge
    # the fp64 chain, for the printed distance only: the fp64 handle's, which tests/test_gpu_em.py holds to 1e-9 of
    # NumPy's (measured 3.4e-12) — a second NumPy chain would double this test's time
    h = make_handle(ctx, corpus, k, "f64")
    h.set_state(ndk0, nwk0)
    h.next(10)
    ref64 = h.state()
    h.close()
    e32 = [rel_err(g, r) for g, r in zip(got, ref32)]
    e64 = [rel_err(g, r) for g, r in zip(got, ref64)]
    print(f"golden graph, k={k}, 10 iterations, fp32 state: against chain32 N_dk {e32[0]:.3g} N_wk {e32[1]:.3g} "
          f"N_k {e32[2]:.3g}; against the fp64 chain N_dk {e64[0]:.3g} N_wk {e64[1]:.3g} N_k {e64[2]:.3g}")
    assert max(e32) <= 1e-6, e32


@pytest.mark.parametrize("k", [5, 100])
def test_init_random_is_the_rounded_fp64_one(ctx, k):
    rng = np.random.default_rng(600 + k)
    corpus = random_corpus(rng, 40, 300)
    st = {}
    for dtype in ("f64", "f32"):
        h = make_handle(ctx, corpus, k, dtype)
        h.init_random(12345)
        st[dtype] = h.state()
        h.close()
    assert np.array_equal(st["f32"][0], F.r32(st["f64"][0])) and np.array_equal(st["f32"][1], F.r32(st["f64"][1]))
    assert not np.array_equal(st["f64"][1], F.r32(st["f64"][1]))
    assert rel_err(st["f32"][2], st["f32"][1].sum(axis=0)) <= 1e-12


@pytest.mark.parametrize("k", [5, 100])
def test_scores_and_labels_are_the_fp64_handles_bitwise(ctx, k):
    rng = np.random.default_rng(800 + k)
    corpus = long_vertex_corpus(rng)
    src, term, cnt = E.edges_of(corpus)
    alpha, eta = E.resolve(k)
    S = [F.r32(x) for x in random_state(rng, *corpus.shape, k)]
    h32 = make_handle(ctx, corpus, k, "f32")
    h32.set_state(*S)
    h32.next(3)
    state = h32.state()
    h64 = make_handle(ctx, corpus, k, "f64")
    h64.set_state(*state[:2])
    assert all(np.array_equal(a, b) for a, b in zip(h64.state(), state))
    ll32, ll64 = h32.log_likelihood(), h64.log_likelihood()
    ta32, ta64 = h32.topic_assignments(), h64.topic_assignments()
    h32.close()
    h64.close()
    assert ll32[0] == ll64[0] and ll32[1] == ll64[1], (ll32, ll64)
    assert all(np.array_equal(a, b) for a, b in zip(ta32, ta64))
    assert ta32[2].size == src.size and len(np.unique(ta32[2])) > 1
    ref_ll = E.log_likelihood(*state, src, term, cnt, alpha, eta)
    ref_lp = E.log_prior(*state, src, term, alpha, eta)
    print(f"k={k}: logLikelihood {ll32[0]!r} (restated {ref_ll!r}), logPrior {ll32[1]!r} (restated {ref_lp!r})")
    assert abs(ll32[0] - ref_ll) <= 1e-12 * abs(ref_ll)
    assert abs(ll32[1] - ref_lp) <= 1e-12 * abs(ref_lp)


@pytest.mark.parametrize("k", [5, 100])
def test_two_fp32_handles_are_bitwise_equal(ctx, k):
    rng = np.random.default_rng(700 + k)
    corpus = long_vertex_corpus(rng)
    out = []
    for _ in range(2):
        h = make_handle(ctx, corpus, k, "f32")
        h.init_random(77)
        h.next(5)
        out.append(h.state() + h.log_likelihood())
        h.close()
    assert all(np.array_equal(x, y) for x, y in zip(out[0], out[1]))


def test_create_as_f64_is_create(ctx):
    import stc

    k = 100
    rng = np.random.default_rng(750)
    corpus = long_vertex_corpus(rng)
    state = random_state(rng, *corpus.shape, k)
    dev = stc.DeviceCsr.upload(ctx, corpus, stc.STC_F64)
    lib, out = ctx.lib, []
    for create in (lambda h: lib.stc_em_create(ctx.handle, dev.handle, k, -1.0, -1.0, C.byref(h)),
                   lambda h: lib.stc_em_create_as(ctx.handle, dev.handle, k, -1.0, -1.0, stc.STC_F64, C.byref(h))):
        raw = C.c_void_p()
        assert create(raw) == 0
        t = C.c_int32(-1)
        assert lib.stc_em_state_dtype(raw, C.byref(t)) == 0 and t.value == stc.STC_F64
        h = stc.EmHandle.__new__(stc.EmHandle)  # the class's readers over a handle made through the C ABI
        h.ctx, h.handle, h.k, h.num_docs, h.vocab_size, h.num_edges = ctx, raw, k, *corpus.shape, corpus.values.size
        h.set_state(*state)
        h.next(3)
        out.append(h.state() + h.log_likelihood())
        h.close()
    dev.free()
    assert all(np.array_equal(x, y) for x, y in zip(out[0], out[1]))


def member_replica(g, i):
    """(N_wk, N_k) of member i, read through stc_em_group_member + stc_em_get_state"""
    h, _ = g.members()[i]
    tt = np.zeros((g.vocab_size, g.k))
    nk = np.zeros(g.k)
    assert g.lib.stc_em_get_state(h, None, tt.ctypes.data_as(C.POINTER(C.c_double)),
                                  nk.ctypes.data_as(C.POINTER(C.c_double)), None, None) == 0
    return tt, nk


@pytest.mark.parametrize("k", [5, 100])
def test_group_members_on_one_device(ctx, k):
    import stc

    M = 3
    rng = np.random.default_rng(900 + k)
    corpus = random_corpus(rng, 60, 400)
    D, V = corpus.shape
    src, term, cnt = E.edges_of(corpus)
    alpha, eta = E.resolve(k)
    S = [F.r32(x) for x in random_state(rng, D, V, k)]
    rd, rw = E.mask_state(*S, src, term)
    with stc.EmGroup([0] * M, corpus, k, dtype="f32") as g:
        assert g.dtype == "f32" and g.transport() == "in-process"
        g.set_state(*S)
        g.next(1)
        got = g.state()
        reps = [member_replica(g, i) for i in range(M)]
    for tt, nk in reps:
        assert np.array_equal(tt, reps[0][0]) and np.array_equal(nk, reps[0][1])
    assert np.array_equal(got[1], reps[0][0]) and np.array_equal(got[2], reps[0][1])
    h = make_handle(ctx, corpus, k, "f32")
    h.set_state(*S)
    h.next(1)
    single = h.state()
    h.close()
    assert np.array_equal(got[0], single[0])  # a document lies in one shard: the same sums, the same rounding
    ref = G.step(corpus, M, rd, rw, rw.sum(axis=0), alpha, eta)
    err = rel_err(got[1], ref[1])
    print(f"{M} fp32 members, k={k}: N_wk' against the sharded restatement {err:.3g} "
          f"(bound {(1 + EPS32) ** M - 1 + 1e-12:.3g}), against the single fp32 handle {rel_err(got[1], single[1]):.3g}")
    assert err <= (1.0 + EPS32) ** M - 1.0 + 1e-12
    assert np.array_equal(got[1], F.r32(got[1])) and rel_err(got[2], got[1].sum(axis=0)) <= 1e-12
    # one member: no collective, the single fp32 handle's numbers
    with stc.EmGroup([0], corpus, k, dtype="f32") as g:
        assert g.transport() == "none" and g.dtype == "f32"
        g.init_random(5)
        g.next(3)
        one = g.state() + g.log_likelihood()
    h = make_handle(ctx, corpus, k, "f32")
    h.init_random(5)
    h.next(3)
    single = h.state() + h.log_likelihood()
    h.close()
    assert all(np.array_equal(x, y) for x, y in zip(one, single))


def check_group_ten_iterations(devices):
    import stc

    k = 5
    rng = np.random.default_rng(950)
    corpus = random_corpus(rng, 60, 400)
    src, term, cnt = E.edges_of(corpus)
    alpha, eta = E.resolve(k)
    ndk0, nwk0 = E.mask_state(*random_state(rng, *corpus.shape, k), src, term)
    ref64 = E.iterate(ndk0, nwk0, src, term, cnt, alpha, eta, 10)
    ref32 = F.chain32(ndk0, nwk0, src, term, cnt, alpha, eta, 10)
    d_ref = max(rel_err(a, b) for a, b in zip(ref32, ref64))
    with stc.EmGroup(devices, corpus, k, dtype="f32") as g:
        g.set_state(ndk0, nwk0)
        g.next(10)
        got = g.state()
        transport = g.transport()
    d = max(rel_err(a, b) for a, b in zip(got, ref64))
    print(f"fp32 group, devices {devices} ({transport}), k={k}, 10 iterations: {d:.3g} from the fp64 chain; "
          f"chain32 is {d_ref:.3g} from it (bound 4x = {4 * d_ref:.3g})")
    assert d_ref > 0.0 and d <= 4.0 * d_ref


def test_group_ten_iterations(ctx):
    check_group_ten_iterations([0, 0, 0])


def test_group_two_real_devices(ctx):
    import stc

    if stc.Context.device_count() < 2:
        pytest.skip("needs two devices")
    check_group_ten_iterations([0, 1])


@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_python_surface(ctx, tmp_path, devices):
    import stc

    rng = np.random.default_rng(7)
    D, V, k = 60, 200, 5
    corpus, _ = planted_corpus(rng, D, V, k)
    lda = stc.MllibLDA(ctx, devices=devices).setOptimizer("em").setK(k).setMaxIterations(5).setSeed(3)
    lda.dtype = "f32"
    model = lda.run(corpus)
    assert isinstance(model, stc.DistributedLDAModel) and len(lda.iterationTimes) == 5
    tm = model.topicsMatrix()
    assert np.array_equal(tm, F.r32(tm)) and np.all(tm >= 0.0) and tm.sum() > 0.0
    lda64 = stc.MllibLDA(ctx, devices=devices).setOptimizer("em").setK(k).setMaxIterations(5).setSeed(3)
    tm64 = lda64.run(corpus).topicsMatrix()
    assert not np.array_equal(tm64, F.r32(tm64))  # the default stays fp64: the rounding above came from dtype
    ll = model.logLikelihood() if devices else model.logLikelihood(ctx)
    path = str(tmp_path / "em_f32_model")
    model.save(path)
    loaded = stc.DistributedLDAModel.load(path)
    assert np.array_equal(loaded.topicsMatrix(), tm)
    assert abs(loaded.logLikelihood(ctx) - ll) <= 1e-12 * abs(ll)  # a loaded model rebuilds an fp64 handle


def test_dtype_attributes_and_error_codes(ctx):
    import stc

    corpus = random_corpus(np.random.default_rng(9), 10, 50)
    dev = stc.DeviceCsr.upload(ctx, corpus, stc.STC_F64)
    for dtype in ("f32", "f64"):
        h = stc.EmHandle(ctx, dev, 5, dtype=dtype)
        assert h.dtype == dtype
        h.close()
        with stc.EmGroup([0, 0], corpus, 5, dtype=dtype) as g:
            assert g.dtype == dtype
            for m, _ in g.members():  # stc_em_state_dtype serves a member
                t = C.c_int32(-1)
                assert g.lib.stc_em_state_dtype(m, C.byref(t)) == 0 and t.value == getattr(stc, "STC_" + dtype.upper())
    lib = ctx.lib
    devs = np.zeros(2, np.int32)
    ip, ix = np.ascontiguousarray(corpus.indptr, np.int64), np.ascontiguousarray(corpus.indices, np.int32)
    vs = np.ascontiguousarray(corpus.values, np.float64)
    for bad in (stc.STC_MIXED, -1, 7):
        raw = C.c_void_p()
        assert lib.stc_em_create_as(ctx.handle, dev.handle, 5, -1.0, -1.0, bad, C.byref(raw)) == stc.STC_ERR_INVALID_ARG
        assert not raw.value
        assert lib.stc_em_group_create_as(
            devs.ctypes.data_as(C.POINTER(C.c_int32)), 2, corpus.num_rows, corpus.num_cols,
            ip.ctypes.data_as(C.POINTER(C.c_int64)), ix.ctypes.data_as(C.POINTER(C.c_int32)),
            vs.ctypes.data_as(C.POINTER(C.c_double)), 5, -1.0, -1.0, bad, C.byref(raw)) == stc.STC_ERR_INVALID_ARG
        assert not raw.value
    # the corpus stays fp64: an fp32 one is refused whatever the state dtype
    f32 = stc.DeviceCsr.upload(ctx, corpus, stc.STC_F32)
    with pytest.raises(stc.StcError) as e:
        stc.EmHandle(ctx, f32, 5, dtype="f32")
    assert e.value.code == stc.STC_ERR_INVALID_ARG
    f32.free()
    dev.free()
