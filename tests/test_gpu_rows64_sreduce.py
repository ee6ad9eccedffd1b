"""The fp64 rows E-step's s reduction (lda_rows64.hip Phase B) at every lane map and row-set count.

Each wave sums its eight row lanes' s partials and one lane per topic stores the wave's sum; which lanes
hold which topics depends on k (KL = 4 / 7 / 13 topics per topic lane, one or two ψ waves, idle reducer
lanes past 8·KL) and which rows exist on the row-set count R = ⌈nnz/32⌉ (1..6 in the common kernel, the
sixth set from LDS; 7..8 in the long-document launch).  One document per nnz at every R and its edges,
against the oracle per document with the bounds of test_gpu_lda.test_estep_gamma_and_stat; then the
resident grid under next() against the oracle's replay.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

V = 2048
# every row-set count and its edges; 161: only wave 0 has a row in set 5; 192: the LDS row set full;
# 193..256: the 7- and 8-set launch; 0: an empty document
NNZ = [1, 8, 31, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 168, 169, 192, 193, 224, 225, 256, 0]
# 104: KT full, two ψ waves; 100: the headline's four pad topics; 66: kp > 64 with the top topic lane
# nearly empty; 64: one ψ wave at KL = 13; 56: KL = 7, reducer lanes 56-63 idle; 33: KL = 7; 32: KL = 4;
# 7: odd k, kp = 8
KS = [104, 100, 66, 64, 56, 33, 32, 7]


def _corpus(rng):
    import stc

    rows = []
    for n in NNZ:
        ids = np.sort(rng.choice(V, size=n, replace=False)).astype(np.int32)
        rows.append((ids, rng.integers(1, 7, n).astype(np.float64)))
    return stc.CsrMatrix.from_rows(rows, V)


def _handle(ctx, corpus, k, lam=None, **kw):
    import stc

    h = stc.LdaHandle(ctx, k, corpus.num_cols, dtype="f64", **kw)
    d = stc.DeviceCsr.upload(ctx, corpus, stc.STC_F64)
    h.set_corpus(d, corpus.num_rows)
    if lam is not None:
        h.set_topics(lam)
    return h, d


@pytest.mark.parametrize("k", KS)
def test_estep_every_row_set_count(ctx, oracle, k):
    rng = np.random.default_rng(700 + k)
    corpus = _corpus(rng)
    D = corpus.num_rows
    lam = rng.gamma(100.0, 0.01, size=(V, k))
    g0 = rng.gamma(100.0, 0.01, size=(D, k))
    h, _ = _handle(ctx, corpus, k, lam)
    ids = np.arange(D)
    gamma, stat, iters = h.estep(ids, g0, want_stat=True)
    eeb = oracle.topics_exp_elog_beta(lam)
    alpha = np.full(k, 1.0 / k)
    stat_o = np.zeros((V, k))
    borderline = 0
    for i in ids:
        cid, cts = corpus.row(i)
        if cid.size == 0:
            assert np.all(gamma[i] == 0) and iters[i] == 0
            continue
        g, ss, it = oracle.variational_topic_inference(cid, cts, eeb, alpha, g0[i])
        if iters[i] != it:
            # a document on the stop rule's boundary (summation order decides): at most one per case, one
            # iteration apart, compared with the oracle run to the same iteration
            assert abs(int(iters[i]) - it) <= 1, (i, iters[i], it)
            borderline += 1
            assert borderline <= 1, (i, iters[i], it)
            g, ss, _ = oracle.variational_topic_inference(cid, cts, eeb, alpha, g0[i], n_iter=int(iters[i]))
        np.testing.assert_allclose(gamma[i], g, rtol=1e-7, err_msg=f"nnz {cid.size}")
        np.add.at(stat_o, cid, ss.T)
    nz = stat_o > 1e-8 * stat_o.max()
    rel = np.abs(stat[nz] - stat_o[nz]) / stat_o[nz]
    assert rel.max() < 1e-7, rel.max()
    assert np.abs(stat - stat_o).sum() / stat_o.sum() < 1e-10
    assert np.all(stat[~nz] < 1e-6 * stat_o.max() + 1e-300)


def test_next_on_the_resident_grid_matches_oracle(ctx, oracle):
    """Two next() steps at k = 100 (device-sampled members, counter-RNG γ₀, the ticket-walking grid and the
    long-document launch) replayed by the oracle on the same members: λ and α to 1e-9."""
    from helpers import random_corpus

    rng = np.random.default_rng(733)
    D, k, f, seed = 400, 100, 0.5, 91
    corpus = random_corpus(rng, D, V, 1, 256, empty_every=29)
    h, _ = _handle(ctx, corpus, k, None, mini_batch_fraction=f, seed=seed, sample_with_replacement=False,
                   optimize_doc_concentration=True)
    h.init_random(seed)
    lam0 = oracle.init_lambda(seed, V, k)
    alpha, eta = oracle.resolve_alpha_eta(k)
    state = oracle.OnlineLDAState(lam=lam0.T.copy(), alpha=alpha, eta=eta, corpus_size=D,
                                  mini_batch_fraction=f, optimize_doc_concentration=True)
    for draw in (1, 2):
        members = oracle.sample_members(seed, draw, 0, D, f, False)
        assert members, draw
        st = h.next()
        assert st["batch_docs"] == len(members), (draw, st["batch_docs"], len(members))
        it = state.iteration + 1
        g0 = [oracle.gamma_init(seed, oracle.train_doc_key(it, 0, pos), k) for pos in range(len(members))]
        oracle.submit_minibatch(state, [corpus.row(d) for d in members], g0)
    np.testing.assert_allclose(h.topics(), state.lam.T, rtol=1e-9)
    np.testing.assert_allclose(h.alpha(), state.alpha, rtol=1e-9)
