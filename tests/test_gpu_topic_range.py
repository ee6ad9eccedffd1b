"""Training steps vs the oracle at every kernel width from k = 2 to the limit k = 4096 (both dtypes).

stc_lda_create takes 2 ≤ k ≤ 4096, and a training step dispatches on k (kp: k rounded up to 2 in fp64, to 4 in
fp32) into one instantiation per stage:
  λ update + expElogβ' rows   k_lambda_eeb Q = 1, 2, 4 (kp ≤ 64, 128, 256), k_lambda_eeb_wide Q = 2, 4, 8, 16
                              (kp ≤ 512, 1024, 2048, 4096)                                   lda_mstep.hip
  sufficient statistics       Q = 1, 2, 4 (kp ≤ 64, 128, 256), then slabs of 256 (fp64) / 512 (fp32) columns,
                              up to 16 of them                                               lda_sstats.hip
  E-step                      fp64 rows64 k ≤ 104 / fp32 grid k ≤ 128, the many-topic kernel to k = 2048 (Q = 1, 2,
                              4), the workgroup kernel k_estep for every document beyond     lda_dispatch.hip
  α Newton step, logphat      one pass per thread to k = 256, strided loops beyond
K has a value on each side of every one of those widths in both paddings (tests/test_topic_range_tables.py reads
the widths from the sources and checks that), the minimum, an odd k with a padding column, the headline k = 100
and the limit.  One tiny shape serves every case: V = 200 (three full 64-row M-step blocks and a ragged one of 8
rows), 40 documents of 1–40 terms, every 13th empty, 24 batch members per step drawn with duplicates.  Every handle
is made with STC_WIDE_TEAM=1, so the E-step is a one-CU kernel at every k and nothing depends on co-residency (the
team kernels have their own tests).

The oracle is run to the kernel's own iteration counts (and once with its own stop rule: the counts may differ
by one for at most one document per case in fp64, by three in fp32 — test_estep_gamma_and_stat's rule), so a
document on the stop rule's boundary costs nothing and a kernel stopping at the wrong iterate is still caught.
Bars: TOL and the stat criteria of tests/test_gpu_lda.py, unchanged.

What the sweep found.  fp32, k = 1024, 1025, 2048 (and the sliced runs at 1000 and 2000): a document of a few
tokens lost all its mass on the many-topic kernel — γ = α after the second iteration, the bound NaN, at k = 2048 a
document running to the iteration cap.  k_estep_wide shifts eθ by ψ(Σγ); a 4-token document at k = 1024 has every
γ_t ≈ 5/k, ψ(γ_t) ≈ −205, and exp flushes to zero in fp32 for all topics at once (fp64, and Spark, are still at
e^{−205}).  The fp32 kernel now shifts such a document's eθ by ψ(max γ) and carries the shift in Spark's 1e-100, so
it also follows Spark where that epsilon empties a document (4 tokens at k = 2048).  The launches at the limit —
k_estep's 98,432 B of LDS at fp64 k = 4096, k_update_alpha's 64 KiB — ran as written; both sizes are now
registered for their kernels.

MEASURED (MI355X), worst over the three steps per case; every width passes the bars as written:
  k      f64 λ     f64 α     f64 stat l1 / rel        f32 λ     f32 α     f32 stat l1 / rel
  2      2.2e-14   1.1e-16   5.0e-15 / 1.5e-13        3.3e-06   6.5e-08   1.6e-06 / 1.6e-05
  3      5.9e-14   3.6e-16   2.7e-14 / 1.1e-12        1.2e-06   1.7e-07   9.9e-07 / 2.5e-04
  64     1.3e-14   0         5.7e-15 / 9.1e-14        5.8e-07   1.5e-09   3.4e-07 / 8.0e-06
  65     2.7e-14   1.1e-16   1.3e-14 / 1.8e-13        7.7e-07   1.8e-09   3.7e-07 / 4.9e-06
  100    7.1e-14   1.7e-16   1.7e-14 / 8.4e-13        2.7e-06   2.0e-09   6.8e-07 / 3.2e-05
  128    1.9e-14   1.1e-16   1.1e-14 / 1.4e-13        4.3e-06   4.3e-09   9.4e-07 / 4.5e-05
  129    1.2e-14   1.1e-16   1.1e-14 / 8.5e-14        6.8e-07   1.6e-09   5.3e-07 / 6.8e-06
  256    2.0e-14   1.8e-14   1.5e-14 / 1.9e-13        3.7e-06   1.3e-06   1.6e-06 / 2.7e-05
  257    2.1e-14   1.7e-15   9.6e-15 / 1.9e-13        4.4e-06   4.6e-07   1.4e-06 / 3.9e-05
  512    1.3e-13   1.6e-14   7.6e-14 / 1.6e-12        4.2e-06   4.6e-06   4.8e-06 / 5.6e-05
  513    2.9e-14   5.7e-14   3.1e-14 / 3.2e-13        4.2e-06   1.6e-05   2.0e-06 / 9.4e-05
  1024   7.0e-14   2.2e-16   2.8e-14 / 1.3e-11        1.6e-05   1.3e-07   6.6e-06 / 8.4e-03
  1025   5.6e-14   1.6e-14   3.1e-14 / 3.7e-11        1.4e-05   6.8e-07   8.6e-06 / 1.3e-03
  2048   4.7e-14   6.1e-15   3.1e-14 / 1.1e-11        8.8e-06   1.9e-06   4.3e-06 / 1.8e-03
  2049   6.3e-15   2.7e-15   1.2e-14 / 1.9e-11        2.8e-06   1.2e-06   3.3e-06 / 7.7e-04
  4095   1.4e-14   3.6e-15   1.8e-14 / 6.1e-12        4.2e-06   2.1e-06   5.4e-06 / 2.5e-04
  4096   8.0e-15   1.8e-15   1.9e-14 / 9.6e-12        1.9e-06   1.7e-07   3.6e-06 / 5.5e-04
  fp64 E-step at the LDS edge, stat l1 / rel: k = 3406 2.5e-14 / 6.1e-12, 3408 2.3e-14 / 9.0e-12, 3410 2.1e-14 / 3.8e-12
  (bars: λ and α 1e-9 / 1e-4, stat l1 1e-10 / 1e-4, stat rel 1e-7 / 1e-2).  The file takes about 21 s.
"""
import numpy as np
import pytest

from helpers import random_corpus
from test_gpu_lda import TOL

pytestmark = pytest.mark.gpu

V, D, BATCH, STEPS, FRAC = 200, 40, 24, 3, 0.4
K = (2, 3, 64, 65, 100, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4095, 4096)
SLICED_K = (100, 200, 1000, 2000, 4096)
# fp64 k_estep: 24·kp + 128 bytes of fixed LDS arrays reach kLdsBudget = 80 KiB at kp = 3408 and pass it at 3410
LDS_EDGE_K = (3406, 3408, 3410)
DESCRIBE_K = (2, 100, 4096)
TEAM_FAMILIES = ("k_estep_wide_mc", "k_estep_wide_tc", "k_estep_tgrid64", "team_fallback")

_CORPUS = {}
_RUNS = {}  # (dtype, k) -> (λ, α, bound) of the unsliced three-step run


def _corpus():
    if not _CORPUS:
        c = random_corpus(np.random.default_rng(2024), D, V, 1, 40, empty_every=13)
        _CORPUS["c"] = c
        _CORPUS["rows"] = [c.row(i) for i in range(D)]
        assert sum(ids.size == 0 for ids, _ in _CORPUS["rows"]) == 3 and np.diff(c.indptr).max() == 40
    return _CORPUS["c"], _CORPUS["rows"]


def _inputs(k):
    """λ₀, the three batches (member ids with duplicates, γ₀ per member) and γ₀ of every document for the bound"""
    rng = np.random.default_rng(9000 + k)
    lam0 = rng.gamma(100.0, 0.01, size=(V, k))
    batches = []
    for _ in range(STEPS):
        ids = np.sort(rng.choice(D, size=BATCH, replace=True))
        assert np.unique(ids).size < BATCH  # drawn with duplicates
        batches.append((ids, rng.gamma(100.0, 0.01, size=(BATCH, k))))
    return lam0, batches, rng.gamma(100.0, 0.01, size=(D, k))


def _handle(ctx, k, dtype, lam0):
    import stc

    corpus, _ = _corpus()
    h = stc.LdaHandle(ctx, k, V, dtype=dtype, mini_batch_fraction=FRAC, optimize_doc_concentration=True)
    d = stc.DeviceCsr.upload(ctx, corpus, stc.STC_F32 if dtype == "f32" else stc.STC_F64)
    h.set_corpus(d, D)
    h.set_topics(lam0)
    return h, d


def _close(h, d):
    h.close()
    d.free()


def _check_estep(O, dtype, k, ids, g0, eeb, alpha, gamma, stat, iters, border):
    """One estep(want_stat=True) call by test_estep_gamma_and_stat's criteria.  Returns the oracle's γ per member
    (None: empty document) and stat, both at the kernel's iteration counts, and the stat errors."""
    _, rows = _corpus()
    stat_o = np.zeros((V, k))
    gam_o = []
    for i, doc in enumerate(ids):
        cid, cts = rows[doc]
        if cid.size == 0:
            assert np.all(gamma[i] == 0) and iters[i] == 0
            gam_o.append(None)
            continue
        g, ss, it = O.variational_topic_inference(cid, cts, eeb, alpha, g0[i])
        if iters[i] != it:
            assert abs(int(iters[i]) - it) <= (1 if dtype == "f64" else 3), (i, iters[i], it)
            if dtype == "f64":
                border.append((i, int(iters[i]), it))
                assert len(border) <= 1, border
            g, ss, _ = O.variational_topic_inference(cid, cts, eeb, alpha, g0[i], n_iter=int(iters[i]))
        if dtype == "f64":
            np.testing.assert_allclose(gamma[i], g, rtol=TOL[dtype]["gamma"])
        else:
            l1 = np.abs(gamma[i] - g).sum()
            assert l1 <= 1e-3 * k + 1e-4 * g.sum(), (i, l1, g.sum())
            big = g >= 1.0
            np.testing.assert_allclose(gamma[i][big], g[big], rtol=TOL[dtype]["gamma"])
        np.add.at(stat_o, cid, ss.T)
        gam_o.append(g)
    absent = np.setdiff1d(np.arange(V), np.concatenate([rows[doc][0] for doc in ids]))
    assert absent.size > 0 and np.all(stat[absent] == 0.0)  # rows of terms outside the batch: exactly zero
    nz = stat_o > (1e-8 if dtype == "f64" else 1e-4) * stat_o.max()
    rel = np.abs(stat[nz] - stat_o[nz]) / stat_o[nz]
    l1 = np.abs(stat - stat_o).sum() / stat_o.sum()
    if dtype == "f64":
        assert rel.max() < TOL[dtype]["gamma"], rel.max()
        assert l1 < 1e-10, l1
        assert np.all(stat[~nz] < 1e-6 * stat_o.max() + 1e-300)
    else:
        assert l1 < 1e-4, l1
        assert rel.max() < 1e-2, rel.max()
    return gam_o, stat_o, l1, rel.max()


def _check_kernels(h, k):
    kernels = h.counters()["kernels"]
    if k > 2048:  # past wide_row_cap no document is "short": every launch is the workgroup kernel
        assert kernels["k_estep"] > 0 and all(n == 0 for f, n in kernels.items() if f != "k_estep"), kernels
    else:
        assert kernels["k_estep"] == 0 and all(kernels[f] == 0 for f in TEAM_FAMILIES), kernels
        assert sum(kernels.values()) > 0, kernels


def _device_run(ctx, k, dtype, with_estep=True):
    """the three steps on the device alone: (λ, α, bound)"""
    lam0, batches, g0_all = _inputs(k)
    h, d = _handle(ctx, k, dtype, lam0)
    for ids, g0 in batches:
        if with_estep:
            h.estep(ids, g0, want_stat=True)
        h.step(ids, g0, stats=False)
    out = (h.topics(), h.alpha(), h.bound(d, gamma0=g0_all)["bound"])
    _close(h, d)
    return out


@pytest.mark.parametrize("k", K)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_steps_match_oracle_at_every_width(ctx, oracle, monkeypatch, dtype, k):
    """(a) three submitMiniBatch steps with fresh batches: after each, γ and stat of the E-step, λ and α of the
    step against the oracle rebuilt at the kernel's iteration counts; after the third, describeTopics, the
    bound's topics part (of the device's own λ: fp32 λ is 1e-4 from the oracle's, the part is fp64 on every
    path) and which E-step kernels ran.  The same steps without the estep() calls between them — estep() clears
    stat, so only then do the rows an earlier step wrote hold stale sums, which the M-step must read as zero
    (stamp ≠ sid) — give the same λ and α bit for bit."""
    monkeypatch.setenv("STC_WIDE_TEAM", "1")
    O = oracle
    _, rows = _corpus()
    lam0, batches, g0_all = _inputs(k)
    h, d = _handle(ctx, k, dtype, lam0)
    alpha, eta = O.resolve_alpha_eta(k)
    st = O.OnlineLDAState(lam=lam0.T.copy(), alpha=alpha, eta=eta, corpus_size=D, mini_batch_fraction=FRAC,
                          optimize_doc_concentration=True)
    border = []
    worst = dict(lam=0.0, alpha=0.0, stat_l1=0.0, stat_rel=0.0)
    for step, (ids, g0) in enumerate(batches):
        gamma, stat, iters = h.estep(ids, g0, want_stat=True)
        s = h.step(ids, g0)
        eeb = O.topics_exp_elog_beta(st.lam.T)
        gam_o, stat_o, l1, rel = _check_estep(O, dtype, k, ids, g0, eeb, st.alpha, gamma, stat, iters, border)
        worst["stat_l1"], worst["stat_rel"] = max(worst["stat_l1"], l1), max(worst["stat_rel"], rel)
        live = [g for g in gam_o if g is not None]
        assert s["batch_docs"] == BATCH and s["nonempty_docs"] == len(live) > 0
        # the oracle's submitMiniBatch from those γ / stat: iteration += 1, updateLambda, updateAlpha
        st.iteration += 1
        assert abs(s["rho"] - st.rho()) < 1e-15
        alpha_before = st.alpha.copy()
        dev_alpha_before = alpha_before if step == 0 else dev_alpha
        logphat = np.sum([O.dirichlet_expectation(g) for g in live], axis=0)
        O.update_lambda(st, stat_o.T * eeb.T, int(np.ceil(FRAC * D)))
        O.update_alpha(st, logphat / len(live), len(live))
        assert not np.array_equal(st.alpha, alpha_before)  # the Newton step is accepted with this input
        lam, dev_alpha = h.topics(), h.alpha()
        assert not np.array_equal(dev_alpha, dev_alpha_before)
        e_lam = np.max(np.abs(lam - st.lam.T) / st.lam.T)
        e_alpha = np.max(np.abs(dev_alpha - st.alpha) / st.alpha)
        worst["lam"], worst["alpha"] = max(worst["lam"], e_lam), max(worst["alpha"], e_alpha)
        print(f"step {step + 1}: lam {e_lam:.3e} alpha {e_alpha:.3e} stat l1 {l1:.3e} rel {rel:.3e} "
              f"iters {int(iters.min())}..{int(iters.max())} border {border}")
        assert e_lam < TOL[dtype]["lam"], (step, e_lam)
        np.testing.assert_allclose(dev_alpha, st.alpha, rtol=TOL[dtype]["lam"])
    print(f"MEASURED {dtype} k={k}: lam {worst['lam']:.3e} alpha {worst['alpha']:.3e} "
          f"stat l1 {worst['stat_l1']:.3e} rel {worst['stat_rel']:.3e}")
    assert h.iteration() == STEPS
    idx, w = h.describe(10)
    idx_o, w_o = O.describe_topics(st.lam.T, 10)
    if dtype == "f64":
        assert np.array_equal(idx, idx_o)
    np.testing.assert_allclose(np.sort(w, axis=1), np.sort(w_o, axis=1), rtol=TOL[dtype]["lam"])
    b = h.bound(d, gamma0=g0_all)
    tp_o = O.topics_bound(lam, eta)
    assert abs(b["topics_part"] - tp_o) / abs(tp_o) < 1e-10, (b["topics_part"], tp_o)
    _check_kernels(h, k)
    _RUNS[dtype, k] = (lam, dev_alpha, b["bound"])
    _close(h, d)
    lam2, alpha2, _ = _device_run(ctx, k, dtype, with_estep=False)
    np.testing.assert_array_equal(lam2, lam)
    np.testing.assert_array_equal(alpha2, dev_alpha)


@pytest.mark.parametrize("k", SLICED_K)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_sliced_mstep_bit_identical_at_every_width(ctx, monkeypatch, dtype, k):
    """(b) the same steps with the M-step over three vocabulary slices of 128 rows (V = 200: one ragged, one
    past V): λ, α and the bound bit for bit those of the unsliced run (test_sharded_mstep_slices_bit_identical's
    assertion at the remaining λ-update instantiations)."""
    monkeypatch.setenv("STC_WIDE_TEAM", "1")
    if (dtype, k) not in _RUNS:
        _RUNS[dtype, k] = _device_run(ctx, k, dtype)
    lam1, alpha1, bound1 = _RUNS[dtype, k]
    monkeypatch.setenv("STC_VIRTUAL_SHARDS", "3")
    lam3, alpha3, bound3 = _device_run(ctx, k, dtype)
    np.testing.assert_array_equal(lam3, lam1)
    np.testing.assert_array_equal(alpha3, alpha1)
    assert bound3 == bound1


@pytest.mark.parametrize("k", LDS_EDGE_K)
def test_workgroup_kernel_lds_edge(ctx, oracle, monkeypatch, k):
    """(c) fp64 k_estep where its fixed LDS arrays (24·kp + 128 B) meet kLdsBudget: below it, at it, and the
    first kp past it (the launch then asks for more than the budget and registers that size): γ and stat by
    (a)'s criteria."""
    monkeypatch.setenv("STC_WIDE_TEAM", "1")
    lam0, batches, _ = _inputs(k)
    h, d = _handle(ctx, k, "f64", lam0)
    ids, g0 = batches[0]
    gamma, stat, iters = h.estep(ids, g0, want_stat=True)
    alpha, _ = oracle.resolve_alpha_eta(k)
    _, _, l1, rel = _check_estep(oracle, "f64", k, ids, g0, oracle.topics_exp_elog_beta(lam0), alpha, gamma, stat,
                                 iters, [])
    print(f"MEASURED f64 k={k} estep: stat l1 {l1:.3e} rel {rel:.3e}")
    _check_kernels(h, k)
    _close(h, d)


@pytest.mark.parametrize("k", DESCRIBE_K)
def test_describe_ties_and_extents(ctx, oracle, k):
    """(d) describeTopics of an integer λ in {1, 2, 3} — hundreds of exact ties per topic: ties keep the
    ascending term index (Scala's stable sortBy over zipWithIndex), and max_terms past V returns V terms."""
    import stc

    lam = np.random.default_rng(77 + k).integers(1, 4, size=(V, k)).astype(float)
    h = stc.LdaHandle(ctx, k, V, dtype="f64")
    h.set_topics(lam)
    for max_terms in (1, 10, V, V + 5):
        idx, w = h.describe(max_terms)
        idx_o, w_o = oracle.describe_topics(lam, max_terms)
        assert idx.shape == w.shape == (k, min(max_terms, V))
        assert np.array_equal(idx, idx_o), max_terms
        np.testing.assert_allclose(w, w_o, rtol=1e-12)
    h.close()
