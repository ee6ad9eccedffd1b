"""Mixed-mode training steps vs the oracle at every kernel width from k = 2 to the limit k = 4096.

dtype="mixed" runs the fp32 E-step for every document and re-solves in fp64 the documents whose fp32 fixed point
took more than `mixed_resolve_iters` iterations (lda_dispatch.hip mixed_resolve).  A mixed step
therefore runs two E-step families per k, and the fp64 one at the fp32 row pitch (kp: k rounded up to 4):
  fp32 first pass      grid k ≤ 128, the many-topic kernel to k = 2048 (from k = 129 a row's entries are taken
                       in the df-ascending row order), the workgroup kernel beyond
  fp64 re-solve        rows64 k ≤ 104 (KL = 4, 7, 13 at k ≤ 32, 56, 104 — at the fp32 pitch, which no fp64
                       handle runs), the many-topic kernel to k = 2048, the workgroup kernel beyond
  M-step               the fp32 λ update, which also writes the fp64 expElogβ' rows (Bp64) the next re-solve reads
MIXED_K has a value on each side of every one of those widths and, inside each rows64 instantiation, a k whose
fp32 and fp64 pitches differ (tests/test_topic_range_tables.py recomputes that from the sources).  The shape,
inputs and helpers are tests/test_gpu_topic_range.py's: V = 200, 40 documents of 1–40 terms, every 13th empty, 24
batch members per step drawn with duplicates, STC_WIDE_TEAM=1 (every E-step launch a one-CU kernel; the team
kernels under a mixed handle are not run here).

The threshold is a percentile of the fp32 handle's iteration counts on step 1's batch at λ₀ (RESOLVE_PCT).  The
median splits step 1's batch 9–12 against 11–13, but the counts fall as λ sharpens (the fp64 oracle at k = 100:
9..643 at step 1, 8..157 at step 3), and the median of step 1 leaves 0–2 documents above it at step 2 or 3 at
k = 2, 3, 54, 100, 512, 513 and 1024.  RESOLVE_PCT[k] is the multiple of 5 that, by the fp64 oracle's counts over the three steps, leaves the
most documents on the smaller side at every step; the condition itself (≥ 3 re-solved, ≥ 3 left on fp32, at every
step) is asserted from the counters.

Every step's oracle is built from the device's own λ and α read before the step, so a re-solved document is
held at the fp32-storage bar (2e-7, tests/test_gpu_mixed.py) and the λ/α check pins that step's M-step alone.

What the sweep found.  At 129 ≤ k ≤ 2048 a re-solved document's sufficient statistics went to the wrong terms.
The fp32 pass on the many-topic kernel writes r, the sort key (the term) and the sort value of a document's
entry e0 + n for the n-th entry of the row order; the fp64 re-solve was launched without that order, so its
r64[e0 + n] belonged to the n-th CSR entry, and k_mixed_fixup copied it beside the fp32 pass's key — the
responsibility of the n-th CSR term scattered into the stat row of the n-th rarest term.  γ, E[log θ] and the
iteration counts were right, which is all the suite looked at.  mixed_resolve now gives the fp64 launch the same
order as the fp32 pass.  k ≤ 128 (no order exists) and the workgroup kernel (reads none) were right.
Before that change every case at 129 ≤ k ≤ 2048 failed at its first stat comparison and every other case passed;
stat l1 against the oracle, before the change: (a) k = 129 0.455, 256 0.458, 257 0.453, 512 0.493, 513 0.495, 1024
0.466, 1025 0.500, 2048 0.467; (b) k = 129 0.486, 513 0.514, 2048 0.490; (c) k = 129 0.347, 600 0.350 (its
workgroup-kernel documents were right); (f) λ of the group 0.545 from the single handle's after step 1 (a member's
row order is its shard's, so the two scattered differently).  (d) is bitwise as written.

MEASURED (MI355X), worst over the three steps per case; every width passes the bars as written:
  k      λ         α         stat l1 / rel        re-solved γ   threshold, re-solved of non-empty per step
  2      1.8e-07   6.2e-09   1.3e-07 / 2.2e-06    5.7e-08       103   14/21 11/21  4/23
  3      1.7e-07   2.8e-09   1.0e-07 / 1.4e-06    5.5e-08        98   15/21 11/22  4/21
  30     6.2e-07   1.2e-09   1.3e-07 / 6.6e-06    5.5e-08        48   16/23 11/24  7/22
  54     3.9e-07   1.4e-09   1.4e-07 / 3.1e-06    5.2e-08        40   18/22  5/21  3/24
  62     1.2e-07   1.4e-09   6.9e-08 / 7.5e-07    5.4e-08        33   20/24  4/22 11/23
  100    6.0e-07   1.1e-09   1.1e-07 / 4.5e-06    5.0e-08        60   16/21 10/23  4/21
  102    6.3e-07   1.3e-09   1.0e-07 / 5.9e-06    5.6e-08        42   15/22  9/20  5/21
  104    2.0e-06   1.2e-09   4.1e-07 / 3.4e-05    4.7e-08        89   14/21  6/23  7/23
  105    1.2e-07   1.1e-09   7.1e-08 / 1.0e-06    4.8e-08        57   15/20 11/23  6/21
  128    1.5e-07   1.3e-09   9.3e-08 / 8.6e-07    5.7e-08        40   17/23 14/23  5/19
  129    5.1e-08   9.2e-10   3.8e-08 / 1.6e-07    5.0e-08        34   18/24 10/22  5/22
  256    5.9e-07   3.1e-08   1.3e-07 / 6.9e-06    5.9e-08        45   18/23  7/21  7/23
  257    3.0e-07   3.6e-08   1.2e-07 / 2.9e-06    4.8e-08        34   15/22  9/23  7/21
  512    3.5e-06   3.5e-07   4.3e-07 / 4.3e-05    5.9e-08        28   19/24 10/20  4/19
  513    2.1e-06   9.3e-07   3.4e-07 / 2.1e-05    5.8e-08        29   19/24 11/21 10/22
  1024   1.6e-05   3.0e-08   6.6e-07 / 2.8e-04    5.9e-08        21   16/23 11/22  8/23
  1025   6.9e-06   4.3e-07   9.4e-07 / 1.3e-03    6.0e-08        27   13/23 13/23  9/22
  2048   8.3e-06   6.9e-08   5.6e-07 / 2.2e-04    5.9e-08         9   15/22 17/22 14/23
  2049   1.3e-06   8.6e-08   6.0e-07 / 1.5e-04    5.9e-08        19   13/22  9/22  5/23
  4096   2.1e-06   9.9e-08   8.6e-07 / 1.3e-04    5.9e-08         6    9/21  9/22 14/23
  (bars: λ and α 1e-4, stat l1 1e-4, stat rel 1e-2, re-solved γ 2e-7; no iteration count was off the oracle's)
  (b) everything re-solved, stat l1 / rel against the f64 handle: k = 100 3.9e-08 / 1.3e-07, 129 3.2e-08 / 1.2e-07,
      513 3.3e-08 / 1.3e-07, 2048 3.4e-08 / 1.3e-07, 2049 3.6e-08 / 1.6e-07 — the fp32 rounding of r and eθ' and
      the fp32 sum; against the oracle the same figures
  (c) both lists, stat l1 / rel, γ: k = 120 3.8e-08 / 1.7e-07, 5.2e-08 (15..1558 iterations); 129 3.7e-08 /
      1.4e-07, 4.0e-08 (6..1962); 600 3.6e-08 / 1.5e-07, 4.7e-08 (4..1222)
  (f) group against the single handle, k = 200: λ 5.1e-08, α 9.7e-11; re-solved 15, 14, 8 in both at the three steps
The file takes about 13 s.
"""
import numpy as np
import pytest

from test_gpu_lda import TOL
from test_gpu_topic_range import (BATCH, D, FRAC, STEPS, TEAM_FAMILIES, V, _check_estep, _check_kernels, _close,
                                  _corpus, _inputs)

pytestmark = pytest.mark.gpu

MIXED_K = (2, 3, 30, 54, 62, 100, 102, 104, 105, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096)
# the percentile of step 1's fp32 iteration counts that becomes mixed_resolve_iters (module docstring)
RESOLVE_PCT = {2: 30, 3: 25, 30: 30, 54: 15, 62: 15, 100: 20, 102: 30, 104: 30, 105: 25, 128: 25, 129: 25, 200: 35,
               256: 20, 257: 30, 512: 20, 513: 20, 1000: 20, 1024: 30, 1025: 45, 2048: 30, 2049: 40, 4096: 50}
ALL_RESOLVED_K = (100, 129, 513, 2048, 2049)
BOTH_LISTS_K = (120, 129, 600)
NONE_RESOLVED_K = (100, 129, 1025)
SLICED_K = (100, 200, 1000)
GROUP_K = 200
ITER_CAP = 100000  # stc_lda_create's default max_inner_iter: no document's fp32 count passes it
GAMMA_RTOL = 2e-7  # a re-solved γ: fp64 arithmetic, fp32 storage (tests/test_gpu_mixed.py)
# (c): lengths around wide_row_cap (512) and grid_row_cap(120) (256), one long, short ones, an empty one
LIST_V = 900
LIST_LENGTHS = (511, 512, 513, 256, 257, 700, 5, 17, 40, 1, 90, 130, 0, 300, 64, 33)

_THR = {}


class _Counting:
    """the oracle, recording the iteration count of every run under its own stop rule"""

    def __init__(self, oracle):
        self._o = oracle
        self.its = []

    def __getattr__(self, name):
        return getattr(self._o, name)

    def variational_topic_inference(self, *a, **kw):
        out = self._o.variational_topic_inference(*a, **kw)
        if kw.get("n_iter") is None:
            self.its.append(out[2])
        return out


class _EstepKernels:
    """a handle's kernel counters without the two re-solve counters, for _check_kernels"""

    def __init__(self, h):
        self._h = h

    def counters(self):
        kernels = self._h.counters()["kernels"]
        return {"kernels": {f: n for f, n in kernels.items() if not f.startswith("mixed_")}}


def _handle(ctx, k, dtype, lam0, corpus=None, **kw):
    import stc

    if corpus is None:
        corpus, _ = _corpus()
    h = stc.LdaHandle(ctx, k, corpus.num_cols, dtype=dtype, mini_batch_fraction=FRAC, optimize_doc_concentration=True,
                      **kw)
    d = stc.DeviceCsr.upload(ctx, corpus, stc.STC_F32 if dtype == "f32" else stc.STC_F64)
    h.set_corpus(d, corpus.num_rows)
    h.set_topics(lam0)
    return h, d


def _threshold(ctx, k):
    """mixed_resolve_iters for the three-step runs at k: RESOLVE_PCT[k] of the fp32 handle's positive iteration
    counts on step 1's batch at λ₀"""
    if k not in _THR:
        lam0, batches, _ = _inputs(k)
        h32, d32 = _handle(ctx, k, "f32", lam0)
        it32 = h32.estep(*batches[0])[2]
        _close(h32, d32)
        _THR[k] = int(np.percentile(it32[it32 > 0], RESOLVE_PCT[k]))
        print(f"k={k}: fp32 counts at step 1 {sorted(int(x) for x in it32[it32 > 0])} threshold {_THR[k]}")
    return _THR[k]


def _kernel_delta(c0, c1):
    return {f: c1[f] - c0[f] for f in c1}


def _stat_errors(stat, stat_o):
    """the fp32 stat criteria of _check_estep (l1, worst relative error over the entries above 1e-4 of the largest)"""
    nz = stat_o > 1e-4 * stat_o.max()
    return np.abs(stat - stat_o).sum() / stat_o.sum(), (np.abs(stat[nz] - stat_o[nz]) / stat_o[nz]).max()


def _check_resolved(i, iters, it_o, gamma, g_o, border):
    """a re-solved member: the oracle's fp64 count (or one off, for at most one document per case — the fp64 rule
    of test_gpu_topic_range.py) and γ at that count within fp32 storage rounding; returns the worst γ error"""
    if iters[i] != it_o:
        assert abs(int(iters[i]) - it_o) <= 1, (i, iters[i], it_o)
        border.append((i, int(iters[i]), it_o))
        assert len(border) <= 1, border
    np.testing.assert_allclose(gamma[i], g_o, rtol=GAMMA_RTOL, atol=1e-30)
    return float(np.max(np.abs(gamma[i] - g_o) / g_o))


def _device_run(ctx, k, thr):
    """(a)'s three steps on a mixed handle alone: (λ, α, bound)"""
    lam0, batches, g0_all = _inputs(k)
    h, d = _handle(ctx, k, "mixed", lam0, mixed_resolve_iters=thr)
    for ids, g0 in batches:
        h.estep(ids, g0, want_stat=True)
        h.step(ids, g0, stats=False)
    assert h.counters()["kernels"]["mixed_docs"] > 0
    out = (h.topics(), h.alpha(), h.bound(d, gamma0=g0_all)["bound"])
    _close(h, d)
    return out


@pytest.mark.parametrize("k", MIXED_K)
def test_mixed_steps_match_oracle_at_every_width(ctx, oracle, monkeypatch, k):
    """(a) three injected training steps.  Per step: which members were re-solved (the fp32 handle's count on the
    same λ and α above the threshold), each of them against the fp64 oracle, every other one bit for bit the fp32
    handle's, stat against the oracle's sum over all members by _check_estep's fp32 criteria, λ and α of the
    step against the oracle's update from the device's own λ and α before it."""
    monkeypatch.setenv("STC_WIDE_TEAM", "1")
    O = _Counting(oracle)
    lam0, batches, _ = _inputs(k)
    thr = _threshold(ctx, k)
    h32, d32 = _handle(ctx, k, "f32", lam0)
    h, d = _handle(ctx, k, "mixed", lam0, mixed_resolve_iters=thr)
    _, eta = oracle.resolve_alpha_eta(k)
    border = []
    worst = dict(lam=0.0, alpha=0.0, stat_l1=0.0, stat_rel=0.0, gamma=0.0)
    for step, (ids, g0) in enumerate(batches):
        lam_b, alpha_b = h.topics(), h.alpha()
        if step > 0:
            h32.set_topics(lam_b)
            h32.set_alpha(alpha_b)
        g32, _, it32 = h32.estep(ids, g0)
        c0 = h.counters()["kernels"]
        gamma, stat, iters = h.estep(ids, g0, want_stat=True)
        c1 = h.counters()["kernels"]
        s = h.step(ids, g0)
        c2 = h.counters()["kernels"]
        slow, live = it32 > thr, it32 > 0
        print(f"step {step + 1}: fp32 counts {sorted(int(x) for x in it32[live])} threshold {thr} "
              f"re-solved {c1['mixed_docs'] - c0['mixed_docs']} of {int(live.sum())}")
        # the condition: both kinds of document in every step, and the counters count exactly the slow ones
        assert s["batch_docs"] == BATCH and s["nonempty_docs"] == live.sum()
        assert c1["mixed_docs"] - c0["mixed_docs"] == c2["mixed_docs"] - c1["mixed_docs"] == slow.sum()
        assert slow.sum() >= 3 and live.sum() - slow.sum() >= 3, (slow.sum(), live.sum())
        assert c1["mixed_resolves"] - c0["mixed_resolves"] == c2["mixed_resolves"] - c1["mixed_resolves"] == 1
        eeb = oracle.topics_exp_elog_beta(lam_b)
        O.its = []
        gam_o, stat_o, l1, rel = _check_estep(O, "f32", k, ids, g0, eeb, alpha_b, gamma, stat, iters, [])
        members = [i for i in range(BATCH) if gam_o[i] is not None]
        assert len(members) == len(O.its) == live.sum()
        for i, it_o in zip(members, O.its):
            if slow[i]:
                worst["gamma"] = max(worst["gamma"], _check_resolved(i, iters, it_o, gamma, gam_o[i], border))
            else:
                assert iters[i] == it32[i], (i, iters[i], it32[i])
                np.testing.assert_array_equal(gamma[i], g32[i])
        # the oracle's submitMiniBatch from the device's λ and α before the step and the oracle's γ / stat
        st = oracle.OnlineLDAState(lam=lam_b.T.copy(), alpha=alpha_b.copy(), eta=eta, corpus_size=D,
                                   mini_batch_fraction=FRAC, optimize_doc_concentration=True, iteration=step + 1)
        assert abs(s["rho"] - st.rho()) < 1e-15
        logphat = np.sum([oracle.dirichlet_expectation(gam_o[i]) for i in members], axis=0)
        oracle.update_lambda(st, stat_o.T * eeb.T, int(np.ceil(FRAC * D)))
        oracle.update_alpha(st, logphat / len(members), len(members))
        assert not np.array_equal(st.alpha, alpha_b)  # the Newton step is accepted with this input
        lam, dev_alpha = h.topics(), h.alpha()
        e_lam = np.max(np.abs(lam - st.lam.T) / st.lam.T)
        e_alpha = np.max(np.abs(dev_alpha - st.alpha) / st.alpha)
        for name, e in (("lam", e_lam), ("alpha", e_alpha), ("stat_l1", l1), ("stat_rel", rel)):
            worst[name] = max(worst[name], e)
        print(f"step {step + 1}: lam {e_lam:.3e} alpha {e_alpha:.3e} stat l1 {l1:.3e} rel {rel:.3e} border {border}")
        assert e_lam < TOL["f32"]["lam"], (step, e_lam)
        np.testing.assert_allclose(dev_alpha, st.alpha, rtol=TOL["f32"]["lam"])
    print(f"MEASURED mixed k={k}: lam {worst['lam']:.3e} alpha {worst['alpha']:.3e} "
          f"stat l1 {worst['stat_l1']:.3e} rel {worst['stat_rel']:.3e} resolved gamma {worst['gamma']:.3e}")
    assert h.iteration() == STEPS
    # the families of both passes: no team family, the workgroup kernel only past k = 2048
    _check_kernels(_EstepKernels(h), k)
    ran = {f for f, n in _EstepKernels(h).counters()["kernels"].items() if n > 0}
    fp32 = "k_estep_grid" if k <= 128 else "k_estep_wide"
    fp64 = "k_estep_rows64" if k <= 104 else "k_estep_wide"
    assert ran == ({fp32, fp64} if k <= 2048 else {"k_estep"}), ran
    _close(h, d)
    _close(h32, d32)


@pytest.mark.parametrize("k", ALL_RESOLVED_K)
def test_everything_resolved_equals_fp64(ctx, oracle, monkeypatch, k):
    """(b) mixed_resolve_iters = 1 (the oracle's smallest count here is 3): every non-empty document is re-solved,
    and one estep is the fp64 handle's — the same iteration counts, γ within fp32 storage rounding — with stat at
    the fp32 bars against the oracle (it is summed in fp32 from the fp32 roundings of r and eθ')."""
    monkeypatch.setenv("STC_WIDE_TEAM", "1")
    lam0, batches, _ = _inputs(k)
    ids, g0 = batches[0]
    hm, dm = _handle(ctx, k, "mixed", lam0, mixed_resolve_iters=1)
    h64, d64 = _handle(ctx, k, "f64", lam0)
    gamma, stat, iters = hm.estep(ids, g0, want_stat=True)
    g64, stat64, it64 = h64.estep(ids, g0, want_stat=True)
    assert iters[iters > 0].min() >= 3
    assert hm.counters()["kernels"]["mixed_docs"] == (it64 > 0).sum() > 0
    np.testing.assert_array_equal(iters, it64)
    np.testing.assert_allclose(gamma, g64, rtol=GAMMA_RTOL, atol=1e-30)
    l1_64, rel_64 = _stat_errors(stat, stat64)
    print(f"MEASURED mixed k={k} all re-solved: stat vs the f64 handle l1 {l1_64:.3e} rel {rel_64:.3e}")
    alpha, _ = oracle.resolve_alpha_eta(k)
    _, _, l1, rel = _check_estep(oracle, "f32", k, ids, g0, oracle.topics_exp_elog_beta(lam0), alpha, gamma, stat,
                                 iters, [])
    print(f"MEASURED mixed k={k} all re-solved: stat vs the oracle l1 {l1:.3e} rel {rel:.3e}")
    _check_kernels(_EstepKernels(hm), k)
    _close(hm, dm)
    _close(h64, d64)


def _list_corpus():
    import stc

    rng = np.random.default_rng(4242)
    rows = []
    for n in LIST_LENGTHS:
        ids = np.sort(rng.choice(LIST_V, size=n, replace=False)).astype(np.int32)
        rows.append((ids, rng.integers(1, 7, n).astype(np.float64)))
    return stc.CsrMatrix.from_rows(rows, LIST_V), rows


@pytest.mark.parametrize("k", BOTH_LISTS_K)
def test_both_resolve_lists_at_wide_k(ctx, oracle, monkeypatch, k):
    """(c) both re-solve lists in one call, every document re-solved (mixed_resolve_iters = 1): the documents the
    fp64 fast kernel holds and, past its 512 rows, the workgroup kernel's.  k = 120: documents of 257–512 terms
    are past the fp32 grid kernel (workgroup kernel, CSR order) but on the fp64 many-topic kernel; k = 129, 600:
    documents on the workgroup kernel in both passes beside ordered short ones.  γ, iteration counts and stat
    against the oracle."""
    monkeypatch.setenv("STC_WIDE_TEAM", "1")
    corpus, rows = _list_corpus()
    n = len(rows)
    rng = np.random.default_rng(7000 + k)
    lam0 = rng.gamma(100.0, 0.01, size=(LIST_V, k))
    ids, g0 = np.arange(n), rng.gamma(100.0, 0.01, size=(n, k))
    hm, dm = _handle(ctx, k, "mixed", lam0, corpus=corpus, mixed_resolve_iters=1)
    h32, d32 = _handle(ctx, k, "f32", lam0, corpus=corpus)
    c0 = hm.counters()["kernels"]
    gamma, stat, iters = hm.estep(ids, g0, want_stat=True)
    ran = _kernel_delta(c0, hm.counters()["kernels"])
    c32 = h32.counters()["kernels"]["k_estep"]
    h32.estep(ids, g0)
    live = [i for i in range(n) if rows[i][0].size > 0]
    assert len(live) == n - 1 and ran["mixed_docs"] == len(live) and ran["mixed_resolves"] == 1
    # the fp64 long list ran: one workgroup-kernel launch more than the fp32 handle's same call
    assert ran["k_estep"] == h32.counters()["kernels"]["k_estep"] - c32 + 1 == 2, ran
    assert ran["k_estep_wide"] == (1 if k <= 128 else 2) and all(ran[f] == 0 for f in TEAM_FAMILIES), ran
    alpha, _ = oracle.resolve_alpha_eta(k)
    eeb = oracle.topics_exp_elog_beta(lam0)
    stat_o = np.zeros((LIST_V, k))
    border, e_gamma = [], 0.0
    for i in range(n):
        cid, cts = rows[i]
        if cid.size == 0:
            assert np.all(gamma[i] == 0) and iters[i] == 0
            continue
        g, ss, it = oracle.variational_topic_inference(cid, cts, eeb, alpha, g0[i])
        if iters[i] != it:
            g, ss, _ = oracle.variational_topic_inference(cid, cts, eeb, alpha, g0[i], n_iter=int(iters[i]))
        e_gamma = max(e_gamma, _check_resolved(i, iters, it, gamma, g, border))
        np.add.at(stat_o, cid, ss.T)
    absent = np.setdiff1d(np.arange(LIST_V), np.concatenate([r[0] for r in rows]))
    assert np.all(stat[absent] == 0.0)
    l1, rel = _stat_errors(stat, stat_o)
    print(f"MEASURED mixed k={k} both lists: stat l1 {l1:.3e} rel {rel:.3e} gamma {e_gamma:.3e} "
          f"iters {int(iters[iters > 0].min())}..{int(iters.max())} border {border}")
    assert l1 < 1e-4, l1
    assert rel < 1e-2, rel
    _close(hm, dm)
    _close(h32, d32)


@pytest.mark.parametrize("k", NONE_RESOLVED_K)
def test_mixed_nothing_resolved_is_the_fp32_handle(ctx, monkeypatch, k):
    """(d) the threshold at the iteration cap: nothing is re-solved, and three steps are the fp32 handle's bit for
    bit — γ, stat, λ and α.  (The term counts are small integers, so the handle's fp32 copy of the values is the
    fp32 upload; λ is fp64 in both, and the M-step writes the fp64 expElogβ' rows beside the fp32 ones from it.)"""
    monkeypatch.setenv("STC_WIDE_TEAM", "1")
    lam0, batches, _ = _inputs(k)
    hm, dm = _handle(ctx, k, "mixed", lam0, mixed_resolve_iters=ITER_CAP)
    h32, d32 = _handle(ctx, k, "f32", lam0)
    for ids, g0 in batches:
        gm, sm, im = hm.estep(ids, g0, want_stat=True)
        g32, s32, i32 = h32.estep(ids, g0, want_stat=True)
        assert i32.max() < ITER_CAP
        np.testing.assert_array_equal(im, i32)
        np.testing.assert_array_equal(gm, g32)
        np.testing.assert_array_equal(sm, s32)
        hm.step(ids, g0, stats=False)
        h32.step(ids, g0, stats=False)
        np.testing.assert_array_equal(hm.topics(), h32.topics())
        np.testing.assert_array_equal(hm.alpha(), h32.alpha())
    kernels = hm.counters()["kernels"]
    assert kernels["mixed_docs"] == 0 and kernels["mixed_resolves"] == 0
    _close(hm, dm)
    _close(h32, d32)


@pytest.mark.parametrize("k", SLICED_K)
def test_mixed_sliced_mstep_bit_identical(ctx, monkeypatch, k):
    """(e) (a)'s steps with the M-step over three vocabulary slices of 128 rows (the Bp64 + v0·kp slices of the
    sliced tail, which the next step's re-solve reads): λ, α and the bound bit for bit those of the unsliced run."""
    monkeypatch.setenv("STC_WIDE_TEAM", "1")
    thr = _threshold(ctx, k)
    lam1, alpha1, bound1 = _device_run(ctx, k, thr)
    monkeypatch.setenv("STC_VIRTUAL_SHARDS", "3")
    lam3, alpha3, bound3 = _device_run(ctx, k, thr)
    np.testing.assert_array_equal(lam3, lam1)
    np.testing.assert_array_equal(alpha3, alpha1)
    assert bound3 == bound1


def test_mixed_group_matches_single_handle(ctx, monkeypatch):
    """(f) a two-member mixed group on the in-process transport against one mixed handle with the same threshold,
    three injected steps: steps 2 and 3 re-solve from the all-gathered Bp64.  After step 1 the two λ differ by
    fp32 rounding (stat is summed per member), so a document on the threshold may change sides."""
    import stc

    monkeypatch.setenv("STC_WIDE_TEAM", "1")
    k = GROUP_K
    corpus, _ = _corpus()
    lam0, batches, _ = _inputs(k)
    thr = _threshold(ctx, k)
    h, d = _handle(ctx, k, "mixed", lam0, mixed_resolve_iters=thr)
    with stc.LdaGroup([0, 0], k, V, dtype="mixed", mini_batch_fraction=FRAC, optimize_doc_concentration=True,
                      mixed_resolve_iters=thr) as g:
        assert g.transport() == "in-process"
        g.set_corpus(corpus)
        g.set_topics(lam0)
        for step, (ids, g0) in enumerate(batches):
            n0 = h.counters()["kernels"]["mixed_docs"]
            m0 = sum(c["kernels"]["mixed_docs"] for c in g.counters())
            sh = h.step(ids, g0)
            sg = g.step(ids, g0)
            n1 = h.counters()["kernels"]["mixed_docs"] - n0
            m1 = sum(c["kernels"]["mixed_docs"] for c in g.counters()) - m0
            assert sg["batch_docs"] == sh["batch_docs"] and sg["nonempty_docs"] == sh["nonempty_docs"]
            e_lam = np.max(np.abs(g.topics() - h.topics()) / h.topics())
            e_alpha = np.max(np.abs(g.alpha() - h.alpha()) / h.alpha())
            print(f"MEASURED mixed group k={k} step {step + 1}: lam {e_lam:.3e} alpha {e_alpha:.3e} "
                  f"re-solved {m1} (group) {n1} (single)")
            assert n1 > 0 and (m1 == n1 if step == 0 else m1 > 0), (step, m1, n1)
            assert e_lam < TOL["f32"]["lam"], (step, e_lam)
            assert e_alpha < TOL["f32"]["lam"], (step, e_alpha)
        assert g.iteration() == h.iteration() == STEPS
    _close(h, d)
