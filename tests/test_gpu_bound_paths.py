"""logLikelihoodBound's corpus part and topicDistribution on every one-CU E-step kernel path, against Spark's
formula (oracle.doc_bound: log-space logSumExp per token) at the oracle's own iterates.

The bound's token term is a BOUND epilogue compiled into each kernel family (lda.hip estep_doc, lda_rows64.hip
rows64_close, lda_grid.hip grid_core, lda_wide.hip k_estep_wide), each with its own arithmetic: which iterate
the last pass uses, the per-term scale m_v beside the scaled expElogβ, and the move from the loop's ψ(Σγ′) to
the exact ψ(Σγ).  launch_split never takes a team kernel when the bound is asked for, so these four are the
whole surface.  One more or one fewer inner iteration moves a document's bound by 1e-8 … 1e-5 relative, so the
fp64 limit (1e-10) also pins the iterate the epilogue used.

The length tables below repeat constants of the kernels; tests/test_bound_path_tables.py reads the constants
from the sources and fails when a retune moves a boundary until the lengths follow.

Largest per-document relative error observed on an MI355X (every parameter prints its own before it asserts).
fp64, |corpus_part − b_j| / |b_j| at the iterate j the kernel stopped on (the neighbouring iterates are 1e-8 or
more away), limit 1e-10:
  rows64 (+ long pass)   3.1e-13  (k = 100; 1.2e-15 or less at the other k)
  many-topic kernel      3.7e-12  (k = 105; Q = 2: 2.2e-12 at k = 1025; Q = 4: 6.1e-15)
  workgroup kernel       1.6e-11  (k = 100; 1.1e-12 at k = 16, 8.0e-14 at k = 2049)
  hard case              1.0e-15  (k = 2000: the log-space rows, 8.7e-16 many-topic, 1.0e-15 workgroup kernel)
fp32, distance to the oracle's interval over |b_it|, limit 1e-5:
  grid 7.3e-8, many-topic 3.3e-8, workgroup 4.1e-8; hard case 2.8e-6 at k = 100 (grid), 0 at k = 300 / 2000.
What these parameters gave before the kernels' bound epilogues were corrected:
  the floored logarithm of an underflowed dot product: many-topic kernel fp64 k = 2000 hard 2.3e-4, fp32 k = 300
  hard 4.3e-5; workgroup kernel (hardwg) fp32 k = 300 / 2000 3.0e-5 / 4.6e-5, fp64 k = 2000 −∞;
  Σγ summed in fp32: fp32 grid k = 100 / 105 1.3e-4 / 1.5e-4 on the one-entry document of value 1e-4·c.
"""
import functools

import numpy as np
import pytest

from helpers import oracle_iterates

pytestmark = pytest.mark.gpu

V = 2048

# ---- boundaries of the kernels (checked against the sources by tests/test_bound_path_tables.py)
ROWS64_REG_SETS, ROWS64_ONCHIP_SETS, ROWS64_MAX_SETS = 5, 6, 8  # RCommon's VGPR sets, kOnChipSets, kMaxSets
GRID_RMAX = {"G32": 8, "G64": 8, "G104": 6, "G104L": 8, "G128": 8}  # lda_grid.hip GShape RMAX
GRID_R7_ROWS = 224  # grid_doc: R = 7 up to 224 rows, R = 8 beyond
# both sides of every 32-row set boundary that changes code, then past rows64_row_cap / grid_row_cap (256)
GRID_LENGTHS = (1, 31, 32, 33, 160, 161, 192, 193, 224, 225, 256, 257, 400)
# lda_wide.hip per (dtype, Q): wide_nr<T, Q>() rows in VGPRs, wide_resident_rows<T>(k) in VGPRs + LDS
WIDE_ROWS = {("f64", 1): (64, 94), ("f64", 2): (24, 39), ("f64", 4): (8, 15),
             ("f32", 1): (176, 245), ("f32", 2): (64, 98), ("f32", 4): (32, 49)}
WIDE_MAX_ROWS = 512  # kWRows; longer documents run the workgroup kernel
# lda.hip estep_lds_rows<T>(k): the longest document whose block the workgroup kernel keeps in LDS
WG_LDS_ROWS = {("f64", 16): 448, ("f64", 100): 88, ("f32", 16): 808, ("f32", 100): 184}
WG_V = 4096  # the workgroup cases' vocabulary: a 3000-term document needs more than 2048 terms

GRID_K = {"f64": (5, 32, 33, 56, 57, 64, 65, 100, 104), "f32": (5, 32, 33, 64, 65, 100, 104, 105, 128)}
WIDE_K = {"f64": (105, 300, 512, 513, 1024, 1025, 2048), "f32": (129, 300, 512, 513, 1024, 1025, 2048)}
HARD_K = (100, 300, 2000)

TEAM_FAMILIES = ("k_estep_wide_mc", "k_estep_wide_tc", "k_estep_tgrid64", "team_fallback")


def wide_q(k):
    return 1 if k <= 512 else 2 if k <= 1024 else 4


# The two dtypes' boundaries go into one corpus per k, so both parameters share the oracle's iterates.
def wide_lengths(k):
    edges = {1, 7, 8, 9, WIDE_MAX_ROWS - 1, WIDE_MAX_ROWS, WIDE_MAX_ROWS + 1}
    for dtype in ("f64", "f32"):
        nr, res = WIDE_ROWS[dtype, wide_q(k)]
        edges |= {nr, nr + 1, res, res + 1}
    return tuple(sorted(edges))


def wg_lengths(k):
    if k > 2048:  # fp64 k = 2049: no fast kernel exists
        return (1, 100)
    edges = {1, 33, 3000}
    for dtype in ("f64", "f32"):
        edges |= {WG_LDS_ROWS[dtype, k], WG_LDS_ROWS[dtype, k] + 1}
    return tuple(sorted(edges))


def _params():
    out = []
    for dtype in ("f64", "f32"):
        out += [(dtype, k, "grid") for k in GRID_K[dtype]]
        out += [(dtype, k, "wide") for k in WIDE_K[dtype]]
        out += [(dtype, k, "wg") for k in (16, 100)]
        out += [(dtype, k, "hard") for k in HARD_K]
        out += [(dtype, k, "hardwg") for k in HARD_K[1:]]  # the same documents on the workgroup kernel
    out.append(("f64", 2049, "wg"))
    # the same (k, path) of the two dtypes side by side: they share the oracle's iterates where the lengths agree
    return sorted(out, key=lambda p: (p[2][:4], p[1], p[2], p[0]))


def lengths_of(dtype, k, path):
    return {"grid": lambda: GRID_LENGTHS, "wide": lambda: wide_lengths(k),
            "wg": lambda: wg_lengths(k), "hard": lambda: None, "hardwg": lambda: None}[path]()


VALUE_SCALES = (1.0, 0.37, 1e-4)  # fractional, as TF·IDF feeds them (1e-4: the reference's floor of a zero idf)


def _values(rng, n):
    v = rng.integers(1, 5, n).astype(np.float64) * rng.choice(VALUE_SCALES, n)
    v[4::5] = 0.0  # an explicit zero at every fifth entry
    return v


@functools.lru_cache(maxsize=2)
def _case(O, k, lengths, nv):
    """Corpus, λ, α, η, γ₀ and the oracle's iterates (±3 around its stopping iteration) of one standard case."""
    rng = np.random.default_rng(1000 + k)
    rows = []
    for n in lengths:
        ids = np.sort(rng.choice(nv, size=n, replace=False)).astype(np.int32)
        rows.append((ids, _values(rng, n)))
    rows.insert(2, (np.zeros(0, np.int32), np.zeros(0)))  # an empty row
    rows.insert(4, (np.sort(rng.choice(nv, size=5, replace=False)).astype(np.int32), np.zeros(5)))  # all zeros
    eta = 1.0 / k
    lam = rng.gamma(100.0, 0.01, size=(nv, k)) * np.exp(rng.uniform(-4.0, 6.0, size=(nv, 1)))
    lam[::7] = eta  # a term never seen
    alpha = rng.uniform(0.05, 0.5, size=k)
    return _finish(O, rng, rows, lam, alpha, eta, nv)


@functools.lru_cache(maxsize=2)
def _hard_case(O, k):
    """α = 1/k; 64 terms whose λ row is η except 50.0 on one topic each, topics on which every other term has
    η, so a document holding such a term once leaves that topic at γ ≈ α.  Its token term is then the logSumExp of
    exponents that are all ≈ ψ(1/k) or lower (≈ −2007 at k = 2000): every product expElogβ·eθ underflows — fp64
    at k = 2000, fp32 from k ≈ 100 — and only a log-space evaluation gives Spark's value.  Each of 8 documents:
    60 ordinary entries, one such term with value 1e-4 (the reference's TF·IDF floor) and one with value 1.0."""
    rng = np.random.default_rng(2000 + k)
    eta = 1.0 / k
    special_t = np.sort(rng.choice(k, size=64, replace=False))
    special_v = np.sort(rng.choice(V, size=64, replace=False))
    ordinary_v = np.setdiff1d(np.arange(V), special_v)
    lam = rng.gamma(100.0, 0.01, size=(V, k)) * np.exp(rng.uniform(-4.0, 6.0, size=(V, 1)))
    lam[:, special_t] = eta
    lam[special_v] = eta
    lam[special_v, special_t] = 50.0
    rows = []
    for d in range(8):
        ids = np.concatenate([rng.choice(ordinary_v, size=60, replace=False), special_v[[2 * d, 2 * d + 1]]])
        vals = np.concatenate([_values(rng, 60), [1e-4, 1.0]])
        order = np.argsort(ids)
        rows.append((ids[order].astype(np.int32), vals[order]))
    rows.insert(2, (np.zeros(0, np.int32), np.zeros(0)))
    rows.insert(4, (np.sort(rng.choice(V, size=5, replace=False)).astype(np.int32), np.zeros(5)))
    return _finish(O, rng, rows, lam, np.full(k, 1.0 / k), eta, V)


def _finish(O, rng, rows, lam, alpha, eta, nv):
    import stc

    k = lam.shape[1]
    corpus = stc.CsrMatrix.from_rows(rows, nv)
    g0 = rng.gamma(100.0, 0.01, size=(len(rows), k))
    elog_beta = O.dirichlet_expectation(lam.T).T
    eeb = np.exp(elog_beta)
    its = []
    for i, (ids, cts) in enumerate(rows):
        its.append(oracle_iterates(O, ids, cts, eeb, elog_beta, alpha, g0[i], 3) if np.any(cts != 0) else None)
    topics_part = O.topics_bound(lam, eta, elog_beta)
    for a in (lam, alpha, g0):
        a.setflags(write=False)  # shared between the two dtypes' parameters
    return dict(corpus=corpus, lam=lam, alpha=alpha, eta=eta, g0=g0, its=its, topics_part=topics_part)


def _expected_kernels(dtype, k, path, lens):
    """The launches of one whole-corpus bound call, by family, from the documents' lengths."""
    exp = dict.fromkeys(("k_estep_rows64", "k_estep_rows64_long", "k_estep_grid", "k_estep_wide", "k_estep"), 0)
    if path in ("wg", "hardwg"):
        exp["k_estep"] = 1
        return exp
    wide = k > (104 if dtype == "f64" else 128)
    cap = WIDE_MAX_ROWS if wide else 32 * ROWS64_MAX_SETS
    if wide:
        exp["k_estep_wide"] = 1
    elif dtype == "f64":
        exp["k_estep_rows64"] = 1
        exp["k_estep_rows64_long"] = int(max(lens) > 32 * ROWS64_ONCHIP_SETS)
    else:
        exp["k_estep_grid"] = 1
    exp["k_estep"] = int(max(lens) > cap)
    return exp


# The fp64 limit is the project's TOL["f64"]["bound"] (test_gpu_lda.py), the fp32 one its logPerplexity bar.
F64_BOUND, F32_BOUND = 1e-10, 1e-5


@pytest.mark.parametrize("dtype,k,path", _params())
def test_bound_and_topic_distribution_paths(ctx, oracle, dtype, k, path, monkeypatch):
    """path "grid": the dtype's grid family (fp64 rows64 and its long pass, fp32 grid) with the workgroup kernel
    past 256 rows; "wide": the many-topic kernel (rows in VGPRs, in LDS, streamed) with the workgroup kernel past
    512 rows; "wg": the workgroup kernel alone (block in LDS, streamed); "hard": see _hard_case ("hardwg": on the workgroup
    kernel)."""
    import stc

    if path in ("wg", "hardwg"):
        monkeypatch.setenv("STC_DISABLE_WAVE", "1")
    lens = lengths_of(dtype, k, path)
    case = _hard_case(oracle, k) if path.startswith("hard") else _case(oracle, k, lens, WG_V if path == "wg" else V)
    corpus, g0, its, alpha = case["corpus"], case["g0"], case["its"], case["alpha"]
    D = corpus.num_rows
    row_len = np.diff(corpus.indptr)
    sdt = stc.STC_F32 if dtype == "f32" else stc.STC_F64
    h = stc.LdaHandle(ctx, k, corpus.num_cols, doc_concentration=alpha, topic_concentration=case["eta"], dtype=dtype)
    h.set_topics(case["lam"])
    width = 1 if dtype == "f64" else 3

    # ---- every document alone (a one-row CSR), against the oracle's b_j
    per_doc = np.zeros(D)
    off_iterate, worst = 0, 0.0
    failures = []
    for i in range(D):
        d1 = stc.DeviceCsr.upload(ctx, corpus.rows([i]), sdt)
        per_doc[i] = h.bound(d1, gamma0=g0[i:i + 1])["corpus_part"]
        d1.free()
        if its[i] is None:  # the empty row and the all-zero row
            assert per_doc[i] == 0.0, (i, per_doc[i])
            continue
        it, win = its[i]
        js = [j for j in win if abs(j - it) <= width]
        if dtype == "f64":
            err = {j: abs(per_doc[i] - win[j][1]) / abs(win[j][1]) for j in js}
            j = min(err, key=err.get)
            worst = max(worst, err[j])
            print(f"doc {i} rows {row_len[i]} it {it} j {j} bound {per_doc[i]:.17g} rel {err[j]:.3e} "
                  f"neighbours {[f'{err[x]:.1e}' for x in js if x != j]}")
            if err[j] > F64_BOUND:
                failures.append((i, int(row_len[i]), it, err))
            off_iterate += j != it
        else:
            lo, hi = min(win[j][1] for j in js), max(win[j][1] for j in js)
            out = max(lo - per_doc[i], per_doc[i] - hi, 0.0) / abs(win[it][1])
            worst = max(worst, out)
            print(f"doc {i} rows {row_len[i]} it {it} bound {per_doc[i]:.9g} in [{lo:.9g}, {hi:.9g}] + {out:.3e}")
            if out > F32_BOUND:
                failures.append((i, int(row_len[i]), it, out))
    print(f"MEASURED {dtype} k={k} {path}: worst per-document relative error {worst:.3e}")
    assert not failures, failures
    assert off_iterate <= 1, off_iterate  # fp64: only a document on the stop rule's boundary may stop elsewhere

    # ---- the whole corpus in one call: partition, long-document list, reduction; and the path it took
    dev = stc.DeviceCsr.upload(ctx, corpus, sdt)
    before = h.counters()["kernels"]
    parts = h.bound(dev, gamma0=g0)
    after = h.counters()["kernels"]
    launched = {f: after[f] - before[f] for f in after}
    print("launched", launched)
    exp = _expected_kernels(dtype, k, path, row_len)
    assert {f: launched[f] for f in exp} == exp, (launched, exp)
    assert all(launched[f] == 0 for f in TEAM_FAMILIES), launched
    if dtype == "f64":
        assert abs(parts["corpus_part"] - per_doc.sum()) <= 1e-12 * abs(per_doc.sum()), (parts, per_doc.sum())
    else:
        live = [x for x in its if x is not None]
        lo = sum(min(b for _, b in win.values()) for _, win in live)
        hi = sum(max(b for _, b in win.values()) for _, win in live)
        mid = abs(sum(win[it][1] for it, win in live))
        assert lo - F32_BOUND * mid <= parts["corpus_part"] <= hi + F32_BOUND * mid, (parts, lo, hi)
    # Σ values as the device holds them (fp32: rounded on upload), summed in fp64 in another order: 1e-12
    tokens = corpus.values.astype(np.float32 if dtype == "f32" else np.float64).astype(np.float64).sum()
    assert abs(parts["token_count"] - tokens) <= 1e-12 * tokens, (parts, tokens)
    assert abs(parts["topics_part"] - case["topics_part"]) <= 1e-10 * abs(case["topics_part"]), (parts, case["topics_part"])

    # ---- topicDistribution on the same corpus and γ₀ (bound off: the wide shapes may take a team kernel)
    theta = h.topic_distribution(dev, gamma0=g0)
    dev.free()
    h.close()
    off_iterate = 0
    for i in range(D):
        if its[i] is None:
            assert np.all(theta[i] == 0), i
            continue
        it, win = its[i]
        js = [j for j in win if abs(j - it) <= width]
        j = min(js, key=lambda x: np.abs(theta[i] - win[x][0] / win[x][0].sum()).sum())
        g = win[j][0]
        off_iterate += j != it
        if dtype == "f64":
            np.testing.assert_allclose(theta[i], g / g.sum(), rtol=1e-7, err_msg=f"doc {i} rows {row_len[i]}")
        else:  # the E-step test's fp32 criteria, on γ = θ·Σγ_j
            got = theta[i] * g.sum()
            l1 = np.abs(got - g).sum()
            assert l1 <= 1e-3 * k + 1e-4 * g.sum(), (i, l1, g.sum())
            big = g >= 1.0
            np.testing.assert_allclose(got[big], g[big], rtol=2e-3, err_msg=f"doc {i} rows {row_len[i]}")
    if dtype == "f64":
        assert off_iterate <= 1, off_iterate
