"""CPU: stc_coherence (host arithmetic of the topic-coherence measures) against tests/coherence_oracle.py, the hand
example of its definition, the reference's EN model on its 51 books, the skip rules and the error returns; and the
plumbing of the new entry points (header, library, JNI, Python).

Tolerance for a coherence value: |got − oracle| <= 1e-12 · max(1, Σ|pair value|).  Both sides add the same pair
values in the same order; what can differ is each log (a few ulp between libm and Python's), and the sum's own
rounding is at most 2016 · 2^-53 ≈ 2.2e-13 of Σ|pair value|.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import coherence_oracle as CO
from helpers import GOLDEN, golden_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_MODEL = os.path.join(GOLDEN, "LdaModel_EN_1591049082850")
UMASS, NPMI = 0, 1
CODE = {"umass": UMASS, "npmi": NPMI}


def _raw(df, codf, n_docs, measure, eps=1.0, null=()):
    """stc_coherence through ctypes: (status, topic float64[k], pairs int32[k])"""
    import stc

    lib = stc.load()
    df = np.ascontiguousarray(df, np.int64)
    codf = np.ascontiguousarray(codf, np.int64)
    k, n = df.shape
    out, pairs = np.full(k, np.nan), np.full(k, -7, np.int32)
    p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    rc = lib.stc_coherence(None if "df" in null else p64(df), None if "codf" in null else p64(codf), k, n, n_docs, measure,
                           eps, out.ctypes.data_as(C.POINTER(C.c_double)), pairs.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, out, pairs


def _close(got, exp, mag):
    return np.all(np.abs(got - exp) <= 1e-12 * np.maximum(1.0, mag))


def _counts(pairs_of, df):
    """k = 1 counts from {(i, j): codf} and a df list"""
    n = len(df)
    codf = np.zeros((1, n, n), np.int64)
    for (i, j), c in pairs_of.items():
        codf[0, i, j] = codf[0, j, i] = c
    for i in range(n):
        codf[0, i, i] = df[i]
    return np.asarray([df], np.int64), codf


def test_hand_example():
    """documents {a, b}, {a, b, c}, {a}, {c}; list [a, b, c]"""
    csr = (np.array([0, 2, 5, 6, 7]), np.array([0, 1, 0, 1, 2, 0, 2]), np.ones(7), 3)
    df, codf, D = CO.cooccurrence(csr, np.array([[0, 1, 2]]))
    assert D == 4 and df.tolist() == [[3, 2, 2]]
    assert codf[0].tolist() == [[3, 2, 1], [2, 2, 1], [1, 1, 2]]
    umass = math.log(3 / 3) + math.log(2 / 3) + math.log(2 / 2)
    npmi = (math.log(2 * 4 / (2 * 3)) / -math.log(2 / 4) + math.log(1 * 4 / (2 * 3)) / -math.log(1 / 4)
            + math.log(1 * 4 / (2 * 2)) / -math.log(1 / 4)) / 3
    assert abs(umass - -0.4054651081) < 1e-9 and abs(npmi - 0.0408520830) < 1e-9
    for name, exp in (("umass", umass), ("npmi", npmi)):
        o, op, mag = CO.coherence(df, codf, D, name, 1.0)
        rc, g, gp = _raw(df, codf, D, CODE[name], 1.0)
        assert rc == 0 and op.tolist() == [3] and gp.tolist() == [3]
        assert abs(o[0] - exp) <= 1e-12 and abs(g[0] - exp) <= 1e-12, (name, o, g, exp)


@pytest.fixture(scope="module")
def en():
    tf = golden_npz("en_idf.npz")
    nwk = golden_npz("en_topics.npz")["nwk"]
    csr = (tf["indptr"], tf["indices"], tf["tfidf"], int(tf["vocab_size"]))
    return csr, nwk


@pytest.mark.parametrize("n,pairs", [(10, 45), (20, 190), (64, 2016)])
def test_en_golden(en, n, pairs):
    """the reference's EN model (top terms by n_wk descending, index ascending) on its 51 books (TF·IDF values)"""
    csr, nwk = en
    terms = CO.top_terms(nwk, n)
    df, codf, D = CO.cooccurrence(csr, terms)
    assert D == 51 and df.min() >= 2 and df.max() <= 43
    off = ~np.eye(n, dtype=bool)
    assert codf[:, off].max() < 51 and np.array_equal(codf, codf.transpose(0, 2, 1))
    for name in ("umass", "npmi"):
        o, op, mag = CO.coherence(df, codf, D, name, 1.0)
        rc, g, gp = _raw(df, codf, D, CODE[name], 1.0)
        assert rc == 0 and op.tolist() == [pairs] * 5 and gp.tolist() == [pairs] * 5
        assert _close(g, o, mag), (name, g - o, mag)
        if n == 10:
            assert abs(o[3] - (-22.1393 if name == "umass" else 0.5106)) < 1e-4, (name, o[3])


def test_python_wrapper_matches_raw(en):
    import stc

    csr, nwk = en
    df, codf, D = CO.cooccurrence(csr, CO.top_terms(nwk, 10))
    for name in ("umass", "npmi"):
        v, p = stc.coherence(df, codf, D, measure=name)
        _, g, gp = _raw(df, codf, D, CODE[name], 1.0)
        assert v.dtype == np.float64 and p.dtype == np.int32
        assert np.array_equal(v, g) and np.array_equal(p, gp)
    assert np.array_equal(stc.coherence(df, codf, D)[0], _raw(df, codf, D, UMASS, 1.0)[1])  # the defaults: UMass, eps 1
    with pytest.raises(ValueError):
        stc.coherence(df, codf, D, measure="c_v")
    with pytest.raises(ValueError):
        stc.coherence(df, codf[:, :, :5], D)


def test_skipped_slots_reduce_pairs():
    """an absent term (df 0) and a −1 slot (all counts 0) are skipped; a list without a countable pair gives 0, 0"""
    csr = (np.array([0, 2, 5, 6, 7]), np.array([0, 1, 0, 1, 2, 0, 2]), np.ones(7), 5)
    terms = np.array([[0, 3, 1, 2], [0, -1, 1, 2], [3, 0, -1, 4], [-1, -1, -1, -1]])  # term 3, 4: in no document
    df, codf, D = CO.cooccurrence(csr, terms)
    assert df.tolist() == [[3, 0, 2, 2], [3, 0, 2, 2], [0, 3, 0, 0], [0, 0, 0, 0]]
    for name in ("umass", "npmi"):
        o, op, mag = CO.coherence(df, codf, D, name, 1.0)
        rc, g, gp = _raw(df, codf, D, CODE[name], 1.0)
        assert rc == 0 and gp.tolist() == [3, 3, 0, 0] and op.tolist() == [3, 3, 0, 0]
        assert _close(g, o, mag)
        assert g[2] == 0.0 and g[3] == 0.0
        base = CO.coherence(*CO.cooccurrence(csr, np.array([[0, 1, 2]])), name, 1.0)[0][0]
        assert abs(g[0] - base) <= 1e-12 and abs(g[1] - base) <= 1e-12  # the skipped slot changes nothing else


def test_npmi_edges():
    """c = 0 → −1, c = D → 0"""
    df, codf = _counts({(0, 1): 0}, [2, 3])
    assert _raw(df, codf, 5, NPMI)[1][0] == -1.0
    df, codf = _counts({(0, 1): 5}, [5, 5])
    rc, g, p = _raw(df, codf, 5, NPMI)
    assert rc == 0 and g[0] == 0.0 and p[0] == 1
    df, codf = _counts({(0, 1): 0, (0, 2): 4, (1, 2): 2}, [4, 2, 4])  # −1, 0 (c = D) and one ordinary pair
    rc, g, p = _raw(df, codf, 4, NPMI)
    exp = (-1.0 + 0.0 + math.log(2 * 4 / (4 * 2)) / -math.log(2 / 4)) / 3
    assert rc == 0 and p[0] == 3 and abs(g[0] - exp) <= 1e-12
    o, _, mag = CO.coherence(df, codf, 4, "npmi")
    assert _close(g, o, mag)
    assert _raw(df, codf, 4, NPMI, eps=-3.0)[0] == 0  # eps is ignored


def test_umass_eps():
    df, codf = _counts({(0, 1): 0}, [2, 3])
    rc, g, _ = _raw(df, codf, 9, UMASS, eps=0.25)
    assert rc == 0 and abs(g[0] - math.log(0.25 / 2)) <= 1e-12  # the denominator is df of the earlier slot l


def test_error_returns():
    import stc

    df, codf = _counts({(0, 1): 1}, [2, 3])
    inv = stc.STC_ERR_INVALID_ARG
    assert _raw(df, codf, 5, UMASS, eps=0.0)[0] == inv
    assert _raw(df, codf, 5, UMASS, eps=-1.0)[0] == inv
    assert _raw(df, codf, 5, 2)[0] == inv and _raw(df, codf, 5, -1)[0] == inv
    assert _raw(df, codf, 0, NPMI)[0] == inv and _raw(df, codf, -4, UMASS)[0] == inv
    bad = df.copy()
    bad[0, 1] = -1
    assert _raw(bad, codf, 5, UMASS)[0] == inv
    bad = codf.copy()
    bad[0, 1, 0] = -2
    assert _raw(df, bad, 5, NPMI)[0] == inv
    assert _raw(df, codf, 5, UMASS, null=("df",))[0] == inv
    assert _raw(df, codf, 5, UMASS, null=("codf",))[0] == inv
    assert b"coherence" in stc.load().stc_last_error()
    with pytest.raises(stc.StcIllegalArgument):
        stc.coherence(df, codf, 5, eps=0.0)


def test_plumbing():
    import stc

    hdr = open(os.path.join(ROOT, "include", "stc.h")).read()
    lib = stc.load()
    for sym in ("stc_term_cooccurrence", "stc_coherence"):
        assert re.search(r"^\s*int\s+%s\s*\(" % sym, hdr, re.M), sym
        assert hasattr(lib, sym), sym
    assert "STC_COH_UMASS = 0" in hdr and "STC_COH_NPMI = 1" in hdr
    assert lib.stc_abi_version() == 2
    jni = open(os.path.join(ROOT, "jni", "stcjni.c")).read()
    java = open(os.path.join(ROOT, "scala", "org", "apache", "spark", "mllib", "clustering", "StcNative.java")).read()
    for name in ("termCooccurrence", "coherence"):
        assert "JNICALL FN(%s)" % name in jni, name
        assert re.search(r"public static native \S+ %s\(" % name, java), name
    assert callable(stc.term_cooccurrence) and callable(stc.coherence)


def test_top_n_limits():
    """topN outside 2 … 64 raises before anything touches a device"""
    import stc

    model = stc.DistributedLDAModel.load(REF_MODEL)
    for bad in (65, 1, 0):
        with pytest.raises(ValueError):
            model.topicCoherence(topN=bad)
        with pytest.raises(ValueError):
            stc.LDAModel.topicCoherence(None, None, topN=bad)
