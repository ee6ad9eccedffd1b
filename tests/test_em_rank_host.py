"""CPU: the ranked-query surface of the EM optimizer (stc_em_describe / _top_documents / _top_topics and their
stc_em_group_* forms) is declared, exported and guarded before any GPU call, and the NumPy restatement
(tests/em_rank_oracle.py) agrees with a brute-force sort on a case with planted ties."""
import ctypes
import os
import re

import numpy as np

import em_rank_oracle as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("stc_em_describe", "stc_em_top_documents", "stc_em_top_topics", "stc_em_group_describe",
       "stc_em_group_top_documents", "stc_em_group_top_topics")


def test_the_header_the_signatures_and_the_library_have_the_entry_points():
    import stc
    from stc import _lib

    header = open(os.path.join(ROOT, "include", "stc.h")).read()
    lib = stc.load()
    for name in NEW:
        assert re.search(r"^\s*int\s+" + name + r"\s*\(", header, re.M), name
        assert name in _lib.SIGNATURES, name
        f = getattr(lib, name)
        assert f.restype is ctypes.c_int and list(f.argtypes) == _lib.SIGNATURES[name][1]
    # a group form takes what the single form takes
    for name in NEW[:3]:
        assert _lib.SIGNATURES[name][1] == _lib.SIGNATURES[name.replace("stc_em_", "stc_em_group_")][1]
    assert lib.stc_abi_version() == 2 and re.search(r"#define\s+STC_ABI_VERSION\s+2\b", header)
    # the header states the tie rule, the sum order and what is unpinned against Spark
    for phrase in ("ascending index", "sequentially in ascending j", "spark-mllib 2.4.3", "BoundedPriorityQueue"):
        assert phrase in header, phrase


def test_null_handles_are_refused_before_any_device_call():
    import stc

    lib = stc.load()
    i32 = (ctypes.c_int32 * 4)()
    i64 = (ctypes.c_int64 * 4)()
    dbl = (ctypes.c_double * 4)()
    n = ctypes.c_int64(-1)
    for prefix in ("stc_em_", "stc_em_group_"):
        assert getattr(lib, prefix + "describe")(None, 1, i32, dbl) == stc.STC_ERR_INVALID_ARG
        assert getattr(lib, prefix + "top_documents")(None, 1, ctypes.byref(n), i64, dbl) == stc.STC_ERR_INVALID_ARG
        assert getattr(lib, prefix + "top_topics")(None, 1, i32, dbl) == stc.STC_ERR_INVALID_ARG
    assert n.value == -1


def test_the_oracle_agrees_with_a_brute_force_sort_on_planted_ties():
    m = np.array([[2.0, 1.0, 1.0],
                  [1.0, 2.0, 1.0],
                  [2.0, 1.0, 1.0],   # row 0 again
                  [0.0, 0.0, 0.0],   # no vertex
                  [4.0, 2.0, 2.0],   # row 0 doubled: the same weights from other counts
                  [1.0, 1.0, 2.0],
                  [3.0, 3.0, 3.0]])
    D, k = m.shape
    vertex = np.array([1, 1, 1, 0, 1, 1, 1], bool)
    # describe: the matrix read as N_wk, every N
    nk = m.sum(axis=0)
    for n in range(1, D + 2):
        idx, w = R.describe(m, nk, n)
        for t in range(k):
            brute = sorted(range(D), key=lambda r: (-m[r, t], r))[:n]
            assert idx[t].tolist() == brute and w[t].tolist() == [m[r, t] / nk[t] for r in brute]
    assert R.describe(m, nk, 7)[0][0].tolist() == [4, 6, 0, 2, 1, 5, 3]
    # top documents: sequential row sums, vertices only, rows 0 / 2 / 4 tie at 0.5 and rank by row
    wts = [[m[r, t] / ((m[r, 0] + m[r, 1]) + m[r, 2]) if vertex[r] else None for t in range(k)] for r in range(D)]
    for n in range(1, D + 2):
        rows, w, undecided, _ = R.top_documents(m, vertex, n)
        assert rows.shape == (k, min(n, 6))
        for t in range(k):
            brute = sorted([r for r in range(D) if vertex[r]], key=lambda r: (-wts[r][t], r))[:n]
            assert rows[t].tolist() == brute and w[t].tolist() == [wts[r][t] for r in brute]
    rows, _, undecided, _ = R.top_documents(m, vertex, 3)
    assert rows[0].tolist() == [0, 2, 4]
    # equal weights from rows that are not bitwise equal: topic 0 rows 2 | 4, topic 2 rows 0 | 1 (across the cut)
    assert undecided == 2
    assert R.top_documents(m, vertex, 2)[2] == 1  # rows 2 | 4 are the N-th and (N+1)-th neighbours of topic 0
    assert R.top_documents(m, vertex, 1)[2] == 0  # rows 0 | 2 are bitwise equal
    # top topics: by the count, ties to the smaller topic; the row without a vertex: 0 … N−1 with weight 0
    for n in range(1, k + 2):
        idx, w = R.top_topics(m, n)
        for r in range(D):
            brute = sorted(range(k), key=lambda t: (-m[r, t], t))[:n]
            assert idx[r].tolist() == brute
            assert w[r].tolist() == [wts[r][t] if vertex[r] else 0.0 for t in brute]
    assert R.top_topics(m, 3)[0][[0, 3, 5]].tolist() == [[0, 1, 2], [0, 1, 2], [2, 0, 1]]
    assert R.bound(5) == 12 * 2.0 ** -53
