"""CPU: the topicAssignments restatement (tests/em_assign_oracle.py) against a plain double loop, and the C ABI
entry stc_em_topic_assignments in the loaded library."""
import ctypes

import numpy as np

import em_assign_oracle as A
import em_oracle as E


def filtered_corpus():
    """the shape of test_gpu_em.filtered_corpus: 8 documents, V = 16, rows 1 and 4 empty, rows 2 and 6 only
    explicit zeros, zeros inside rows 0 and 5"""
    import stc

    rows = [([0, 1, 3, 5], [2.0, 0.0, 0.0, 1.0]), ([], []), ([3, 8], [0.0, 0.0]), ([1, 2, 9], [1.0, 3.0, 2.0]),
            ([], []), ([0, 4, 8], [1.0, 2.0, 0.0]), ([0], [0.0]), ([6, 7, 9], [4.0, 1.0, 1.0])]
    return stc.CsrMatrix.from_rows(rows, 16)


def test_oracle_equals_a_double_loop():
    corpus, k = filtered_corpus(), 5
    D, V = corpus.shape
    src, term, cnt = E.edges_of(corpus)
    assert (D, V, src.size) == (8, 16, 10)
    alpha, eta = E.resolve(k)
    rng = np.random.default_rng(11)
    ndk, nwk = E.mask_state(rng.uniform(0.5, 5.0, (D, k)), rng.uniform(0.5, 5.0, (V, k)), src, term)
    nk = nwk.sum(axis=0)
    topic, margin = A.assignments(ndk, nwk, nk, src, term, alpha, eta)
    assert topic.shape == (10,) and margin.shape == (10,) and np.all(margin > 0.0)
    for e in range(src.size):
        best, bj, second = -1.0, -1, -1.0
        for j in range(k):
            f = (nwk[term[e], j] + (eta - 1.0)) * (ndk[src[e], j] + (alpha - 1.0)) / (nk[j] + V * (eta - 1.0))
            if f > best:  # strict: the first maximum
                best, bj, second = f, j, best
            elif f > second:
                second = f
        assert topic[e] == bj and margin[e] == (best - second) / best
    # an exact tie: the first index, margin 0
    ndk[:, 3], nwk[:, 3] = ndk[:, 1] + 50.0, nwk[:, 1] + 50.0
    ndk[:, 1], nwk[:, 1] = ndk[:, 3], nwk[:, 3]
    ndk, nwk = E.mask_state(ndk, nwk, src, term)
    topic, margin = A.assignments(ndk, nwk, nwk.sum(axis=0), src, term, alpha, eta)
    assert np.all(topic == 1) and np.all(margin == 0.0)


def test_library_has_the_entry_point():
    import stc
    from stc import _lib

    lib = stc.load()
    f = lib.stc_em_topic_assignments
    assert _lib.SIGNATURES["stc_em_topic_assignments"] == (
        ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32),
                       ctypes.POINTER(ctypes.c_int32)])
    assert f.restype is ctypes.c_int and list(f.argtypes) == _lib.SIGNATURES["stc_em_topic_assignments"][1]
    rc = f(None, None, None, None)
    assert rc == lib.stc_em_log_likelihood(None, None, None) == stc.STC_ERR_INVALID_ARG
    assert lib.stc_last_error()
    assert callable(stc.EmHandle.topic_assignments) and callable(stc.DistributedLDAModel.topicAssignments)
