"""stc_lda_describe on the column selection (csrc/rank.hip) at the smallest shapes where a selection can go wrong.

V = 1600 is three full 512-row tiles of k_rank_hist / k_rank_collect and a 64-row rest; k = 5 is one narrow topic
group, k = 33 leaves a second group of width 1, k = 100 is the headline's three full groups and one of 4.  Two λ,
both put in with set_topics:
  ties      integers in {1, 2, 3}: hundreds of exact ties through every cut, ranked by ascending term
  distinct  per topic its own permutation of 1 … V, divided by 1024: all values of a column distinct
In both every partial sum of a column is a multiple of 2^-10 below 2^21, so the column sum is exact in fp64
whatever the order it is added in, and the expected weight is lam[idx, t] / lam[:, t].sum() bit for bit — the
correctly rounded fp64 division the device does — with no recorded fixture.
max_terms: 1 and 10; 1536 and 1537 (1536 + the selection's slack of 512 is exactly 2048, the last candidate list
sorted in LDS; 1537 is the first one sorted in global memory); 1600 = V and 1605, past V.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

V = 1600
K = (5, 33, 100)
MAX_TERMS = (1, 10, 1536, 1537, 1600, 1605)
KINDS = ("ties", "distinct")


def _lam(kind, k):
    rng = np.random.default_rng(500 + k)
    if kind == "ties":
        return rng.integers(1, 4, size=(V, k)).astype(np.float64)
    return np.stack([rng.permutation(V) + 1 for _ in range(k)], axis=1) / 1024.0


def _check(describe, oracle, lam, max_terms):
    """shape, the oracle's indices, bitwise weights, and a second call's bytes"""
    k = lam.shape[1]
    idx, w = describe(max_terms)
    n = min(max_terms, V)
    assert idx.shape == w.shape == (k, n)
    idx_o, _ = oracle.describe_topics(lam, max_terms)
    assert np.array_equal(idx, idx_o), max_terms
    want = lam[idx_o, np.arange(k)[:, None]] / lam.sum(axis=0)[:, None]
    assert np.array_equal(np.ascontiguousarray(w).view(np.uint64), want.view(np.uint64)), max_terms
    idx2, w2 = describe(max_terms)
    assert idx2.tobytes() == idx.tobytes() and w2.tobytes() == w.tobytes(), max_terms


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", K)
def test_describe_selection(ctx, oracle, k, kind):
    import stc

    lam = _lam(kind, k)
    assert np.all(lam.sum(axis=0) == np.cumsum(lam, axis=0)[-1])  # the column sum does not depend on the order
    h = stc.LdaHandle(ctx, k, V, dtype="f64")
    h.set_topics(lam)
    for max_terms in MAX_TERMS:
        _check(h.describe, oracle, lam, max_terms)
    h.close()


@pytest.mark.parametrize("kind", KINDS)
def test_describe_selection_group(ctx, oracle, kind):
    """the same λ through a two-member group on one device: member 0 describes the gathered λ"""
    import stc

    lam = _lam(kind, 33)
    with stc.LdaGroup([0, 0], 33, V, dtype="f64") as g:
        g.set_topics(lam)
        for max_terms in MAX_TERMS:
            _check(g.describe, oracle, lam, max_terms)
