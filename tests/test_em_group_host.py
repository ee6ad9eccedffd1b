"""CPU: the sharded EM decomposition of stc_em_group, restated in NumPy (tests/em_group_oracle.py), against the
single-graph restatement (tests/em_oracle.py).

Bound 1e-13: the two differ only in the order in which a term's messages are added (per member, then over the
members, against one pass in CSR order); every message is positive, a term here has at most a few hundred
edges, and two such orders differ by a few units of 2^-53 per addition."""
import numpy as np
import pytest

import em_group_oracle as G
import em_oracle as E
from helpers import random_corpus


def filtered_corpus():
    """as test_gpu_em.filtered_corpus: rows 1 and 4 empty, rows 2 and 6 only explicit zeros, zeros inside rows
    0 and 5"""
    import stc

    rows = [([0, 1, 3, 5], [2.0, 0.0, 0.0, 1.0]), ([], []), ([3, 8], [0.0, 0.0]), ([1, 2, 9], [1.0, 3.0, 2.0]),
            ([], []), ([0, 4, 8], [1.0, 2.0, 0.0]), ([0], [0.0]), ([6, 7, 9], [4.0, 1.0, 1.0])]
    return stc.CsrMatrix.from_rows(rows, 16)


def rel_err(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    zero = ref == 0.0
    assert np.all(got[zero] == 0.0)
    return float(np.max(np.abs(got[~zero] - ref[~zero]) / np.abs(ref[~zero]))) if not zero.all() else 0.0


def test_the_filtered_corpus_splits_by_entries_and_bases_count_edges():
    m = filtered_corpus()
    assert m.indptr.tolist() == [0, 4, 4, 6, 9, 9, 12, 13, 16]
    assert G.shard_rows(m.indptr, 2) == [0, 4, 8]
    s = G.shards(m, 2)
    assert [(lo, hi, base) for lo, hi, base, *_ in s] == [(0, 4, 0), (4, 8, 5)]  # 9 entries, 5 of them edges
    assert [x[3].size for x in s] == [5, 5]
    # more members than rows with entries: ranges stay ordered, some are empty
    assert G.shard_rows(m.indptr, 4) == [0, 1, 4, 6, 8]
    assert [base for _, _, base, *_ in G.shards(m, 4)] == [0, 2, 5, 7]
    assert G.shard_rows(np.array([0, 3, 5]), 3) == [0, 1, 2, 2]  # member 2 has no row
    assert G.shard_rows(np.array([0, 0, 0]), 2) == [0, 0, 2]  # no entry at all


def corpora():
    return [("filtered", filtered_corpus()), ("random", random_corpus(np.random.default_rng(11), 40, 300))]


@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("which", [0, 1])
def test_the_sharded_step_is_the_single_step(which, n):
    name, m = corpora()[which]
    k = 5
    D, V = m.shape
    src, term, cnt = E.edges_of(m)
    alpha, eta = E.resolve(k)
    rng = np.random.default_rng(5 + n)
    ndk, nwk = E.mask_state(rng.uniform(0.5, 5.0, (D, k)), rng.uniform(0.5, 5.0, (V, k)), src, term)
    nk = nwk.sum(axis=0)
    ref = E.step(ndk, nwk, nk, src, term, cnt, alpha, eta)
    got = G.step(m, n, ndk, nwk, nk, alpha, eta)
    errs = [rel_err(g, r) for g, r in zip(got, ref)]
    print(f"{name}, {n} members: rel err N_dk {errs[0]:.2e} N_wk {errs[1]:.2e} N_k {errs[2]:.2e}")
    assert errs[0] == 0.0  # a document lies in one shard: the same additions in the same order
    assert max(errs) <= 1e-13
    # a second step from the sharded state stays on the single one
    ref2 = E.step(*ref, src, term, cnt, alpha, eta)
    got2 = G.step(m, n, *got, alpha, eta)
    assert max(rel_err(g, r) for g, r in zip(got2, ref2)) <= 1e-13


@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("which", [0, 1])
def test_the_sharded_initial_state_uses_global_edge_positions(which, n):
    name, m = corpora()[which]
    k = 5
    D, V = m.shape
    src, term, cnt = E.edges_of(m)
    ref = E.init_state(77, src, term, cnt, D, V, k)
    got = G.init_state(77, m, n, k)
    assert np.array_equal(got[0], ref[0])
    assert max(rel_err(g, r) for g, r in zip(got, ref)) <= 1e-13
    assert max(E.mass_identities(*got, src, term, cnt)) <= 1e-13


def test_the_python_surface_declares_the_group():
    """no GPU needed: the header's stc_em_group_* symbols all have a ctypes signature, and the classes that use
    them exist with EmHandle's methods"""
    import os
    import re

    import stc

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = set(re.findall(r"^int\s+(stc_em_group_\w+)\s*\(", open(os.path.join(root, "include", "stc.h")).read(), re.M))
    assert len(names) == 13 and names <= set(stc._lib.SIGNATURES)
    for meth in ("init_random", "set_state", "state", "concentrations", "next", "log_likelihood", "topic_assignments",
                 "close", "members", "transport", "synchronize"):
        assert callable(getattr(stc.EmGroup, meth))
    assert stc.MllibLDA(devices=[0, 0]).devices == [0, 0] and stc.MllibLDA().devices is None
    assert stc.MllibLDA().setDevices([0, 1]).devices == [0, 1]


def test_a_base_that_counts_entries_is_caught():
    """what the check above is for: with indptr[row0] (9) as member 1's base instead of its edge count (5), the
    filtered corpus's initial state is another one"""
    m = filtered_corpus()
    k = 5
    src, term, cnt = E.edges_of(m)
    g, _ = E.init_gamma(77, 14, k)
    wrong = np.concatenate([g[:5], g[9:14]])  # keys 0..4 and 9..13
    ndk_wrong = E._scatter(src, cnt[:, None] * wrong, m.num_rows)
    assert not np.array_equal(ndk_wrong, G.init_state(77, m, 2, k)[0])
