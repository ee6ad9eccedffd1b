"""CPU: tests/score_oracle.py against the reference's recorded run (tests/golden/en_report.json, written by
LDALoader.scala: main topics, books per topic, "Book most important words").

Inputs: the books' term counts (en_idf.npz ``tf``), the saved model's topicsMatrix (en_topics.npz), the vocabulary
(en_vocab.txt) and the recorded θ of the same run (en_topicdist.json).  The word lists' allowance: Spark's order
among equal counts is the book's local vocabulary order, which nothing here pins, and a tie at the 100-entry cut
changes membership — so with c100 the book's 100th-largest count, both lists are compared after dropping the
entries whose count equals c100, as sequences of counts.  Without the allowance 40 of the 51 lists are equal
term for term.
"""
import os

import numpy as np
import pytest

import score_oracle as S
from helpers import GOLDEN, golden_json, golden_npz


@pytest.fixture(scope="module")
def recorded():
    rep = golden_json("en_report.json")
    meta = golden_json("en_topicdist.json")
    tf = golden_npz("en_idf.npz")
    lam = golden_npz("en_topics.npz")["nwk"]
    with open(os.path.join(GOLDEN, "en_vocab.txt"), encoding="utf-8") as f:
        vocab = f.read().split("\n")[:-1]
    th = np.array([[float(x) for x in r] for r in meta[rep["run"]]])
    assert [b["name"] for b in rep["books"]] == meta["books"] and len(vocab) == lam.shape[0]
    return rep, th, tf, lam, vocab


def test_main_topics_and_counts(recorded):
    rep, th, _, _, _ = recorded
    g, s = S.build(th)
    topic, weight, counts = S.main_topics(g, s)
    assert topic.tolist() == [b["main_topic"] for b in rep["books"]]
    assert counts.tolist() == rep["books_per_topic"] == [14, 16, 2, 9, 10]
    for d, b in enumerate(rep["books"]):  # θ of a recorded row sums to 1 ± a few ulp
        assert abs(weight[d] - float(b["main_topic_weight"])) < 1e-15
    gap = np.sort(th, axis=1)
    assert (gap[:, -1] - gap[:, -2]).min() > 3e-3  # far above the device θ tolerances (2e-6 / 1e-5)
    indptr, rows = S.members(topic, th.shape[1])
    assert np.diff(indptr).tolist() == rep["books_per_topic"]
    for t in range(th.shape[1]):
        m = rows[indptr[t]:indptr[t + 1]]
        assert np.all(np.diff(m) > 0) and np.all(topic[m] == t)


def test_word_lists(recorded):
    rep, th, tf, lam, vocab = recorded
    indptr, indices, counts = tf["indptr"], tf["indices"], tf["tf"].astype(np.float64)
    topic = np.array([b["main_topic"] for b in rep["books"]], np.int32)
    sets = S.topic_sets(lam, rep["topic_terms"])
    idx, val, n = S.important_terms(indptr, indices, counts, topic, sets, rep["doc_terms"], rep["n"])
    exact = 0
    for d, b in enumerate(rep["books"]):
        row_i, row_c = indices[indptr[d]:indptr[d + 1]], counts[indptr[d]:indptr[d + 1]]
        count_of = {vocab[i]: c for i, c in zip(row_i[::-1], row_c[::-1])}
        got = [vocab[i] for i in idx[d, :n[d]]]
        exact += got == b["words"]
        c100 = np.sort(row_c)[::-1][min(rep["doc_terms"], row_c.size) - 1]
        want_c = [count_of[w] for w in b["words"] if count_of[w] != c100]
        got_c = [c for c in val[d, :n[d]] if c != c100]
        assert got_c == want_c, (d, b["name"], got, b["words"])
        assert np.all(idx[d, n[d]:] == -1) and np.all(val[d, n[d]:] == 0.0)
    print("word lists equal term for term:", exact, "of", len(rep["books"]))
    assert exact == 40


def test_oracle_rules_on_planted_values():
    g, s = S.build([[1, 3, 3], [2, 2, 2], [0, 0, 0], [5, 1, 1], [4, 4, 1]], empty=[0, 0, 0, 1, 0])
    assert s.tolist() == [7, 6, 0, -1, 9]
    topic, weight, counts = S.main_topics(g, s)
    assert topic.tolist() == [2, 2, 2, -1, 1] and counts.tolist() == [0, 1, 3]
    assert weight.tolist() == [3 / 7, 2 / 6, 0.0, 0.0, 4 / 9]
    indptr, rows = S.members(topic, 3)
    assert indptr.tolist() == [0, 0, 1, 4] and rows.tolist() == [4, 0, 1, 2]
    n, r, w = S.top_documents(g, s, 10)
    assert n == 4 and r[0].tolist() == [4, 1, 0, 2]
    ti, tw = S.top_topics(g, s, 2)
    assert ti[3].tolist() == [0, 1] and tw[3].tolist() == [0.0, 0.0] and ti[0].tolist() == [1, 2]
    # important terms: ties by term index whatever the entries' order; −0 reads as 0; negatives last
    ip = np.array([0, 6, 6])
    ix = np.array([9, 2, 7, 4, 0, 5], np.int32)
    v = np.array([2.0, 2.0, -0.0, 3.0, -1.0, 0.0])
    assert ix[S.doc_order(ix, v, 6)].tolist() == [4, 2, 9, 5, 7, 0]
    sets = np.zeros((2, 10), bool)
    sets[1, [9, 5, 0, 4]] = True
    i, x, m = S.important_terms(ip, ix, v, [1, 1], sets, 4, 3)
    assert i.tolist() == [[4, 9, 5], [-1, -1, -1]] and x.tolist() == [[3.0, 2.0, 0.0], [0, 0, 0]] and m.tolist() == [3, 0]
