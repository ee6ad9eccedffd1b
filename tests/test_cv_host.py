"""CPU: CountVectorizer's host side — the Python surface and its validation, the C ABI's declarations, the
vocabulary file format, and the restatement (tests/cv_oracle.py) against the reference's own artefacts: the
51 books' term frequencies recovered from the saved EN model (en_idf.npz) and that model's vocabulary
(en_vocab.txt), which pin "by total count, descending" and the vocabulary-indexed counts."""
import os
import re

import numpy as np
import pytest

import cv_oracle
from helpers import GOLDEN, golden_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CV_SYMBOLS = ("stc_cv_fit", "stc_cv_fit_tokens", "stc_cv_from_vocabulary", "stc_cv_shape", "stc_cv_get",
              "stc_cv_index_of", "stc_cv_transform_dev", "stc_cv_transform_tokens", "stc_cv_free")


def reference_books():
    """(tf fixture, vocabulary list[str], the 51 token streams: term i repeated tf times, in index order)"""
    tf = golden_npz("en_idf.npz")
    vocab = open(os.path.join(GOLDEN, "en_vocab.txt"), encoding="utf-8").read().split("\n")[:-1]
    assert len(vocab) == int(tf["vocab_size"])
    ip, ix, cnt = tf["indptr"], tf["indices"], tf["tf"]
    docs = [[vocab[i] for i, c in zip(ix[ip[d]:ip[d + 1]], cnt[ip[d]:ip[d + 1]]) for _ in range(int(c))]
            for d in range(ip.size - 1)]
    return tf, vocab, docs


def reference_counts(tf):
    """the reference's total count of every vocabulary term, in vocabulary order"""
    total = np.zeros(int(tf["vocab_size"]), np.int64)
    np.add.at(total, tf["indices"], tf["tf"].astype(np.int64))
    return total


def assert_same_vocabulary_up_to_ties(got_terms, got_counts, ref_terms, ref_counts):
    """equal count sequences, and for every count value the same set of terms"""
    assert np.array_equal(got_counts, ref_counts)
    bounds = np.flatnonzero(np.diff(ref_counts)) + 1
    for s, e in zip(np.r_[0, bounds], np.r_[bounds, ref_counts.size]):
        assert set(got_terms[s:e]) == set(ref_terms[s:e]), int(ref_counts[s])


def test_surface_and_parameter_validation():
    import stc

    cv = stc.CountVectorizer()
    assert (cv.getVocabSize(), cv.getMinDF(), cv.getMaxDF(), cv.getMinTF(), cv.getBinary()) == \
        (1 << 18, 1.0, float(2 ** 63 - 1), 1.0, False)
    assert cv.setVocabSize(10).setMinDF(2).setMaxDF(5).setMinTF(0.5).setBinary(True) is cv
    assert (cv.vocabSize, cv.minDF, cv.maxDF, cv.minTF, cv.binary) == (10, 2.0, 5.0, 0.5, True)
    for kw in ({"vocabSize": 0}, {"vocabSize": -3}, {"minDF": -1.0}, {"maxDF": -0.5}, {"minTF": -1.0},
               {"minDF": 3, "maxDF": 2}, {"minDF": float("nan")}):
        with pytest.raises(ValueError):
            stc.CountVectorizer(**kw)
    with pytest.raises(ValueError):
        stc.CountVectorizer(minDF=4).setMaxDF(3)
    with pytest.raises(ValueError):
        stc.CountVectorizer(maxDF=3).setMinDF(4)
    stc.CountVectorizer(minDF=0.5, maxDF=3)  # a fraction against a count: decided by the corpus size
    for name in ("from_vocabulary", "vocabulary", "termCounts", "docFreq", "indexOf", "indices_of", "transform",
                 "transform_device", "transform_tokens_device", "free"):
        assert hasattr(stc.CountVectorizerModel, name), name
    with pytest.raises(ValueError):
        stc.CountVectorizerModel.from_vocabulary([])


def test_header_declares_and_library_exports_every_cv_symbol():
    import stc
    from stc import _lib

    txt = open(os.path.join(ROOT, "include", "stc.h")).read()
    declared = set(re.findall(r"^\s*int\s+(stc_cv_\w+)\s*\(", txt, re.M))
    assert declared == set(CV_SYMBOLS)
    lib = stc.load()
    for s in CV_SYMBOLS:
        assert hasattr(lib, s) and s in _lib.SIGNATURES, s
    assert "typedef struct stc_cvm stc_cvm;" in txt
    assert lib.stc_abi_version() == 2  # additive: the ABI version stays


def test_vocabulary_file_round_trip(tmp_path):
    import stc

    terms = ["the", "ж", "a b", "", "x"]
    p = tmp_path / "vocab"
    stc.io.save_vocabulary(p, terms)
    assert open(p, encoding="utf-8").read() == "the,ж,a b,,x"  # vocabArray.mkString(",")
    assert stc.io.load_vocabulary(p) == terms
    for bad in ("a,b", "line\nbreak", "cr\r"):
        with pytest.raises(ValueError):
            stc.io.save_vocabulary(tmp_path / "bad", ["ok", bad])
    # Java's split(",") drops trailing empty strings
    stc.io.save_vocabulary(p, ["a", "", ""])
    assert stc.io.load_vocabulary(p) == ["a"]


def test_oracle_small_cases():
    docs = [["b", "a", "b", "c"], [], ["a", "c", "c", "d"], ["é", "z"]]
    vocab, cnt, df = cv_oracle.fit(docs)
    # counts 2,2,3 → c first; ties by unsigned bytes: "z" (0x7A) before "é" (0xC3 0xA9)
    assert vocab == [b"c", b"a", b"b", b"d", b"z", "é".encode()]
    assert cnt.tolist() == [3, 2, 2, 1, 1, 1] and df.tolist() == [2, 2, 1, 1, 1, 1]
    assert cv_oracle.fit(docs, vocabSize=2)[0] == [b"c", b"a"]
    assert cv_oracle.fit(docs, minDF=2)[0] == [b"c", b"a"]
    assert cv_oracle.fit(docs, minDF=0.5)[0] == [b"c", b"a"]  # 0.5 · 4 documents (the empty one counts)
    assert cv_oracle.fit(docs, maxDF=1)[0] == [b"b", b"d", b"z", "é".encode()]
    with pytest.raises(ValueError, match="Lower minDF"):
        cv_oracle.fit(docs, minDF=3)
    with pytest.raises(ValueError):
        cv_oracle.fit(docs, minDF=3, maxDF=2)
    ip, ix, vv = cv_oracle.transform(docs, vocab[:3], minTF=0.5)
    # thresholds 2, 0, 2, 1 (every token counts, "d" / "é" / "z" outside the vocabulary too): the counts of 1 go
    assert ip.tolist() == [0, 1, 1, 2, 2] and ix.tolist() == [2, 0] and vv.tolist() == [2.0, 2.0]
    ip, ix, vv = cv_oracle.transform(docs, vocab[:3], binary=True)
    assert ip.tolist() == [0, 3, 3, 5, 5] and ix.tolist() == [0, 1, 2, 0, 1] and vv.tolist() == [1.0] * 5
    assert cv_oracle.indices_of(["c", "q", ""], vocab).tolist() == [0, -1, -1]
    with pytest.raises(ValueError):
        cv_oracle.index_map(["a", "b", "a"])


@pytest.fixture(scope="module")
def books():
    return reference_books()


def test_restatement_fit_reproduces_the_reference_vocabulary(books):
    tf, vocab, docs = books
    assert sum(len(d) for d in docs) == 2_147_864 and max(len(d) for d in docs) == 261_417
    ref = reference_counts(tf)
    assert np.all(np.diff(ref) <= 0) and ref[0] == 14625 and ref[-1] == 1  # count descending, ties unspecified
    terms, cnt, df = cv_oracle.fit(docs, vocabSize=39380)
    assert_same_vocabulary_up_to_ties([t.decode() for t in terms], cnt, vocab, ref)
    ref_df = np.bincount(tf["indices"], minlength=ref.size)
    assert np.array_equal(df, ref_df[cv_oracle.indices_of(terms, vocab)])


def test_restatement_transform_reproduces_the_reference_counts(books):
    tf, vocab, docs = books
    ip, ix, vv = cv_oracle.transform(docs, vocab)
    assert np.array_equal(ip, tf["indptr"]) and np.array_equal(ix, tf["indices"])
    assert np.array_equal(vv, tf["tf"].astype(np.float64))
