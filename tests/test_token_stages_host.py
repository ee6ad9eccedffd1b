"""CPU: the token stages' surface (stc_tokenize_tokens, stc_swr_*, stc_ngram_tokens) is declared, exported and bound;
the restatement tests/token_stage_oracle.py gives Spark's documented answers; the Python classes check their arguments
without a GPU."""
import os
import re

import pytest

import token_stage_oracle as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("stc_tokens_max_doc", "stc_tokenize_tokens", "stc_swr_create", "stc_swr_free", "stc_swr_tokens", "stc_ngram_tokens")


def test_symbols_declared_bound_and_exported():
    import stc
    from stc import _lib

    header = open(os.path.join(ROOT, "include", "stc.h")).read()
    declared = set(re.findall(r"^\s*int\s+(stc_\w+)\s*\(", header, re.M))
    lib = stc.load()
    for s in SYMBOLS:
        assert s in declared, s
        assert s in _lib.SIGNATURES, s
        assert hasattr(lib, s), s
    assert "#define STC_ABI_VERSION 2" in header and lib.stc_abi_version() == 2
    for name in ("StopWordsRemover", "NGram"):
        assert name in stc.__all__ and hasattr(stc, name)
    assert hasattr(stc.Tokenizer, "transform_device")


def test_jvm_boundary_names():
    jni = open(os.path.join(ROOT, "jni", "stcjni.c")).read()
    java = open(os.path.join(ROOT, "scala", "org", "apache", "spark", "mllib", "clustering", "StcNative.java")).read()
    for name in ("tokensMaxDoc", "tokenizeTokens", "swrCreate", "swrFree", "swrTokens", "ngramTokens"):
        assert f"FN({name})" in jni, name
        assert re.search(r"public static native \S+ %s\(" % name, java), name


def test_stop_words_remover_known_answers():
    # the example of Spark's ml-features guide
    assert T.swr([["I", "saw", "the", "red", "balloon"]], {"i", "the"}, False) == [["saw", "red", "balloon"]]
    assert T.swr([["I", "saw", "the", "red", "balloon"]], {"i", "the"}, True) == [["I", "saw", "red", "balloon"]]
    # kept tokens keep their bytes; both sides are lower-cased; the empty word drops empty tokens; rows stay
    assert T.swr([["The", "", "CAT"], [], ["the"]], ["THE", ""], False) == [["CAT"], [], []]
    assert T.swr([["The", "", "CAT"]], [], False) == [["The", "", "CAT"]]
    # Java 8 root-locale lower-casing of the token as a string of its own: İ → "i̇", Σ by Final_Sigma
    assert T.swr([["İ", "i̇", "I", "ΟΔΟΣ", "οδοσ", "ΣΟΣ"]], ["İ", "οδος"], False) == [["I", "οδοσ", "ΣΟΣ"]]
    assert T.swr([["ẞ", "ß", "SS"]], ["ß"], False) == [["SS"]]
    assert T.swr([[b"\xff", "a"]], ["a"], True) == [[b"\xff"]]


def test_ngram_known_answers():
    # the example of Spark's ml-features guide
    assert T.ngram([["Hi", "I", "heard", "about", "Spark"]], 2) == [["Hi I", "I heard", "heard about", "about Spark"]]
    assert T.ngram([["a", "b"], [], ["a", "b", "c"]], 3) == [[], [], ["a b c"]]  # T < n → []
    assert T.ngram([["a", "", "b"]], 2) == [["a ", " b"]]  # empty tokens join as they are
    assert T.ngram([["a", "", "b"], []], 1) == [["a", "", "b"], []]
    with pytest.raises(ValueError):
        T.ngram([["a"]], 0)


def test_python_argument_checks():
    import stc

    with pytest.raises(ValueError):
        stc.NGram(n=0)
    with pytest.raises(ValueError):
        stc.NGram().setN(-1)
    assert stc.NGram().getN() == 2 and stc.NGram(n=3).setN(5).getN() == 5
    for loc in ("tr", "tr_TR", "az-AZ", "LT", "lt_LT"):
        with pytest.raises(ValueError):
            stc.StopWordsRemover(["a"], locale=loc)
    s = stc.StopWordsRemover(["The", "the"], locale="en_US")
    assert s.getStopWords() == ["The", "the"] and s.getCaseSensitive() is False and s.getLocale() == "en_US"
    assert s.setCaseSensitive(True).getCaseSensitive() is True
    assert s.setStopWords([b"x", "y"]).getStopWords() == ["x", "y"]
    assert stc.StopWordsRemover(["a"], locale="true").getLocale() == "true"  # only the language part counts
    with pytest.raises(ValueError):
        s.setLocale("tr")
    with pytest.raises(TypeError):
        stc.StopWordsRemover("the")
