"""GPU: the text preprocessing kernels (text_prep.hip) against the restatement tests/prep_oracle.py.  Every
comparison is exact: the blob's bytes, the token offsets and the document offsets.

Not covered: the "more than 2^31-1 tokens" refusal, which needs gigabytes of text to reach."""
import ctypes as C
import os

import numpy as np
import pytest

import cv_oracle
import prep_oracle as P
from helpers import GOLDEN, golden_json
from test_prep_oracle import TOKEN_VECTORS, en_vocab, ge_vocab_nonascii, stem_vectors

pytestmark = pytest.mark.gpu

CHUNK = 2048  # text bytes per workgroup of k_classify / k_tokens (text_prep.hip kChunk)


def _triple(docs):
    import stc

    return stc.encode_tokens(docs)


def _same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)


def _check_stem(ctx, words):
    import stc

    blob, off, _ = _triple([words])
    want = _triple([[P.stem(w) for w in words]])
    _same(stc.PorterStemmer(ctx).stem_encoded(blob, off), want[:2])


def _check_prep(ctx, texts, stop=(), stem=False, strip=None):
    """transform_device on the GPU == the restatement; returns (the device tokens, the restatement's documents)"""
    import stc

    pre = stc.TextPreprocessor(stopWords=stop, stem=stem, stripChars=strip, ctx=ctx)
    dev = pre.transform_device(texts)
    want_docs = P.preprocess_docs(texts, stop, stem, P.DEFAULT_STRIP if strip is None else frozenset(map(ord, strip)))
    want = _triple(want_docs)
    assert (dev.n_bytes, dev.n_tok, dev.n_docs) == (want[0].size, want[1].size - 1, len(texts))
    _same(dev.download(), want)
    pre.free()
    return dev, want_docs


@pytest.fixture(scope="module")
def book_texts():
    books = golden_json("books_text.json")
    texts = [e["text"] for lang, entries in books.items() if lang != "targets" for e in entries]
    assert len(texts) == 24
    return texts


@pytest.fixture(scope="module")
def stop_en():
    import stc

    return stc.io.load_stop_words(os.path.join(GOLDEN, "stop_words_en.txt"))


# ---- stc_stem_tokens --------------------------------------------------------------------------------------------
def test_stem_known_answers(ctx):
    import stc

    words = [w for w, _ in stem_vectors()]
    assert stc.PorterStemmer(ctx).stem(words) == [s for _, s in stem_vectors()]


def test_stem_en_vocabulary(ctx):
    _check_stem(ctx, en_vocab())


def test_stem_ge_nonascii_vocabulary(ctx):
    _check_stem(ctx, ge_vocab_nonascii())


def generated_words():
    """every suffix of every step table (and step 1's) on stems of measure 0, 1 and 2, on stems ending in a double
    consonant (ll, ss, zz too) and in consonant-vowel-consonant (final w, x, y too), and on the same with a
    non-ASCII character where doublec / cvc look"""
    suffixes = {"", "s", "ss", "sses", "ies", "eed", "ed", "ing", "at", "bl", "iz", "y", "e", "l", "ll", "sion", "tion"}
    for table in (P._Stemmer._STEP3, P._Stemmer._STEP4):
        for rows in table.values():
            suffixes.update(s for s, _ in rows)
    for rows in P._Stemmer._STEP5.values():
        suffixes.update(rows)
    stems = ["tr", "ee", "b", "y", "by", "tree",            # measure 0
             "oat", "ivy", "trouble", "ab",                  # measure 1
             "oaten", "orrery", "private", "abab",           # measure 2
             "fall", "hiss", "fizz", "hopp", "tann", "add",  # double consonant
             "hop", "fil", "snow", "box", "tray", "say",     # consonant-vowel-consonant
             "feéé", "hoßß", "aжж", "féll", "ééll",          # non-ASCII double consonant (and before an ASCII one)
             "feé", "éop", "hoж", "éoж", "中a中", "ya中", "éy", "éyé",  # non-ASCII in cvc's three positions
             "a\U0001F600\U0001F600", "\U0001F600o\U0001F600"]  # two Java chars each: never a double
    words = []
    for st in stems:
        for su in sorted(suffixes):
            words += [st + su, st + su + "s", st + su + "ed", st + su + "ing", st + "e" + su]
    return [w for w in words if w]


def test_stem_generated_set(ctx):
    words = generated_words()
    assert len(words) > 10000
    _check_stem(ctx, words)


def test_stem_short_and_long_tokens(ctx):
    long_token = ("ab" * 2500)[:4993] + "ization"
    assert len(long_token) == 5000 and len(P.stem(long_token)) == 4993
    _check_stem(ctx, ["", "a", "é", "\U0001F600", "ed", "és", "éé", "ies", "éed", "aed", "ing", "\U0001F600s", "a\U0001F600",
                      long_token, "y" * 5000, "", "abilities", ""])


# ---- stc_prep_tokens, no stop words, no stemming ----------------------------------------------------------------
def test_tokens_of_the_books(ctx, book_texts):
    _check_prep(ctx, book_texts)
    _check_prep(ctx, ["".join(book_texts)])


def test_tokenizer_known_answers(ctx):
    import stc

    texts = [t for t, _ in TOKEN_VECTORS]
    assert stc.TextPreprocessor(stem=False, ctx=ctx).transform(texts) == [w for _, w in TOKEN_VECTORS]
    _check_prep(ctx, texts)
    _check_prep(ctx, ["a b　c\x1cd\x85e", "١٢٣abc123", "--/-//", "x\U0001F600\U0001F601\U0001F601"])


def test_pattern_slides_over_every_chunk_offset(ctx):
    """a two-token pattern with a 3-byte character, 9 bytes a period: over 2304 periods it starts at every byte offset
    modulo the workgroup's chunk, so a token boundary and a multi-byte character cross every wave and chunk edge"""
    unit = "a中b//  "
    assert len(unit.encode()) == 9 and P.tokenize(unit) == ["a中b", "//"]
    reps = CHUNK + 256
    assert {(9 * r) % CHUNK for r in range(reps)} == set(range(CHUNK))
    _check_prep(ctx, [unit * reps])
    # the same bytes as documents that end inside the pattern: the state resets at every offset too
    _check_prep(ctx, ["a中", "b/", "/  "] * reps)
    _check_prep(ctx, ["//", "/", "/a", "中", "中b  "] * 700)


def test_empty_documents(ctx):
    _check_prep(ctx, [])
    _check_prep(ctx, [""])
    _check_prep(ctx, ["", "", "ab cd", "", " . ", "", "ef", "", ""])
    _check_prep(ctx, ["", "x"])


def test_custom_strip_set(ctx, book_texts):
    _check_prep(ctx, ["a/b中c-d e.f", "//", "中"], strip="/中")
    _check_prep(ctx, ["a-b c.d"], strip="")
    _check_prep(ctx, book_texts[:6], strip="aeiouéа ")


# ---- the full path ----------------------------------------------------------------------------------------------
def test_full_path_feeds_count_vectorizer_and_hashing_tf(ctx, book_texts, stop_en):
    import stc

    texts = book_texts + ["", "The being is: " + ("ab" * 2500)[:4993] + "ization of generalizations"]
    dev, docs = _check_prep(ctx, texts, stop=stop_en, stem=True)
    assert docs[-1][:2] == ["The", "be"]
    # CountVectorizer.fit on the device tokens == the restatement on the oracle's tokens
    m = stc.CountVectorizer(ctx=ctx).fit_tokens(dev)
    vocab, cnt, df = cv_oracle.fit(docs)
    assert m.vocabulary_bytes == vocab and np.array_equal(m.termCounts, cnt) and np.array_equal(m.docFreq, df)
    # the reference's saved vocabulary applied to them
    ref = stc.CountVectorizerModel.from_vocabulary(en_vocab(), ctx=ctx)
    d = ref.transform_tokens_device(dev)
    got = d.download()
    d.free()
    ip, ix, vv = cv_oracle.transform(docs, en_vocab())
    assert got.num_cols == 39380 and ix.size > 1000
    assert np.array_equal(got.indptr, ip) and np.array_equal(got.indices, ix) and np.array_equal(got.values, vv)
    # HashingTF takes them as it takes an upload
    htf = stc.HashingTF(numFeatures=1 << 12, ctx=ctx)
    d = htf.transform_tokens_device(dev)
    got = d.download()
    d.free()
    want = htf.transform(docs)
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
    assert np.array_equal(got.values, want.values)
    dev.free()


def test_two_runs_are_bitwise_equal(ctx, book_texts, stop_en):
    import stc

    pre = stc.TextPreprocessor(stopWords=stop_en, stem=True, ctx=ctx)
    runs = []
    for _ in range(2):
        d = pre.transform_device(book_texts)
        runs.append([a.tobytes() for a in d.download()])
        d.free()
    assert runs[0] == runs[1]


# ---- errors ------------------------------------------------------------------------------------------------------
def test_errors(ctx):
    import stc
    from stc import _lib as L

    lib = ctx.lib
    h = C.c_void_p()

    def create(c, strip=None, n_strip=-1, stop=(), stem=1):
        blob, off, _ = stc.encode_tokens([list(stop)])
        cps = None if strip is None else np.array(strip, np.uint32)
        return lib.stc_prep_create(c.handle, L.ptr(cps, C.c_uint32), n_strip, L.ptr(blob, C.c_uint8), blob.size,
                                   L.ptr(off, C.c_int64), off.size - 1, stem, C.byref(h))

    def tokens(c, prep, docs):
        text, off = stc.encode_texts(docs)
        return lib.stc_prep_tokens(c.handle, prep, L.ptr(text, C.c_uint8), text.size, L.ptr(off, C.c_int64), off.size - 1,
                                   C.byref(h))

    def message():
        return lib.stc_last_error().decode()

    # a strip code point outside the BMP, a surrogate; a bad stemmer switch; bad pointers
    assert create(ctx, [0x2E, 0x10000], 2) == stc.STC_ERR_INVALID_ARG
    assert create(ctx, [0xD800], 1) == stc.STC_ERR_INVALID_ARG
    assert create(ctx, stem=2) == stc.STC_ERR_INVALID_ARG
    assert create(ctx, None, 3) == stc.STC_ERR_INVALID_ARG
    assert lib.stc_prep_free(None) == L.STC_OK
    assert lib.stc_tokens_shape(None, None, None, None) == stc.STC_ERR_INVALID_ARG
    # malformed UTF-8 in the stop words: the byte offset is named
    assert create(ctx, stop=[b"ok", b"b\xe4d"]) == stc.STC_ERR_INVALID_ARG and "offset 3" in message()
    assert create(ctx, stop=[b"\xed\xa0\x80"]) == stc.STC_ERR_INVALID_ARG and "offset 0" in message()  # a surrogate
    assert create(ctx, stop=["be", "be", ""]) == L.STC_OK  # a word twice, an empty word: accepted
    prep = C.c_void_p(h.value)
    # malformed UTF-8 in the text
    for docs, at in (([b"ab\xffcd"], 2), ([b"abc", b"\x80"], 3), ([b"a\xc3", b"\xa9b"], 1), ([b"ab\xe4\xb8"], 2),
                     ([b"a\xc0\xafb"], 1), ([b"\xf4\x90\x80\x80"], 0), ([b"x" * 5000 + b"\xe4\xb8"], 5000)):
        assert tokens(ctx, prep, docs) == stc.STC_ERR_INVALID_ARG, docs
        assert f"offset {at}" in message(), (docs, message())
    blob, off, _ = stc.encode_tokens([[b"abc", b"\xc3"]])
    out, out_off = np.zeros(8, np.uint8), np.zeros(3, np.int64)
    assert lib.stc_stem_tokens(ctx.handle, L.ptr(blob, C.c_uint8), blob.size, L.ptr(off, C.c_int64), 2,
                               L.ptr(out, C.c_uint8), L.ptr(out_off, C.c_int64)) == stc.STC_ERR_INVALID_ARG
    assert "offset 3" in message()
    # another context's preprocessor and tokens; a context connected to other ranks
    c1 = stc.Context(0)
    assert tokens(c1, prep, ["a b"]) == stc.STC_ERR_INVALID_ARG
    assert tokens(ctx, prep, ["being a b"]) == L.STC_OK
    toks = stc.DeviceTokens.from_handle(ctx, C.c_void_p(h.value))
    assert lib.stc_tokens_download(c1.handle, toks.handle, None, None, None) == stc.STC_ERR_INVALID_ARG
    assert [bytes(a) for a in toks.download()][0] == b"beab"
    c1.comm_init(stc.Context.unique_id(), 1, 0)
    assert create(c1) == stc.STC_ERR_STATE
    assert lib.stc_stem_tokens(c1.handle, L.ptr(blob, C.c_uint8), 3, L.ptr(off, C.c_int64), 1, L.ptr(out, C.c_uint8),
                               L.ptr(out_off, C.c_int64)) == stc.STC_ERR_STATE
    c1.close()
    # the first context is untouched
    assert stc.TextPreprocessor(stopWords=["be"], ctx=ctx).transform(["being be hopping"]) == [["be", "hop"]]
    toks.free()
    assert lib.stc_prep_free(prep) == L.STC_OK
