"""GPU: Tokenizer.transform_device, StopWordsRemover and NGram (token_stages.hip) against the restatement
tests/token_stage_oracle.py.  Every comparison is exact: the blob's bytes, the token offsets and the document
offsets; a result fed to HashingTF or CountVectorizer must give bitwise the CSR that an upload of the restatement's
tokens gives.  Every corpus builder asserts that its corpus really holds the situations it is there for.

Not covered: results of 4 GiB and more (int64 token offsets) and the 2^31-1 token limit, which need gigabytes."""
import ctypes as C

import numpy as np
import pytest

import cv_oracle
import token_stage_oracle as T
from helpers import golden_json
from oracle.oracle import java_lower

pytestmark = pytest.mark.gpu

DESERET = "\U00010400"  # 𐐀, lower case U+10428: the one cased supplementary block of Unicode 6.2
# ASCII of both cases, é/É, ж/Ж, İ, Σ (ends and middles of tokens come from the random draws), ẞ, a 4-byte character
ALPHABET = list("abehTHEIS") + ["é", "É", "ж", "Ж", "İ", "Σ", "σ", "ς", "ẞ", "ß", DESERET, "\U0001F642"]
FIXED = ["", "the", "The", "THE", "I", "i", "saw", "İ", "i̇", "İSTANBUL", "ΟΔΟΣ", "οδος", "οδοσ", "ΣΟΣ", "aΣb", "ÉTÉ", "été",
         "ЖЖ", "жж", "ẞ", "straẞe", DESERET + "x", "balloon", "a-much-longer-token-than-any-stop-word"]
STOP = ["The", "the", "i", "saw", "", "İ", "the", "ÉTÉ", "жЖ", "οδος", "ΣΟΣ", "ß", DESERET + "X", "aσB"]


def _triple(docs):
    import stc

    return stc.encode_tokens(docs)


def _same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)


def _upload(ctx, docs):
    import stc

    return stc.DeviceTokens(ctx, *_triple(docs))


def _check(dev, want_docs):
    """device tokens == the restatement's documents, in all three arrays"""
    want = _triple(want_docs)
    assert (dev.n_bytes, dev.n_tok, dev.n_docs) == (want[0].size, want[1].size - 1, len(want_docs))
    _same(dev.download(), want)
    assert dev.max_doc == max(map(len, want_docs), default=0)  # exact: neither stale (the input's) nor too small


def _check_swr(ctx, docs, stop, case_sensitive):
    """returns (the filtered device tokens, the restatement's documents)"""
    import stc

    swr = stc.StopWordsRemover(stop, caseSensitive=case_sensitive, ctx=ctx)
    src = _upload(ctx, docs)
    out = swr.transform_device(src)
    want = T.swr(docs, stop, case_sensitive)
    _check(out, want)
    _check(src, docs)  # the input is left as it was
    src.free()
    swr.free()
    return out, want


def _check_ngram(ctx, docs, n):
    import stc

    src = _upload(ctx, docs)
    out = stc.NGram(n, ctx=ctx).transform_device(src)
    want = T.ngram(docs, n)
    _check(out, want)
    src.free()
    return out, want


def mixed_corpus():
    """about 300 documents of 0–40 tokens over the mixed alphabet, plus documents of exactly 1–6, 63, 64 and 65 tokens"""
    rng = np.random.default_rng(20260)
    vocab = FIXED + ["".join(rng.choice(ALPHABET, size=int(rng.integers(1, 7)))) for _ in range(300)]
    docs = []
    for _ in range(300):
        docs.append([vocab[i] for i in rng.integers(0, len(vocab), size=int(rng.integers(0, 41)))])
    docs[0], docs[150], docs[299] = [], [], []  # empty documents first, in the middle and last
    docs[7] = ["the", "THE", "I", "", "İ", "i̇", "SAW", "ΟΔΟΣ"]  # every token is a stop word (case-insensitively)
    for k, n in enumerate((1, 2, 3, 4, 5, 6, 63, 64, 65)):
        docs[20 + k] = [vocab[i] for i in rng.integers(0, len(vocab), size=n)]
    docs[298] = ["the", "red", "the"]
    return docs


def _assert_mixed_preconditions(docs):
    for cs in (False, True):
        out = T.swr(docs, STOP, cs)
        assert not docs[0] and not docs[150] and not docs[299]
        dropped = sum(len(d) - len(o) for d, o in zip(docs, out))
        assert 0 < dropped < sum(map(len, docs))
    assert docs[7] and not T.swr(docs, STOP, False)[7] and T.swr(docs, STOP, True)[7]
    longest = max(len(java_lower(w).encode()) for w in STOP)
    toks = {t for d in docs for t in d}
    assert any(len(java_lower(t).encode()) > longest for t in toks)  # tokens that skip the table
    assert any(len(java_lower(t).encode()) != len(t.encode()) for t in toks)  # lower-casing changes a length
    assert any(t.endswith("Σ") and len(t) > 1 for t in toks) and any("Σ" in t[1:-1] for t in toks)
    assert "" in toks and any(DESERET in t for t in toks) and any("ẞ" in t for t in toks)
    # case matters: some token is dropped only case-insensitively
    assert any(java_lower(t) in {java_lower(w) for w in STOP} and t not in STOP for t in toks)


@pytest.fixture(scope="module")
def mixed():
    docs = mixed_corpus()
    _assert_mixed_preconditions(docs)
    return docs


def _fnv1a(b):
    h = 0xCBF29CE484222325
    for c in b:
        h = ((h ^ c) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def big_stop_list():
    """5,000 distinct words: at load ≤ 0.5 of a 16,384-slot open-addressing table, hundreds of them do not sit in
    their home slot, so probes walk chains"""
    rng = np.random.default_rng(5000)
    letters = list("abcdefghijklmnopqrstuvwxyz") + ["é", "ж", "ß"]
    words = set()
    while len(words) < 5000:
        words.add("".join(rng.choice(letters, size=int(rng.integers(2, 9)))))
    return sorted(words)


def _displaced(words):
    """how many words an FNV-1a linear-probing table of the library's size places away from their home slot"""
    slots = 2
    while slots < 2 * len(words):
        slots *= 2
    used, moved = set(), 0
    for w in words:
        s = home = _fnv1a(w.encode()) & (slots - 1)
        while s in used:
            s = (s + 1) & (slots - 1)
        used.add(s)
        moved += s != home
    return moved


def boundary_corpus(upto):
    """1,500-token documents that the filter cuts to 200 (HashingTF's register path: ≤ 256), to 600 (CountVectorizer's
    sort path: ≤ 1,024) and to 1,300 (above both), beside 1-token documents; `upto` classes of them, so that the
    longest filtered document is 200, 600 or 1,300 tokens"""
    rng = np.random.default_rng(1500 + upto)
    words = [f"w{j}" for j in range(400)] + ["Ünï", "ΟΔΟΣ", "x" * 40]
    stop = ["Stop", "AND", "the"]
    docs = [["solo"]]
    for kept in (200, 600, 1300)[:upto]:
        d = [words[i] for i in rng.integers(0, len(words), size=kept)] + \
            [("stop", "and", "THE")[i] for i in rng.integers(0, 3, size=1500 - kept)]
        docs += [[d[i] for i in rng.permutation(1500)], ["the"], ["w1"]]
    return docs, stop


# ---- 1. Tokenizer to device -------------------------------------------------------------------------------------
def test_tokenizer_to_device(ctx):
    import stc

    books = golden_json("books_text.json")
    texts = [e["text"] for lang, entries in books.items() if lang != "targets" for e in entries]
    assert len(texts) == 24
    texts += ["", "   ", "a  b", "İSTANBUL ΟΔΟΣ", DESERET + "B \t" + DESERET, "", "Z"]
    tok = stc.Tokenizer(ctx=ctx)
    for batch in (texts, [], [""], texts[-7:]):
        dev = tok.transform_device(batch)
        want = tok.encode(batch)
        assert (dev.n_bytes, dev.n_tok, dev.n_docs) == (want[0].size, want[1].size - 1, len(batch))
        _same(dev.download(), want)
        assert dev.max_doc == int(np.diff(want[2]).max(initial=0))
        if batch:  # the device tokens feed HashingTF as an upload of the same triple does (padding, offsets, max_doc)
            htf = stc.HashingTF(numFeatures=1 << 10, ctx=ctx)
            _same_csr(htf.transform_tokens_device(dev), htf.transform_tokens_device(stc.DeviceTokens(ctx, *want)))
        dev.free()
    assert tok.transform(["İSTANBUL ΟΔΟΣ"]) == [["i̇stanbul", "οδος"]]


def _same_csr(a, b):
    ga, gb = a.download(), b.download()
    a.free()
    b.free()
    assert ga.shape == gb.shape
    for x, y in ((ga.indptr, gb.indptr), (ga.indices, gb.indices), (ga.values, gb.values)):
        assert x.dtype == y.dtype and np.array_equal(x, y)


# ---- 2. StopWordsRemover ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_sensitive", [False, True])
def test_swr_mixed_corpus(ctx, mixed, case_sensitive):
    out, want = _check_swr(ctx, mixed, STOP, case_sensitive)
    assert want[7] == ([] if not case_sensitive else ["THE", "I", "i̇", "SAW", "ΟΔΟΣ"])
    out.free()


@pytest.mark.parametrize("case_sensitive", [False, True])
def test_swr_large_stop_list(ctx, case_sensitive):
    stop = big_stop_list()
    assert len(stop) == 5000 and _displaced(stop) > 100
    rng = np.random.default_rng(7)
    pool = stop[::3] + [w.upper() for w in stop[1::3]] + [w + "q" for w in stop[2::50]] + ["", "É"]
    docs = [[pool[i] for i in rng.integers(0, len(pool), size=int(rng.integers(0, 60)))] for _ in range(200)]
    out, want = _check_swr(ctx, docs, stop, case_sensitive)
    kept, total = sum(map(len, want)), sum(map(len, docs))
    assert 0 < kept < total and (case_sensitive or kept < total // 5)
    out.free()


def test_swr_degenerate_inputs(ctx):
    for cs in (False, True):
        for docs in ([], [[]], [[], [], []], [[""]], [["", ""], [], [""]]):
            _check_swr(ctx, docs, STOP, cs)[0].free()      # zero documents, zero tokens, only empty tokens
            _check_swr(ctx, docs, [], cs)[0].free()        # n_stop = 0 keeps everything
        _check_swr(ctx, [["a", "B", ""], ["É"]], [], cs)[0].free()
        _check_swr(ctx, [["a", "B", ""], ["É"]], [""], cs)[0].free()  # the empty word alone


# ---- 3. max_doc across the vectorizers' path boundaries ---------------------------------------------------------
@pytest.mark.parametrize("upto", [1, 2, 3])
def test_filtered_tokens_feed_the_vectorizers(ctx, upto):
    import stc

    docs, stop = boundary_corpus(upto)
    want = T.swr(docs, stop, False)
    longest = (200, 600, 1300)[upto - 1]
    assert max(map(len, docs)) == 1500 and max(map(len, want)) == longest
    assert sorted(set(map(len, want))) == sorted({0, 1} | set((200, 600, 1300)[:upto]))
    grams = T.ngram(want, 2)
    assert max(map(len, grams)) == longest - 1 and (longest - 1 > 256) == (longest > 256)
    assert (longest - 1 > 1024) == (longest > 1024)
    filtered, _ = _check_swr(ctx, docs, stop, False)
    bigrams = stc.NGram(2, ctx=ctx).transform_device(filtered)
    _check(bigrams, grams)
    htf = stc.HashingTF(numFeatures=1 << 12, ctx=ctx)
    for dev, ref_docs in ((filtered, want), (bigrams, grams)):
        ref = _upload(ctx, ref_docs)
        _same_csr(htf.transform_tokens_device(dev), htf.transform_tokens_device(ref))
        cvm = stc.CountVectorizer(ctx=ctx).fit_tokens(ref)
        _same_csr(cvm.transform_tokens_device(dev), cvm.transform_tokens_device(ref))
        cvm.free()
        ref.free()
        dev.free()


# ---- 4. one long document ---------------------------------------------------------------------------------------
def test_long_document(ctx):
    import stc

    rng = np.random.default_rng(70000)
    vocab = FIXED + [f"t{j}" for j in range(50)]
    docs = [["the"], [vocab[i] for i in rng.integers(0, len(vocab), size=70000)], ["red"]]
    filtered, want = _check_swr(ctx, docs, STOP, False)
    assert 20000 < len(want[1]) < 69000 and want[0] == [] and want[2] == ["red"]
    grams = stc.NGram(3, ctx=ctx).transform_device(filtered)
    _check(grams, T.ngram(want, 3))
    assert grams.n_tok == len(want[1]) - 2
    grams.free()
    filtered.free()
    _check_ngram(ctx, docs, 3)[0].free()


# ---- 5. NGram ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 5, 64])
def test_ngram_mixed_corpus(ctx, mixed, n):
    lens = set(map(len, mixed))
    assert {0, n, n + 1} <= lens and (n == 1 or any(0 < t < n for t in lens))  # T = 0, T < n, T = n, T = n + 1
    out, want = _check_ngram(ctx, mixed, n)
    assert [len(w) for w in want] == [max(len(d) - n + 1, 0) for d in mixed]
    if n == 1:  # a copy, bit for bit
        _same(out.download(), _triple(mixed))
    out.free()


def test_ngram_small_cases(ctx):
    for n in (1, 2, 3):
        for docs in ([], [[]], [[], []], [["a", "", "b"]], [["", ""]], [["a"], [], ["b", "c"], []]):
            _check_ngram(ctx, docs, n)[0].free()
    import stc

    assert stc.NGram(2, ctx=ctx).transform([["a", "", "b"], ["x"]]) == [["a ", " b"], []]
    assert stc.StopWordsRemover(["i", "the"], ctx=ctx).transform([["I", "saw", "the", "red", "balloon"]]) == \
        [["saw", "red", "balloon"]]


# ---- 6. the chain -----------------------------------------------------------------------------------------------
def test_chain_tokenizer_swr_ngram_count_vectorizer(ctx, oracle):
    import stc

    books = golden_json("books_text.json")
    texts = [e["text"] for lang, entries in books.items() if lang != "targets" for e in entries][:8]
    texts += ["", "The THE the", "İ saw ΟΔΟΣ  twice"]
    stop = ["the", "and", "of", "a", "i", "", "der", "die", "und"]
    swr = stc.StopWordsRemover(stop, ctx=ctx)
    toks = stc.Tokenizer(ctx=ctx).transform_device(texts)
    kept = swr.transform_device(toks)
    grams = stc.NGram(2, ctx=ctx).transform_device(kept)
    want = T.ngram(T.swr([oracle.tokenize(t) for t in texts], stop, False), 2)
    assert sum(map(len, want)) > 1000 and want[-3] == [] and want[-2] == [] and want[-1] == ["i̇ saw", "saw οδος", "οδος twice"]
    _check(grams, want)
    m = stc.CountVectorizer(ctx=ctx).fit_tokens(grams)
    vocab, cnt, df = cv_oracle.fit(want)
    assert m.vocabulary_bytes == vocab and np.array_equal(m.termCounts, cnt) and np.array_equal(m.docFreq, df)
    m.free()
    for d in (grams, kept, toks):
        d.free()
    swr.free()


# ---- 7. determinism ---------------------------------------------------------------------------------------------
def test_two_runs_are_bitwise_equal(ctx, mixed):
    import stc

    texts = [" ".join(d) for d in mixed]
    src = _upload(ctx, mixed)
    swr_ci, swr_cs = stc.StopWordsRemover(STOP, ctx=ctx), stc.StopWordsRemover(STOP, caseSensitive=True, ctx=ctx)
    stages = (lambda: stc.Tokenizer(ctx=ctx).transform_device(texts), lambda: swr_ci.transform_device(src),
              lambda: swr_cs.transform_device(src), lambda: stc.NGram(3, ctx=ctx).transform_device(src))
    for stage in stages:
        runs = []
        for _ in range(2):
            d = stage()
            runs.append([a.tobytes() for a in d.download()])
            d.free()
        assert runs[0] == runs[1] and len(runs[0][1]) > 8
    src.free()


# ---- 8. errors --------------------------------------------------------------------------------------------------
def test_errors(ctx):
    import stc
    from stc import _lib as L

    lib = ctx.lib
    h = C.c_void_p()

    def message():
        return lib.stc_last_error().decode()

    def create(c, stop, cs=0):
        blob, off, _ = stc.encode_tokens([list(stop)])
        return lib.stc_swr_create(c.handle, L.ptr(blob, C.c_uint8), blob.size, L.ptr(off, C.c_int64), off.size - 1, cs,
                                  C.byref(h))

    # a malformed token: refused case-insensitively with its byte offset in the blob, passed through case-sensitively
    bad_docs = [[b"ok", b"a\xffb"], [b"\xe4\xb8"], [b"fine"]]
    src = _upload(ctx, bad_docs)
    with pytest.raises(stc.StcIllegalArgument, match="byte offset 3"):
        stc.StopWordsRemover(["ok"], ctx=ctx).transform_device(src)
    cs = stc.StopWordsRemover(["ok", "fine"], caseSensitive=True, ctx=ctx)
    out = cs.transform_device(src)
    _check(out, T.swr(bad_docs, ["ok", "fine"], True))
    assert [bytes(a) for a in out.download()][0] == b"a\xffb\xe4\xb8"
    out.free()
    for toks, at in (([b"abc", b"\x80"], 3), ([b"a\xc3", b"\xa9b"], 1), ([b"a\xc0\xafb"], 1), ([b"\xf4\x90\x80\x80"], 0),
                     ([b"\xed\xa0\x80"], 0), ([b"x" * 300 + b"\xe4\xb8"], 300)):
        one = _upload(ctx, [toks])
        with pytest.raises(stc.StcIllegalArgument, match=f"byte offset {at}$"):
            stc.StopWordsRemover([], ctx=ctx).transform_device(one)  # validated even with no stop words
        one.free()
    # malformed stop words are refused in both modes; a bad switch; null handles
    for mode in (0, 1):
        assert create(ctx, [b"ok", b"b\xe4d"], mode) == stc.STC_ERR_INVALID_ARG and "offset 3" in message()
    assert create(ctx, ["a"], 2) == stc.STC_ERR_INVALID_ARG
    assert lib.stc_swr_free(None) == L.STC_OK
    assert lib.stc_swr_tokens(ctx.handle, None, src.handle, C.byref(h)) == stc.STC_ERR_INVALID_ARG
    # n = 0 through the C ABI
    assert lib.stc_ngram_tokens(ctx.handle, src.handle, 0, C.byref(h)) == stc.STC_ERR_INVALID_ARG
    assert lib.stc_ngram_tokens(ctx.handle, src.handle, -3, C.byref(h)) == stc.STC_ERR_INVALID_ARG
    # handles of another context
    assert create(ctx, ["ok", "OK", ""]) == L.STC_OK
    swr = C.c_void_p(h.value)
    c1 = stc.Context(0)
    other = _upload(c1, [["ok", "x"]])
    assert lib.stc_swr_tokens(c1.handle, swr, other.handle, C.byref(h)) == stc.STC_ERR_INVALID_ARG  # the remover
    assert lib.stc_swr_tokens(ctx.handle, swr, other.handle, C.byref(h)) == stc.STC_ERR_INVALID_ARG  # the tokens
    assert lib.stc_ngram_tokens(ctx.handle, other.handle, 2, C.byref(h)) == stc.STC_ERR_INVALID_ARG
    assert create(c1, ["x"]) == L.STC_OK
    swr1 = C.c_void_p(h.value)
    assert lib.stc_swr_tokens(c1.handle, swr1, other.handle, C.byref(h)) == L.STC_OK
    got = stc.DeviceTokens.from_handle(c1, C.c_void_p(h.value))
    assert bytes(got.download()[0]) == b"ok"
    got.free()
    other.free()
    c1.close()
    assert lib.stc_swr_free(swr1) == L.STC_OK  # after its context has been closed
    # the first context is untouched
    assert lib.stc_swr_tokens(ctx.handle, swr, src.handle, C.byref(h)) == stc.STC_ERR_INVALID_ARG  # (malformed tokens)
    good = _upload(ctx, [["OK", "go", ""]])
    assert lib.stc_swr_tokens(ctx.handle, swr, good.handle, C.byref(h)) == L.STC_OK
    got = stc.DeviceTokens.from_handle(ctx, C.c_void_p(h.value))
    assert bytes(got.download()[0]) == b"go"
    for d in (got, good, src):
        d.free()
    cs.free()
    assert lib.stc_swr_free(swr) == L.STC_OK


def test_connected_context_is_refused(ctx):
    """single device: every token-stage call on a context connected to other ranks returns STC_ERR_STATE"""
    import stc
    from stc import _lib as L

    lib, h = ctx.lib, C.c_void_p()
    c1 = stc.Context(0)
    toks = _upload(c1, [["a", "b"]])
    blob, off, _ = stc.encode_tokens([["a"]])
    assert lib.stc_swr_create(c1.handle, L.ptr(blob, C.c_uint8), blob.size, L.ptr(off, C.c_int64), 1, 0, C.byref(h)) == L.STC_OK
    swr = C.c_void_p(h.value)
    c1.comm_init(stc.Context.unique_id(), 1, 0)
    text, text_off = stc.encode_texts(["a b"])
    assert lib.stc_swr_create(c1.handle, L.ptr(blob, C.c_uint8), blob.size, L.ptr(off, C.c_int64), 1, 0,
                              C.byref(h)) == stc.STC_ERR_STATE
    assert lib.stc_swr_tokens(c1.handle, swr, toks.handle, C.byref(h)) == stc.STC_ERR_STATE
    assert lib.stc_ngram_tokens(c1.handle, toks.handle, 2, C.byref(h)) == stc.STC_ERR_STATE
    assert lib.stc_tokenize_tokens(c1.handle, L.ptr(text, C.c_uint8), text.size, L.ptr(text_off, C.c_int64), 1,
                                   C.byref(h)) == stc.STC_ERR_STATE
    toks.free()
    c1.close()
    assert lib.stc_swr_free(swr) == L.STC_OK
