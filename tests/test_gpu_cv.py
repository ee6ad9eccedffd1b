"""GPU: CountVectorizer.fit / CountVectorizerModel.transform (count_vectorizer.hip) against the restatement
tests/cv_oracle.py.  Every comparison is exact; STC_CV_HASH_BITS=3 makes almost every pair of terms collide
in the internal hash, and no result may change."""
import ctypes as C

import numpy as np
import pytest

import cv_oracle
from helpers import golden_json, golden_npz
from test_cv_host import assert_same_vocabulary_up_to_ties, reference_books, reference_counts

pytestmark = pytest.mark.gpu


def _b(docs):
    return [[cv_oracle.as_bytes(t) for t in d] for d in docs]


def _check_fit(ctx, docs, **kw):
    """fit on the GPU == the restatement (vocabulary, counts, df); returns the model"""
    import stc

    m = stc.CountVectorizer(ctx=ctx, **kw).fit(docs)
    vocab, cnt, df = cv_oracle.fit(docs, **{"vocabSize": 1 << 18, **kw})
    assert m.vocabulary_bytes == vocab
    assert np.array_equal(m.termCounts, cnt) and np.array_equal(m.docFreq, df)
    assert m.vocabSize == len(vocab)
    return m, vocab


def _check_transform(m, docs, vocab, minTF=1.0, binary=False, value_dtype=None):
    import stc

    m.setMinTF(minTF).setBinary(binary)
    d = m.transform_device(docs, stc.STC_F64 if value_dtype is None else value_dtype)
    got = d.download()
    d.free()
    ip, ix, vv = cv_oracle.transform(docs, vocab, minTF, binary)
    assert got.num_cols == len(vocab)
    assert np.array_equal(got.indptr, ip) and np.array_equal(got.indices, ix) and np.array_equal(got.values, vv)
    return got


def shape_corpus():
    """Terms of every kind the byte order and the dword reads can get wrong, each exactly 3 times over 3
    documents (equal counts: the order is decided by the bytes alone).  The tokens are laid out so that the
    lengths 1..40 start at every byte alignment mod 16."""
    terms = [b"", b"a", b"aa", b"aaaaaaaa", b"aaaaaaaab", b"aaaaaaaa\x00", b"z", "é".encode(),
             b"p" * 32 + b"x", b"p" * 32 + b"y"]
    for n in range(1, 41):
        terms.append(bytes([0x62 + (n * 7 + i) % 20 for i in range(n)]))  # 'b'..'u': distinct from the above
    assert len(set(terms)) == len(terms)
    starts = set()
    docs = []
    for rot in (0, 5, 11):  # three documents, each a rotation: different offsets for every term
        order = terms[rot:] + terms[:rot]
        off = 0
        for t in order:
            if 1 <= len(t) <= 40:
                starts.add(off % 16)
            off += len(t)
        docs.append(order)
    assert starts == set(range(16))
    return docs, terms


@pytest.fixture(scope="module")
def random_terms_corpus():
    """2,000 random terms (lengths 0..24 over a 4-letter alphabet: many shared prefixes), Zipf-drawn into
    300 documents of 0..200 tokens"""
    rng = np.random.default_rng(77)
    terms = set()
    while len(terms) < 2000:
        terms.add(bytes(rng.choice([97, 98, 99, 0xC3], size=int(rng.integers(0, 25))).astype(np.uint8)))
    terms = sorted(terms)
    p = 1.0 / np.arange(1, len(terms) + 1)
    p /= p.sum()
    order = rng.permutation(len(terms))
    return [[terms[order[i]] for i in rng.choice(len(terms), size=int(rng.integers(0, 201)), p=p)] for _ in range(300)]


def _token_shapes(ctx):
    docs, terms = shape_corpus()
    m, vocab = _check_fit(ctx, docs)
    assert np.array_equal(m.termCounts, np.full(len(terms), 3)) and np.array_equal(m.docFreq, np.full(len(terms), 3))
    assert vocab == sorted(terms)
    assert vocab.index(b"z") < vocab.index("é".encode())  # unsigned bytes
    assert vocab.index(b"aaaaaaaa") < vocab.index(b"aaaaaaaa\x00") < vocab.index(b"aaaaaaaab")
    absent = [b"p" * 32 + b"z", b"p" * 32, b"aaaaaaa", b"aaaaaaaa\x00\x00", b"q"]
    got = m.indices_of(vocab + absent)
    assert np.array_equal(got, np.r_[np.arange(len(vocab)), np.full(len(absent), -1)].astype(np.int32))
    assert m.indexOf(b"") == 0 and m.indexOf("é") == vocab.index("é".encode())
    _check_transform(m, docs + [absent, []], vocab)
    return m.vocabulary_bytes, m.termCounts.copy(), m.docFreq.copy()


def test_token_shapes(ctx):
    _token_shapes(ctx)


def test_collisions_change_nothing(ctx, monkeypatch, random_terms_corpus):
    import stc

    docs = random_terms_corpus
    plain_shapes = _token_shapes(ctx)
    plain = stc.CountVectorizer(ctx=ctx).fit(docs)
    monkeypatch.setenv("STC_CV_HASH_BITS", "3")
    masked_shapes = _token_shapes(ctx)
    assert masked_shapes[0] == plain_shapes[0]
    assert np.array_equal(masked_shapes[1], plain_shapes[1]) and np.array_equal(masked_shapes[2], plain_shapes[2])
    masked, vocab = _check_fit(ctx, docs)
    assert masked.vocabulary_bytes == plain.vocabulary_bytes
    assert np.array_equal(masked.termCounts, plain.termCounts) and np.array_equal(masked.docFreq, plain.docFreq)
    got = _check_transform(masked, docs, vocab)
    from_list = stc.CountVectorizerModel.from_vocabulary(vocab, ctx=ctx)  # built under the mask too
    monkeypatch.delenv("STC_CV_HASH_BITS")
    ref = plain.transform(docs)  # the mask lives in the model: an unmasked one beside it
    assert np.array_equal(got.indptr, ref.indptr) and np.array_equal(got.indices, ref.indices)
    assert np.array_equal(got.values, ref.values)
    _check_transform(from_list, docs, vocab)
    probe = vocab[::7] + [b"abcabcabcabcabcabcabcabcabc", b"\xc3"]
    assert np.array_equal(masked.indices_of(probe), cv_oracle.indices_of(probe, vocab))
    with pytest.raises(ValueError):
        monkeypatch.setenv("STC_CV_HASH_BITS", "0")
        stc.CountVectorizer(ctx=ctx).fit(docs)


# 0, 1 and both sides of every size at which the per-document sort takes another path (64·P keys in registers,
# P = 1, 2, 4, 8, 16; past 1024 the segmented radix sort)
LENGTHS = (0, 1, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025)
BIG, OOV, TEN = len(LENGTHS), len(LENGTHS) + 1, len(LENGTHS) + 2


@pytest.fixture(scope="module")
def length_corpus():
    rng = np.random.default_rng(5)
    words = [f"w{i}".encode() for i in range(300)]
    draw = lambda n: [words[i] for i in rng.integers(0, len(words), n)]
    docs = [draw(n) for n in LENGTHS]
    big = [b"hot"] * 66_000 + draw(4_000)
    docs.append([big[i] for i in rng.permutation(len(big))])  # one term 66,000 times among 70,000 tokens
    docs.append([b"oov1", b"oov2", b"oov1"])
    # 10 tokens, 4 outside the vocabulary: minTF = 0.25 gives the threshold 2.5, so the counts of 2 go
    docs.append([b"w1"] * 3 + [b"w2"] * 2 + [b"w3"] + [b"oov1", b"oov2", b"oov3", b"oov3"])
    vocab = words + [b"hot"]
    return docs, vocab


@pytest.mark.parametrize("min_tf", [1.0, 3.0, 0.25])
@pytest.mark.parametrize("binary", [False, True])
def test_document_lengths(ctx, length_corpus, min_tf, binary):
    import stc

    docs, vocab = length_corpus
    m = stc.CountVectorizerModel.from_vocabulary(vocab, ctx=ctx)
    for dt in (stc.STC_F64, stc.STC_F32):
        got = _check_transform(m, docs, vocab, min_tf, binary, dt)
    hot = vocab.index(b"hot")
    row = dict(zip(*got.row(BIG)))
    assert row[hot] == (1.0 if binary else 66_000.0)
    assert got.indptr[OOV + 1] == got.indptr[OOV]  # the document of out-of-vocabulary tokens only
    if min_tf == 0.25:
        assert got.row(TEN)[0].tolist() == [vocab.index(b"w1")]
    # resident tokens take the same path
    toks = stc.DeviceTokens(ctx, *stc.encode_tokens(docs))
    d = m.transform_tokens_device(toks)
    again = d.download()
    d.free()
    toks.free()
    assert np.array_equal(again.indptr, got.indptr) and np.array_equal(again.indices, got.indices)
    assert np.array_equal(again.values, got.values)


def test_only_empty_documents(ctx):
    import stc

    m = stc.CountVectorizerModel.from_vocabulary(["a", "b"], ctx=ctx)
    got = m.transform([[], [], []])
    assert got.shape == (3, 2) and got.nnz == 0 and got.indptr.tolist() == [0, 0, 0, 0]
    assert m.transform([]).shape == (0, 2)
    with pytest.raises(ValueError, match="The vocabulary size should be > 0. Lower minDF as necessary."):
        stc.CountVectorizer(ctx=ctx).fit([[], [], []])


def test_fit_parameters(ctx):
    import stc

    docs = _b([["a", "b", "c", "d", "e", "a"], ["a", "b", "c", "d"], ["a", "b", "c", "f", "f", "f"], ["a", "b", "g"],
               ["a", "h", "h"], []])
    assert len(docs) == 6
    full, vocab = _check_fit(ctx, docs)
    assert full.termCounts.tolist() == [6, 4, 3, 3, 2, 2, 1, 1]  # a b | c f | d h | e g
    for size in (1, 3, 5, 7):  # 3, 5 and 7 cut through the middle of a tie group
        _check_fit(ctx, docs, vocabSize=size)
    _check_fit(ctx, docs, minDF=2)
    _check_fit(ctx, docs, minDF=0.5)      # 0.5 · 6 documents (the empty one counts) = 3
    _check_fit(ctx, docs, maxDF=3)
    _check_fit(ctx, docs, minDF=2, maxDF=3, vocabSize=2)
    _check_fit(ctx, docs, minDF=0.2, maxDF=0.5)
    with pytest.raises(ValueError, match="Lower minDF"):
        stc.CountVectorizer(minDF=6, ctx=ctx).fit(docs)
    with pytest.raises(ValueError):
        stc.CountVectorizer(minDF=4, maxDF=3, ctx=ctx)
    with pytest.raises(ValueError):  # 0.9 · 6 = 5.4 > 3: known only with the corpus
        stc.CountVectorizer(minDF=0.9, maxDF=3, ctx=ctx).fit(docs)
    lib = ctx.lib
    blob, tok_off, doc_off = stc.encode_tokens(docs)
    h = C.c_void_p()
    from stc import _lib as L

    def raw_fit(vocab_size, min_df, max_df):
        return lib.stc_cv_fit(ctx.handle, L.ptr(blob, C.c_uint8), blob.size, L.ptr(tok_off, C.c_int64), tok_off.size - 1,
                              L.ptr(doc_off, C.c_int64), doc_off.size - 1, vocab_size, min_df, max_df, C.byref(h))

    assert raw_fit(0, 1.0, 10.0) == stc.STC_ERR_INVALID_ARG
    assert raw_fit(5, -1.0, 10.0) == stc.STC_ERR_INVALID_ARG
    assert raw_fit(5, 1.0, -2.0) == stc.STC_ERR_INVALID_ARG
    assert raw_fit(5, 4.0, 3.0) == stc.STC_ERR_INVALID_ARG
    with pytest.raises(ValueError, match='"b"'):
        stc.CountVectorizerModel.from_vocabulary(["a", "b", "c", "b", "a"][1:], ctx=ctx)
    one = stc.CountVectorizerModel.from_vocabulary(["b"], ctx=ctx)
    assert one.vocabulary == ["b"] and one.termCounts.tolist() == [0] and one.docFreq.tolist() == [0]
    _check_transform(one, docs, [b"b"])
    fitted_one, v1 = _check_fit(ctx, docs, vocabSize=1)
    _check_transform(fitted_one, docs, v1)
    # the fitted model transforms the corpus it was fitted on, and feeds IDF unchanged
    d = full.transform_device(docs)
    idf = stc.IDF(minDocFreq=0, ctx=ctx).fit_device(d)
    assert np.array_equal(idf.docFreq, full.docFreq) and idf.numDocs == 6
    d.free()


def _permute_docs(blob, tok_off, doc_off, perm):
    def gather(starts, lens):
        total = int(lens.sum())
        return np.repeat(starts - (np.cumsum(lens) - lens), lens) + np.arange(total)

    dlen = np.diff(doc_off)[perm]
    toks = gather(doc_off[:-1][perm], dlen)
    tlen = np.diff(tok_off)[toks]
    new_blob = blob[gather(tok_off[:-1][toks], tlen)]
    new_tok = np.zeros(toks.size + 1, np.int64)
    np.cumsum(tlen, out=new_tok[1:])
    new_doc = np.zeros(perm.size + 1, np.int64)
    np.cumsum(dlen, out=new_doc[1:])
    return np.ascontiguousarray(new_blob), new_tok, new_doc


def _raw_model(ctx, m):
    from stc import _lib as L

    n, nb = C.c_int64(), C.c_int64()
    L.check(ctx.lib.stc_cv_shape(m._dev, C.byref(n), C.byref(nb)))
    blob, off = np.zeros(nb.value, np.uint8), np.zeros(n.value + 1, np.int64)
    cnt, df = np.zeros(n.value, np.int64), np.zeros(n.value, np.int64)
    L.check(ctx.lib.stc_cv_get(ctx.handle, m._dev, L.ptr(blob, C.c_uint8), L.ptr(off, C.c_int64), L.ptr(cnt, C.c_int64),
                               L.ptr(df, C.c_int64)))
    return blob.tobytes(), off.tobytes(), cnt.tobytes(), df.tobytes()


def test_determinism_and_document_order(ctx):
    import stc
    from stc import synth

    (blob, tok_off, doc_off), _ = synth.token_corpus(20_000, 40, n_words=1 << 14, seed=11)
    cv = stc.CountVectorizer(vocabSize=10_000, minDF=2, ctx=ctx)
    a = _raw_model(ctx, cv.fit(None, encoded=(blob, tok_off, doc_off)))
    b = _raw_model(ctx, cv.fit(None, encoded=(blob, tok_off, doc_off)))
    assert a == b
    toks = stc.DeviceTokens(ctx, blob, tok_off, doc_off)
    assert _raw_model(ctx, cv.fit_tokens(toks)) == a  # u32 offsets, resident
    toks.free()
    perm = np.random.default_rng(3).permutation(doc_off.size - 1)
    c = _raw_model(ctx, cv.fit(None, encoded=_permute_docs(blob, tok_off, doc_off, perm)))
    assert c == a
    cnt = np.frombuffer(a[2], np.int64)
    assert cnt.size == 10_000 and np.all(np.diff(cnt) <= 0) and np.frombuffer(a[3], np.int64).min() >= 2


def test_reference_books(ctx, oracle):
    """The LDALoader path from strings: the 51 books → fit (the reference's vocabulary up to its ties) →
    from_vocabulary(en_vocab).transform == the reference's TF CSR → IDF(2) with the 1e-4 floor == its stored
    TF·IDF → topicDistribution == both recorded Spark runs."""
    import stc

    tf, vocab, docs = reference_books()
    enc = stc.encode_tokens(docs)
    assert enc[1].size - 1 == 2_147_864 and int(np.diff(enc[2]).max()) == 261_417
    fitted = stc.CountVectorizer(vocabSize=39380, ctx=ctx).fit(None, encoded=enc)
    assert_same_vocabulary_up_to_ties(fitted.vocabulary, fitted.termCounts, vocab, reference_counts(tf))
    fitted.free()

    V = int(tf["vocab_size"])
    model = stc.CountVectorizerModel.from_vocabulary(vocab, ctx=ctx)
    d_tf = model.transform_device(None, stc.STC_F64, encoded=enc)
    got = d_tf.download()
    assert got.num_cols == V and np.array_equal(got.indptr, tf["indptr"]) and np.array_equal(got.indices, tf["indices"])
    assert np.array_equal(got.values, tf["tf"].astype(np.float64))

    # IDF(2) + the 1e-4 floor on that output: test_gpu_feature.py's assertion on the stored TF·IDF edges, and
    # bit for bit what the same stages give from the reference's own CSR
    idf = stc.IDF(minDocFreq=int(tf["min_doc_freq"]), ctx=ctx).fit_device(d_tf)
    idf.transform_device(d_tf, zero_floor=1e-4)
    out = d_tf.download()
    d_tf.free()
    rel = np.abs(out.values - tf["tfidf"]) / tf["tfidf"]
    print(f"books: TF·IDF max rel {rel.max():.3e}, {np.mean(out.values == tf['tfidf']):.6f} of the edges bit for bit")
    assert rel.max() <= 1e-15, rel.max()
    d_ref = stc.DeviceCsr.upload(ctx, stc.CsrMatrix(tf["indptr"], tf["indices"], tf["tf"].astype(np.float64), V))
    stc.IDF(minDocFreq=int(tf["min_doc_freq"]), ctx=ctx).fit_device(d_ref).transform_device(d_ref, zero_floor=1e-4)
    assert np.array_equal(out.values, d_ref.download().values)
    d_ref.free()

    topics = golden_npz("en_topics.npz")["nwk"]
    meta = golden_json("en_topicdist.json")
    lda = stc.LDAModel.from_topics(topics, meta["docConcentration"], meta["topicConcentration"],
                                   gamma_shape=meta["gammaShape"], seed=7, dtype="f64", ctx=ctx)
    dist = lda.transform(got)
    for run in ("Result_EN_1591066624209", "Result_EN_1591723228815"):
        exp = np.array([[float(x) for x in r] for r in meta[run]])
        err = np.abs(dist - exp).max()
        print(f"books: topicDistribution vs {run}: max abs err {err:.3e}")
        assert err < 2e-6, (run, err)


def test_ownership_and_state(ctx):
    import stc
    from stc import _lib as L

    lib = ctx.lib
    docs = _b([["a", "b"], ["b"]])
    blob, tok_off, doc_off = stc.encode_tokens(docs)
    m = stc.CountVectorizer(ctx=ctx).fit(docs)
    h = C.c_void_p()

    def transform(c, model, dtype):
        return lib.stc_cv_transform_dev(c.handle, model, L.ptr(blob, C.c_uint8), blob.size, L.ptr(tok_off, C.c_int64),
                                        tok_off.size - 1, L.ptr(doc_off, C.c_int64), doc_off.size - 1, 1.0, 0, dtype,
                                        C.byref(h))

    assert transform(ctx, m._dev, 7) == stc.STC_ERR_INVALID_ARG  # value_dtype
    assert transform(ctx, m._dev, stc.STC_MIXED) == stc.STC_ERR_INVALID_ARG
    assert transform(ctx, None, stc.STC_F64) == stc.STC_ERR_INVALID_ARG
    assert lib.stc_cv_shape(None, None, None) == stc.STC_ERR_INVALID_ARG
    assert lib.stc_cv_free(None) == L.STC_OK
    c1 = stc.Context(0)
    # a model used with another context
    assert transform(c1, m._dev, stc.STC_F64) == stc.STC_ERR_INVALID_ARG
    out = np.zeros(3, np.int32)
    assert lib.stc_cv_index_of(c1.handle, m._dev, L.ptr(blob, C.c_uint8), blob.size, L.ptr(tok_off, C.c_int64), 3,
                               L.ptr(out, C.c_int32)) == stc.STC_ERR_INVALID_ARG
    assert lib.stc_cv_get(c1.handle, m._dev, None, None, None, None) == stc.STC_ERR_INVALID_ARG
    toks1 = stc.DeviceTokens(c1, blob, tok_off, doc_off)
    assert lib.stc_cv_transform_tokens(ctx.handle, m._dev, toks1.handle, 1.0, 0, stc.STC_F64, C.byref(h)) == \
        stc.STC_ERR_INVALID_ARG
    assert lib.stc_cv_fit_tokens(ctx.handle, toks1.handle, 10, 1.0, 10.0, C.byref(h)) == stc.STC_ERR_INVALID_ARG
    toks1.free()
    # a model outlives its context: stc_cv_free after stc_destroy
    m1 = stc.CountVectorizer(ctx=c1).fit(docs)
    assert m1.vocabulary == ["b", "a"]
    dev1, m1._dev = m1._dev, None
    # single device: a context connected to other ranks is refused
    c1.comm_init(stc.Context.unique_id(), 1, 0)
    assert lib.stc_cv_fit(c1.handle, L.ptr(blob, C.c_uint8), blob.size, L.ptr(tok_off, C.c_int64), 3,
                          L.ptr(doc_off, C.c_int64), 2, 10, 1.0, 10.0, C.byref(h)) == stc.STC_ERR_STATE
    assert transform(c1, dev1, stc.STC_F64) == stc.STC_ERR_STATE
    assert lib.stc_cv_get(c1.handle, dev1, None, None, None, None) == stc.STC_ERR_STATE
    c1.close()
    assert lib.stc_cv_free(dev1) == L.STC_OK
    assert m.indices_of(["a", "b", "c"]).tolist() == [1, 0, -1]  # the first context's model is untouched
