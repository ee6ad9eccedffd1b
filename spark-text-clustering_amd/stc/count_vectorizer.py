"""CountVectorizer / CountVectorizerModel with the Spark ML surface, backed by count_vectorizer.hip.

Mirrors ``org.apache.spark.ml.feature.{CountVectorizer, CountVectorizerModel}`` ([U] spark 2.4.3,
build.sbt:10): the vocabulary-indexed counting the reference does itself at LDAClustering.scala:143-171
(fit: the ``vocabSize`` most frequent terms) and LDALoader.scala:83-105 (the saved vocabulary's lookup and
per-document counts).  Parameter names, defaults and validation follow Spark (vocabSize = 2^18, minDF = 1,
maxDF = 2^63 − 1, minTF = 1, binary = false).  Ties of the term count, which Spark leaves to its
partitioning, are ordered by the terms' UTF-8 bytes.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .core import Context, CsrMatrix, DeviceCsr
from .feature import DeviceTokens, encode_tokens

_MAX_DF = float(2 ** 63 - 1)


def _non_negative(name, v):
    v = float(v)
    if not v >= 0.0:
        raise ValueError(f"{name} must be >= 0 but got {v}")
    return v


def _check_df(minDF, maxDF):
    # fractions scale with the corpus; two absolute counts can be compared before any data is seen
    if minDF >= 1.0 and maxDF >= 1.0 and maxDF < minDF:
        raise ValueError(f"maxDF ({maxDF}) must be >= minDF ({minDF})")


class CountVectorizerModel:
    """A vocabulary on the GPU (stc_cvm): term → index = position, with the fit's term counts and document
    frequencies.  ``vocabulary``, ``termCounts`` and ``docFreq`` are copied out only when read."""

    def __init__(self, _dev, minTF=1.0, binary=False, inputCol=None, outputCol=None, ctx: Context | None = None):
        self._dev = _dev
        self._ctx = ctx
        # freeing the device model needs only the library, never a context (a __del__ at interpreter
        # shutdown must not create or initialise one)
        self._lib = L.load()
        self.setMinTF(minTF)
        self.setBinary(binary)
        self.inputCol, self.outputCol = inputCol, outputCol
        n, nb = C.c_int64(), C.c_int64()
        L.check(self._lib.stc_cv_shape(_dev, C.byref(n), C.byref(nb)))
        self._n, self._nbytes = n.value, nb.value
        self._vocab = self._count = self._df = None

    @classmethod
    def from_vocabulary(cls, terms, minTF=1.0, binary=False, ctx: Context | None = None, encoded=None):
        """A model over a given list of terms (str or bytes), index = position; a term given twice raises
        ValueError.  ``encoded`` = (utf8 blob, term_off int64[n_terms+1]) skips the encoding of ``terms``."""
        if encoded is not None:
            blob, off = np.ascontiguousarray(encoded[0], np.uint8), L.as_i64(encoded[1])
        else:
            blob, off, _ = encode_tokens([list(terms)])
        if off.size < 2:
            raise ValueError("the vocabulary must hold at least one term")
        c = ctx or Context.get()
        h = C.c_void_p()
        L.check(c.lib.stc_cv_from_vocabulary(c.handle, L.ptr(blob, C.c_uint8), blob.size, L.ptr(off, C.c_int64),
                                             off.size - 1, C.byref(h)))
        return cls(h, minTF, binary, ctx=ctx)

    @property
    def ctx(self):
        return self._ctx or Context.get()

    def _handle(self):
        if self._dev is None:
            raise ValueError("the model's device copy was freed")
        return self._dev

    def setMinTF(self, v):
        self.minTF = _non_negative("minTF", v)
        return self

    def getMinTF(self):
        return self.minTF

    def setBinary(self, b):
        self.binary = bool(b)
        return self

    def getBinary(self):
        return self.binary

    @property
    def vocabSize(self):
        return self._n

    def _fetch(self):
        blob = np.zeros(max(self._nbytes, 1), np.uint8)
        off = np.zeros(self._n + 1, np.int64)
        cnt = np.zeros(self._n, np.int64)
        df = np.zeros(self._n, np.int64)
        L.check(self.ctx.lib.stc_cv_get(self.ctx.handle, self._handle(), L.ptr(blob, C.c_uint8), L.ptr(off, C.c_int64),
                                        L.ptr(cnt, C.c_int64), L.ptr(df, C.c_int64)))
        raw = blob.tobytes()
        self._vocab_bytes = [raw[off[j]:off[j + 1]] for j in range(self._n)]
        self._vocab = [b.decode("utf-8", "surrogateescape") for b in self._vocab_bytes]
        self._count, self._df = cnt, df

    @property
    def vocabulary(self):
        """the terms in index order (list of str)"""
        if self._vocab is None:
            self._fetch()
        return self._vocab

    @property
    def vocabulary_bytes(self):
        """the terms' UTF-8 bytes in index order"""
        if self._vocab is None:
            self._fetch()
        return self._vocab_bytes

    @property
    def termCounts(self):
        """occurrences of each term over the fitted corpus (zeros for a model made from a list)"""
        if self._count is None:
            self._fetch()
        return self._count

    @property
    def docFreq(self):
        """documents of the fitted corpus holding each term (zeros for a model made from a list)"""
        if self._df is None:
            self._fetch()
        return self._df

    def indices_of(self, terms):
        """int32 index of every term, −1 for one outside the vocabulary"""
        terms = list(terms)
        blob, tok_off, _ = encode_tokens([terms])
        out = np.zeros(len(terms), np.int32)
        L.check(self.ctx.lib.stc_cv_index_of(self.ctx.handle, self._handle(), L.ptr(blob, C.c_uint8), blob.size,
                                             L.ptr(tok_off, C.c_int64), len(terms), L.ptr(out, C.c_int32)))
        return out

    def indexOf(self, term) -> int:
        return int(self.indices_of([term])[0])

    def transform_device(self, docs, value_dtype=L.STC_F64, encoded=None) -> DeviceCsr:
        """Vocabulary-indexed term counts of every doc, left resident in HBM (for IDF / LDA on the same GPU)."""
        blob, tok_off, doc_off = encoded if encoded is not None else encode_tokens(docs)
        h = C.c_void_p()
        L.check(self.ctx.lib.stc_cv_transform_dev(
            self.ctx.handle, self._handle(), L.ptr(blob, C.c_uint8), blob.size, L.ptr(tok_off, C.c_int64),
            tok_off.size - 1, L.ptr(doc_off, C.c_int64), doc_off.size - 1, self.minTF, int(self.binary),
            int(value_dtype), C.byref(h)))
        return DeviceCsr(self.ctx, h)

    def transform_tokens_device(self, tokens: DeviceTokens, value_dtype=L.STC_F64) -> DeviceCsr:
        """The same for tokens already resident on the GPU (no host → device copy)."""
        h = C.c_void_p()
        L.check(self.ctx.lib.stc_cv_transform_tokens(self.ctx.handle, self._handle(), tokens.handle, self.minTF,
                                                     int(self.binary), int(value_dtype), C.byref(h)))
        return DeviceCsr(self.ctx, h)

    def transform(self, docs, encoded=None) -> CsrMatrix:
        d = self.transform_device(docs, L.STC_F64, encoded)
        try:
            return d.download()
        finally:
            d.free()

    def free(self, keep_host=True):
        """releases the device copy; the host arrays are fetched first, so they stay readable
        (``keep_host=False``: not fetched)"""
        if self._dev is not None:
            if keep_host and self._vocab is None:
                self._fetch()
            self._lib.stc_cv_free(self._dev)
            self._dev = None

    def __del__(self):
        try:
            if self._dev is not None:
                self._lib.stc_cv_free(self._dev)
                self._dev = None
        except Exception:
            pass


class CountVectorizer:
    """Extracts a vocabulary from document collections and generates a CountVectorizerModel."""

    def __init__(self, vocabSize=1 << 18, minDF=1.0, maxDF=_MAX_DF, minTF=1.0, binary=False, inputCol=None,
                 outputCol=None, ctx: Context | None = None):
        self.setVocabSize(vocabSize)
        self.minDF = _non_negative("minDF", minDF)
        self.maxDF = _non_negative("maxDF", maxDF)
        _check_df(self.minDF, self.maxDF)
        self.setMinTF(minTF)
        self.setBinary(binary)
        self.inputCol, self.outputCol = inputCol, outputCol
        self._ctx = ctx

    @property
    def ctx(self):
        return self._ctx or Context.get()

    def setVocabSize(self, n):
        if int(n) <= 0:
            raise ValueError(f"vocabSize must be > 0 but got {n}")
        self.vocabSize = int(n)
        return self

    def getVocabSize(self):
        return self.vocabSize

    def setMinDF(self, v):
        v = _non_negative("minDF", v)
        _check_df(v, self.maxDF)
        self.minDF = v
        return self

    def getMinDF(self):
        return self.minDF

    def setMaxDF(self, v):
        v = _non_negative("maxDF", v)
        _check_df(self.minDF, v)
        self.maxDF = v
        return self

    def getMaxDF(self):
        return self.maxDF

    def setMinTF(self, v):
        self.minTF = _non_negative("minTF", v)
        return self

    def getMinTF(self):
        return self.minTF

    def setBinary(self, b):
        self.binary = bool(b)
        return self

    def getBinary(self):
        return self.binary

    def _model(self, h):
        return CountVectorizerModel(h, self.minTF, self.binary, self.inputCol, self.outputCol, self._ctx)

    def fit(self, docs, encoded=None) -> CountVectorizerModel:
        """docs: list[list[str|bytes]] (or ``encoded`` = the (utf8, tok_off, doc_off) triple of encode_tokens)"""
        blob, tok_off, doc_off = encoded if encoded is not None else encode_tokens(docs)
        h = C.c_void_p()
        L.check(self.ctx.lib.stc_cv_fit(self.ctx.handle, L.ptr(blob, C.c_uint8), blob.size, L.ptr(tok_off, C.c_int64),
                                        tok_off.size - 1, L.ptr(doc_off, C.c_int64), doc_off.size - 1, self.vocabSize,
                                        self.minDF, self.maxDF, C.byref(h)))
        return self._model(h)

    def fit_tokens(self, tokens: DeviceTokens) -> CountVectorizerModel:
        """fit on tokens already resident on the GPU"""
        h = C.c_void_p()
        L.check(self.ctx.lib.stc_cv_fit_tokens(self.ctx.handle, tokens.handle, self.vocabSize, self.minDF, self.maxDF,
                                               C.byref(h)))
        return self._model(h)
