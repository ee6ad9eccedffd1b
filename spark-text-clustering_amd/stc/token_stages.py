"""StopWordsRemover and NGram with the Spark ML surface, on device tokens (token_stages.hip).

Mirror ``org.apache.spark.ml.feature.{StopWordsRemover, NGram}`` ([U] spark 2.4.3, build.sbt:10), the stages a Spark
LDA pipeline puts between its tokenizer and its vectorizer.  ``transform_device`` takes and returns DeviceTokens, so
``Tokenizer.transform_device`` (or ``TextPreprocessor.transform_device``) → StopWordsRemover → NGram → HashingTF /
CountVectorizer never leaves the GPU.  The exact semantics: include/stc.h, "Token stages".
"""
from __future__ import annotations

import ctypes as C
import re

from . import _lib as L
from .core import Context
from .feature import DeviceTokens, encode_tokens

# languages whose lower-casing differs from the root locale's (dotted / dotless i, Lithuanian dot retention)
_UNSUPPORTED_LANGUAGES = ("tr", "az", "lt")


def _split_docs(dev: DeviceTokens):
    blob, tok_off, doc_off = dev.download()
    raw = blob.tobytes()
    toks = [raw[tok_off[t]:tok_off[t + 1]].decode("utf-8") for t in range(tok_off.size - 1)]
    return [toks[doc_off[i]:doc_off[i + 1]] for i in range(doc_off.size - 1)]


class _TokenStage:
    """transform (host lists in and out) on top of a stage's transform_device"""

    _ctx = None

    @property
    def ctx(self):
        return self._ctx or Context.get()

    def transform(self, docs) -> list[list[str]]:
        """list[list[str]] → list[list[str]] (the tokens of each document)"""
        src = DeviceTokens(self.ctx, *encode_tokens(docs))
        try:
            out = self.transform_device(src)
            try:
                return _split_docs(out)
            finally:
                out.free()
        finally:
            src.free()


class StopWordsRemover(_TokenStage):
    """Drops the stop words from every document's tokens, on the GPU.

    stopWords: the words to drop — always the caller's list (Spark's bundled language lists are not part of this
    package; ``stc.io.load_stop_words`` reads a one-word-per-line file).  caseSensitive=False (Spark's default)
    compares Java 8 root-locale lower cases; a ``locale`` whose language is tr, az or lt lower-cases differently
    and is refused, any other value is accepted and means the root locale's rules.  Kept tokens keep their
    original bytes."""

    def __init__(self, stopWords=(), caseSensitive=False, locale=None, inputCol=None, outputCol=None,
                 ctx: Context | None = None):
        self._dev = None
        self._lib = None
        self.setLocale(locale)
        self.setStopWords(stopWords)
        self.setCaseSensitive(caseSensitive)
        self.inputCol, self.outputCol = inputCol, outputCol
        self._ctx = ctx

    def setStopWords(self, words):
        if isinstance(words, (str, bytes, bytearray)):
            raise TypeError("stopWords must be a sequence of words, not one string")
        self.stopWords = [w.decode("utf-8") if isinstance(w, (bytes, bytearray)) else str(w) for w in words]
        self.free()
        return self

    def getStopWords(self):
        return list(self.stopWords)

    def setCaseSensitive(self, v):
        self.caseSensitive = bool(v)
        self.free()
        return self

    def getCaseSensitive(self):
        return self.caseSensitive

    def setLocale(self, locale):
        if locale is not None:
            lang = re.split(r"[_\-]", str(locale).strip(), maxsplit=1)[0].lower()
            if lang in _UNSUPPORTED_LANGUAGES:
                raise ValueError(f"StopWordsRemover lower-cases by the root locale's rules; locale {locale!r} "
                                 f"(language {lang!r}) lower-cases differently and is not supported")
        self.locale = None if locale is None else str(locale)
        return self

    def getLocale(self):
        return self.locale

    def _handle(self):
        if self._dev is None:
            blob, off, _ = encode_tokens([self.stopWords])
            h = C.c_void_p()
            L.check(self.ctx.lib.stc_swr_create(self.ctx.handle, L.ptr(blob, C.c_uint8), blob.size, L.ptr(off, C.c_int64),
                                                off.size - 1, int(self.caseSensitive), C.byref(h)))
            self._lib = self.ctx.lib  # freeing needs only the library, never a context
            self._dev = h
        return self._dev

    def transform_device(self, tokens: DeviceTokens) -> DeviceTokens:
        """device tokens → the same documents without their stop words, left resident in HBM"""
        h = C.c_void_p()
        L.check(self.ctx.lib.stc_swr_tokens(self.ctx.handle, self._handle(), tokens.handle, C.byref(h)))
        return DeviceTokens.from_handle(self.ctx, h)

    def free(self):
        """releases the device table (made again on the next use)"""
        if self._dev is not None:
            self._lib.stc_swr_free(self._dev)
            self._dev = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class NGram(_TokenStage):
    """Every run of n consecutive tokens of a document, joined by one space, on the GPU (a document of fewer than
    n tokens yields none)."""

    def __init__(self, n=2, inputCol=None, outputCol=None, ctx: Context | None = None):
        self.setN(n)
        self.inputCol, self.outputCol = inputCol, outputCol
        self._ctx = ctx

    def setN(self, n):
        if int(n) < 1:
            raise ValueError(f"n must be >= 1 but got {n}")
        self.n = int(n)
        return self

    def getN(self):
        return self.n

    def transform_device(self, tokens: DeviceTokens) -> DeviceTokens:
        """device tokens → the documents' n-grams, left resident in HBM"""
        h = C.c_void_p()
        L.check(self.ctx.lib.stc_ngram_tokens(self.ctx.handle, tokens.handle, self.n, C.byref(h)))
        return DeviceTokens.from_handle(self.ctx, h)
