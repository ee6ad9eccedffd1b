"""The reference's text preprocessing between its lemmatiser and its vocabulary, backed by text_prep.hip.

Mirrors what LDAClustering.scala:121-139 (training) and :221-238 (scoring) run on every book:
``filterSpecialCharacters`` → OpenNLP ``SimpleTokenizer`` → drop the stop words → OpenNLP ``PorterStemmer``
(the exact semantics: include/stc.h, "Text preprocessing").  The result stays on the GPU as DeviceTokens, the
input of CountVectorizer / CountVectorizerModel / HashingTF.  Every document yields a row, possibly empty; the
reference drops empty documents and renumbers the rest, which is left to the caller.  CoreNLP's lemmatiser, the
step in front, needs trained models and is out of scope.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .core import Context
from .feature import DeviceTokens, encode_texts, encode_tokens

# the regex class of LDAClustering.scala:283-284 under java.util.regex (its trailing "' ' '-' '-'" is U+0020–U+002D)
DEFAULT_STRIP_CHARS = "".join(map(chr, range(0x20, 0x2E))) + ".:;?@^_`«»’”−"


def _split(blob, tok_off):
    raw = blob.tobytes()
    return [raw[tok_off[t]:tok_off[t + 1]].decode("utf-8") for t in range(tok_off.size - 1)]


class TextPreprocessor:
    """strip → SimpleTokenizer → stop words → Porter stemmer on the GPU.

    stopWords: the words to drop (exact, case-sensitive, tested before stemming); stem: apply the Porter stemmer;
    stripChars: the characters treated as white space (BMP only), None = the reference's set
    (``DEFAULT_STRIP_CHARS``)."""

    def __init__(self, stopWords=(), stem=True, stripChars=None, ctx: Context | None = None):
        self.stopWords = [w.decode("utf-8") if isinstance(w, (bytes, bytearray)) else str(w) for w in stopWords]
        self.stem = bool(stem)
        self.stripChars = None if stripChars is None else "".join(stripChars)
        self._ctx = ctx
        self._lib = L.load()  # freeing needs only the library, never a context
        self._dev = None

    @property
    def ctx(self):
        return self._ctx or Context.get()

    def _handle(self):
        if self._dev is None:
            blob, off, _ = encode_tokens([self.stopWords])
            if self.stripChars is None:
                cps, n = None, -1
            else:
                cps = np.array([ord(ch) for ch in self.stripChars], np.uint32)
                n = cps.size
            h = C.c_void_p()
            L.check(self.ctx.lib.stc_prep_create(self.ctx.handle, L.ptr(cps, C.c_uint32) if n > 0 else None, n,
                                                 L.ptr(blob, C.c_uint8), blob.size, L.ptr(off, C.c_int64), off.size - 1,
                                                 int(self.stem), C.byref(h)))
            self._dev = h
        return self._dev

    def transform_device(self, texts) -> DeviceTokens:
        """list[str|bytes] → the documents' tokens, left resident in HBM"""
        text, off = encode_texts(texts)
        h = C.c_void_p()
        L.check(self.ctx.lib.stc_prep_tokens(self.ctx.handle, self._handle(), L.ptr(text, C.c_uint8), text.size,
                                             L.ptr(off, C.c_int64), off.size - 1, C.byref(h)))
        return DeviceTokens.from_handle(self.ctx, h)

    def transform(self, texts) -> list[list[str]]:
        """list[str] → list[list[str]] (the tokens of each document)"""
        d = self.transform_device(texts)
        try:
            blob, tok_off, doc_off = d.download()
        finally:
            d.free()
        toks = _split(blob, tok_off)
        return [toks[doc_off[i]:doc_off[i + 1]] for i in range(doc_off.size - 1)]

    def free(self):
        if self._dev is not None:
            self._lib.stc_prep_free(self._dev)
            self._dev = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PorterStemmer:
    """OpenNLP's PorterStemmer on the GPU, each token on its own (the library's test hook stc_stem_tokens)."""

    def __init__(self, ctx: Context | None = None):
        self._ctx = ctx

    @property
    def ctx(self):
        return self._ctx or Context.get()

    def stem_encoded(self, blob, tok_off):
        """(utf8 blob, tok_off) in, the stems' (utf8 blob, tok_off) out"""
        blob = np.ascontiguousarray(blob, np.uint8)
        tok_off = L.as_i64(tok_off)
        out = np.zeros(max(blob.size, 1), np.uint8)
        out_off = np.zeros(tok_off.size, np.int64)
        L.check(self.ctx.lib.stc_stem_tokens(self.ctx.handle, L.ptr(blob, C.c_uint8), blob.size, L.ptr(tok_off, C.c_int64),
                                             tok_off.size - 1, L.ptr(out, C.c_uint8), L.ptr(out_off, C.c_int64)))
        return out[:out_off[-1]], out_off

    def stem(self, tokens) -> list[str]:
        blob, tok_off, _ = encode_tokens([list(tokens)])
        return _split(*self.stem_encoded(blob, tok_off))
