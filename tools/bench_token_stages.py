#!/usr/bin/env python3
"""Time the token stages on device-resident tokens — one JSON line.

Corpus: tools/bench_cv.py's — stc.synth.token_corpus, --docs (100k) documents × --tokens (200) tokens drawn Zipf(1)
over a seeded dictionary of --words (2^18) words, uploaded once (stc.DeviceTokens).  The stop list is the --stop (150)
most frequent words of the corpus (the head of a CountVectorizer fit's vocabulary).

Timed, each as --warmup (3) untimed calls and then the median of --repeats (5) calls that end in a stream
synchronisation:
  tokenize_tokens   Tokenizer.transform_device of the same documents as strings (tokens joined by one space): the one
                    stage whose input is host text, so its time includes the text's host → device copy
  swr_sensitive     StopWordsRemover(caseSensitive=True).transform_device
  swr_insensitive   StopWordsRemover(caseSensitive=False).transform_device
  ngram2            NGram(2).transform_device
  hashing_tf        HashingTF(2^18).transform_tokens_device on the same tokens — the yardstick
The line carries input tokens/s for each and what each stage kept.

    python tools/bench_token_stages.py [--docs 100000] [--tokens 200] [--words 262144] [--stop 150] [--warmup 3]
        [--repeats 5] [--workers 16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "spark-text-clustering_amd"), ROOT]


def timed(ctx, fn, warmup, repeats):
    """median / min / max milliseconds of fn() (its result is released by `fn` itself)"""
    for _ in range(warmup):
        fn()
    ctx.synchronize()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}


def joined_text(blob, tok_off, doc_off):
    """the documents as strings, tokens joined by one space: (text uint8, text_off int64[n_docs+1])"""
    n_tok, n_docs = tok_off.size - 1, doc_off.size - 1
    lens = np.diff(tok_off)
    doc_of = np.repeat(np.arange(n_docs, dtype=np.int64), np.diff(doc_off))
    assert np.all(np.diff(doc_off) > 0)  # (an empty document has no string form: "" is one empty token)
    shift = np.arange(n_tok, dtype=np.int64) - doc_of  # separators in front of each token
    text_off = tok_off[doc_off] + doc_off - np.arange(n_docs + 1, dtype=np.int64)
    text = np.full(int(text_off[-1]), 0x20, np.uint8)
    text[np.arange(blob.size, dtype=np.int64) + np.repeat(shift, lens)] = blob
    return text, text_off


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--docs", type=int, default=100_000)
    p.add_argument("--tokens", type=int, default=200)
    p.add_argument("--words", type=int, default=1 << 18)
    p.add_argument("--stop", type=int, default=150)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--workers", type=int, default=16)  # 1 under rocprofv3 (forked workers inherit the profiler)
    a = p.parse_args()
    import ctypes as C

    import stc
    from stc import _lib as L
    from stc import synth

    # (the corpus first: its worker processes are forked before this process opens the GPU)
    (blob, tok_off, doc_off), _ = synth.token_corpus(a.docs, a.tokens, n_words=a.words,
                                                     workers=min(a.workers, os.cpu_count() or 1))
    ctx = stc.Context.get(0)
    n_tok = tok_off.size - 1
    toks = stc.DeviceTokens(ctx, blob, tok_off, doc_off)
    model = stc.CountVectorizer(ctx=ctx).fit_tokens(toks)
    stop = model.vocabulary_bytes[:a.stop]
    model.free(keep_host=False)
    text, text_off = joined_text(blob, tok_off, doc_off)
    swr_cs = stc.StopWordsRemover(stop, caseSensitive=True, ctx=ctx)
    swr_ci = stc.StopWordsRemover(stop, caseSensitive=False, ctx=ctx)
    ngram = stc.NGram(2, ctx=ctx)
    htf = stc.HashingTF(numFeatures=1 << 18, ctx=ctx)

    def tokenize():
        h = C.c_void_p()
        L.check(ctx.lib.stc_tokenize_tokens(ctx.handle, L.ptr(text, C.c_uint8), text.size, L.ptr(text_off, C.c_int64),
                                            text_off.size - 1, C.byref(h)))
        return stc.DeviceTokens.from_handle(ctx, h)

    stages = {"tokenize_tokens": tokenize, "swr_sensitive": lambda: swr_cs.transform_device(toks),
              "swr_insensitive": lambda: swr_ci.transform_device(toks), "ngram2": lambda: ngram.transform_device(toks),
              "hashing_tf": lambda: htf.transform_tokens_device(toks)}
    res = {}
    for name, fn in stages.items():
        res[name] = timed(ctx, lambda: fn().free(), a.warmup, a.repeats)
        res[name]["tokens_per_s"] = n_tok / (res[name]["ms"] * 1e-3)
        if name != "hashing_tf":
            d = fn()
            res[name].update(out_tokens=int(d.n_tok), out_bytes=int(d.n_bytes))
            d.free()
    assert res["tokenize_tokens"]["out_tokens"] == n_tok and res["tokenize_tokens"]["out_bytes"] == blob.size
    out = dict(docs=a.docs, tokens_per_doc=a.tokens, n_tokens=int(n_tok), n_bytes=int(blob.size), words=a.words,
               stop_words=len(stop), text_bytes=int(text.size), warmup=a.warmup, repeats=a.repeats, **res)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
