#!/usr/bin/env python3
"""Time CountVectorizer on device-resident tokens — one JSON line.

Corpus: stc.synth.token_corpus, --docs (100k) documents × --tokens (200) tokens drawn Zipf(1) over a seeded
dictionary of --words (2^18) words, uploaded once (stc.DeviceTokens); nothing crosses PCIe inside a timed call.

Timed, each as --warmup (3) untimed calls and then the median of --repeats (5) calls that end in a stream
synchronisation:
  fit             CountVectorizer(vocabSize = --vocab-size).fit_tokens: hash, sort, runs, order, gather, table
  from_vocabulary CountVectorizerModel.from_vocabulary of the fitted vocabulary, already encoded as a blob +
                  offsets (upload + table build with its duplicate check)
  transform       CountVectorizerModel.transform_tokens_device (lookup, per-document sort, runs, CSR)
  hashing_tf      HashingTF(2^18).transform_tokens_device on the same tokens — the yardstick
The line carries tokens/s for each (from_vocabulary: terms/s) and the transform ÷ HashingTF time ratio.

    python tools/bench_cv.py [--docs 100000] [--tokens 200] [--words 262144] [--warmup 3] [--repeats 5]
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


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--docs", type=int, default=100_000)
    p.add_argument("--tokens", type=int, default=200)
    p.add_argument("--words", type=int, default=1 << 18)
    p.add_argument("--vocab-size", type=int, default=1 << 18)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--repeats", type=int, default=5)
    a = p.parse_args()
    import stc
    from stc import synth

    ctx = stc.Context.get(0)
    (blob, tok_off, doc_off), _ = synth.token_corpus(a.docs, a.tokens, n_words=a.words,
                                                     workers=min(16, os.cpu_count() or 1))
    n_tok = tok_off.size - 1
    toks = stc.DeviceTokens(ctx, blob, tok_off, doc_off)
    cv = stc.CountVectorizer(vocabSize=a.vocab_size, ctx=ctx)
    model = cv.fit_tokens(toks)
    terms = model.vocabulary_bytes
    enc = stc.encode_tokens([terms])[:2]
    htf = stc.HashingTF(numFeatures=1 << 18, ctx=ctx)

    def drop(m):  # a model: freed without copying its vocabulary to the host first
        m.free(keep_host=False)

    def release(x):
        x.free()

    res = {
        "fit": timed(ctx, lambda: drop(cv.fit_tokens(toks)), a.warmup, a.repeats),
        "from_vocabulary": timed(ctx, lambda: drop(stc.CountVectorizerModel.from_vocabulary(None, ctx=ctx, encoded=enc)),
                                 a.warmup, a.repeats),
        "transform": timed(ctx, lambda: release(model.transform_tokens_device(toks)), a.warmup, a.repeats),
        "hashing_tf": timed(ctx, lambda: release(htf.transform_tokens_device(toks)), a.warmup, a.repeats),
    }
    for name, r in res.items():
        items = len(terms) if name == "from_vocabulary" else n_tok
        r["terms_per_s" if name == "from_vocabulary" else "tokens_per_s"] = items / (r["ms"] * 1e-3)
    d = model.transform_tokens_device(toks)
    out = dict(docs=a.docs, tokens_per_doc=a.tokens, n_tokens=int(n_tok), n_bytes=int(blob.size), words=a.words,
               vocabulary_terms=len(terms), transform_nnz=int(d.nnz), warmup=a.warmup, repeats=a.repeats, **res,
               transform_over_hashing_tf=res["transform"]["ms"] / res["hashing_tf"]["ms"])
    d.free()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
