#!/usr/bin/env python3
"""Time the text preprocessing (text_prep.hip) on a corpus of the EN corpus's size — one JSON line.

Corpus: the 24 texts of tests/golden/books_text.json (8 languages) tiled to --mbytes (32) MB in --docs (51)
documents, encoded once; every timed call takes the host bytes, as the ABI does, so each includes the host → device
copy of the text (stc_tokenize, the yardstick, also copies its three output arrays back).

Timed, each as --warmup (3) untimed calls and then the median of --repeats (5) calls that end in a stream
synchronisation:
  prep_stem       stc_prep_tokens with the EN stop words and the Porter stemmer
  prep_nostem     the same without the stemmer
  prep_transform  prep_stem followed by CountVectorizerModel.transform_tokens_device over the reference's EN
                  vocabulary (the reference's BuildCountVector without the lemmatiser)
  tokenize        stc_tokenize (Spark's Tokenizer: lower-case, split on white space) on the same bytes
The line carries MB/s of input text for each and the prep_stem ÷ tokenize time ratio.

The per-kernel split comes from a profiler run of its own, of one warmed-up prep_transform:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_prep.py --once

    python tools/bench_prep.py [--mbytes 32] [--docs 51] [--warmup 3] [--repeats 5] [--once]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "spark-text-clustering_amd"), ROOT]
GOLDEN = os.path.join(ROOT, "tests", "golden")


def corpus(mbytes, n_docs):
    """the fixture's texts, repeated in turn until every one of n_docs documents holds its share of the bytes"""
    books = json.load(open(os.path.join(GOLDEN, "books_text.json"), encoding="utf-8"))
    texts = [e["text"].encode("utf-8") for lang, entries in books.items() if lang != "targets" for e in entries]
    per_doc = int(mbytes * 1e6) // n_docs
    docs, q = [], 0
    for _ in range(n_docs):
        parts, size = [], 0
        while size < per_doc:
            parts.append(texts[q % len(texts)])
            size += len(parts[-1]) + 1
            q += 1
        docs.append(b"\n".join(parts))
    return docs


def timed(ctx, fn, warmup, repeats):
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
    p.add_argument("--mbytes", type=float, default=32.0)
    p.add_argument("--docs", type=int, default=51)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--once", action="store_true", help="one warmed-up prep_transform and nothing else (for a profiler)")
    a = p.parse_args()
    import stc
    from stc import _lib as L

    ctx = stc.Context.get(0)
    text, off = stc.encode_texts(corpus(a.mbytes, a.docs))
    stop = stc.io.load_stop_words(os.path.join(GOLDEN, "stop_words_en.txt"))
    vocab = open(os.path.join(GOLDEN, "en_vocab.txt"), encoding="utf-8").read().split("\n")[:-1]
    model = stc.CountVectorizerModel.from_vocabulary(vocab, ctx=ctx)
    pre = {True: stc.TextPreprocessor(stopWords=stop, stem=True, ctx=ctx),
           False: stc.TextPreprocessor(stopWords=stop, stem=False, ctx=ctx)}

    def prep(stem):
        h = C.c_void_p()
        L.check(ctx.lib.stc_prep_tokens(ctx.handle, pre[stem]._handle(), L.ptr(text, C.c_uint8), text.size,
                                        L.ptr(off, C.c_int64), off.size - 1, C.byref(h)))
        return stc.DeviceTokens.from_handle(ctx, h)

    def prep_transform():
        t = prep(True)
        d = model.transform_tokens_device(t)
        nnz = d.nnz
        d.free()
        t.free()
        return nnz

    if a.once:
        prep_transform()
        ctx.synchronize()
        prep_transform()
        ctx.synchronize()
        return
    out_blob = np.zeros(text.size + text.size // 2 + 1, np.uint8)
    out_tok = np.zeros(text.size + off.size + 1, np.int64)
    out_doc = np.zeros(off.size, np.int64)
    nb, nt = C.c_int64(), C.c_int64()

    def tokenize():
        L.check(ctx.lib.stc_tokenize(ctx.handle, L.ptr(text, C.c_uint8), text.size, L.ptr(off, C.c_int64), off.size - 1,
                                     L.ptr(out_blob, C.c_uint8), out_blob.size, C.byref(nb), L.ptr(out_tok, C.c_int64),
                                     C.byref(nt), L.ptr(out_doc, C.c_int64)))

    res = {
        "prep_stem": timed(ctx, lambda: prep(True).free(), a.warmup, a.repeats),
        "prep_nostem": timed(ctx, lambda: prep(False).free(), a.warmup, a.repeats),
        "prep_transform": timed(ctx, prep_transform, a.warmup, a.repeats),
        "tokenize": timed(ctx, tokenize, a.warmup, a.repeats),
    }
    for r in res.values():
        r["mb_per_s"] = text.size / 1e6 / (r["ms"] * 1e-3)
    t = prep(True)
    out = dict(n_bytes=int(text.size), docs=a.docs, prep_tokens=int(t.n_tok), prep_bytes=int(t.n_bytes),
               tokenize_tokens=int(nt.value), transform_nnz=int(prep_transform()), stop_words=len(stop),
               vocabulary_terms=len(vocab), warmup=a.warmup, repeats=a.repeats, **res,
               prep_stem_over_tokenize=res["prep_stem"]["ms"] / res["tokenize"]["ms"])
    t.free()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
