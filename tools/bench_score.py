#!/usr/bin/env python3
"""Time the clustering report's questions on the device against the host path — one JSON line.

Shape: bench.py's (stc.synth.zipf_corpus, --docs 1,000,000 × --tokens 200, V = 2^18, k = 100, fp64, λ from
init_random).  The same answers two ways:
  (a) device   LDAModel.score + mainTopics + members + importantTerms(100, 300, 10)    (stc_lda_score, stc_score_*)
  (b) host     LDAModel.transform (γ copied out, normalised on the host) + NumPy argmax (last maximum) / stable
               argsort for the members + describeTopics(300) + a NumPy restatement of the term lists.  The term
               lists are restated for the first --host-term-docs documents (a Python loop per document) and the
               time is scaled to the corpus; the line says so.
Discipline: one process, the corpus resident on the device for both paths, --warmup untimed rounds, --repeats timed
ones, medians and spreads reported; each stage ends in its copy to the host.  "estep_bound_ms" is stc_lda_bound over
the same documents: the same E-step plus its bound epilogue and two reductions, with nothing but four numbers copied
out — an upper estimate of the E-step's share of either path.  "bytes": what each new kernel must move (header of
csrc/lda_score.hip), to be read against the stage's time.

    python tools/bench_score.py [--docs 1000000] [--tokens 200] [--vocab 262144] [--k 100] [--repeats 5] [--warmup 1]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "spark-text-clustering_amd"), ROOT]


def timed(f, sync):
    sync()
    t0 = time.perf_counter()
    out = f()
    sync()
    return (time.perf_counter() - t0) * 1e3, out


def host_terms(corpus, topic, sets, rows, doc_terms=100, n=10):
    out = []
    for d in rows:
        i, v = corpus.row(d)
        o = np.lexsort((i, -v))[:doc_terms]
        out.append(i[o][sets[topic[d], i[o]]][:n] if topic[d] >= 0 else i[:0])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--tokens", type=int, default=200)
    ap.add_argument("--vocab", type=int, default=1 << 18)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-term-docs", type=int, default=2000)
    ap.add_argument("--workers", type=int, default=None)
    a = ap.parse_args()
    import stc
    from stc import synth

    ctx = stc.Context.get(0)
    corpus = synth.zipf_corpus(a.docs, a.tokens, a.vocab, workers=a.workers)
    D, V, k = corpus.num_rows, a.vocab, a.k
    h = stc.LdaHandle(ctx, k, V, dtype="f64", seed=1)
    h.init_random(1)
    model = stc.LDAModel(h)
    dev = stc.DeviceCsr.upload(ctx, corpus, stc.STC_F64)
    sync = ctx.synchronize
    stages = {n: [] for n in ("score", "main_topics", "members", "important_terms", "transform", "host_argmax",
                              "host_members", "describe300", "host_terms_scaled")}
    check = {}
    for rep in range(a.warmup + a.repeats):
        t = {}
        t["score"], s = timed(lambda: h.score(dev, model.gammaSeed), sync)
        t["main_topics"], (topic, weight, counts) = timed(s.mainTopics, sync)
        t["members"], (indptr, rows) = timed(s.members, sync)
        t["important_terms"], (idx, val, cnt) = timed(lambda: s.importantTerms(dev, 100, 300, 10), sync)
        s.close()
        t["transform"], theta = timed(lambda: h.topic_distribution(dev, model.gammaSeed), sync)
        t0 = time.perf_counter()
        h_topic = (k - 1 - np.argmax(theta[:, ::-1], axis=1)).astype(np.int32)
        h_topic[np.diff(corpus.indptr) == 0] = -1
        t["host_argmax"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        keep = np.flatnonzero(h_topic >= 0)
        h_rows = keep[np.argsort(h_topic[keep], kind="stable")]
        t["host_members"] = (time.perf_counter() - t0) * 1e3
        t["describe300"], (d_idx, _) = timed(lambda: h.describe(300), sync)
        sets = np.zeros((k, V), bool)
        np.put_along_axis(sets, d_idx.astype(np.int64), True, axis=1)
        sub = np.arange(min(a.host_term_docs, D))
        t0 = time.perf_counter()
        h_terms = host_terms(corpus, h_topic, sets, sub)
        t["host_terms_scaled"] = (time.perf_counter() - t0) * 1e3 * D / max(sub.size, 1)
        if rep >= a.warmup:
            for n, v in t.items():
                stages[n].append(v)
        check = {"main_topics_equal": bool(np.array_equal(topic, h_topic)), "members_equal": bool(np.array_equal(rows, h_rows)),
                 "terms_equal_on_sample": all(np.array_equal(idx[d, :cnt[d]], h_terms[j]) for j, d in enumerate(sub))}
    med = {n: float(np.median(v)) for n, v in stages.items()}
    spread = {n: [float(min(v)), float(max(v))] for n, v in stages.items()}
    est = []
    for _ in range(a.warmup + a.repeats):
        ms, _ = timed(lambda: h.bound(dev, model.gammaSeed), sync)
        est.append(ms)
    device_ms = med["score"] + med["main_topics"] + med["members"] + med["important_terms"]
    host_ms = med["transform"] + med["host_argmax"] + med["host_members"] + med["describe300"] + med["host_terms_scaled"]
    nnz = corpus.nnz
    print(json.dumps({
        "tool": "bench_score", "docs": D, "tokens": a.tokens, "vocab": V, "k": k, "nnz": int(nnz), "dtype": "f64",
        "repeats": a.repeats, "warmup": a.warmup, "median_ms": med, "min_max_ms": spread,
        "device_path_ms": device_ms, "host_path_ms": host_ms, "host_terms_sampled_docs": int(min(a.host_term_docs, D)),
        "estep_bound_ms": float(np.median(est[a.warmup:])),
        "bytes": {"widen_rowsum": 16 * D * k + 8 * D, "main_topic": 8 * D * k + 8 * D + 12 * D,
                  "grouping": 3 * 4 * D + 8 * int((topic >= 0).sum()), "select_lambda_per_pass": 8 * V * k,
                  "terms_select": 12 * int(nnz) + 8 * (D + 1) + 4 * D + 12 * D * 10},
        "check": check}))
    dev.free()
    h.close()


if __name__ == "__main__":
    main()
