#!/usr/bin/env python3
"""Time the topic-coherence counting pass (stc_term_cooccurrence) against its two yardsticks — one JSON line.

Shape: bench.py's corpus (stc.synth.zipf_corpus, --docs 1,000,000 × --tokens 200, V = 2^18; --corpus zipf-lda: the
planted-topic corpus), resident on the device as STC_F64, and the top 10 and top 20 terms of the k = 100 planted
model (stc.synth.planted_topics of the same seed).  Timed per top-N, each call ending in its copy to the host:
  count        stc.term_cooccurrence(dev, terms)                     (csrc/coherence.hip)
Yardsticks:
  idf_fit_dev  stc_idf_fit_dev on the same matrix: it reads the same entries (index + value) once
  host         SciPy: the boolean contains-matrix as CSC (built once, timed apart), then S.T @ S per topic over the
               topic's columns — what a user without the library would write; timed once
Discipline: one process, --warmup untimed rounds, --repeats timed ones, medians and spreads; the device counts are
compared with the host's (==).  "bytes": what the pass must move — entries × (4 + value bytes) + the row offsets,
the term table (4·V, written once and gathered per entry), the slot list, and per workgroup its private counters
(4·k·n(n+1)/2, zeroed and written out once).

    python tools/bench_coherence.py [--docs 1000000] [--tokens 200] [--vocab 262144] [--k 100] [--repeats 5] [--no-host]
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


def timed(f, sync):
    sync()
    t0 = time.perf_counter()
    out = f()
    sync()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--tokens", type=int, default=200)
    ap.add_argument("--vocab", type=int, default=1 << 18)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--corpus", default="zipf", choices=["zipf", "zipf-lda"])
    ap.add_argument("--top", type=int, nargs="+", default=[10, 20])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=20261015)
    ap.add_argument("--workers", type=int, default=None)
    ap.add_argument("--no-host", action="store_true", help="skip the SciPy yardstick (and the equality check)")
    a = ap.parse_args()
    import stc
    from stc import _lib as L
    from stc import synth

    ctx = stc.Context.get(0)
    corpus = synth.make_corpus(a.corpus, a.docs, a.tokens, a.vocab, a.k, a.seed, workers=a.workers)
    D, V, k = corpus.num_rows, a.vocab, a.k
    lam = synth.planted_topics(V, k, seed=a.seed)
    order = np.argsort(-lam, axis=0, kind="stable")  # per topic: weight descending, term ascending
    terms = {n: np.ascontiguousarray(order[:n].T.astype(np.int32)) for n in a.top}
    dev = stc.DeviceCsr.upload(ctx, corpus, stc.STC_F64)
    sync = ctx.synchronize

    def idf_fit():
        h = C.c_void_p()
        L.check(ctx.lib.stc_idf_fit_dev(ctx.handle, dev.handle, 0, C.byref(h)))
        return h

    count_ms = {n: [] for n in a.top}
    idf_ms = []
    got = {}
    for rep in range(a.warmup + a.repeats):
        for n in a.top:
            ms, got[n] = timed(lambda: stc.term_cooccurrence(dev, terms[n]), sync)
            if rep >= a.warmup:
                count_ms[n].append(ms)
        ms, h = timed(idf_fit, sync)
        ctx.lib.stc_didf_free(h)
        if rep >= a.warmup:
            idf_ms.append(ms)

    host, check = None, None
    if not a.no_host:
        import scipy.sparse as sp

        t0 = time.perf_counter()
        b = sp.csr_matrix((np.ones(corpus.nnz, np.int32), corpus.indices, corpus.indptr), shape=(D, V))
        b.data[corpus.values <= 0] = 0
        b.eliminate_zeros()
        b = b.tocsc()
        host = {"build_csc_ms": (time.perf_counter() - t0) * 1e3, "products_ms": {}}
        check = {}
        for n in a.top:
            t0 = time.perf_counter()
            codf = np.stack([np.asarray((b[:, terms[n][t]].T @ b[:, terms[n][t]]).todense(), np.int64) for t in range(k)])
            host["products_ms"][str(n)] = (time.perf_counter() - t0) * 1e3
            df = np.stack([np.diag(codf[t]) for t in range(k)])
            check[str(n)] = bool(np.array_equal(got[n][0], df) and np.array_equal(got[n][1], codf) and got[n][2] == D)

    med = lambda v: float(np.median(v))
    idf_med = med(idf_ms)
    nnz = int(corpus.nnz)
    out = {
        "tool": "bench_coherence", "corpus": a.corpus, "docs": D, "tokens": a.tokens, "vocab": V, "k": k, "nnz": nnz,
        "value_dtype": "f64", "repeats": a.repeats, "warmup": a.warmup,
        "count_ms": {str(n): med(v) for n, v in count_ms.items()},
        "count_min_max_ms": {str(n): [float(min(v)), float(max(v))] for n, v in count_ms.items()},
        "idf_fit_dev_ms": idf_med, "idf_fit_dev_min_max_ms": [float(min(idf_ms)), float(max(idf_ms))],
        "count_over_idf": {str(n): med(v) / idf_med for n, v in count_ms.items()},
        "host_scipy": host, "counts_equal_host": check,
        "coherence_mean": {str(n): {m: float(stc.coherence(got[n][0], got[n][1], got[n][2], measure=m)[0].mean())
                                    for m in ("umass", "npmi")} for n in a.top},
        "bytes": {"entries": nnz * (4 + 8) + 8 * (D + 1), "term_table": 4 * V,
                  "slots": {str(n): 8 * k * n for n in a.top},
                  "counters_per_workgroup": {str(n): 4 * k * n * (n + 1) // 2 for n in a.top},
                  "result": {str(n): 8 * k * n * (n + 1) for n in a.top}},
    }
    print(json.dumps(out))
    dev.free()


if __name__ == "__main__":
    main()
