#!/usr/bin/env python3
"""Time the EM optimizer's iteration (stc_em_next) and its topicAssignments pass — one JSON line per case.

Cases:
  golden   the reference's saved EN model's graph (tests/golden/LdaModel_EN_1591049082850: 51 documents,
           V = 39,380, 253,368 edges) at k = 5, from its saved state.  The model's own metadata records the
           reference's iterationTimes for exactly this graph (median 0.702 s per iteration over its 50, on an
           unknown PC under Spark local[*]); the line reports the ratio with that caveat.
  zipf     stc.synth.zipf_corpus, 100k documents × 200 tokens, V = 2^18, k = 100, from init_random.

Per case: --warmup (3) untimed iterations, then --iters (20) timed as ONE enqueued batch between two stream
synchronisations (an iteration has no host round trip), repeated --repeats (5) times; the line carries the
median and the spread.  edges·k per second and algorithmic bytes per second follow from the median.
Algorithmic bytes per iteration = for each of the two passes, the edge arrays once (4 B index + 8 B count
per edge) plus one gathered k-row (8k B) per edge: 2·E·(12 + 8k).  With --dtype f32 (the state stored as fp32,
stc_em_create_as) a gathered row is 4k B: 2·E·(12 + 4k).

The topicAssignments pass (stc_em_topic_assignments with every output NULL: the pass is enqueued, nothing is
copied out) is timed in the same run under the same discipline, from the state the timed iterations left:
--warmup untimed passes, --iters passes as one enqueued batch, --repeats times.  Its algorithmic bytes are the
term index, one gathered k-row and the 4 B result per edge: E·(8 + 8k), at --dtype f32 E·(8 + 4k).  The row pass it is to be read
against is one kernel of the iteration; its time comes from a kernel trace of this tool's run.

The ranked queries ("ranked" in the line; --no-ranked skips them): describe(10), describe(300), top_documents(10)
and top_topics(1) from the state the timed iterations left, each warm (one untimed call) as the median of
--repeats calls that end in the copy to the host — on the device selection (csrc/rank.hip) and, in the same
run, the way the question was answered before it: toLocal().describeTopics (the upload into an online handle
untimed, reported as to_local_ms) and a download of N_dk plus NumPy.  floor_bytes is one read of the matrix.

--devices 0,0 or 0,1,… runs the same cases through an EmGroup (stc_em_group: documents sharded over the members,
one all-reduce of N_wk' per iteration) and reports the same lines, with "devices" and "transport" added.  A
repeated device shows the decomposition's overhead on one GPU only: the in-process transport synchronises the
host inside every all-reduce, so it says nothing about scaling.  STC_GROUP_RCCL=1 with --devices 0 is the
one-member group over a real RCCL communicator.

    python tools/bench_em.py [--case golden|zipf|all] [--iters 20] [--warmup 3] [--repeats 5] [--workers N]
                             [--devices 0,0] [--dtype f64|f32]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "spark-text-clustering_amd"), ROOT]

GOLDEN_MODEL = os.path.join(ROOT, "tests", "golden", "LdaModel_EN_1591049082850")


def make_handle(stc, ctx, devices, corpus, k, alpha=-1.0, eta=-1.0, dtype="f64"):
    """(handle, synchronize): an EmHandle on ctx, or an EmGroup over `devices`.  The default dtype goes through
    the constructors' own default, so the tool also drives a library from before --dtype existed."""
    kw = {} if dtype == "f64" else {"dtype": dtype}
    if devices:
        g = stc.EmGroup(devices, corpus, k, alpha, eta, **kw)
        return g, g.synchronize
    dev = stc.DeviceCsr.upload(ctx, corpus, stc.STC_F64)
    h = stc.EmHandle(ctx, dev, k, alpha, eta, **kw)
    dev.free()
    return h, ctx.synchronize


def golden_case(stc, ctx, devices, dtype):
    m = stc.io.load_distributed(GOLDEN_MODEL)
    src, term, cnt = m["edges"]
    row = np.searchsorted(m["doc_ids"], src)
    order = np.argsort(row, kind="stable")
    indptr = np.zeros(m["doc_ids"].size + 1, np.int64)
    np.cumsum(np.bincount(row, minlength=m["doc_ids"].size), out=indptr[1:])
    corpus = stc.CsrMatrix(indptr, term[order], cnt[order], m["vocab_size"])
    h, sync = make_handle(stc, ctx, devices, corpus, m["k"], float(m["alpha"][0]), m["eta"], dtype)
    h.set_state(m["doc_topics"], m["topics"])
    ref = float(np.median(m["iteration_times"]))
    return h, sync, {"case": "golden", "reference_s_per_iteration": ref,
               "reference_note": "median of the saved model's 50 iterationTimes; unknown PC, Spark local[*]"}


def zipf_case(stc, ctx, devices, docs, tokens, vocab, k, workers, dtype):
    from stc import synth

    corpus = synth.zipf_corpus(docs, tokens, vocab, workers=workers)
    h, sync = make_handle(stc, ctx, devices, corpus, k, dtype=dtype)
    h.init_random(1)
    return h, sync, {"case": "zipf", "docs": docs, "tokens_per_doc": tokens}


def assign_pass_ms(ctx, h, sync, iters, warmup, repeats):
    """ms per topicAssignments pass without the copy-out, per repeat"""
    from stc import _lib as L

    fn = ctx.lib.stc_em_group_topic_assignments if hasattr(h, "members") else ctx.lib.stc_em_topic_assignments

    def enqueue(n):
        for _ in range(n):
            L.check(fn(h.handle, None, None, None))

    enqueue(warmup)
    sync()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        enqueue(iters)
        sync()
        ms.append((time.perf_counter() - t0) * 1e3 / iters)
    return ms


def median_ms(f, repeats):
    """median and spread of `repeats` timed calls of f() after one untimed call (every f ends in a copy to the host)"""
    f()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def ranked_queries(stc, ctx, h, repeats):
    """describe(10), describe(300), top_documents(10), top_topics(1): the device selection (stc_em_describe, …)
    against the way the same question was answered before it — toLocal().describeTopics (the V×k counts uploaded
    into an online LdaHandle once, untimed; each call its full segmented sort), and a download of N_dk plus NumPy
    (normalise, then a stable argsort per topic / per row).  floor_bytes: one read of the matrix, R·k·sizeof(T)."""
    elem = 4 if getattr(h, "dtype", "f64") == "f32" else 8
    out = {}
    local = None
    try:
        _, nwk, _ = h.state()
        alpha, eta = h.concentrations()
        t0 = time.perf_counter()
        local = stc.LDAModel.from_topics(nwk, np.full(h.k, alpha), eta, ctx=ctx)
        out["to_local_ms"] = (time.perf_counter() - t0) * 1e3
    except stc.StcError as e:  # a term without an edge has a 0 row, which the online handle refuses
        out["to_local_error"] = str(e)

    def host_top_documents(n):
        dt = h.state()[0]
        td = dt / dt.sum(axis=1, keepdims=True)
        return [np.argsort(-td[:, t], kind="stable")[:n] for t in range(h.k)]

    def host_top_topics(n):
        dt = h.state()[0]
        td = dt / dt.sum(axis=1, keepdims=True)
        return np.argsort(-td, axis=1, kind="stable")[:, :n]

    for name, n, dev, host, rows in (
            ("describe_10", 10, h.describe, local and local.describeTopics, h.vocab_size),
            ("describe_300", 300, h.describe, local and local.describeTopics, h.vocab_size),
            ("top_documents_10", 10, h.top_documents, host_top_documents, h.num_docs),
            ("top_topics_1", 1, h.top_topics, host_top_topics, h.num_docs)):
        r = {"device": median_ms(lambda: dev(n), repeats), "floor_bytes": rows * h.k * elem}
        if host:
            r["host"] = median_ms(lambda: host(n), repeats)
        out[name] = r
    if local:
        local._h.close()
    return out


def measure(stc, ctx, h, sync, info, iters, warmup, repeats, ranked):
    h.next(warmup)
    sync()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        h.next(iters)
        sync()  # a group: every member, once per timed batch
        ms.append((time.perf_counter() - t0) * 1e3 / iters)
    med = float(np.median(ms))
    E, k = h.num_edges, h.k
    row = (4 if getattr(h, "dtype", "f64") == "f32" else 8) * k  # bytes of one gathered state row
    algo_bytes = 2.0 * E * (12 + row)
    ll, lp = h.log_likelihood()
    ams = assign_pass_ms(ctx, h, sync, iters, warmup, repeats)
    if hasattr(h, "members"):
        info = dict(info, devices=h.devices, transport=h.transport())
    amed = float(np.median(ams))
    out = dict(info, dtype=getattr(h, "dtype", "f64"), n_docs=h.num_docs, vocab=h.vocab_size, k=k, edges=E, iters=iters, warmup=warmup, repeats=repeats,
               ms_per_iteration=med, ms_per_iteration_min=float(min(ms)), ms_per_iteration_max=float(max(ms)),
               edges_k_per_s=E * k / (med * 1e-3), algorithmic_bytes_per_iteration=algo_bytes,
               algorithmic_bytes_per_s=algo_bytes / (med * 1e-3), log_likelihood=ll, log_prior=lp,
               ms_per_assign_pass=amed, ms_per_assign_pass_min=float(min(ams)), ms_per_assign_pass_max=float(max(ams)),
               assign_algorithmic_bytes_per_s=E * (8.0 + row) / (amed * 1e-3))
    if "reference_s_per_iteration" in info:
        out["speedup_vs_reference"] = info["reference_s_per_iteration"] / (med * 1e-3)
    if ranked:
        out["ranked"] = ranked_queries(stc, ctx, h, repeats)
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--case", choices=("golden", "zipf", "all"), default="all")
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--docs", type=int, default=100_000)
    p.add_argument("--tokens", type=int, default=200)
    p.add_argument("--vocab", type=int, default=1 << 18)
    p.add_argument("--k", type=int, default=100)
    p.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1),
                   help="corpus-generation processes of the zipf case (1 under a profiler: nothing is forked)")
    p.add_argument("--devices", default="",
                   help="comma-separated device ids of an EmGroup (0,0: two members on device 0); empty: one EmHandle")
    p.add_argument("--dtype", choices=("f64", "f32"), default="f64",
                   help="how the handle or group stores N_dk / N_wk (f32: rounded when stored; arithmetic stays fp64)")
    p.add_argument("--no-ranked", action="store_true",
                   help="skip the ranked queries (describe, top_documents, top_topics: device against the host's way)")
    a = p.parse_args()
    import stc

    devices = [int(d) for d in a.devices.split(",") if d.strip()]
    ctx = stc.Context.get(0)
    for case in (("golden", "zipf") if a.case == "all" else (a.case,)):
        h, sync, info = (golden_case(stc, ctx, devices, a.dtype) if case == "golden" else
                         zipf_case(stc, ctx, devices, a.docs, a.tokens, a.vocab, a.k, a.workers, a.dtype))
        print(json.dumps(measure(stc, ctx, h, sync, info, a.iters, a.warmup, a.repeats, not a.no_ranked)), flush=True)
        h.close()


if __name__ == "__main__":
    main()
