"""A/B parity of two builds of libstc: the same E-step + a few next() steps, outputs compared bit for bit.

    python tools/ab_bitwise.py LIB_A LIB_B [--docs N] [--len TOKENS] [--k K] [--vocab V] [--dtype f64|f32|mixed]
                               [--mixed-resolve-iters N] [--env-a VAR=VAL] [--env-b VAR=VAL]

Each library runs in its own child process (STC_LIB selects it); the child writes γ, stat, the iteration
counts, topic_distribution and the four values of bound() on the same corpus and γ₀ (the no-stats and the
BOUND kernel instantiations), λ and α after three next() steps, and the launches per kernel family
(counters()["kernels"], so a changed dispatch shows up), to an .npz, and the parent compares the arrays with
array_equal.
--dtype goes to LdaHandle as it is, so "mixed" runs the mixed-precision handle on the fp64 corpus;
--mixed-resolve-iters is its re-solve threshold (0: the library's 500, which these small corpora never reach, so
that the fp64 re-solve only runs with a value below their fp32 iteration counts: the printed kernel counts end
in the re-solves and the re-solved documents).
Used to show a kernel variant (a build-time switch) or a host-side change leaves every output unchanged
before timing it.
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(out, docs, tokens, k, dtype, V, resolve_iters):
    sys.path.insert(0, os.path.join(ROOT, "spark-text-clustering_amd"))
    import stc
    from stc import synth

    ctx = stc.Context.get(0)
    corpus = synth.zipf_corpus(docs, tokens, V, seed=7)
    # a few longer rows: R = 6 (the LDS row set) and the 7-8-set launch
    rng = np.random.default_rng(3)
    lam = rng.gamma(100.0, 0.01, size=(V, k))
    g0 = rng.gamma(100.0, 0.01, size=(docs, k))
    h = stc.LdaHandle(ctx, k, V, dtype=dtype, mini_batch_fraction=0.05, seed=5, mixed_resolve_iters=resolve_iters)
    d = stc.DeviceCsr.upload(ctx, corpus, stc.STC_F32 if dtype == "f32" else stc.STC_F64)
    h.set_corpus(d, docs)
    h.set_topics(lam)
    gamma, stat, iters = h.estep(np.arange(docs), g0, want_stat=True)
    theta = h.topic_distribution(d, gamma0=g0)
    bound = h.bound(d, gamma0=g0)
    for _ in range(3):
        h.next(stats=False)
    kernels = h.counters()["kernels"]
    np.savez(out, gamma=gamma, stat=stat, iters=iters, topic_distribution=theta,
             bound=np.array([bound[n] for n in ("bound", "corpus_part", "topics_part", "token_count")]),
             lam=h.topics(), alpha=h.alpha(),
             kernels=np.array(list(kernels.values()), np.int64))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("libs", nargs=2)
    p.add_argument("--docs", type=int, default=20000)
    p.add_argument("--len", type=int, default=200, help="tokens per document")
    p.add_argument("--k", type=int, default=100)
    p.add_argument("--vocab", type=int, default=1 << 18)
    p.add_argument("--dtype", default="f64")
    p.add_argument("--mixed-resolve-iters", type=int, default=0, help="--dtype mixed: the re-solve threshold")
    p.add_argument("--child", default=None)
    p.add_argument("--env-a", action="append", default=[], help="VAR=VAL set for the first run only")
    p.add_argument("--env-b", action="append", default=[], help="VAR=VAL set for the second run only")
    a = p.parse_args()
    if a.child:
        child(a.child, a.docs, a.len, a.k, a.dtype, a.vocab, a.mixed_resolve_iters)
        return
    outs = []
    with tempfile.TemporaryDirectory() as td:
        for i, lib in enumerate(a.libs):
            out = os.path.join(td, f"{i}.npz")
            env = dict(os.environ, STC_LIB=os.path.abspath(lib))
            env.update(kv.split("=", 1) for kv in (a.env_a if i == 0 else a.env_b))
            subprocess.run([sys.executable, __file__, *a.libs, "--docs", str(a.docs), "--len", str(a.len), "--k", str(a.k),
                            "--vocab", str(a.vocab), "--dtype", a.dtype, "--mixed-resolve-iters",
                            str(a.mixed_resolve_iters), "--child", out], env=env, check=True)
            outs.append(dict(np.load(out)))
    ok = True
    for key in outs[0]:
        same = np.array_equal(outs[0][key], outs[1][key])
        ok &= same
        print(f"{key}: {'bitwise equal' if same else 'DIFFERENT'}"
              + ("" if same else f" (max abs diff {np.max(np.abs(outs[0][key] - outs[1][key])):.3e})"))
    print(f"mean iters {outs[0]['iters'].mean():.2f}, kernels {outs[0]['kernels'].tolist()}")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
