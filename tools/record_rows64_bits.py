"""The fp64 rows E-step's outputs bit for bit: the cases tests/test_gpu_rows64_layout_bits.py compares with
tests/golden/rows64_parent_bits.npz, and the recorder of that fixture.

    python tools/record_rows64_bits.py [OUT.npz]          (on MI355X; STC_LIB selects the library)

The fixture was recorded once from the library built at the commit before the sb / pa LDS layouts changed
(lda_rows64.hip R64_SB_SWZ, R64_PA_LAYOUT).  A layout change moves addresses only, so γ, the iteration counts
and the stat rows must stay array_equal; record again only when the fixed point's arithmetic changes on purpose.

Documents: one per nnz of tests/test_gpu_rows64_sreduce.py's list (every row-set count 1..8 and its edges, an
empty document), V = 2048, λ and γ₀ from a seeded generator; k covers both ψ-wave modes at KL = 13, the
headline's four pad topics, KL = 7 and KL = 4 with an odd k.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 2048
NNZ = [1, 8, 31, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 168, 169, 192, 193, 224, 225, 256, 0]
KS = [100, 104, 64, 40, 7]
STAT_ROWS = 64  # the stat rows kept: term ids 0..63


def case(k):
    """(rows, λ, γ₀) of case k: numpy only."""
    rng = np.random.default_rng(8100 + k)
    rows = []
    for n in NNZ:
        ids = np.sort(rng.choice(V, size=n, replace=False)).astype(np.int32)
        rows.append((ids, rng.integers(1, 7, n).astype(np.float64)))
    lam = rng.gamma(100.0, 0.01, size=(V, k))
    g0 = rng.gamma(100.0, 0.01, size=(len(NNZ), k))
    return rows, lam, g0


def run(stc, ctx, k):
    """γ, iteration counts and the first STAT_ROWS stat rows of the device E-step on case k."""
    rows, lam, g0 = case(k)
    corpus = stc.CsrMatrix.from_rows(rows, V)
    h = stc.LdaHandle(ctx, k, V, dtype="f64")
    d = stc.DeviceCsr.upload(ctx, corpus, stc.STC_F64)
    h.set_corpus(d, corpus.num_rows)
    h.set_topics(lam)
    gamma, stat, iters = h.estep(np.arange(corpus.num_rows), g0, want_stat=True)
    return np.asarray(gamma), np.asarray(iters), np.asarray(stat)[:STAT_ROWS].copy()


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "rows64_parent_bits.npz")
    sys.path.insert(0, os.path.join(ROOT, "spark-text-clustering_amd"))
    import stc

    ctx = stc.Context.get(0)
    arrays = {}
    for k in KS:
        gamma, iters, stat = run(stc, ctx, k)
        arrays[f"gamma_{k}"], arrays[f"iters_{k}"], arrays[f"stat_{k}"] = gamma, iters, stat
        print(f"k = {k}: iterations {iters.tolist()}")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **arrays)
    print(f"wrote {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
