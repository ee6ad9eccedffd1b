"""The fp64 rows E-step on a resident grid that walks several documents per workgroup, and on its ε'-visible
path, bit for bit: the cases tests/test_gpu_rows64_resident_bits.py compares with
tests/golden/rows64_resident_parent_bits.npz, and the recorder of that fixture.

    python tools/record_rows64_resident_bits.py [OUT.npz]          (on MI355X; STC_LIB selects the library)

The fixture was recorded once from the library built at the commit before the ψ wave's path through an
iteration was shortened (DESIGN.md §3 "r09": the Σ|Δγ| read, the ε' test, the worker phase and the shift block of
the ψ chain moved; no fp operation, operand or order changed).  Record again only when the fixed point's
arithmetic changes on purpose.

Case A: 1,600 documents in one launch, more than three times the 512 workgroups a 256-CU device keeps resident,
so every workgroup of k_estep_rows64_pers walks several documents (state carried from one document to the next
would show); nnz cycles through every row-set count's edges, an empty document and the long-document kernel.
Case B: 64 documents a quarter of whose terms have λ = 1e-3 in every topic: their m_v is about −1000, 2^53·ε'
sits at its 1e300 cap, ε' is visible at fp64 resolution in every iteration and the worker phase's ballot path
and the ψ phase's digamma of Σα + Σcts − Σ r·ε' run every time.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 2048
K = 100
STAT_ROWS = 64  # the stat rows kept: term ids 0..63
FULL_DOCS = 64  # documents whose γ is kept in full; the rest as a wrapping sum of bit patterns

A_DOCS = 1600
A_NNZ = [1, 31, 32, 33, 96, 129, 160, 161, 168, 192, 0, 200, 256]
A_CHUNK = 64  # the same documents as A_DOCS / A_CHUNK launches

B_DOCS = 64
B_NNZ = [8, 33, 65, 100, 128]  # (a quarter of them from the B_TINY terms: at most 4·B_TINY)
B_TINY = 32  # term ids 0..B_TINY-1: λ = 1e-3 in every topic


def case_a():
    """(rows, λ, γ₀) of case A: numpy only."""
    rng = np.random.default_rng(9100)
    rows = []
    for i in range(A_DOCS):
        n = A_NNZ[i % len(A_NNZ)]
        ids = np.sort(rng.choice(V, size=n, replace=False)).astype(np.int32)
        rows.append((ids, rng.integers(1, 7, n).astype(np.float64)))
    lam = rng.gamma(100.0, 0.01, size=(V, K))
    g0 = rng.gamma(100.0, 0.01, size=(A_DOCS, K))
    return rows, lam, g0


def case_b():
    """(rows, λ, γ₀) of case B: numpy only."""
    rng = np.random.default_rng(9200)
    rows = []
    for i in range(B_DOCS):
        n = B_NNZ[i % len(B_NNZ)]
        nt = max(1, n // 4)
        tiny = rng.choice(B_TINY, size=nt, replace=False)
        rest = B_TINY + rng.choice(V - B_TINY, size=n - nt, replace=False)
        ids = np.sort(np.concatenate([tiny, rest])).astype(np.int32)
        assert (ids < B_TINY).any() and (ids >= B_TINY).any() and np.unique(ids).size == n
        rows.append((ids, rng.integers(1, 7, n).astype(np.float64)))
    lam = rng.gamma(100.0, 0.01, size=(V, K))
    lam[:B_TINY] = 1e-3
    g0 = rng.gamma(100.0, 0.01, size=(B_DOCS, K))
    return rows, lam, g0


def handle(stc, ctx, rows, lam):
    corpus = stc.CsrMatrix.from_rows(rows, V)
    h = stc.LdaHandle(ctx, K, V, dtype="f64")
    d = stc.DeviceCsr.upload(ctx, corpus, stc.STC_F64)
    h.set_corpus(d, corpus.num_rows)
    h.set_topics(lam)
    return h, d


def run(stc, ctx, case):
    """γ, iteration counts and the first STAT_ROWS stat rows of one device E-step over all of the case's documents."""
    rows, lam, g0 = case
    h, _d = handle(stc, ctx, rows, lam)
    gamma, stat, iters = h.estep(np.arange(len(rows)), g0, want_stat=True)
    return np.asarray(gamma), np.asarray(iters), np.asarray(stat)[:STAT_ROWS].copy()


def run_chunked(stc, ctx, case, chunk):
    """γ and iteration counts of the same documents, `chunk` of them per launch."""
    rows, lam, g0 = case
    h, _d = handle(stc, ctx, rows, lam)
    gamma = np.zeros((len(rows), K))
    iters = np.zeros(len(rows), np.int32)
    for s in range(0, len(rows), chunk):
        g, _, it = h.estep(np.arange(s, min(s + chunk, len(rows))), g0[s:s + chunk])
        gamma[s:s + chunk], iters[s:s + chunk] = g, it
    return gamma, iters


def bit_sums(gamma):
    """one uint64 per document: the wrapping sum of γ's bit patterns"""
    return np.ascontiguousarray(gamma).view(np.uint64).sum(axis=1, dtype=np.uint64)


def pack(name, gamma, iters, stat):
    return {f"{name}_iters": iters, f"{name}_stat": stat, f"{name}_gamma": gamma[:FULL_DOCS].copy(),
            f"{name}_gsum": bit_sums(gamma[FULL_DOCS:])}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "rows64_resident_parent_bits.npz")
    sys.path.insert(0, os.path.join(ROOT, "spark-text-clustering_amd"))
    import stc

    ctx = stc.Context.get(0)
    arrays = {}
    for name, case in (("a", case_a()), ("b", case_b())):
        gamma, iters, stat = run(stc, ctx, case)
        arrays.update(pack(name, gamma, iters, stat))
        print(f"case {name}: {len(iters)} documents, iterations min {iters.min()} max {iters.max()} mean {iters.mean():.2f}")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **arrays)
    print(f"wrote {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
