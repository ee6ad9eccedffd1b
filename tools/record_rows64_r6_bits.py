"""The fp64 rows E-step's six-row-set loop (documents of 161–192 terms: five row sets in VGPRs, the sixth in
LDS) at every topics-per-lane width, bit for bit: the cases tests/test_gpu_rows64_r6_bits.py compares with
tests/golden/rows64_r6_parent_bits.npz, and the recorder of that fixture.

    python tools/record_rows64_r6_bits.py [OUT.npz]          (on MI355X; STC_LIB selects the library)

The fixture was recorded once from the library built at the commit before the R = 6 loop's LDS reads and FMA
chains were re-scheduled (DESIGN.md §3 "r10": no fp operation, operand or summation order changed).  Record again
only when the fixed point's arithmetic changes on purpose.

Three launches of 64 documents, k = 100 (KL = 13, two ψ waves), 40 (KL = 7) and 24 (KL = 4): the three
RShape<KL, 5, 6> R = 6 loops.  nnz cycles through 161, 168, 169, 176, 177, 184, 185, 192 — the edges at which each
of the four waves gains a row of set 5 — and 160 and 129, which run the R = 5 loop in the same launch.  The last
document takes 32 of its 176 terms, the B_TINY terms whose λ is 1e-3 in every topic (m_v about −1000,
2^53·ε' at its 1e300 cap: ε' visible at fp64 resolution in every iteration, as in case B of
tools/record_rows64_resident_bits.py); no other document holds one of those terms.  λ is sparse (most of a
term's mass in a few topics) so that the fixed point takes long: some document runs past 100 iterations.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 512
KS = [100, 40, 24]
DOCS = 64
NNZ = [161, 168, 169, 176, 177, 184, 185, 192, 160, 129]
B_TINY = 32      # term ids 0..B_TINY-1: λ = 1e-3 in every topic; only the last document holds them
EPS_NNZ = 176    # the visible-ε' document (the last one)
FULL_DOCS = 16   # documents whose γ is kept in full (every nnz of the list); the rest, and the last, as bit sums
FULL_ROWS = 48   # stat rows kept in full (the B_TINY rows and 16 more); every row as a bit sum


def case(k):
    """(rows, λ, γ₀) of case k: numpy only."""
    rng = np.random.default_rng(10100 + k)
    rows = []
    for i in range(DOCS - 1):
        n = NNZ[i % len(NNZ)]
        ids = np.sort(B_TINY + rng.choice(V - B_TINY, size=n, replace=False)).astype(np.int32)
        rows.append((ids, rng.integers(1, 7, n).astype(np.float64)))
    nt = B_TINY
    tiny = rng.choice(B_TINY, size=nt, replace=False)
    rest = B_TINY + rng.choice(V - B_TINY, size=EPS_NNZ - nt, replace=False)
    ids = np.sort(np.concatenate([tiny, rest])).astype(np.int32)
    assert np.unique(ids).size == EPS_NNZ
    rows.append((ids, rng.integers(1, 7, EPS_NNZ).astype(np.float64)))
    lam = rng.gamma(0.05, 1.0, size=(V, k)) + 0.01
    lam[:B_TINY] = 1e-3
    g0 = rng.gamma(100.0, 0.01, size=(DOCS, k))
    return rows, lam, g0


def run(stc, ctx, k):
    """γ, iteration counts and the stat matrix of one device E-step over the case's 64 documents."""
    rows, lam, g0 = case(k)
    corpus = stc.CsrMatrix.from_rows(rows, V)
    h = stc.LdaHandle(ctx, k, V, dtype="f64")
    d = stc.DeviceCsr.upload(ctx, corpus, stc.STC_F64)
    h.set_corpus(d, corpus.num_rows)
    h.set_topics(lam)
    gamma, stat, iters = h.estep(np.arange(corpus.num_rows), g0, want_stat=True)
    return np.asarray(gamma), np.asarray(iters), np.asarray(stat)


def bit_sums(x):
    """one uint64 per row: the wrapping sum of the row's bit patterns"""
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64).sum(axis=1, dtype=np.uint64)


def pack(k, gamma, iters, stat):
    return {f"iters_{k}": iters, f"gamma_{k}": gamma[:FULL_DOCS].copy(), f"gsum_{k}": bit_sums(gamma),
            f"stat_{k}": stat[:FULL_ROWS].copy(), f"ssum_{k}": bit_sums(stat)}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "rows64_r6_parent_bits.npz")
    sys.path.insert(0, os.path.join(ROOT, "spark-text-clustering_amd"))
    import stc

    ctx = stc.Context.get(0)
    arrays = {}
    for k in KS:
        gamma, iters, stat = run(stc, ctx, k)
        arrays.update(pack(k, gamma, iters, stat))
        print(f"k = {k}: iterations {iters.tolist()}")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **arrays)
    print(f"wrote {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
