"""The fp64 rows E-step's six-row-set loop at every topics-per-lane width: every output bit the recorded
library's.

Documents of 161–192 terms keep five row sets in VGPRs and the sixth in LDS (RShape<KL, 5, 6>, R = 6): the one
loop of the common kernel whose Phase A and Phase B read LDS beside their FMAs.  The cases
(tools/record_rows64_r6_bits.py): three launches of 64 documents at k = 100, 40 and 24 — KL = 13 with two ψ
waves, KL = 7 and KL = 4 — whose nnz cycles through the eight edges at which a wave gains a row of set 5, through
160 and 129 (the R = 5 loop in the same launch), and whose last document has a visible ε' in every iteration.
γ₀ is injected.  γ, the iteration counts and the documents' stat rows must be equal as bit patterns to
tests/golden/rows64_r6_parent_bits.npz, recorded on MI355X from the library of the commit before the R = 6 loop
was re-scheduled (DESIGN.md §3 "r10").
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_rows64_r6_bits as rec  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "rows64_r6_parent_bits.npz")))


@pytest.fixture(scope="module")
def runs(ctx):
    import stc

    return {k: rec.run(stc, ctx, k) for k in rec.KS}


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def test_cases_cover_the_row_set_edges():
    assert rec.KS == [100, 40, 24] and rec.DOCS == 64
    assert set(rec.NNZ) == {161, 168, 169, 176, 177, 184, 185, 192, 160, 129}
    for k in rec.KS:
        rows, lam, g0 = rec.case(k)
        nnz = [len(ids) for ids, _ in rows]
        assert len(rows) == 64 and set(nnz) == set(rec.NNZ) and g0.shape == (64, k)
        # the visible-ε' terms are the last document's alone
        assert all((ids >= rec.B_TINY).all() for ids, _ in rows[:-1]) and (rows[-1][0] < rec.B_TINY).sum() == rec.B_TINY
        assert (lam[:rec.B_TINY] == 1e-3).all()


@pytest.mark.parametrize("k", rec.KS)
def test_r6_loop_bitwise_the_recorded_library(golden, runs, k):
    gamma, iters, stat = runs[k]
    assert gamma.shape == (rec.DOCS, k) and stat.shape == (rec.V, k)
    want = golden[f"iters_{k}"]
    assert np.array_equal(iters, want), f"iteration counts differ in documents {np.nonzero(iters != want)[0].tolist()}"
    same = (bits(gamma[:rec.FULL_DOCS]) == bits(golden[f"gamma_{k}"])).all(axis=1)
    assert same.all(), f"γ differs in documents {np.nonzero(~same)[0].tolist()}"
    sums = rec.bit_sums(gamma)
    assert np.array_equal(sums, golden[f"gsum_{k}"]), f"γ differs in documents {np.nonzero(sums != golden[f'gsum_{k}'])[0].tolist()}"
    # bit patterns: the λ = 1e-3 terms have NaN / inf statistics (0 · inf in the recorded library too)
    assert np.array_equal(bits(stat[:rec.FULL_ROWS]), bits(golden[f"stat_{k}"]))
    rsum = rec.bit_sums(stat)
    assert np.array_equal(rsum, golden[f"ssum_{k}"]), f"stat differs in rows {np.nonzero(rsum != golden[f'ssum_{k}'])[0][:20].tolist()}"


def test_the_run_is_not_trivial(runs):
    import stc  # noqa: F401

    iters = np.concatenate([runs[k][1] for k in rec.KS])
    assert iters.max() > 100, "no document past 100 iterations"
    assert iters.max() < 100000, "a document stopped at the iteration cap"  # lda_online.hip: max_inner_iter 0 → 100000
    assert iters.min() >= 1
