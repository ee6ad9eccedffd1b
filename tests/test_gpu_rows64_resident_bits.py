"""The fp64 rows E-step where a workgroup walks several documents, and on its ε'-visible path: every output
bit the recorded library's.

tests/test_gpu_rows64_layout_bits.py pins the fixed point's arithmetic on 21 documents, fewer than the resident
grid has workgroups, none of them with a visible ε'.  Here (tools/record_rows64_resident_bits.py): case A, 1,600
documents in one launch, so every workgroup of k_estep_rows64_pers takes several tickets; case B, 64 documents
whose ε' is visible in every iteration (the worker phase's ballot path, the ψ phase's digamma of
Σα + Σcts − Σ r·ε').  γ, the iteration counts and the sufficient statistics must be array_equal to
tests/golden/rows64_resident_parent_bits.npz, recorded on MI355X from the library of the commit before the ψ wave's
path through an iteration was shortened; and case A run 64 documents per launch must give every document the γ
and the iteration count of the one launch (nothing carried from one document of a workgroup to its next).
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_rows64_resident_bits as rec  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "rows64_resident_parent_bits.npz")))


@pytest.fixture(scope="module")
def case_a():
    return rec.case_a()


@pytest.fixture(scope="module")
def one_launch_a(ctx, case_a):
    import stc

    return rec.run(stc, ctx, case_a)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def check(golden, name, n_docs, gamma, iters, stat):
    assert gamma.shape == (n_docs, rec.K) and stat.shape == (rec.STAT_ROWS, rec.K)
    want = golden[f"{name}_iters"]
    assert np.array_equal(iters, want), f"iteration counts differ in documents {np.nonzero(iters != want)[0][:20].tolist()}"
    same = gamma[:rec.FULL_DOCS] == golden[f"{name}_gamma"]
    assert same.all(), f"γ differs in documents {sorted(set(np.nonzero(~same)[0].tolist()))}"
    sums = rec.bit_sums(gamma[rec.FULL_DOCS:])
    assert np.array_equal(sums, golden[f"{name}_gsum"]), \
        f"γ differs in documents {(rec.FULL_DOCS + np.nonzero(sums != golden[f'{name}_gsum'])[0])[:20].tolist()}"
    # bit patterns: case B's λ = 1e-3 terms have NaN / inf statistics (0 · inf in the recorded library too), and
    # NaN != NaN as values
    assert np.array_equal(bits(stat), bits(golden[f"{name}_stat"]))


def test_many_documents_per_workgroup_bitwise_the_recorded_library(golden, one_launch_a):
    gamma, iters, stat = one_launch_a
    assert rec.A_DOCS > 3 * 512
    check(golden, "a", rec.A_DOCS, gamma, iters, stat)


def test_visible_epsilon_bitwise_the_recorded_library(ctx, golden):
    import stc

    gamma, iters, stat = rec.run(stc, ctx, rec.case_b())
    check(golden, "b", rec.B_DOCS, gamma, iters, stat)


def test_launches_of_64_documents_give_the_one_launch(ctx, case_a, one_launch_a):
    import stc

    gamma, iters, _ = one_launch_a
    assert rec.A_DOCS // rec.A_CHUNK == 25
    g, it = rec.run_chunked(stc, ctx, case_a, rec.A_CHUNK)
    assert np.array_equal(it, iters), f"iteration counts differ in documents {np.nonzero(it != iters)[0][:20].tolist()}"
    same = (g == gamma).all(axis=1)
    assert same.all(), f"γ differs in documents {np.nonzero(~same)[0][:20].tolist()}"
