"""The fp64 rows E-step after an LDS layout change: every output bit the recorded library's.

lda_rows64.hip's sb / pa layouts (rows64_layout.h: R64_SB_SWZ, R64_PA_LAYOUT) move addresses only; the sums are
formed from the same values in orders that differ by commuted fp additions at most, so γ, the iteration counts
and the sufficient statistics must be array_equal to tests/golden/rows64_parent_bits.npz, recorded on MI355X by
tools/record_rows64_bits.py from the library of the commit before the layouts changed.  21 documents (every
row-set count and its edges), k over both ψ-wave modes, the pad topics, KL = 7 and KL = 4.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_rows64_bits as rec  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "rows64_parent_bits.npz")))


@pytest.mark.parametrize("k", rec.KS)
def test_outputs_bitwise_the_recorded_library(ctx, golden, k):
    import stc

    gamma, iters, stat = rec.run(stc, ctx, k)
    assert gamma.shape == (len(rec.NNZ), k) and stat.shape == (rec.STAT_ROWS, k)
    assert np.array_equal(iters, golden[f"iters_{k}"]), (iters.tolist(), golden[f"iters_{k}"].tolist())
    same = gamma == golden[f"gamma_{k}"]
    assert same.all(), f"γ differs in documents {sorted(set(np.nonzero(~same)[0].tolist()))}"
    assert np.array_equal(stat, golden[f"stat_{k}"])
