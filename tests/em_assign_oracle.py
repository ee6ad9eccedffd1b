"""NumPy restatement of [U] DistributedLDAModel.topicAssignments (spark-mllib 2.4.3), the checker of
stc_em_topic_assignments: per edge the first topic with the largest em_oracle.edge_factors value (Breeze
argmax returns the first index of the maximum; the normalisation of γ does not move it)."""
import numpy as np

import em_oracle as E

# The device forms (a·b)·(1/c), NumPy (a·b)/c: each a few units of 2^-53 from the exact factor.  An edge whose
# two largest factors are further apart than this (relatively) has one answer; a closer one may go either way.
DECIDED = 1e-12


def assignments(ndk, nwk, nk, src, term, alpha, eta):
    """(topic[E], margin[E]): np.argmax of the edge's factors (first maximum) and the relative gap between the
    largest and the second-largest factor (0 for an exact tie)"""
    f = E.edge_factors(ndk, nwk, nk, src, term, alpha, eta)
    topic = np.argmax(f, axis=1).astype(np.int32)
    if f.shape[0] == 0:
        return topic, np.zeros(0)
    top2 = np.partition(f, f.shape[1] - 2, axis=1)[:, -2:]
    return topic, (top2[:, 1] - top2[:, 0]) / top2[:, 1]


def compare(got, ndk, nwk, nk, src, term, alpha, eta):
    """the comparison rule of the GPU tests: a decided edge (margin > DECIDED) must match exactly, an undecided
    one must name a topic whose factor is within DECIDED (relative) of the maximum → (undecided edges, the
    smallest margin); asserts the rule"""
    f = E.edge_factors(ndk, nwk, nk, src, term, alpha, eta)
    topic, margin = assignments(ndk, nwk, nk, src, term, alpha, eta)
    got = np.asarray(got)
    assert got.shape == topic.shape and got.dtype == np.int32
    assert np.all((got >= 0) & (got < f.shape[1]))
    decided = margin > DECIDED
    bad = np.flatnonzero(decided & (got != topic))
    assert bad.size == 0, (bad[:10], got[bad[:10]], topic[bad[:10]], margin[bad[:10]])
    und = np.flatnonzero(~decided)
    fmax = f.max(axis=1)
    assert np.all(f[und, got[und]] >= fmax[und] * (1.0 - DECIDED))
    return int(und.size), float(margin.min()) if margin.size else np.inf
