"""NumPy restatement of the EM optimizer with fp32 state storage (stc_em_create_as(..., STC_F32), include/stc.h),
built on tests/em_oracle.py.

The contract: an fp32-state handle runs exactly the fp64 iteration on the values it stores and rounds each new
N_dk / N_wk element to the nearest fp32 once, when it is stored.  N_k is the fp64 column sum of the stored N_wk.
"""
import numpy as np

import em_oracle as E


def r32(x):
    """x rounded to the nearest fp32, as float64"""
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def step32(ndk, nwk, nk, src, term, cnt, alpha, eta):
    """one iteration of an fp32-state handle: the fp64 step, its N_dk' / N_wk' rounded, N_k' from the rounded N_wk'"""
    ndk2, nwk2, _ = E.step(ndk, nwk, nk, src, term, cnt, alpha, eta)
    nwk2 = r32(nwk2)
    return r32(ndk2), nwk2, nwk2.sum(axis=0)


def chain32(ndk, nwk, src, term, cnt, alpha, eta, n):
    """n iterations from the injected state (ndk, nwk), which is rounded as stc_em_set_state stores it"""
    ndk, nwk = r32(ndk), r32(nwk)
    nk = nwk.sum(axis=0)
    for _ in range(n):
        ndk, nwk, nk = step32(ndk, nwk, nk, src, term, cnt, alpha, eta)
    return ndk, nwk, nk
