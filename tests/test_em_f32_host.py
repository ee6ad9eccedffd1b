"""CPU: the fp32-state surface of the EM optimizer (stc_em_create_as, stc_em_state_dtype, stc_em_group_create_as)
is declared, exported and guarded before any GPU call, and the NumPy restatement of fp32 storage
(tests/em_f32_oracle.py) stays where it was measured against the fp64 chain.

Bound 1e-5 for ten iterations on the golden graph, chain32 against fp64: measured ≤ 5.5e-6 (k = 5: N_dk 1.95e-6,
N_wk 4.97e-6; k = 100: 2.33e-6, 5.50e-6).  Ten roundings of 2^-24 = 6e-8 each, fed back through the iteration:
the figure is what fp32 storage costs, and it pins the helper the GPU tests compare against."""
import ctypes
import os
import re

import numpy as np
import pytest

import em_f32_oracle as F
import em_oracle as E
from helpers import GOLDEN, random_corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_MODEL = os.path.join(GOLDEN, "LdaModel_EN_1591049082850")
NEW = ("stc_em_create_as", "stc_em_state_dtype", "stc_em_group_create_as")


def rel_err(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    zero = ref == 0.0
    assert np.all(got[zero] == 0.0)
    return float(np.max(np.abs(got[~zero] - ref[~zero]) / np.abs(ref[~zero]))) if not zero.all() else 0.0


def test_the_header_the_signatures_and_the_library_have_the_entry_points():
    import stc
    from stc import _lib

    header = open(os.path.join(ROOT, "include", "stc.h")).read()
    lib = stc.load()
    for name in NEW:
        assert re.search(r"^\s*int\s+" + name + r"\s*\(", header, re.M), name
        assert name in _lib.SIGNATURES, name
        f = getattr(lib, name)
        assert f.restype is ctypes.c_int and list(f.argtypes) == _lib.SIGNATURES[name][1]
    # the dtype sits before the out pointer, after stc_em_create's / stc_em_group_create's arguments
    for plain, typed in (("stc_em_create", "stc_em_create_as"), ("stc_em_group_create", "stc_em_group_create_as")):
        a, b = _lib.SIGNATURES[plain][1], _lib.SIGNATURES[typed][1]
        assert b[:-2] == a[:-1] and b[-2] is ctypes.c_int and b[-1] == a[-1]
    assert lib.stc_abi_version() == 2
    assert "2^-126" in header  # the contract names what it leaves unpinned
    # NULL handles are refused by the argument check, before anything touches a device
    t = ctypes.c_int32(-1)
    assert lib.stc_em_state_dtype(None, ctypes.byref(t)) == stc.STC_ERR_INVALID_ARG
    h = ctypes.c_void_p()
    assert lib.stc_em_create_as(None, None, 5, -1.0, -1.0, stc.STC_F32, ctypes.byref(h)) == stc.STC_ERR_INVALID_ARG


class _NoGpu:
    """stands where a Context / DeviceCsr would: any use of it is a GPU call that should not have happened"""

    def __getattr__(self, name):
        raise AssertionError(f"touched .{name} before the dtype was checked")


@pytest.mark.parametrize("dtype", ["mixed", "f16"])
def test_handles_reject_other_dtypes_before_any_gpu_call(dtype):
    import stc

    corpus = random_corpus(np.random.default_rng(1), 6, 20)
    with pytest.raises(ValueError):
        stc.EmHandle(_NoGpu(), _NoGpu(), 5, dtype=dtype)
    with pytest.raises(ValueError):
        stc.EmGroup([0, 0], corpus, 5, dtype=dtype)


def test_mllib_lda_with_em_refuses_mixed():
    import stc

    corpus = random_corpus(np.random.default_rng(2), 6, 20)
    lda = stc.MllibLDA(_NoGpu()).setOptimizer("em").setK(5).setMaxIterations(1)
    lda.dtype = "mixed"
    with pytest.raises(ValueError):
        lda.run(corpus)
    lda.setDevices([0, 0])
    with pytest.raises(ValueError):
        lda.run(corpus)


def test_r32_and_the_step():
    x = np.array([0.0, 1.0, 1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50, 1.0 + 3 * 2.0 ** -24, 0.1, 1e10])
    # ties to even (1 + 2^-24 → 1, 1 + 3·2^-24 → 1 + 2^-22), anything past the midpoint goes up
    assert F.r32(x).tolist() == [0.0, 1.0, 1.0, 1.0 + 2.0 ** -23, 1.0 + 2.0 ** -22, float(np.float32(0.1)), 1e10]
    m = random_corpus(np.random.default_rng(3), 20, 60)
    k = 5
    src, term, cnt = E.edges_of(m)
    alpha, eta = E.resolve(k)
    rng = np.random.default_rng(4)
    ndk, nwk = E.mask_state(F.r32(rng.uniform(0.5, 5.0, (20, k))), F.r32(rng.uniform(0.5, 5.0, (60, k))), src, term)
    nk = nwk.sum(axis=0)
    ref = E.step(ndk, nwk, nk, src, term, cnt, alpha, eta)
    got = F.step32(ndk, nwk, nk, src, term, cnt, alpha, eta)
    assert np.array_equal(got[0], F.r32(ref[0])) and np.array_equal(got[1], F.r32(ref[1]))
    assert np.array_equal(got[2], got[1].sum(axis=0))  # N_k of the stored values, not the rounded fp64 N_k
    assert all(np.array_equal(a, F.r32(a)) for a in got[:2])
    assert 0.0 < rel_err(got[1], ref[1]) <= 2.0 ** -24
    one = F.chain32(ndk, nwk, src, term, cnt, alpha, eta, 1)
    assert all(np.array_equal(a, b) for a, b in zip(one, got))


@pytest.fixture(scope="module")
def golden():
    import stc

    m = stc.io.load_distributed(REF_MODEL)
    return (m,) + E.edges_of_model(m)


@pytest.mark.parametrize("k", [5, 100])
def test_ten_golden_iterations_of_chain32_stay_near_fp64(golden, k):
    m, src, term, cnt = golden
    D, V = m["doc_ids"].size, m["vocab_size"]
    rng = np.random.default_rng(400 + k)
    alpha, eta = E.resolve(k)
    ndk0, nwk0 = rng.uniform(0.5, 5.0, size=(D, k)), rng.uniform(0.5, 5.0, size=(V, k))
    ref = E.iterate(ndk0, nwk0, src, term, cnt, alpha, eta, 10)  # every vertex of the golden graph has an edge
    got = F.chain32(ndk0, nwk0, src, term, cnt, alpha, eta, 10)
    errs = [rel_err(g, r) for g, r in zip(got, ref)]
    print(f"golden graph, k={k}, 10 iterations, chain32 against fp64: N_dk {errs[0]:.3g} N_wk {errs[1]:.3g} "
          f"N_k {errs[2]:.3g}")
    assert max(errs) <= 1e-5, errs
    assert max(errs) > 1e-9  # it is not the fp64 chain
