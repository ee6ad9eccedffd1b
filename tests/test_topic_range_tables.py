"""The topic counts of tests/test_gpu_topic_range.py follow the kernels' sources (CPU only).

Its K list claims a value on each side of every width at which a training step changes kernel instantiation.
Here those widths are read from the .hip / .h text and the claim is recomputed, in both paddings (kp = k rounded
up to 2 in fp64, to 4 in fp32), so a retune that moves a width fails this test until the k list follows it.
"""
import os
import re

import test_gpu_topic_range as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spark-text-clustering_amd", "csrc")
PAD = {"f64": 2, "f32": 4}


def _src(name):
    with open(os.path.join(CSRC, name), encoding="utf-8") as f:
        return f.read()


def _const(text, name):
    """`constexpr <type> name = <integer expression>;`"""
    m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*([0-9*+\- ()/]+);", text)
    assert m, name
    return int(eval(m.group(1), {"__builtins__": {}}))  # digits and arithmetic only, by the pattern above


def _kps(ks, w):
    return {-(-k // w) * w for k in ks}


def _both_sides(width, what):
    """some k of K has kp = width and some k the next kp past it, in fp64's and in fp32's padding"""
    for dtype, w in PAD.items():
        kps = _kps(T.K, w)
        assert width in kps and width + w in kps, (what, width, dtype)


def _lambda_eeb_dispatch():
    """launch_lambda_eeb: ([(kp limit, Q)] of k_lambda_eeb, [(kp limit, Q)] of k_lambda_eeb_wide)"""
    src = _src("lda_mstep.hip")
    body = src[src.index("void launch_lambda_eeb("):src.index("__global__ __launch_bounds__(256) void k_colsum_reduce")]
    switch = int(re.search(r"if \(kp > (\d+)\) \{  // a row per workgroup", body).group(1))
    assert "const int qw = (kp + 255) / 256;" in body and "const int q = (kp + 63) / 64;" in body
    wide = [(int(a), int(b)) for a, b in re.findall(r"if \(qw <= (\d+)\) STC_LEEBW\((\d+)\);", body)]
    assert wide == [(2, 2), (4, 4), (8, 8), (16, 16)], wide  # Q = qw's bound: thread i owns topics i + 256·j
    assert 'else throw Error(STC_ERR_INVALID_ARG, "k > 4096 topics is not supported");' in body
    narrow = [(int(a), int(b)) for a, b in re.findall(r"if \(q <= (\d+)\) STC_LEEB\((\d+)\);", body)]
    last = int(re.search(r"else STC_LEEB\((\d+)\);", body).group(1))
    assert narrow == [(1, 1), (2, 2)] and 64 * last == switch, (narrow, last, switch)
    return ([(64 * a, q) for a, q in narrow] + [(switch, last)], [(256 * a, q) for a, q in wide])


def _lambda_q(kp):
    narrow, wide = _lambda_eeb_dispatch()
    for limit, q in narrow:
        if kp <= limit:
            return ("k_lambda_eeb", q)
    for limit, q in wide:
        if kp <= limit:
            return ("k_lambda_eeb_wide", q)
    raise AssertionError(kp)


def test_lambda_update_widths():
    narrow, wide = _lambda_eeb_dispatch()
    assert [w for w, _ in narrow + wide] == [64, 128, 256, 512, 1024, 2048, 4096]
    for width, _ in (narrow + wide)[:-1]:
        _both_sides(width, "launch_lambda_eeb")
    limit = wide[-1][0]  # the widest instantiation ends at the API's limit: only its near side exists
    assert f'STC_REQUIRE(cfg->k <= {limit}, "k <= {limit}");' in _src("lda_online.hip")
    assert max(T.K) == limit and limit - 1 in T.K
    for dtype, w in PAD.items():
        assert {_lambda_q(kp) for kp in _kps(T.K, w)} == set(x for x in
                                                                [("k_lambda_eeb", q) for _, q in narrow] +
                                                                [("k_lambda_eeb_wide", q) for _, q in wide]), dtype
        # the sliced run: test_sharded_mstep_slices_bit_identical has k = 12 and 300, SLICED_K the other instantiations
        assert {_lambda_q(kp) for kp in _kps(T.SLICED_K + (12, 300), w)} == {_lambda_q(kp) for kp in _kps(T.K, w)}
    # V = 200: full 64-row blocks and a ragged one; three slices of 128 rows, one ragged, one past V
    rb = _const(_src("lda_step_kernels.h"), "kRowsPerBlock")
    assert T.V // rb >= 2 and 0 < T.V % rb < rb
    vs = -(-(-(-T.V // 3)) // rb) * rb
    assert (vs, 0 < T.V - vs < vs, 2 * vs >= T.V) == (128, True, True)


def test_sstats_widths():
    src = _src("lda_sstats.hip")
    body = src[src.index("void launch_sstats("):src.index("__global__ __launch_bounds__(256) void k_entry_pairs")]
    assert "const int q = (kp + 63) / 64;" in body
    m = re.search(r"constexpr int QMAX = sizeof\(T\) == 8 \? (\d+) : (\d+);", body)
    qmax = {"f64": int(m.group(1)), "f32": int(m.group(2))}
    assert qmax == {"f64": 4, "f32": 8}
    assert [(int(a), int(b)) for a, b in re.findall(r"if \(q <= (\d+)\) sstats_q<T, (\d+)>", body)] == [(1, 1), (2, 2)]
    assert "else if (q <= 4 || QMAX == 4) sstats_q<T, 4>" in body and "else sstats_q<T, QMAX>" in body
    limit = int(re.search(r'if \(kp > (\d+)\) throw Error\(STC_ERR_INVALID_ARG, "k > 4096', body).group(1))
    assert limit == max(T.K)
    assert "const dim3 grid((unsigned)ceil_div(nchunks, 4), (unsigned)ceil_div(kp, 64 * Q));" in src
    for width in (64, 128, 256):  # Q = 1 | 2 | 4
        _both_sides(width, "launch_sstats")
    _both_sides(64 * qmax["f32"], "launch_sstats Q = 8")  # fp32: the whole row in one slab | two slabs
    for dtype, w in PAD.items():
        slab = 64 * qmax[dtype]
        slabs = {-(-kp // slab) for kp in _kps(T.K, w)}
        assert max(slabs) == limit // slab and {1, 2, 3} <= slabs, (dtype, slabs)  # 16 slabs (fp64) / 8 (fp32)
        assert any(kp > slab and kp % slab for kp in _kps(T.K, w)), dtype  # a ragged last slab


def test_estep_family_widths():
    wide = _src("lda_wide.hip")
    threads = _const(wide, "kWThreads")
    assert "return k <= kWThreads * 4 ? kWRows : 0;" in wide  # wide_row_cap: 0 past it — every document on k_estep
    cap = threads * 4
    assert cap in T.K and cap + 1 in T.K and cap == 2048
    for edge in (threads, 2 * threads):  # the many-topic kernel's Q = 1 | 2 | 4 topics per lane
        assert edge in T.K and edge + 1 in T.K, edge
    with open(T.__file__, encoding="utf-8") as f:  # the kernel-count check's threshold is that cap
        assert f"if k > {cap}:  # past wide_row_cap" in f.read()
    # the grid families: a k on each (fp64 rows64 k ≤ 104, fp32 grid k ≤ 128), and past both
    assert "return k <= 104 ? 32 * kMaxSets : 0;" in _src("lda_rows64.hip")
    assert any(k <= 104 for k in T.K) and any(104 < k <= 128 for k in T.K) and any(128 < k <= cap for k in T.K)


def test_workgroup_kernel_lds_edge():
    budget = _const(_src("lda_kernels.h"), "kLdsBudget")
    src = _src("lda.hip")
    for line in ("b += 2 * (size_t)kp * sizeof(T);", "b += (size_t)part_elems<T>(kp) * sizeof(T);",
                 "b += 16 * sizeof(double);", "return (256 * VecOf<T>::W > kp) ? 256 * VecOf<T>::W : kp;",
                 "if (fixed >= (size_t)kLdsBudget) return 0;",
                 # a launch whose fixed arrays pass the budget registers their size
                 "const size_t want = lds > (size_t)kLdsBudget ? lds : (size_t)kLdsBudget;"):
        assert line in src, line

    def fixed(kp, size, w):
        return 2 * kp * size + max(256 * w, kp) * size + 16 * 8

    limit = max(T.K)
    at = min(kp for kp in range(2, limit + 1, 2) if fixed(kp, 8, 2) >= budget)
    over = min(kp for kp in range(2, limit + 1, 2) if fixed(kp, 8, 2) > budget)
    assert (at, over) == (3408, 3410)
    assert {at - 2, at, over} <= set(T.LDS_EDGE_K) and all(k % 2 == 0 and k > 2048 for k in T.LDS_EDGE_K)
    assert fixed(limit, 8, 2) == 24 * limit + 128 == 98432  # what k = 4095 / 4096 register (LDS: 160 KiB per CU)
    assert fixed(limit, 4, 4) < budget  # fp32 never reaches it


def test_alpha_step_widths():
    src = _src("lda_mstep.hip")
    body = src[src.index("void k_update_alpha("):src.index("void launch_init_lambda(")]
    assert body.count("for (int t = threadIdx.x; t < k; t += 256)") == 4  # one pass per thread to k = 256
    assert "for (int t = threadIdx.x; t <= k; t += 256) {" in src  # k_logphat_part
    assert 256 in T.K and 257 in T.K
    # gradf[k] and q[k] in dynamic LDS: the registered size holds the limit's
    assert "k_update_alpha<<<1, 256, 2 * sizeof(double) * k, s>>>(alpha, small, k, rho);" in body
    m = re.search(r"hipFuncAttributeMaxDynamicSharedMemorySize,\s*\(int\)\(2 \* sizeof\(double\) \* (\d+)\)\)", body)
    assert m and int(m.group(1)) == max(T.K)


def test_mixed_k_list_follows_the_sources():
    """tests/test_gpu_mixed_range.py's MIXED_K: a k on each side of every width at which a mixed step changes
    instantiation — the fp64 re-solve's family (rows64 and its KL dispatch, then the many-topic kernel), the fp32
    first pass's (grid, then the many-topic kernel and its row order), the many-topic kernel's limit — and, inside
    each rows64 instantiation, a k whose fp32 pitch (the one the re-solve runs at) is not the fp64 pitch."""
    import test_gpu_mixed_range as M

    ks = M.MIXED_K
    rows64 = _src("lda_rows64.hip")
    m = re.search(r"int rows64_row_cap\(int k\) \{ return k <= (\d+) \? 32 \* kMaxSets : 0; \}", rows64)
    rows64_limit = int(m.group(1))
    body = rows64[rows64.index("void launch_estep_rows64("):]
    kl = [(int(a), int(b)) for a, b in re.findall(r"if \(a\.k <= (\d+)\) launch_r<(\d+), kOne>", body)]
    assert kl == [(32, 4), (56, 7)], kl
    assert "else if (kTwo == 0 || a.kp > 64) launch_r<13, kTwo>" in body and "else launch_r<13, kOne>" in body
    assert "if (a.kp > 8 * 13 || a.kp < a.k || (a.kp & 1)) throw" in body and rows64_limit == 8 * 13
    kl.append((rows64_limit, 13))
    grid = _src("lda_grid.hip")
    body = grid[grid.index("int grid_row_cap(int k) {"):grid.index("int grid_onchip_rows(int k)")]
    grid_limit = max(int(x) for x in re.findall(r"if \(k <= (\d+)\) return 32 \* G\w+::RMAX;", body))
    assert "return 0;" in body and grid_limit == 128
    wide = _src("lda_wide.hip")
    assert "int wide_row_cap(int k) { return k <= kWThreads * 4 ? kWRows : 0; }" in wide
    wide_limit = 4 * _const(wide, "kWThreads")
    assert (rows64_limit, grid_limit, wide_limit) == (104, 128, 2048)
    for limit in (rows64_limit, grid_limit, wide_limit):  # the last k of a family and the first of the next
        assert limit in ks and limit + 1 in ks, limit
    assert any(rows64_limit < k <= grid_limit for k in ks)  # fp32 grid, fp64 many-topic kernel
    lo = 0
    for hi, width in kl:  # every rows64 instantiation, with a k whose two pitches differ
        inside = [k for k in ks if lo < k <= hi]
        assert inside and any(-(-k // 4) * 4 != -(-k // 2) * 2 for k in inside), (width, inside)
        assert all(-(-k // 4) * 4 <= 8 * width for k in inside), (width, inside)  # the fp32 pitch fits the slices
        lo = hi
    # KL = 13 runs with one ψ wave at kp ≤ 64 and two beyond: the differing pitch in both
    wide13 = [k for k in ks if kl[1][0] < k <= rows64_limit and -(-k // 4) * 4 != -(-k // 2) * 2]
    assert any(-(-k // 4) * 4 <= 64 for k in wide13) and any(-(-k // 4) * 4 > 64 for k in wide13), wide13
    # the many-topic kernel's Q = 1 | 2 | 4 topics per lane, and the limit of the API
    threads = _const(wide, "kWThreads")
    for edge in (threads, 2 * threads):
        assert edge in ks and edge + 1 in ks, edge
    assert min(ks) == min(T.K) and max(ks) == max(T.K)
    # the λ-update (it writes the Bp64 rows) and sstats instantiations at the fp32 pitch: those K reaches
    assert {_lambda_q(kp) for kp in _kps(ks, PAD["f32"])} == {_lambda_q(kp) for kp in _kps(T.K, PAD["f32"])}
    assert {1 << (-(-kp // 64) - 1).bit_length() for kp in _kps(ks, 4) if kp <= 256} == {1, 2, 4}  # sstats Q
    assert {1, 2, 3} <= {-(-kp // 512) for kp in _kps(ks, 4)} and any(kp > 512 and kp % 512 for kp in _kps(ks, 4))
    # the other cases' k: every k has a threshold percentile, the fixed lists sit in the families they name
    assert set(ks) | set(M.SLICED_K) | {M.GROUP_K} == set(M.RESOLVE_PCT)
    assert any(k <= rows64_limit for k in M.ALL_RESOLVED_K) and any(k > wide_limit for k in M.ALL_RESOLVED_K)
    assert any(grid_limit < k <= wide_limit for k in M.ALL_RESOLVED_K)
    assert [rows64_limit < k <= grid_limit for k in M.BOTH_LISTS_K] == [True, False, False]
    assert all(k <= wide_limit for k in M.BOTH_LISTS_K)
    rows = _const(wide, "kWRows")
    g128 = re.search(r"using G128 = GShape<\d+, \d+, (\d+), \d+>;", grid)
    assert "if (k <= 128) return 32 * G128::RMAX;" in grid
    grid_rows = 32 * int(g128.group(1))  # grid_row_cap(120)
    for edge in (rows, grid_rows):
        assert edge in M.LIST_LENGTHS and edge + 1 in M.LIST_LENGTHS, edge
    assert rows - 1 in M.LIST_LENGTHS and 0 in M.LIST_LENGTHS and max(M.LIST_LENGTHS) < M.LIST_V
    assert f"L->cfg.max_inner_iter = {M.ITER_CAP};" in _src("lda_online.hip")
    assert {_lambda_q(kp) for kp in _kps(M.SLICED_K, 4)} == {("k_lambda_eeb", 2), ("k_lambda_eeb", 4),
                                                            ("k_lambda_eeb_wide", 4)}


def test_shape_and_describe_cases():
    assert (T.V, T.D, T.BATCH, T.STEPS, T.FRAC) == (200, 40, 24, 3, 0.4)
    assert set(T.DESCRIBE_K) == {min(T.K), 100, max(T.K)}
    assert T.V * max(T.K) < 1 << 31  # stc_lda_describe's extent
    assert 'STC_REQUIRE(L->V * L->k < (int64_t(1) << 31), "describe: V*k must be < 2^31");' in _src("lda_online.hip")
