"""The document lengths of tests/test_gpu_bound_paths.py follow the kernels' sources (CPU only).

Its tables repeat row-capacity constants of the E-step kernels.  Here the constants are read from the .hip / .h
text and the tables recomputed from them, so a retune that moves a boundary fails this test until the lengths
follow it.
"""
import os
import re

import test_gpu_bound_paths as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spark-text-clustering_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name), encoding="utf-8") as f:
        return f.read()


def _const(text, name):
    """`constexpr <type> name = <integer expression>;` or `#define name <integer>`"""
    m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*([0-9*+\- ()/]+);", text) or \
        re.search(r"#define\s+" + name + r"\s+(\d+)\s*$", text, re.M)
    assert m, name
    return int(eval(m.group(1), {"__builtins__": {}}))  # digits and arithmetic only, by the patterns above


def test_rows64_sets():
    src = _src("lda_rows64.hip")
    onchip, most = _const(src, "kOnChipSets"), _const(src, "kMaxSets")
    m = re.search(r"using RCommon = RShape<KL, (\d+), kOnChipSets>;", src)
    assert m and re.search(r"using RLong = RShape<KL, kMaxSets, kMaxSets>;", src)
    assert (int(m.group(1)), onchip, most) == (T.ROWS64_REG_SETS, T.ROWS64_ONCHIP_SETS, T.ROWS64_MAX_SETS)
    assert "return k <= 104 ? 32 * kMaxSets : 0;" in src and "return k <= 104 ? 32 * kOnChipSets : 0;" in src
    # 5 sets in VGPRs, the 6th in LDS, 7–8 in the long pass, then the workgroup kernel
    for sets in (1, T.ROWS64_REG_SETS, T.ROWS64_ONCHIP_SETS, T.ROWS64_ONCHIP_SETS + 1, T.ROWS64_MAX_SETS):
        assert {32 * sets, 32 * sets + 1} <= set(T.GRID_LENGTHS), sets
    assert max(T.GRID_LENGTHS) > 32 * most
    assert max(T.GRID_K["f64"]) == 104 and min(T.WIDE_K["f64"]) == 105


def test_grid_shapes():
    src = _src("lda_grid.hip")
    shapes = {n: tuple(int(x) for x in a.split(","))
              for n, a in re.findall(r"using (G\w+) = GShape<([\d, ]+)>;", src)}
    assert {n: s[2] for n, s in shapes.items()} == T.GRID_RMAX
    assert f"if (d.nnz <= {T.GRID_R7_ROWS}) nonempty = grid_core<S, 7, STATS, BOUND>" in src
    assert T.GRID_R7_ROWS == 32 * 7
    # R ≤ G104::RMAX in the common kernel (G104L beyond), R = 7 up to 224 rows, R = 8; every shape caps at 8 sets
    for rows in (32, 32 * T.GRID_RMAX["G104"], T.GRID_R7_ROWS, 32 * T.GRID_RMAX["G104L"]):
        assert {rows, rows + 1} <= set(T.GRID_LENGTHS), rows
    assert {32 * T.GRID_RMAX[g] for g in ("G32", "G64", "G104L", "G128")} == {32 * T.ROWS64_MAX_SETS}
    assert max(T.GRID_LENGTHS) > 32 * max(T.GRID_RMAX.values())
    # k per shape: G32 ≤ 32 < G64 ≤ 64 < G104 ≤ 104 < G128 ≤ 128 < the many-topic kernel
    for edge in (32, 64, 104, 128):
        assert edge in T.GRID_K["f32"] and (edge + 1 in T.GRID_K["f32"] or edge + 1 in T.WIDE_K["f32"]), edge


def test_wide_rows():
    src = _src("lda_wide.hip")
    threads, waves_of, rows = _const(src, "kWThreads"), 64, _const(src, "kWRows")
    chunk, lds = _const(src, "kWChunk"), _const(src, "kWLds")
    assert rows == T.WIDE_MAX_ROWS and "return k <= kWThreads * 4 ? kWRows : 0;" in src
    # struct WLds<T>: xs[kWWaves][kWRows], rr[kWRows], red[2][kWWaves] of T; ids[kWRows] int; bd[kWWaves][4] double
    body = re.search(r"struct WLds \{(.*?)\};", src, re.S).group(1)
    fields = re.findall(r"^\s*(T|int|double) (\w+)((?:\[\w+\])+);", body, re.M)
    assert [(t, n, d) for t, n, d in fields] == [("T", "xs", "[kWWaves][kWRows]"), ("T", "rr", "[kWRows]"),
                                                  ("T", "red", "[2][kWWaves]"), ("int", "ids", "[kWRows]"),
                                                  ("double", "bd", "[kWWaves][4]")], fields
    assert "return (sizeof(WLds<T>) + 255) / 256 * 256;" in src
    waves = threads // waves_of
    nr64 = {q: _const(src, f"WIDE_NR64_Q{q}") for q in (1, 2, 4)}
    assert "(sizeof(T) == 4 && Q == 1) ? 176" in src and "(int)(128 * 4 / (sizeof(T) * Q)) / kWChunk * kWChunk" in src
    # wide_resident_rows counts the team kernels' register rows, which are the one-CU kernel's (no cut), and the
    # LDS rows planned with 256 B less
    assert "wide_nr_mc" not in src and "WIDE_MC_NR_CUT" not in src
    assert "return wide_nr<T, Q>() + wide_lds_plan<T, Q>(wide_lds_fixed<T>(), true).nl;" in src
    assert "const int nl = (int)((kWLds - fixed - (static_word ? 256 : 0)) / row_bytes);" in src
    for (dtype, q), table in T.WIDE_ROWS.items():
        size = 8 if dtype == "f64" else 4
        fixed = (size * (waves * rows + rows + 2 * waves) + 4 * rows + 8 * waves * 4 + 255) // 256 * 256
        nr = nr64[q] if size == 8 else 176 if q == 1 else 128 * 4 // (size * q) // chunk * chunk
        row_bytes = size * threads * q
        # the one-CU kernel keeps (kWLds − fixed) / row_bytes rows in LDS, the team size is planned with 256 B less
        assert (lds - fixed) // row_bytes == (lds - fixed - 256) // row_bytes
        assert table == (nr, nr + (lds - fixed - 256) // row_bytes), (dtype, q)
    for k in set(T.WIDE_K["f64"]) | set(T.WIDE_K["f32"]):
        lens = set(T.wide_lengths(k))
        for dtype in ("f64", "f32"):
            nr, res = T.WIDE_ROWS[dtype, T.wide_q(k)]
            assert {nr, nr + 1, res, res + 1, rows - 1, rows, rows + 1} <= lens, (dtype, k)
    # Q = 1, 2, 4 at both ends: k ≤ 512·Q
    for dtype in ("f64", "f32"):
        assert {threads, threads + 1, 2 * threads, 2 * threads + 1, 4 * threads} <= set(T.WIDE_K[dtype])
    assert [T.wide_q(k) for k in (threads, threads + 1, 2 * threads, 2 * threads + 1, 4 * threads)] == [1, 2, 2, 4, 4]


def test_workgroup_lds_rows():
    """lda.hip estep_lds_rows<T>(k, kp, P) with the handle's kp / P (lda_online.hip stc_lda_create)."""
    budget = _const(_src("lda_kernels.h"), "kLdsBudget")
    src, host = _src("lda.hip"), _src("lda_online.hip")
    for line in ("b += 2 * (size_t)kp * sizeof(T);", "b += (size_t)part_elems<T>(kp) * sizeof(T);",
                 "b += 16 * sizeof(double);", "b += (size_t)lds_rows * sizeof(int32_t);",
                 "b += 3 * (size_t)lds_rows * sizeof(T);", "b += (size_t)lds_rows * P * sizeof(T);",
                 "return (256 * VecOf<T>::W > kp) ? 256 * VecOf<T>::W : kp;", "return rows & ~3;",
                 "if (nnz <= a.lds_rows)"):
        assert line in src, line
    assert "const int W = L->dtype == STC_F32 ? 4 : 2;" in host
    assert "L->P = ((L->kp / W) % 2 == 1) ? L->kp : L->kp + W;" in host
    for (dtype, k), rows in T.WG_LDS_ROWS.items():
        size, w = (8, 2) if dtype == "f64" else (4, 4)
        kp = -(-k // w) * w
        p = kp if (kp // w) % 2 == 1 else kp + w
        fixed = 2 * kp * size + max(256 * w, kp) * size + 16 * 8
        assert rows == (budget - fixed) // (4 + 3 * size + p * size) & ~3, (dtype, k)
        assert {rows, rows + 1} <= set(T.wg_lengths(k))
