"""The LDS bank model of the fp64 rows E-step's sb / pa exchanges (csrc/rows64_layout.h), on the CPU.

The header is plain constexpr C++: the kernel takes its addresses from its index functions and its
static_asserts prove the shipped layouts at library build time.  Here a stand-alone host program that includes
only that header prints the modelled extra LDS cycles (SQ_LDS_BANK_CONFLICT's unit) per document-iteration for
each layout and (KL, ψ waves) class; the numbers are the ones DESIGN.md §3 "r08" reports.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spark-text-clustering_amd", "csrc")

PROGRAM = r"""
#include "rows64_layout.h"
#include <cstdio>
using namespace stc::lda::r64;
int main() {
  const int kl[3] = {13, 7, 4};
  for (int s = 0; s < 2; ++s) {
    for (int i = 0; i < 3; ++i) std::printf("sb_store KL=%d swz=%d %d\n", kl[i], s, sb_store_extra(kl[i], s != 0));
    // the kernel's (KL, psi waves) classes by k: 65-104 (13, 2), 57-64 (13, 1), 33-56 (7, 1), 1-32 (4, 1)
    std::printf("sb_read KL=13 npsi=2 swz=%d %d\n", s, sb_read_extra_max(65, 104, 2, s != 0));
    std::printf("sb_read KL=13 npsi=1 swz=%d %d\n", s, sb_read_extra_max(57, 64, 1, s != 0));
    std::printf("sb_read KL=7 npsi=1 swz=%d %d\n", s, sb_read_extra_max(33, 56, 1, s != 0));
    std::printf("sb_read KL=4 npsi=1 swz=%d %d\n", s, sb_read_extra_max(1, 32, 1, s != 0));
    std::printf("sb_read k=100 swz=%d %d\n", s, sb_read_extra(100, 2, s != 0));
    for (int r = 1; r <= 8; ++r) {
      std::printf("pa_store R=%d layout=%d %d\n", r, s, pa_store_extra(r, s));
      std::printf("pa_read R=%d layout=%d %d\n", r, s, pa_read_extra(r, s));
    }
    std::printf("pa_rows_fit layout=%d %d\n", s, (int)(pa_rows_fit(s, 48) && pa_rows_fit(s, 64)));
    for (int i = 0; i < 3; ++i) std::printf("sb_pair_adjacent KL=%d swz=%d %d\n", kl[i], s, (int)sb_pair_adjacent(kl[i], s != 0));
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("rows64_layout")
    src, exe = str(d / "model.cpp"), str(d / "model")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", CSRC, src, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    print(out)
    return {line.rsplit(" ", 1)[0]: int(line.rsplit(" ", 1)[1]) for line in out.splitlines()}


def test_swizzled_sb_is_conflict_free(model):
    """(KL, ψ waves) = (13, 2), (13, 1), (7, 1): no extra cycle in the stores or the reads, at every k of the class."""
    assert model["sb_store KL=13 swz=1"] == 0
    assert model["sb_store KL=7 swz=1"] == 0
    assert model["sb_read KL=13 npsi=2 swz=1"] == 0
    assert model["sb_read KL=13 npsi=1 swz=1"] == 0
    assert model["sb_read KL=7 npsi=1 swz=1"] == 0


def test_kl4_bound(model):
    """k ≤ 32: the reads are conflict-free; the stores stay 2-way (8 extra cycles, 56 before): at four slots per
    topic a store's 16 lanes reach eight distinct slots."""
    assert model["sb_read KL=4 npsi=1 swz=1"] == 0
    assert model["sb_store KL=4 swz=1"] == 8
    assert model["sb_store KL=4 swz=0"] == 56


def test_unswizzled_sb_as_reported(model):
    assert [model[f"sb_store KL={kl} swz=0"] for kl in (13, 7)] == [76, 40]
    assert model["sb_read k=100 swz=0"] == 24 and model["sb_read k=100 swz=1"] == 0
    assert [model[f"sb_read KL={kl} npsi={n} swz=0"] for kl, n in ((13, 2), (13, 1), (7, 1), (4, 1))] == [24, 8, 8, 4]


def test_pa_layouts(model):
    """Layout 1: no extra cycle in a store or a worker read at any row-set count, rows disjoint inside layout 0's
    footprint; layout 0: 2-way stores in every group (16 extra cycles per row set over the four waves)."""
    for r in range(1, 9):
        assert model[f"pa_store R={r} layout=1"] == 0 and model[f"pa_read R={r} layout=1"] == 0
        assert model[f"pa_store R={r} layout=0"] == 16 * r and model[f"pa_read R={r} layout=0"] == 0
    assert model["pa_rows_fit layout=0"] == 1 and model["pa_rows_fit layout=1"] == 1


def test_one_store_address_per_lane(model):
    for kl in (13, 7, 4):
        assert model[f"sb_pair_adjacent KL={kl} swz=1"] == 1
