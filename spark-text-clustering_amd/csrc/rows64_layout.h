// rows64_layout.h — the LDS layouts of the fp64 rows E-step's two exchanges (lda_rows64.hip) and a bank model
// of them.  Plain constexpr C++17, no HIP: the kernel takes its addresses from these functions, the model below
// evaluates the same functions at compile time, and the static_asserts at the end make the library build the
// proof that the shipped layouts are conflict-free (tests/test_rows64_lds_layout.py compiles the header alone
// and prints the numbers).
//
//   sb  s partials, [topic][wave], kSbPitch = 4 doubles per topic.  Written before block barrier 1 by every
//       lane (tl, rl) of the four waves (topics KL·tl + 2·rl and + 1, 8-byte stores), read after it by the ψ /
//       mirror lanes (lane tt: its topic's 32-byte record as two 16-byte reads).
//   pa  φ partials of one wave, [wave row][topic lane].  Written by every lane (one 8-byte store per row set),
//       read by worker lane q < 8·R (its row's eight doubles as four 16-byte reads).
//
// Bank rules (MI355X_MICROARCH.md §LDS): a wave64 access is served in fixed lane groups, one LDS cycle per
// group when conflict-free; every further distinct address on a busy bank inside a group costs one more cycle.
//   ds_write_b64   4 groups of 16 contiguous lanes, bank = (byte address / 4) mod 32
//   ds_read_b128   4 groups of 16 lanes {0–3,12–15,20–27} {4–11,16–19,28–31} {32–35,44–47,52–59}
//                  {36–43,48–51,60–63}, bank = (byte address / 4) mod 64
// Both accesses are naturally aligned here, so 16 units of the access size span the banks in either case.
#pragma once

namespace stc {
namespace lda {
namespace r64 {

constexpr int kSbPitch = 4;   // s-partial row pitch (doubles): one sum per wave (rs_rows8), 16-B reads
constexpr int kPaPitch = 10;  // φ-partial pitch (doubles) per wave row: 8 used; a row set is 8·kPaPitch doubles

// ---- sb -------------------------------------------------------------------------------------------------------
// The wave slot of topic t = KL·tl + p is w ^ sb_swz: inside a 16-lane store group only t mod 4 varies the
// bank of 4·t + w (4-way), the XOR spreads the group over the record's four slots.  KL = 13 / 7: bit 2 of tl
// and bit 0 of rl (p >> 1 = rl) are exactly what t mod 4 does not see.  KL = 4: t mod 4 = p takes two values
// per store, so eight distinct slots at most are reachable at this pitch: tl's low bits, 2-way.
// The reader adds a record's four slots as (x0 + x1) + (x2 + x3): an XOR on the slot index permutes inside the
// pairs and swaps the pairs, and fp addition commutes, so the sum is bitwise the unswizzled one.
constexpr int sb_swz(int KL, int tl, int p, bool swz) {
  if (!swz) return 0;
  return KL == 4 ? (tl & 3) : (((tl >> 2) & 1) | (((p >> 1) & 1) << 1));
}
// double index of (topic KL·tl + p, wave w) in sb
constexpr int sb_slot(int KL, int tl, int p, int w, bool swz) {
  return (KL * tl + p) * kSbPitch + (w ^ sb_swz(KL, tl, p, swz));
}
// a lane's two topics 2·rl and 2·rl + 1 lie kSbPitch apart in every wave: the kernel stores both off one address
constexpr bool sb_pair_adjacent(int KL, bool swz) {
  for (int tl = 0; tl < 8; ++tl)
    for (int p = 0; p + 1 < KL; p += 2)
      for (int w = 0; w < 4; ++w)
        if (sb_slot(KL, tl, p + 1, w, swz) != sb_slot(KL, tl, p, w, swz) + kSbPitch) return false;
  return true;
}
// which 16-byte half of its record reader lane tt reads first (the other second): 2·tt + half is then a
// bijection of tt mod 16 onto the 16 chunk banks, and a read group's lanes are distinct mod 16
constexpr int sb_read_first(int tt, bool swz) { return swz ? (tt >> 3) & 1 : 0; }

// ---- pa -------------------------------------------------------------------------------------------------------
// double index of wave row q = 8·set + rl, column 0.  Layout 0: pitch 10 (worker reads conflict-free, rows rl
// and rl + 1 of a store group share two slots mod 16: 2-way).  Layout 1: inside a set's 80 doubles row rl
// starts at 18·(rl >> 1) + 8·(rl & 1): the two rows of a store group are 8 doubles apart (16 distinct slots),
// the start chunks mod 16 of rows 0–3 and 4–7 are {0,4,9,13} and {2,6,11,15}, and a set adds 40 chunks ≡ 8, so
// each read group (rows of four sets, alternating halves) covers the 16 chunk banks once.  Same footprint.
constexpr int pa_row(int q, int layout) {
  const int set = q >> 3, rl = q & 7;
  return 8 * kPaPitch * set + (layout ? 18 * (rl >> 1) + 8 * (rl & 1) : kPaPitch * rl);
}

// ---- the bank model ----------------------------------------------------------------------------------------------
struct WaveAccess {
  int addr[64];  // byte address per lane
  bool on[64];   // EXEC
};

enum Inst { kDsWriteB64, kDsReadB128 };

constexpr int kReadB128Group[4][16] = {
    {0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
    {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
    {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
    {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};

// LDS cycles of one wave-instruction beyond the conflict-free count (SQ_LDS_BANK_CONFLICT's unit)
constexpr int extra_cycles(const WaveAccess& a, Inst inst) {
  const int bytes = inst == kDsWriteB64 ? 8 : 16;
  const int banks = (inst == kDsWriteB64 ? 32 : 64) * 4 / bytes;  // in units of the access size
  int extra = 0;
  for (int g = 0; g < 4; ++g) {
    int unit[16] = {}, n = 0;  // the addresses of the group's active lanes, in units of the access size
    for (int i = 0; i < 16; ++i) {
      const int l = inst == kDsWriteB64 ? 16 * g + i : kReadB128Group[g][i];
      if (a.on[l]) unit[n++] = a.addr[l] / bytes;
    }
    int worst = 0;
    for (int b = 0; b < banks; ++b) {
      int distinct = 0;  // identical addresses broadcast: counted once
      for (int i = 0; i < n; ++i) {
        if (unit[i] % banks != b) continue;
        bool seen = false;
        for (int j = 0; j < i; ++j) seen = seen || unit[j] == unit[i];
        if (!seen) ++distinct;
      }
      if (distinct > worst) worst = distinct;
    }
    if (worst > 1) extra += worst - 1;
  }
  return extra;
}

// the sb stores of one document-iteration: four waves, two stores each (topics 2·rl and 2·rl + 1 of the lane)
constexpr int sb_store_extra(int KL, bool swz) {
  int extra = 0;
  for (int w = 0; w < 4; ++w) {
    for (int i = 0; i < 2; ++i) {
      WaveAccess a{};
      for (int lane = 0; lane < 64; ++lane) {
        const int tl = lane & 7, rl = lane >> 3, p = 2 * rl + i;
        a.on[lane] = p < KL;
        a.addr[lane] = 8 * sb_slot(KL, tl, p < KL ? p : 0, w, swz);
      }
      extra += extra_cycles(a, kDsWriteB64);
    }
  }
  return extra;
}

// the sb reads of one document-iteration at k topics (kp = k rounded up to even): two ψ waves of (kp + 1) / 2
// lanes and their two mirror waves (npsi = 2), or one ψ wave of kp lanes; lanes past k are off
constexpr int sb_read_extra(int k, int npsi, bool swz) {
  const int kp = (k + 1) / 2 * 2, half = npsi == 2 ? (kp + 1) / 2 : kp;
  int extra = 0;
  for (int w = 0; w < (npsi == 2 ? 4 : 1); ++w) {
    const int pw = npsi == 2 ? (w & 1) : 0;
    for (int c = 0; c < 2; ++c) {
      WaveAccess a{};
      for (int lane = 0; lane < 64; ++lane) {
        const int tt = pw * half + lane;
        a.on[lane] = lane < half && tt < k;
        a.addr[lane] = 8 * (tt * kSbPitch + 2 * (sb_read_first(tt, swz) ^ c));
      }
      extra += extra_cycles(a, kDsReadB128);
    }
  }
  return extra;
}
// the worst of a range of k (the kernel's (KL, ψ waves) classes: 65–104, 57–64, 33–56, 1–32)
constexpr int sb_read_extra_max(int k0, int k1, int npsi, bool swz) {
  int worst = 0;
  for (int k = k0; k <= k1; ++k) {
    const int e = sb_read_extra(k, npsi, swz);
    if (e > worst) worst = e;
  }
  return worst;
}

// the pa stores (R per wave) and worker reads (four per wave, lanes < 8·R) of one document-iteration
constexpr int pa_store_extra(int R, int layout) {
  int extra = 0;
  for (int j = 0; j < R; ++j) {
    WaveAccess a{};
    for (int lane = 0; lane < 64; ++lane) {
      a.on[lane] = true;
      a.addr[lane] = 8 * (pa_row(8 * j + (lane >> 3), layout) + (lane & 7));
    }
    extra += extra_cycles(a, kDsWriteB64);
  }
  return 4 * extra;  // a wave's rows are its own: the four waves' accesses are the same up to the base
}
constexpr int pa_read_extra(int R, int layout) {
  int extra = 0;
  for (int c = 0; c < 4; ++c) {
    WaveAccess a{};
    for (int lane = 0; lane < 64; ++lane) {
      a.on[lane] = lane < 8 * R;
      a.addr[lane] = 8 * (pa_row(lane, layout) + 2 * c);
    }
    extra += extra_cycles(a, kDsReadB128);
  }
  return 4 * extra;
}
// layout 1 fits the rows layout 0 reserves, and no two rows overlap
constexpr bool pa_rows_fit(int layout, int rows) {
  for (int q = 0; q < rows; ++q) {
    if (pa_row(q, layout) < 0 || pa_row(q, layout) + 8 > kPaPitch * rows || pa_row(q, layout) % 2 != 0) return false;
    for (int r = 0; r < q; ++r) {
      const int d = pa_row(q, layout) - pa_row(r, layout);
      if (d > -8 && d < 8) return false;
    }
  }
  return true;
}

// ---- what the build proves --------------------------------------------------------------------------------------
// the layouts before the swizzle, as measured in DESIGN.md §3 "r08"
static_assert(sb_store_extra(13, false) == 76 && sb_store_extra(7, false) == 40 && sb_store_extra(4, false) == 56, "sb");
static_assert(sb_read_extra(100, 2, false) == 24 && pa_store_extra(6, 0) == 96 && pa_read_extra(6, 0) == 0, "sb / pa");
// the swizzled sb: conflict-free for (KL, ψ waves) = (13, 2), (13, 1), (7, 1); KL = 4 stores stay 2-way
static_assert(sb_store_extra(13, true) == 0 && sb_store_extra(7, true) == 0, "sb stores: KL = 13, 7");
static_assert(sb_store_extra(4, true) == 8, "sb stores: KL = 4");
static_assert(sb_pair_adjacent(13, true) && sb_pair_adjacent(7, true) && sb_pair_adjacent(4, true) &&
                  sb_pair_adjacent(13, false), "sb stores: one address per lane");
static_assert(sb_read_extra(100, 2, true) == 0 && sb_read_extra(104, 2, true) == 0 && sb_read_extra(65, 2, true) == 0,
              "sb reads: KL = 13, two ψ waves");
static_assert(sb_read_extra(64, 1, true) == 0 && sb_read_extra(57, 1, true) == 0, "sb reads: KL = 13, one ψ wave");
static_assert(sb_read_extra(56, 1, true) == 0 && sb_read_extra(40, 1, true) == 0 && sb_read_extra(33, 1, true) == 0,
              "sb reads: KL = 7");
static_assert(sb_read_extra(32, 1, true) == 0 && sb_read_extra(7, 1, true) == 0, "sb reads: KL = 4");
// pa layout 1: no conflict in a store or a worker read at any row-set count, inside layout 0's rows
static_assert(pa_rows_fit(0, 64) && pa_rows_fit(1, 64) && pa_rows_fit(1, 48), "pa rows");
static_assert(pa_store_extra(1, 1) == 0 && pa_store_extra(6, 1) == 0 && pa_store_extra(8, 1) == 0, "pa stores");
static_assert(pa_read_extra(1, 1) == 0 && pa_read_extra(2, 1) == 0 && pa_read_extra(3, 1) == 0 && pa_read_extra(4, 1) == 0 &&
                  pa_read_extra(5, 1) == 0 && pa_read_extra(6, 1) == 0 && pa_read_extra(7, 1) == 0 && pa_read_extra(8, 1) == 0,
              "pa reads");

}  // namespace r64
}  // namespace lda
}  // namespace stc
