// java_lower.h — Java 8 String.toLowerCase (root locale) on the device, one code point at a time: the helpers
// tokenizer.hip (K0) and token_stages.hip (StopWordsRemover) share.  The rules are stated at the top of
// tokenizer.hip; the tables are case_table.h's, which have internal linkage — every translation unit that
// includes this header carries its own copy of them (about 18 KiB of device constants).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "case_table.h"

namespace stc {
namespace tokenizer {

// UTF-8 length from the lead byte (0: a continuation byte)
__device__ __forceinline__ int utf8_len(uint32_t b) { return b < 0x80u ? 1 : b < 0xC0u ? 0 : b < 0xE0u ? 2 : b < 0xF0u ? 3 : 4; }

// Java 8 lower case of a BMP code point (0: rejected — see case_table.h)
__device__ __forceinline__ uint32_t lower_bmp(uint32_t cp) {
  const uint32_t pg = kCasePage[cp >> 8];
  return pg ? kCasePages[pg - 1][cp & 0xFFu] : cp;
}
// ... of any code point: the BMP table, Deseret U+10400–U+10427 → +0x28, the rest unchanged
__device__ __forceinline__ uint32_t lower_cp(uint32_t cp) {
  if (cp < 0x10000u) return lower_bmp(cp);
  return (cp >= 0x10400u && cp <= 0x10427u) ? cp + 0x28u : cp;
}
// the code point of the n-byte UTF-8 sequence at text[j] (j + n <= e), or ~0 when malformed
__device__ __forceinline__ uint32_t decode_at(const uint8_t* __restrict__ text, int64_t j, int n) {
  uint32_t cp = text[j] & (0xFFu >> (n + 1));
  for (int q = 1; q < n; ++q) {
    const uint32_t c = text[j + q];
    if ((c & 0xC0u) != 0x80u) return ~0u;
    cp = (cp << 6) | (c & 0x3Fu);
  }
  return cp;
}
// byte `pos` (0 = lead) of code point cp's n-byte UTF-8 form
__device__ __forceinline__ uint32_t utf8_byte(uint32_t cp, int n, int pos) {
  if (pos == 0) return n == 2 ? (0xC0u | (cp >> 6)) : n == 3 ? (0xE0u | (cp >> 12)) : (0xF0u | (cp >> 18));
  return 0x80u | ((cp >> (6 * (n - 1 - pos))) & 0x3Fu);
}

// the Final_Sigma class of cp: 0 other, 1 case-ignorable, 2 cased (case_table.h kSig*)
__device__ __forceinline__ int sigma_class(uint32_t cp) {
  const uint32_t pg = cp < 0x110000u ? kSigPage[cp >> 8] : 0u;
  return pg ? (kSigPages[pg - 1][(cp & 0xFFu) >> 2] >> (2 * (cp & 3u))) & 3 : 0;
}
// the code point of the character at text[j] (its length in *n), or ~0 when malformed / truncated at e
__device__ __forceinline__ uint32_t cp_at(const uint8_t* __restrict__ text, int64_t j, int64_t e, int* n) {
  const uint32_t b = text[j];
  *n = utf8_len(b);
  if (*n == 1) return b;
  if (*n == 0 || j + *n > e) {
    *n = 1;
    return ~0u;
  }
  return decode_at(text, j, *n);
}
// Final_Sigma for the Σ at text[i] (2 bytes) of the document [s, e): preceded by a cased letter with only
// case-ignorables between, and not followed by case-ignorables then a cased letter (the Unicode rule, as the
// oracle's str.lower() applies it).  A malformed byte ends a scan as a non-cased character.
// KNOWN DIVERGENCE from Spark's JVM (parity unpinned: no artefact or test of the reference holds it): Java
// 8's ConditionalSpecialCasing.isFinalCased scans the whole BreakIterator word instead, where letters AND
// digits belong to one word, so a digit between Σ and a cased letter changes the answer — "Α1Σ" gives Java
// ς but this rule σ, "ΑΣ1Β" Java σ but this rule ς.  Letters, marks, spaces and punctuation around Σ agree.
__device__ inline bool final_sigma(const uint8_t* __restrict__ text, int64_t s, int64_t e, int64_t i) {
  bool pre = false;
  for (int64_t j = i; j > s;) {  // backwards, one character at a time
    int64_t p = j - 1;
    while (p > s && j - p < 4 && (text[p] & 0xC0u) == 0x80u) --p;
    int n = 0;
    const uint32_t cp = cp_at(text, p, j, &n);
    if (cp == ~0u || p + n != j) break;
    const int c = sigma_class(cp);
    if (c == 1) {
      j = p;
      continue;
    }
    pre = c == 2;
    break;
  }
  if (!pre) return false;
  for (int64_t j = i + 2; j < e;) {
    int n = 0;
    const uint32_t cp = cp_at(text, j, e, &n);
    if (cp == ~0u) return true;
    const int c = sigma_class(cp);
    if (c != 1) return c != 2;
    j += n;
  }
  return true;
}
__device__ __forceinline__ int utf8_size(uint32_t cp) { return cp < 0x80u ? 1 : cp < 0x800u ? 2 : 3; }
// the lower case of a character the table leaves to rule (kCasePages entry 0): its UTF-8 bytes packed
// little-endian into *out, their count returned
__device__ inline int special_lower(const uint8_t* __restrict__ text, int64_t s, int64_t e, int64_t i, uint32_t cp,
                                    uint32_t* out) {
  if (cp == 0x130u) {  // İ → i + U+0307 COMBINING DOT ABOVE
    *out = 0x69u | (0xCCu << 8) | (0x87u << 16);
    return 3;
  }
  uint32_t lc = cp;
  if (cp == 0x3A3u) {
    lc = final_sigma(text, s, e, i) ? 0x3C2u : 0x3C3u;
  } else {
    for (int q = 0; q < kSpecialN; ++q)
      if (kSpecialFrom[q] == cp) lc = kSpecialTo[q];
  }
  const int n = utf8_size(lc);
  uint32_t w = 0;
  for (int q = 0; q < n; ++q) w |= (n == 1 ? lc : utf8_byte(lc, n, q)) << (8 * q);
  *out = w;
  return n;
}
// the lead byte at text[i] (i < e) starts a character the table leaves to rule: its code point, else 0
__device__ __forceinline__ uint32_t special_at(const uint8_t* __restrict__ text, int64_t i, int64_t e) {
  const int n = utf8_len(text[i]);
  if (n < 2 || n > 3 || i + n > e) return 0u;
  const uint32_t cp = decode_at(text, i, n);
  return (cp != ~0u && lower_bmp(cp) == 0u) ? cp : 0u;
}
// its UTF-8 length change (Σ keeps its length; İ and U+023A / U+023E grow by one; the rest shrink)
__device__ __forceinline__ int special_delta(uint32_t cp, int n_in) {
  if (cp == 0x130u) return 1;
  if (cp == 0x3A3u) return 0;
  for (int q = 0; q < kSpecialN; ++q)
    if (kSpecialFrom[q] == cp) return utf8_size(kSpecialTo[q]) - n_in;
  return 0;
}

}  // namespace tokenizer
}  // namespace stc
