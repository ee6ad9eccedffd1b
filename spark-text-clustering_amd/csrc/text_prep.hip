// text_prep.hip — the reference's text preprocessing between its lemmatiser and its vocabulary, on gfx950:
//
//   filterSpecialCharacters → OpenNLP SimpleTokenizer → drop stop words → OpenNLP PorterStemmer
//
// (LDAClustering.scala:121-139 for training, :221-238 for scoring; the semantics are stated in include/stc.h,
// "Text preprocessing", and restated in plain Python by tests/prep_oracle.py).  Everything runs on the device;
// the host reads back sizes only (the first malformed byte, the token and byte counts, the longest document).
//
//   k_mark_docs   a byte per text byte: does a (non-empty) document start here
//   k_classify    one lane per byte: strict UTF-8 decode at each lead byte, the character's class from the
//                 preprocessor's table (the strip set already folded in as WHITESPACE), a token-start flag from
//                 the previous character and a token-last flag from the next one (look-back / look-ahead of one
//                 character, never across a document start: no serial state), the start flags counted per
//                 workgroup chunk
//   (scan)        the chunks' counts → every chunk's first token id
//   k_tokens      the same chunks again: token id of every flagged byte from ballots → each raw token's
//                 [start, end) in the text
//   k_doc_first   every document's first raw token id (one wave per document boundary)
//   k_stem        one lane per raw token: the stop-word table (open addressing, FNV-1a), then the Porter stemmer
//                 in place on the device copy of the text → kept flag and output length
//   (scans)       kept lengths → output byte offsets, kept flags → output token ids
//   k_emit        the compact blob and tok_off; k_doc_off: doc_off and the longest document
//
// The stemmer works on UTF-8 bytes yet decides as the Java code does on chars: every suffix it tests or writes
// is ASCII, every non-ASCII byte is a consonant, and a run of consonant bytes changes neither the measure nor
// "y after a consonant", so only the three places that count or compare chars — the ≤ 2 chars gate, doublec
// and cvc — step over whole characters.  Integer arithmetic only; no atomics but the first-bad-byte minimum
// and the longest-document maximum (both order-independent), so results are bitwise reproducible.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "class_table.h"
#include "stc_handles.h"
#include "token_compact.h"  // UTF-8 decoding, the stop-word table, k_emit / k_doc_off (shared with token_stages.hip)

struct stc_prep {
  stc::Ctx* ctx = nullptr;  // the context that made it; only it may use it
  int device = -1;          // for stc_prep_free, which may run after that context is gone
  int stem = 1;
  int64_t n_stop = 0;
  int64_t max_stop_len = 0;  // longer tokens skip the table
  uint64_t table_mask = 0;   // slots − 1 (a power of two ≥ 2 · n_stop)
  stc::DevBuf cls;           // uint8[16384]: 2 bits per BMP code point, the strip set stored as WHITESPACE
  stc::DevBuf stop_blob;     // uint8[the words' bytes]
  stc::DevBuf stop_tab;      // StopSlot[table_mask + 1]
};

namespace stc {
namespace prep {

constexpr int kIter = 8;
constexpr int64_t kChunk = int64_t(kBlock) * kIter;  // text bytes per workgroup
constexpr uint32_t kOther = 0, kSpace = 1;           // (2 ALPHABETIC, 3 NUMERIC: class_table.h)

__host__ __device__ inline uint32_t cls_of(const uint8_t* __restrict__ tab, uint32_t cp) {
  return cp < 0x10000u ? (tab[cp >> 2] >> (2 * (cp & 3u))) & 3u : kOther;  // ≥ U+10000: always OTHER
}
// do two neighbouring non-WHITESPACE characters belong to different tokens (symmetric in its two characters)
__host__ __device__ inline bool differs(uint32_t c, uint32_t cp, uint32_t c2, uint32_t cp2) {
  return c2 != c || (c == kOther && (cp2 != cp || cp >= 0x10000u));
}
__device__ __forceinline__ int lanes_below(uint64_t m, int lane) {
  return __popcll(m & (lane ? (~0ull >> (64 - lane)) : 0ull));
}

__global__ __launch_bounds__(kBlock) void k_mark_docs(const int64_t* __restrict__ text_off, int64_t n_docs,
                                                      uint8_t* __restrict__ ds) {
  const int64_t d = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (d < n_docs && text_off[d + 1] > text_off[d]) ds[text_off[d]] = 1;  // (then text_off[d] < n_bytes)
}

// the flags of byte i: bit 0 a token starts here, bit 1 the character here is its token's last; −1: byte i is not
// part of well-formed UTF-8 inside its document
__host__ __device__ inline int classify_byte(const uint8_t* __restrict__ text, int64_t n, const uint8_t* __restrict__ ds,
                                             const uint8_t* __restrict__ tab, int64_t i) {
  const uint32_t b = text[i];
  if ((b & 0xC0u) == 0x80u) {  // a continuation byte: a lead ≤ 3 bytes back, in this document, must cover it
    if (ds[i]) return -1;
    for (int q = 1; q <= 3 && i - q >= 0; ++q) {
      const uint32_t c = text[i - q];
      if ((c & 0xC0u) != 0x80u) return lead_len(c) > q ? 0 : -1;
      if (ds[i - q]) return -1;
    }
    return -1;
  }
  const int len = lead_len(b);
  if (len == 0 || i + len > n) return -1;
  const uint32_t cp = decode_strict(text + i, len);
  if (cp == kBadCp) return -1;
  for (int q = 1; q < len; ++q)
    if (ds[i + q]) return -1;  // the document ends inside the sequence
  const uint32_t c = cls_of(tab, cp);
  if (c == kSpace) return 0;
  bool start = true, last = true;
  if (i > 0 && !ds[i]) {  // the previous character of this document
    int64_t j = i - 1;
    while (j > 0 && i - j < 4 && (text[j] & 0xC0u) == 0x80u && !ds[j]) --j;
    const int pl = lead_len(text[j]);
    if (pl > 0 && j + pl == i) {
      const uint32_t pcp = decode_strict(text + j, pl);
      if (pcp != kBadCp) start = differs(c, cp, cls_of(tab, pcp), pcp);
    }
  }
  const int64_t e = i + len;
  if (e < n && !ds[e]) {  // the next one
    const int nl = lead_len(text[e]);
    if (nl > 0 && e + nl <= n) {
      const uint32_t ncp = decode_strict(text + e, nl);
      if (ncp != kBadCp) last = differs(c, cp, cls_of(tab, ncp), ncp);
    }
  }
  return (start ? 1 : 0) | (last ? 2 : 0);
}

__global__ __launch_bounds__(kBlock) void k_classify(const uint8_t* __restrict__ text, int64_t n,
                                                     const uint8_t* __restrict__ ds, const uint8_t* __restrict__ tab,
                                                     uint8_t* __restrict__ code, int64_t* __restrict__ blk_cnt,
                                                     unsigned long long* __restrict__ bad) {
  __shared__ int wsum[kBlock / 64];
  int starts = 0;  // wave-uniform
  for (int it = 0; it < kIter; ++it) {
    const int64_t i = (int64_t)blockIdx.x * kChunk + it * kBlock + threadIdx.x;
    int flag = 0;
    if (i < n) {
      flag = classify_byte(text, n, ds, tab, i);
      if (flag < 0) {
        atomicMin(bad, (unsigned long long)i);
        flag = 0;
      }
      code[i] = (uint8_t)flag;
    }
    starts += __popcll(__ballot(flag & 1));
  }
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = starts;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t t = 0;
    for (int w = 0; w < kBlock / 64; ++w) t += wsum[w];
    blk_cnt[blockIdx.x] = t;
  }
}

// raw token r = the r-th start flag: [tok_start[r], tok_end[r]) in the text
__global__ __launch_bounds__(kBlock) void k_tokens(const uint8_t* __restrict__ text, int64_t n,
                                                   const uint8_t* __restrict__ code,
                                                   const int64_t* __restrict__ blk_base, int64_t n_raw,
                                                   int64_t* __restrict__ tok_start, int64_t* __restrict__ tok_end) {
  __shared__ int wsum[2][kBlock / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int64_t run = blk_base[blockIdx.x];  // start flags before this iteration's bytes
  for (int it = 0; it < kIter; ++it) {
    const int64_t i = (int64_t)blockIdx.x * kChunk + it * kBlock + threadIdx.x;
    const uint32_t f = i < n ? code[i] : 0u;
    const uint64_t m = __ballot(f & 1u);
    if (lane == 0) wsum[it & 1][w] = __popcll(m);
    __syncthreads();  // (two buffers: the next iteration's writes cannot pass this iteration's reads)
    int before = 0, total = 0;
    for (int q = 0; q < kBlock / 64; ++q) {
      const int s = wsum[it & 1][q];
      before += q < w ? s : 0;
      total += s;
    }
    const int64_t incl = run + before + lanes_below(m, lane) + (f & 1u);  // start flags at or before byte i
    if (incl >= 1 && incl <= n_raw) {
      if (f & 1u) tok_start[incl - 1] = i;
      if (f & 2u) tok_end[incl - 1] = i + lead_len(text[i]);
    }
    run += total;
  }
}

// raw_doc[d] = start flags before byte text_off[d], d = 0 … n_docs: one wave each
__global__ __launch_bounds__(kBlock) void k_doc_first(const int64_t* __restrict__ text_off, int64_t n_docs,
                                                      const uint8_t* __restrict__ code,
                                                      const int64_t* __restrict__ blk_base,
                                                      int64_t* __restrict__ raw_doc) {
  const int lane = threadIdx.x & 63;
  const int64_t d = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (d > n_docs) return;
  const int64_t p = text_off[d], blk = p / kChunk;
  int cnt = 0;
  for (int64_t q = blk * kChunk + lane; q < p; q += 64) cnt += code[q] & 1;
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (lane == 0) raw_doc[d] = blk_base[blk] + cnt;
}

// ---- Porter stemmer (opennlp.tools.stemmer.PorterStemmer 1.6.0, Lucene's) on the UTF-8 bytes b[0 .. k] -------
struct Porter {
  uint8_t* b;
  int64_t k, j;

  __host__ __device__ static bool vowel5(uint32_t c) { return c == 'a' || c == 'e' || c == 'i' || c == 'o' || c == 'u'; }
  // cons(i): 'y' is a consonant at the front and after a vowel; a run of y's alternates from its first
  __host__ __device__ bool cons(int64_t i) const {
    const uint32_t c = b[i];
    if (vowel5(c)) return false;
    if (c != 'y') return true;
    int64_t p = i;
    while (p > 0 && b[p - 1] == 'y') --p;
    const bool first = p == 0 ? true : vowel5(b[p - 1]);
    return first != (((i - p) & 1) != 0);
  }
  // m(): the measure of b[0 .. j] = the vowel → consonant steps in it
  __host__ __device__ int64_t m() const {
    int64_t n = 0;
    bool pc = true;
    for (int64_t i = 0; i <= j; ++i) {
      const uint32_t c = b[i];
      const bool cs = vowel5(c) ? false : (c == 'y' ? (i == 0 ? true : !pc) : true);
      n += (cs && !pc) ? 1 : 0;
      pc = cs;
    }
    return n;
  }
  __host__ __device__ bool vowelinstem() const {
    bool pc = true;
    for (int64_t i = 0; i <= j; ++i) {
      const uint32_t c = b[i];
      const bool cs = vowel5(c) ? false : (c == 'y' ? (i == 0 ? true : !pc) : true);
      if (!cs) return true;
      pc = cs;
    }
    return false;
  }
  // first byte of the character whose last byte is b[i]
  __host__ __device__ int64_t char_start(int64_t i) const {
    while (i > 0 && (b[i] & 0xC0u) == 0x80u) --i;
    return i;
  }
  // doublec on chars: the last two chars are equal and a consonant; *n = the last char's bytes.  A code point
  // ≥ U+10000 is two different Java chars (a surrogate pair), so it never doubles
  __host__ __device__ bool doublec(int64_t i, int* n) const {
    *n = 1;
    if (b[i] < 0x80u) return i >= 1 && b[i - 1] == b[i] && cons(i);
    const int64_t s = char_start(i);
    const int len = (int)(i - s) + 1;
    *n = len;
    if (len >= 4 || s - len < 0) return false;
    for (int q = 0; q < len; ++q)
      if (b[s - len + q] != b[s + q]) return false;
    return true;  // (equal lead bytes: the bytes before are one whole character; non-ASCII: a consonant)
  }
  // cvc on chars, i = the last byte of the char it ends at: consonant – vowel – consonant (not w x y)
  __host__ __device__ bool cvc(int64_t i) const {
    if (i < 0) return false;
    const int64_t s = char_start(i);
    if (s == i) {
      const uint32_t c = b[i];
      if (!cons(i) || c == 'w' || c == 'x' || c == 'y') return false;
    } else if (i - s == 3) {
      return false;  // ≥ U+10000: two Java chars, both consonants — no vowel before the last
    }
    const int64_t p = s - 1;  // the vowel: one ASCII byte
    if (p < 1 || cons(p)) return false;
    return cons(p - 1);
  }
  template <int L>
  __host__ __device__ bool ends(const char (&s)[L]) {
    constexpr int l = L - 1;
    const int64_t o = k - l + 1;
    if (o < 0) return false;
    for (int q = 0; q < l; ++q)
      if (b[o + q] != (uint8_t)s[q]) return false;
    j = k - l;
    return true;
  }
  template <int L>
  __host__ __device__ void setto(const char (&s)[L]) {
    constexpr int l = L - 1;
    for (int q = 0; q < l; ++q) b[j + 1 + q] = (uint8_t)s[q];
    k = j + l;
  }
  template <int L>
  __host__ __device__ void r(const char (&s)[L]) {
    if (m() > 0) setto(s);
  }

  __host__ __device__ void step1() {
    if (b[k] == 's') {
      if (ends("sses")) k -= 2;
      else if (ends("ies")) setto("i");
      else if (b[k - 1] != 's') k--;
    }
    if (ends("eed")) {
      if (m() > 0) k--;
    } else if ((ends("ed") || ends("ing")) && vowelinstem()) {
      k = j;
      int n = 1;
      if (ends("at")) setto("ate");
      else if (ends("bl")) setto("ble");
      else if (ends("iz")) setto("ize");
      else if (doublec(k, &n)) {
        const uint32_t ch = b[k];
        if (!(ch == 'l' || ch == 's' || ch == 'z')) k -= n;
      } else if (m() == 1 && cvc(k)) setto("e");
    }
  }
  __host__ __device__ void step2() {
    if (ends("y") && vowelinstem()) b[k] = 'i';
  }
  // every case of the switches of steps 3-5 stops at its first matching suffix, replaced or not
  __host__ __device__ void step3() {
    if (char_start(k) == 0) return;
    switch (b[k - 1]) {
      case 'a':
        if (ends("ational")) { r("ate"); break; }
        if (ends("tional")) { r("tion"); break; }
        break;
      case 'c':
        if (ends("enci")) { r("ence"); break; }
        if (ends("anci")) { r("ance"); break; }
        break;
      case 'e':
        if (ends("izer")) { r("ize"); break; }
        break;
      case 'l':
        if (ends("bli")) { r("ble"); break; }
        if (ends("alli")) { r("al"); break; }
        if (ends("entli")) { r("ent"); break; }
        if (ends("eli")) { r("e"); break; }
        if (ends("ousli")) { r("ous"); break; }
        break;
      case 'o':
        if (ends("ization")) { r("ize"); break; }
        if (ends("ation")) { r("ate"); break; }
        if (ends("ator")) { r("ate"); break; }
        break;
      case 's':
        if (ends("alism")) { r("al"); break; }
        if (ends("iveness")) { r("ive"); break; }
        if (ends("fulness")) { r("ful"); break; }
        if (ends("ousness")) { r("ous"); break; }
        break;
      case 't':
        if (ends("aliti")) { r("al"); break; }
        if (ends("iviti")) { r("ive"); break; }
        if (ends("biliti")) { r("ble"); break; }
        break;
      case 'g':
        if (ends("logi")) { r("log"); break; }
        break;
      default:
        break;
    }
  }
  __host__ __device__ void step4() {
    switch (b[k]) {
      case 'e':
        if (ends("icate")) { r("ic"); break; }
        if (ends("ative")) { r(""); break; }
        if (ends("alize")) { r("al"); break; }
        break;
      case 'i':
        if (ends("iciti")) { r("ic"); break; }
        break;
      case 'l':
        if (ends("ical")) { r("ic"); break; }
        if (ends("ful")) { r(""); break; }
        break;
      case 's':
        if (ends("ness")) { r(""); break; }
        break;
      default:
        break;
    }
  }
  __host__ __device__ void step5() {
    if (char_start(k) == 0) return;
    bool hit = false;
    switch (b[k - 1]) {
      case 'a': hit = ends("al"); break;
      case 'c': hit = ends("ance") || ends("ence"); break;
      case 'e': hit = ends("er"); break;
      case 'i': hit = ends("ic"); break;
      case 'l': hit = ends("able") || ends("ible"); break;
      case 'n': hit = ends("ant") || ends("ement") || ends("ment") || ends("ent"); break;
      case 'o': hit = (ends("ion") && j >= 0 && (b[j] == 's' || b[j] == 't')) || ends("ou"); break;
      case 's': hit = ends("ism"); break;
      case 't': hit = ends("ate") || ends("iti"); break;
      case 'u': hit = ends("ous"); break;
      case 'v': hit = ends("ive"); break;
      case 'z': hit = ends("ize"); break;
      default: break;
    }
    if (hit && m() > 1) k = j;
  }
  __host__ __device__ void step6() {
    j = k;
    if (b[k] == 'e') {
      const int64_t a = m();
      if (a > 1 || (a == 1 && !cvc(k - 1))) k--;
    }
    int n = 1;
    if (b[k] == 'l' && doublec(k, &n) && m() > 1) k--;
  }
};

// the stem's length in bytes of the token b[0 .. len), stemmed in place (tokens of ≤ 2 Java chars unchanged)
__host__ __device__ int64_t porter_stem(uint8_t* b, int64_t len) {
  int chars = 0;  // UTF-16 code units, counted up to 3
  for (int64_t i = 0; i < len && chars < 3; ++i) {
    const uint32_t c = b[i];
    if ((c & 0xC0u) != 0x80u) chars += c >= 0xF0u ? 2 : 1;
  }
  if (chars < 3) return len;
  Porter p{b, len - 1, 0};
  p.step1();
  p.step2();
  p.step3();
  p.step4();
  p.step5();
  p.step6();
  return p.k + 1;
}

// raw token t = text[tok_start[t] .. tok_end[t]): kept unless it is a stop word; its stem written over it
__global__ __launch_bounds__(kBlock) void k_stem(uint8_t* __restrict__ text, const int64_t* __restrict__ tok_start,
                                                 const int64_t* __restrict__ tok_end, int64_t n_tok, int64_t n_bytes,
                                                 const StopSlot* __restrict__ stop_tab, uint64_t stop_mask,
                                                 const uint8_t* __restrict__ stop_blob, int64_t n_stop,
                                                 int64_t max_stop_len, int stem, int64_t* __restrict__ out_len,
                                                 int32_t* __restrict__ keep) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= n_tok) return;
  const int64_t s = tok_start[t], e = tok_end[t];
  int64_t len = (s >= 0 && e >= s && e <= n_bytes) ? e - s : 0;  // (always so; a guard for the stores below)
  bool kept = true;
  if (n_stop > 0 && len <= max_stop_len) kept = !is_stop(text + s, len, stop_tab, stop_mask, stop_blob);
  if (kept && stem && len > 0) len = porter_stem(text + s, len);
  out_len[t] = kept ? len : 0;
  if (keep) keep[t] = kept ? 1 : 0;
}

// each token alone must be well-formed UTF-8 (stc_stem_tokens)
__global__ __launch_bounds__(kBlock) void k_validate_tokens(const uint8_t* __restrict__ utf8,
                                                            const int64_t* __restrict__ tok_off, int64_t n_tok,
                                                            unsigned long long* __restrict__ bad) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= n_tok) return;
  const int64_t s = tok_off[t], r = first_bad_utf8(utf8 + s, tok_off[t + 1] - s);
  if (r >= 0) atomicMin(bad, (unsigned long long)(s + r));
}

// ---- host side ------------------------------------------------------------------------------------------------
static void single_device(Ctx& c) {
  if (c.coll()) throw Error(STC_ERR_STATE, "prep: the context is connected to other ranks (text preprocessing is single-device)");
}

static stc_prep* create(Ctx& c, const uint32_t* strip_cp, int64_t n_strip, const uint8_t* stop_utf8, int64_t n_bytes,
                        const int64_t* stop_off, int64_t n_stop, int stem) {
  single_device(c);
  STC_REQUIRE(stem == 0 || stem == 1, "stem must be 0 (none) or 1 (Porter)");
  STC_REQUIRE(n_strip >= -1 && (n_strip <= 0 || strip_cp), "strip_cp / n_strip (NULL, -1: the reference's set)");
  STC_REQUIRE(n_strip != -1 || !strip_cp, "n_strip = -1 goes with strip_cp = NULL");
  STC_REQUIRE(n_stop >= 0 && n_bytes >= 0, "sizes must be >= 0");
  STC_REQUIRE(n_stop == 0 || stop_off, "stop_off");
  // the reference's regex class (LDAClustering.scala:283-284) under java.util.regex
  static const uint32_t kDefault[] = {0x20, 0x21, 0x22, 0x23, 0x24, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x2B, 0x2C, 0x2D,
                                      '.', ':', ';', '?', '@', '^', '_', '`', 0xAB, 0xBB, 0x2019, 0x201D, 0x2212};
  if (n_strip < 0) {
    strip_cp = kDefault;
    n_strip = (int64_t)(sizeof(kDefault) / sizeof(kDefault[0]));
  }
  std::vector<uint8_t> cls(16384);
  for (uint32_t cp = 0; cp < 0x10000u; cp += 4) cls[cp >> 2] = kClassPages[kClassPage[cp >> 8]][(cp & 0xFFu) >> 2];
  for (int64_t q = 0; q < n_strip; ++q) {
    const uint32_t cp = strip_cp[q];
    if (cp >= 0x10000u || (cp >= 0xD800u && cp <= 0xDFFFu))
      throw Error(STC_ERR_INVALID_ARG, "strip code point " + std::to_string(q) + " (" + std::to_string(cp) +
                                           ") must be a BMP code point and no surrogate");
    uint8_t& w = cls[cp >> 2];
    w = (uint8_t)((w & ~(3u << (2 * (cp & 3u)))) | (kSpace << (2 * (cp & 3u))));
  }
  int64_t max_len = 0;
  uint64_t slots = 2;
  std::vector<StopSlot> tab;
  if (n_stop > 0) {
    check_offsets("stop_off", stop_off, n_stop, n_bytes, "n_bytes", true);
    STC_REQUIRE(n_bytes == 0 || stop_utf8, "stop_utf8");
    for (int64_t w = 0; w < n_stop; ++w) {
      const int64_t r = first_bad_utf8(stop_utf8 + stop_off[w], stop_off[w + 1] - stop_off[w]);
      if (r >= 0) throw_bad_utf8("the stop words", stop_off[w] + r);
    }
    while (slots < 2 * (uint64_t)n_stop) slots <<= 1;
  }
  tab.assign(slots, StopSlot{0, 0, -1});
  for (int64_t w = 0; w < n_stop; ++w) {
    const int64_t off = stop_off[w], len = stop_off[w + 1] - off;
    if (len == 0) continue;  // no token is empty
    const uint64_t h = fnv1a(stop_utf8 + off, len);
    uint64_t s = h & (slots - 1);
    bool dup = false;
    for (; tab[s].len >= 0; s = (s + 1) & (slots - 1))
      if (tab[s].hash == h && tab[s].len == len && !memcmp(stop_utf8 + tab[s].off, stop_utf8 + off, (size_t)len)) {
        dup = true;
        break;
      }
    if (!dup) tab[s] = StopSlot{h, off, len};
    max_len = std::max(max_len, len);
  }
  c.use();
  auto p = new_handle<stc_prep>(c);
  p->stem = stem;
  p->n_stop = n_stop;
  p->max_stop_len = max_len;
  p->table_mask = slots - 1;
  p->cls.reserve(cls.size());
  p->stop_blob.reserve((size_t)std::max<int64_t>(n_bytes, 1));
  p->stop_tab.reserve(sizeof(StopSlot) * slots);
  hipStream_t s = c.stream;
  HIP_CHECK(hipMemcpyAsync(p->cls.p, cls.data(), cls.size(), hipMemcpyHostToDevice, s));
  if (n_stop > 0 && n_bytes > 0) HIP_CHECK(hipMemcpyAsync(p->stop_blob.p, stop_utf8, n_bytes, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(p->stop_tab.p, tab.data(), sizeof(StopSlot) * slots, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipStreamSynchronize(s));  // the host tables die at scope exit
  return p.release();
}

static stc_dtok* tokens(Ctx& c, const stc_prep& p, const uint8_t* text, int64_t n, const int64_t* text_off,
                        int64_t n_docs) {
  single_device(c);
  STC_REQUIRE(n >= 0 && n_docs >= 0, "sizes must be >= 0");
  STC_REQUIRE(n_docs < (int64_t(1) << 31) - 1, "at most 2^31-2 documents per call");
  STC_REQUIRE(text_off && (n == 0 || text), "text/text_off");
  check_offsets("text_off", text_off, n_docs, n, "n_bytes", true);
  c.use();
  hipStream_t s = c.stream;
  auto t = new_handle<stc_dtok>(c);
  t->n_docs = n_docs;
  t->doc_off.reserve(8 * (n_docs + 1));
  int64_t n_raw = 0, n_keep = 0, n_out = 0;
  const int64_t n_blk = ceil_div(n, kChunk);
  DevBuf d_text, d_off, ds, code, blk_cnt, blk_base, small, tok_start, tok_end, raw_doc, out_len, out_off, keep, keep_pre;
  d_off.reserve(8 * (n_docs + 1));
  small.reserve(16);  // [0] the first malformed byte, [1] the longest document
  raw_doc.reserve(8 * (n_docs + 1));
  HIP_CHECK(hipMemcpyAsync(d_off.p, text_off, 8 * (n_docs + 1), hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemsetAsync(small.p, 0xFF, 8, s));
  HIP_CHECK(hipMemsetAsync(small.as<uint8_t>() + 8, 0, 8, s));
  blk_base.reserve(8 * (n_blk + 1));
  if (n > 0) {
    d_text.reserve(n);
    ds.reserve(n);
    code.reserve(n);
    blk_cnt.reserve(8 * n_blk);
    HIP_CHECK(hipMemcpyAsync(d_text.p, text, n, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemsetAsync(ds.p, 0, n, s));
    k_mark_docs<<<grid_for(n_docs), kBlock, 0, s>>>(d_off.as<int64_t>(), n_docs, ds.as<uint8_t>());
    KERNEL_CHECK();
    k_classify<<<(int)n_blk, kBlock, 0, s>>>(d_text.as<uint8_t>(), n, ds.as<uint8_t>(), p.cls.as<uint8_t>(),
                                             code.as<uint8_t>(), blk_cnt.as<int64_t>(),
                                             small.as<unsigned long long>());
    KERNEL_CHECK();
  }
  exclusive_sums(s, blk_cnt.as<int64_t>(), blk_base.as<int64_t>(), n_blk);
  {
    int64_t h[2];
    HIP_CHECK(hipMemcpyAsync(&h[0], small.p, 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&h[1], blk_base.as<int64_t>() + n_blk, 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (h[0] != -1) throw_bad_utf8("the text", h[0]);
    n_raw = h[1];
  }
  if (n_raw > (int64_t(1) << 31) - 1)
    throw Error(STC_ERR_INVALID_ARG, "the text holds " + std::to_string(n_raw) + " tokens, at most 2^31-1 per call");
  out_len.reserve(8 * std::max<int64_t>(n_raw, 1));
  out_off.reserve(8 * (n_raw + 1));
  keep.reserve(4 * std::max<int64_t>(n_raw, 1));
  keep_pre.reserve(4 * (n_raw + 1));
  if (n_raw > 0) {
    tok_start.reserve(8 * n_raw);
    tok_end.reserve(8 * n_raw);
    k_tokens<<<(int)n_blk, kBlock, 0, s>>>(d_text.as<uint8_t>(), n, code.as<uint8_t>(), blk_base.as<int64_t>(), n_raw,
                                           tok_start.as<int64_t>(), tok_end.as<int64_t>());
    KERNEL_CHECK();
  }
  if (n > 0) {
    k_doc_first<<<(int)ceil_div(n_docs + 1, kBlock / 64), kBlock, 0, s>>>(d_off.as<int64_t>(), n_docs, code.as<uint8_t>(),
                                                                         blk_base.as<int64_t>(), raw_doc.as<int64_t>());
    KERNEL_CHECK();
  } else {
    HIP_CHECK(hipMemsetAsync(raw_doc.p, 0, 8 * (n_docs + 1), s));
  }
  if (n_raw > 0) {
    k_stem<<<grid_for(n_raw), kBlock, 0, s>>>(d_text.as<uint8_t>(), tok_start.as<int64_t>(), tok_end.as<int64_t>(), n_raw, n,
                                              p.stop_tab.as<StopSlot>(), p.table_mask, p.stop_blob.as<uint8_t>(),
                                              p.n_stop, p.max_stop_len, p.stem, out_len.as<int64_t>(),
                                              keep.as<int32_t>());
    KERNEL_CHECK();
  }
  exclusive_sums(s, out_len.as<int64_t>(), out_off.as<int64_t>(), n_raw);
  exclusive_sums(s, keep.as<int32_t>(), keep_pre.as<int32_t>(), n_raw);
  {
    int32_t hk = 0;
    HIP_CHECK(hipMemcpyAsync(&n_out, out_off.as<int64_t>() + n_raw, 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&hk, keep_pre.as<int32_t>() + n_raw, 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    n_keep = hk;
  }
  // the invariants of stc_tokens_upload: kHashPad (zero) bytes behind the blob, u32 offsets when they fit
  t->off32 = n_out + kHashPad <= (int64_t(1) << 32);
  t->utf8.reserve(n_out + kHashPad);
  t->tok_off.reserve((t->off32 ? 4 : 8) * (n_keep + 1));
  HIP_CHECK(hipMemsetAsync(t->utf8.as<uint8_t>() + n_out, 0, kHashPad, s));
  if (t->off32)
    k_emit<uint32_t><<<grid_for(n_raw + 1), kBlock, 0, s>>>(d_text.as<uint8_t>(), tok_start.as<int64_t>(), out_off.as<int64_t>(),
                                                            keep_pre.as<int32_t>(), n_raw, t->utf8.as<uint8_t>(),
                                                            t->tok_off.as<uint32_t>());
  else
    k_emit<int64_t><<<grid_for(n_raw + 1), kBlock, 0, s>>>(d_text.as<uint8_t>(), tok_start.as<int64_t>(), out_off.as<int64_t>(),
                                                           keep_pre.as<int32_t>(), n_raw, t->utf8.as<uint8_t>(),
                                                           t->tok_off.as<int64_t>());
  KERNEL_CHECK();
  k_doc_off<<<grid_for(n_docs + 1), kBlock, 0, s>>>(raw_doc.as<int64_t>(), keep_pre.as<int32_t>(), n_docs,
                                                    t->doc_off.as<int64_t>(), small.as<unsigned long long>() + 1);
  KERNEL_CHECK();
  HIP_CHECK(hipMemcpyAsync(&t->max_doc, small.as<int64_t>() + 1, 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));  // the scratch buffers die at scope exit
  t->n_bytes = n_out;
  t->n_tok = n_keep;
  return t.release();
}

static void stem_tokens(Ctx& c, const uint8_t* utf8, int64_t n_bytes, const int64_t* tok_off, int64_t n_tok,
                        uint8_t* utf8_out, int64_t* tok_off_out) {
  single_device(c);
  STC_REQUIRE(n_bytes >= 0 && n_tok >= 0, "sizes must be >= 0");
  STC_REQUIRE(n_tok <= (int64_t(1) << 31) - 1, "at most 2^31-1 tokens per call");
  STC_REQUIRE(tok_off && tok_off_out && (n_bytes == 0 || (utf8 && utf8_out)), "utf8/tok_off/outputs");
  check_offsets("tok_off", tok_off, n_tok, n_bytes, "n_bytes", false);
  c.use();
  hipStream_t s = c.stream;
  DevBuf blob, off, bad, out_len, out_off, out, new_off;
  blob.reserve((size_t)std::max<int64_t>(n_bytes, 1));
  off.reserve(8 * (n_tok + 1));
  bad.reserve(8);
  out_len.reserve(8 * std::max<int64_t>(n_tok, 1));
  out_off.reserve(8 * (n_tok + 1));
  out.reserve((size_t)std::max<int64_t>(n_bytes, 1));
  new_off.reserve(8 * (n_tok + 1));
  if (n_bytes) HIP_CHECK(hipMemcpyAsync(blob.p, utf8, n_bytes, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(off.p, tok_off, 8 * (n_tok + 1), hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemsetAsync(bad.p, 0xFF, 8, s));
  if (n_tok > 0) {
    k_validate_tokens<<<grid_for(n_tok), kBlock, 0, s>>>(blob.as<uint8_t>(), off.as<int64_t>(), n_tok,
                                                         bad.as<unsigned long long>());
    KERNEL_CHECK();
  }
  int64_t hb = -1;
  HIP_CHECK(hipMemcpyAsync(&hb, bad.p, 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  if (hb != -1) throw_bad_utf8("the tokens", hb);
  if (n_tok > 0) {
    k_stem<<<grid_for(n_tok), kBlock, 0, s>>>(blob.as<uint8_t>(), off.as<int64_t>(), off.as<int64_t>() + 1, n_tok, n_bytes, nullptr,
                                              0, nullptr, 0, 0, 1, out_len.as<int64_t>(), nullptr);
    KERNEL_CHECK();
  }
  exclusive_sums(s, out_len.as<int64_t>(), out_off.as<int64_t>(), n_tok);
  k_emit<int64_t><<<grid_for(n_tok + 1), kBlock, 0, s>>>(blob.as<uint8_t>(), off.as<int64_t>(), out_off.as<int64_t>(), nullptr,
                                                         n_tok, out.as<uint8_t>(), new_off.as<int64_t>());
  KERNEL_CHECK();
  HIP_CHECK(hipMemcpyAsync(tok_off_out, new_off.p, 8 * (n_tok + 1), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  if (tok_off_out[n_tok] > 0) HIP_CHECK(hipMemcpyAsync(utf8_out, out.p, tok_off_out[n_tok], hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
}

}  // namespace prep
}  // namespace stc

using namespace stc;

extern "C" {

int stc_prep_create(stc_ctx* ctx, const uint32_t* strip_cp, int64_t n_strip, const uint8_t* stop_utf8, int64_t n_bytes,
                    const int64_t* stop_off, int64_t n_stop, int stem, stc_prep** out) {
  return guard([&] {
    STC_REQUIRE(ctx && out, "ctx/out");
    *out = prep::create(*ctx, strip_cp, n_strip, stop_utf8, n_bytes, stop_off, n_stop, stem);
  });
}

int stc_prep_free(stc_prep* p) {
  return guard([&] {
    if (!p) return;
    if (p->device >= 0) (void)hipSetDevice(p->device);
    delete p;
  });
}

int stc_prep_tokens(stc_ctx* ctx, const stc_prep* p, const uint8_t* text, int64_t n_bytes, const int64_t* text_off,
                    int64_t n_docs, stc_dtok** out) {
  return guard([&] {
    STC_REQUIRE(ctx && p && out, "ctx/prep/out");
    STC_REQUIRE(p->ctx == ctx, "the preprocessor belongs to another stc_ctx");
    *out = prep::tokens(*ctx, *p, text, n_bytes, text_off, n_docs);
  });
}

int stc_tokens_shape(const stc_dtok* t, int64_t* n_bytes, int64_t* n_tok, int64_t* n_docs) {
  return guard([&] {
    STC_REQUIRE(t, "tokens");
    if (n_bytes) *n_bytes = t->n_bytes;
    if (n_tok) *n_tok = t->n_tok;
    if (n_docs) *n_docs = t->n_docs;
  });
}

int stc_tokens_max_doc(const stc_dtok* t, int64_t* max_doc_out) {
  return guard([&] {
    STC_REQUIRE(t && max_doc_out, "tokens/max_doc_out");
    *max_doc_out = t->max_doc;
  });
}

int stc_tokens_download(stc_ctx* ctx, const stc_dtok* t, uint8_t* utf8_out, int64_t* tok_off_out, int64_t* doc_off_out) {
  return guard([&] {
    STC_REQUIRE(ctx && t, "ctx/tokens");
    STC_REQUIRE(t->ctx == ctx, "tokens were uploaded on another stc_ctx");
    ctx->use();
    hipStream_t s = ctx->stream;
    std::vector<uint32_t> narrow;
    if (utf8_out && t->n_bytes) HIP_CHECK(hipMemcpyAsync(utf8_out, t->utf8.p, t->n_bytes, hipMemcpyDeviceToHost, s));
    if (tok_off_out) {
      if (t->off32) {
        narrow.resize((size_t)t->n_tok + 1);
        HIP_CHECK(hipMemcpyAsync(narrow.data(), t->tok_off.p, 4 * (t->n_tok + 1), hipMemcpyDeviceToHost, s));
      } else {
        HIP_CHECK(hipMemcpyAsync(tok_off_out, t->tok_off.p, 8 * (t->n_tok + 1), hipMemcpyDeviceToHost, s));
      }
    }
    if (doc_off_out) HIP_CHECK(hipMemcpyAsync(doc_off_out, t->doc_off.p, 8 * (t->n_docs + 1), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    for (size_t q = 0; q < narrow.size(); ++q) tok_off_out[q] = narrow[q];
  });
}

int stc_stem_tokens(stc_ctx* ctx, const uint8_t* utf8, int64_t n_bytes, const int64_t* tok_off, int64_t n_tok,
                    uint8_t* utf8_out, int64_t* tok_off_out) {
  return guard([&] {
    STC_REQUIRE(ctx, "ctx");
    prep::stem_tokens(*ctx, utf8, n_bytes, tok_off, n_tok, utf8_out, tok_off_out);
  });
}

}  // extern "C"
