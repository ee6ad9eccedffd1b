"""Plain-Python restatement of the reference's text preprocessing between the lemmatiser and the vocabulary
(LDAClustering.scala:121-139 and :221-238), the checker of text_prep.hip:

    filterSpecialCharacters -> OpenNLP SimpleTokenizer -> drop stop words -> OpenNLP PorterStemmer

as include/stc.h states it ("Text preprocessing").  Works on ``str``; no third-party code.  A "char" is a
Java char (a UTF-16 code unit), so the stemmer runs on the UTF-16 code units of a token.
"""
from __future__ import annotations

import unicodedata

# the regex class of LDAClustering.scala:283-284 under java.util.regex: the trailing "' ' '-' '-'" is the
# range U+0020-U+002D
DEFAULT_STRIP = frozenset(list(range(0x20, 0x2E)) + [ord(c) for c in ".:;?@^_`"]
                          + [0x00AB, 0x00BB, 0x2019, 0x201D, 0x2212])

WHITESPACE, ALPHABETIC, NUMERIC, OTHER = "W", "A", "N", "O"
_JAVA_WS_CONTROLS = frozenset([0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x1C, 0x1D, 0x1E, 0x1F])


def char_class(cp: int) -> str:
    """SimpleTokenizer's class of a code point (>= U+10000: always OTHER, the stated departure)"""
    if cp >= 0x10000:
        return OTHER
    cat = unicodedata.category(chr(cp))
    # Character.isWhitespace (Zs/Zl/Zp but the no-break spaces, and nine controls) or category Zs
    if cp in _JAVA_WS_CONTROLS or cat in ("Zs", "Zl", "Zp"):
        return WHITESPACE
    if cat[0] == "L":
        return ALPHABETIC
    if cat == "Nd":
        return NUMERIC
    return OTHER


def tokenize(text: str, strip=DEFAULT_STRIP) -> list[str]:
    """steps 1 and 2: the stripped characters count as white space; a token is a maximal run of one class,
    an OTHER run also ends where the character changes, a code point >= U+10000 is a token of its own"""
    out = []
    start, state, pc = -1, WHITESPACE, -1
    for i, ch in enumerate(text):
        cp = ord(ch)
        c = WHITESPACE if cp in strip else char_class(cp)
        if state == WHITESPACE:
            if c != WHITESPACE:
                start = i
        elif c != state or (c == OTHER and (cp != pc or cp >= 0x10000)):
            out.append(text[start:i])
            start = i
        state, pc = c, cp
    if state != WHITESPACE:
        out.append(text[start:])
    return out


# ---- Porter stemmer: opennlp.tools.stemmer.PorterStemmer 1.6.0 (the Lucene-derived one) -----------------
class _Stemmer:
    def __init__(self, units):
        self.b = units  # list of UTF-16 code units
        self.k = len(units) - 1
        self.j = 0

    def cons(self, i):
        c = self.b[i]
        if c in (0x61, 0x65, 0x69, 0x6F, 0x75):
            return False
        if c == 0x79:
            return True if i == 0 else not self.cons(i - 1)
        return True

    def m(self):
        n, i, j = 0, 0, self.j
        while True:
            if i > j:
                return n
            if not self.cons(i):
                break
            i += 1
        i += 1
        while True:
            while True:
                if i > j:
                    return n
                if self.cons(i):
                    break
                i += 1
            i += 1
            n += 1
            while True:
                if i > j:
                    return n
                if not self.cons(i):
                    break
                i += 1
            i += 1

    def vowelinstem(self):
        return any(not self.cons(i) for i in range(0, self.j + 1))

    def doublec(self, j):
        if j < 1 or self.b[j] != self.b[j - 1]:
            return False
        return self.cons(j)

    def cvc(self, i):
        if i < 2 or not self.cons(i) or self.cons(i - 1) or not self.cons(i - 2):
            return False
        return self.b[i] not in (0x77, 0x78, 0x79)

    def ends(self, s):
        n = len(s)
        o = self.k - n + 1
        if o < 0:
            return False
        if any(self.b[o + q] != ord(s[q]) for q in range(n)):
            return False
        self.j = self.k - n
        return True

    def setto(self, s):
        o = self.j + 1
        for q, ch in enumerate(s):
            self.b[o + q] = ord(ch)
        self.k = self.j + len(s)

    def r(self, s):
        if self.m() > 0:
            self.setto(s)

    def step1(self):
        b = self.b
        if b[self.k] == 0x73:  # s
            if self.ends("sses"):
                self.k -= 2
            elif self.ends("ies"):
                self.setto("i")
            elif b[self.k - 1] != 0x73:
                self.k -= 1
        if self.ends("eed"):
            if self.m() > 0:
                self.k -= 1
        elif (self.ends("ed") or self.ends("ing")) and self.vowelinstem():
            self.k = self.j
            if self.ends("at"):
                self.setto("ate")
            elif self.ends("bl"):
                self.setto("ble")
            elif self.ends("iz"):
                self.setto("ize")
            elif self.doublec(self.k):
                ch = b[self.k]
                self.k -= 1
                if ch in (0x6C, 0x73, 0x7A):  # l s z
                    self.k += 1
            elif self.m() == 1 and self.cvc(self.k):
                self.setto("e")

    def step2(self):
        if self.ends("y") and self.vowelinstem():
            self.b[self.k] = 0x69

    _STEP3 = {"a": (("ational", "ate"), ("tional", "tion")),
              "c": (("enci", "ence"), ("anci", "ance")),
              "e": (("izer", "ize"),),
              "l": (("bli", "ble"), ("alli", "al"), ("entli", "ent"), ("eli", "e"), ("ousli", "ous")),
              "o": (("ization", "ize"), ("ation", "ate"), ("ator", "ate")),
              "s": (("alism", "al"), ("iveness", "ive"), ("fulness", "ful"), ("ousness", "ous")),
              "t": (("aliti", "al"), ("iviti", "ive"), ("biliti", "ble")),
              "g": (("logi", "log"),)}
    _STEP4 = {"e": (("icate", "ic"), ("ative", ""), ("alize", "al")),
              "i": (("iciti", "ic"),),
              "l": (("ical", "ic"), ("ful", "")),
              "s": (("ness", ""),)}
    _STEP5 = {"a": ("al",), "c": ("ance", "ence"), "e": ("er",), "i": ("ic",), "l": ("able", "ible"),
              "n": ("ant", "ement", "ment", "ent"), "o": ("ion", "ou"), "s": ("ism",), "t": ("ate", "iti"),
              "u": ("ous",), "v": ("ive",), "z": ("ize",)}

    def _switch(self, table, key):
        # each case breaks after its first matching suffix, whether or not r() replaces it
        for suf, rep in table.get(chr(key) if key < 0x80 else "", ()):
            if self.ends(suf):
                self.r(rep)
                return

    def step3(self):
        if self.k == 0:
            return
        self._switch(self._STEP3, self.b[self.k - 1])

    def step4(self):
        self._switch(self._STEP4, self.b[self.k])

    def step5(self):
        if self.k == 0:
            return
        key = self.b[self.k - 1]
        for suf in self._STEP5.get(chr(key) if key < 0x80 else "", ()):
            if self.ends(suf):
                if suf == "ion" and not (self.j >= 0 and self.b[self.j] in (0x73, 0x74)):
                    continue  # falls through to the next test of the case ("ou")
                if self.m() > 1:
                    self.k = self.j
                return

    def step6(self):
        self.j = self.k
        if self.b[self.k] == 0x65:
            a = self.m()
            if a > 1 or (a == 1 and not self.cvc(self.k - 1)):
                self.k -= 1
        if self.b[self.k] == 0x6C and self.doublec(self.k) and self.m() > 1:
            self.k -= 1

    def run(self):
        if self.k > 1:
            self.step1()
            self.step2()
            self.step3()
            self.step4()
            self.step5()
            self.step6()
        return self.b[:self.k + 1]


def _utf16(s: str) -> list[int]:
    raw = s.encode("utf-16-le", "surrogatepass")
    return [raw[i] | (raw[i + 1] << 8) for i in range(0, len(raw), 2)]


def stem(word: str) -> str:
    """PorterStemmer.stem(String): words of <= 2 chars unchanged; only a e i o u (and y after a consonant)
    are vowels"""
    u = _Stemmer(_utf16(word)).run()
    return b"".join(x.to_bytes(2, "little") for x in u).decode("utf-16-le", "surrogatepass")


def preprocess(text: str, stop_words=(), do_stem=True, strip=DEFAULT_STRIP) -> list[str]:
    """steps 1-4 of one document"""
    stop = stop_words if isinstance(stop_words, (set, frozenset)) else frozenset(stop_words)
    toks = [t for t in tokenize(text, strip) if t not in stop]
    return [stem(t) for t in toks] if do_stem else toks


def preprocess_docs(texts, stop_words=(), do_stem=True, strip=DEFAULT_STRIP) -> list[list[str]]:
    """step 5: every document yields a row, possibly empty (the reference drops empty ones; the caller's job)"""
    stop = frozenset(stop_words)
    return [preprocess(t, stop, do_stem, strip) for t in texts]


def parse_stop_words(text: str) -> list[str]:
    """the reference's stop-word file: every line split on ',' (Java's split: trailing empty strings dropped)"""
    out = []
    for line in text.splitlines():
        parts = line.split(",")
        while parts and parts[-1] == "":
            parts.pop()
        out.extend(parts)
    return out
