"""CPU: the host side of the text preprocessing — the C ABI's declarations and bindings, the stop-word file
format, and the generated character-class table."""
import ctypes as C
import importlib.util
import os
import re

import prep_oracle as P
from helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREP_SYMBOLS = ("stc_prep_create", "stc_prep_free", "stc_prep_tokens", "stc_tokens_shape", "stc_tokens_download",
                "stc_stem_tokens")


def _generator():
    spec = importlib.util.spec_from_file_location("gen_class_table", os.path.join(ROOT, "tools", "gen_class_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_symbols_are_declared_bound_and_exported():
    from stc import _lib

    header = open(os.path.join(ROOT, "include", "stc.h"), encoding="utf-8").read()
    lib = _lib.load()
    for name in PREP_SYMBOLS:
        assert re.search(r"^int\s+" + name + r"\s*\(", header, re.M), name
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None, name
    p, pu8, pi64 = C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_int64)
    want = {
        "stc_prep_create": [p, C.POINTER(C.c_uint32), C.c_int64, pu8, C.c_int64, pi64, C.c_int64, C.c_int, C.POINTER(p)],
        "stc_prep_free": [p],
        "stc_prep_tokens": [p, p, pu8, C.c_int64, pi64, C.c_int64, C.POINTER(p)],
        "stc_tokens_shape": [p, pi64, pi64, pi64],
        "stc_tokens_download": [p, p, pu8, pi64, pi64],
        "stc_stem_tokens": [p, pu8, C.c_int64, pi64, C.c_int64, pu8, pi64],
    }
    for name, args in want.items():
        res, got = _lib.SIGNATURES[name]
        assert res is C.c_int and got == args, name


def test_abi_version_is_unchanged():
    from stc import _lib

    assert _lib.load().stc_abi_version() == 2


def test_python_surface():
    import stc

    assert stc.DEFAULT_STRIP_CHARS and {ord(c) for c in stc.DEFAULT_STRIP_CHARS} == set(P.DEFAULT_STRIP)
    t = stc.TextPreprocessor(stopWords=["a", b"be"], stem=False, stripChars=".,")
    assert t.stopWords == ["a", "be"] and t.stem is False and t.stripChars == ".,"
    assert hasattr(stc.DeviceTokens, "download") and hasattr(stc.DeviceTokens, "from_handle")
    assert hasattr(stc.PorterStemmer, "stem")


def test_load_stop_words(tmp_path):
    import stc

    words = stc.io.load_stop_words(os.path.join(GOLDEN, "stop_words_en.txt"))
    assert len(words) == 120 and words[:3] == ["a", "able", "about"] and words[-1] == "thou"
    assert words == P.parse_stop_words(open(os.path.join(GOLDEN, "stop_words_en.txt"), encoding="utf-8").read())
    path = tmp_path / "stop.txt"
    path.write_text("der,die,,das,,\n\nund,oder\n", encoding="utf-8")  # Java's split drops trailing empty strings only
    assert stc.io.load_stop_words(str(path)) == ["der", "die", "", "das", "und", "oder"]


def test_class_table_is_what_the_generator_writes():
    gen = _generator()
    assert open(gen.OUT, encoding="utf-8").read() == gen.render()


def test_class_table_agrees_with_the_oracle():
    gen = _generator()
    name = {gen.OTHER: P.OTHER, gen.WHITESPACE: P.WHITESPACE, gen.ALPHABETIC: P.ALPHABETIC, gen.NUMERIC: P.NUMERIC}
    idx, data = gen.pages()
    for cp in range(0x10000):
        got = (data[idx[cp >> 8]][(cp & 0xFF) >> 2] >> (2 * (cp & 3))) & 3
        assert name[got] == P.char_class(cp), hex(cp)
    for cp in (0x09, 0x0D, 0x1C, 0x1F, 0x20, 0xA0, 0x2007, 0x202F, 0x2028, 0x2029, 0x3000):
        assert P.char_class(cp) == P.WHITESPACE, hex(cp)
    assert P.char_class(0x85) == P.OTHER and P.char_class(0x0661) == P.NUMERIC and P.char_class(0xB2) == P.OTHER
