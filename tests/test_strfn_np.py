"""The plain-Python restatement of the string transforms (tests/strfn_np.py, the oracle of
tests/test_gpu_strfn.py) against pyarrow and Python's ``str`` where the definitions coincide,
and differing exactly where the reference's C++ is pinned; the case-table builder of
vaex_amd/strings.py and the offset-width rule.  No GPU."""
import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import strfn_np
import strings_np
from vaex_amd import strings

EDGE = strings_np.edge_strings()
TEXT = EDGE[:200] + ["  a b \t", "MiXed É ß İ ɐ Ɐ ẞ \U00010400\U00010428", "-5", "aaaa", "xaax", "é€\U0001d11e", "abc", ""]


# ---- case ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("upper", [False, True])
def test_case_equals_pyarrow_on_every_code_point(upper):
    cps = [cp for cp in range(0x110000) if not 0xD800 <= cp < 0xE000]
    ar = pa.array([chr(cp) for cp in cps], type=pa.string())
    want = (pc.utf8_upper if upper else pc.utf8_lower)(ar).to_pylist()
    fn = strfn_np.upper_bytes if upper else strfn_np.lower_bytes
    bad = [hex(cp) for cp, w in zip(cps, want) if fn(chr(cp).encode()) != w.encode()]
    assert not bad, bad[:10]
    # one code point to one code point; some images change their UTF-8 length
    assert all(len(w) == 1 for w in want)
    changed = sum(chr(cp) != w for cp, w in zip(cps, want))
    resized = sum(len(chr(cp).encode()) != len(w.encode()) for cp, w in zip(cps, want))
    assert (changed, resized) == ((1506, 34) if upper else (1488, 27))


def test_case_equals_pyarrow_on_the_edge_strings():
    ar = pa.array(EDGE, type=pa.string())
    assert strfn_np.lower(EDGE) == pc.utf8_lower(ar).to_pylist()
    assert strfn_np.upper(EDGE) == pc.utf8_upper(ar).to_pylist()
    assert strfn_np.upper(EDGE, ascii=True) == pc.ascii_upper(ar).to_pylist()
    assert strfn_np.upper(["straße", "ɐ", "İ"]) == ["STRAẞE", "Ɐ", "İ"] and strfn_np.lower(["İx", "ẞ"]) == ["ix", "ß"]


def test_malformed_bytes_are_copied_through():
    for raw in (b"AB\xc3", b"ab\xe2\x82", b"\xf0\x90\x90", b"\xa9Ab\x80", b"\xe2A\x82\xac", b"\xc1\x81", b"\xe0\x83\x9f",
                b"\xf4\x90\x80\x80", b"\xf8\x88\x80\x80\x80", b"\xed\xa0\x80"):
        low, up = strfn_np.lower_bytes(raw), strfn_np.upper_bytes(raw)
        assert len(low) == len(raw) and len(up) == len(raw)
        assert all(a == b or (a < 0x80 and b < 0x80) for a, b in zip(raw, low)) and low == raw.lower()
        assert up == raw.upper()
        assert strfn_np.slice_bytes(raw, 0, None) == raw and strfn_np.slice_bytes(raw, 0, 100) == raw
        assert strfn_np.pad_bytes(raw, 0) == raw and strfn_np.strip_bytes(raw) == raw


# ---- where Python's str is the definition ------------------------------------------------------
BOUNDS = [None, 0, 1, 2, 3, 5, 17, 18, 100, -1, -2, -5, -18, -100]


def test_slice_equals_python():
    for a in BOUNDS:
        for b in BOUNDS:
            assert strfn_np.slice_(TEXT, a or 0, b) == [s[(a or 0):b] for s in TEXT], (a, b)


@pytest.mark.parametrize("width", [0, 1, 4, 5, 6, 7, 18, 19, 40])
def test_justify_and_center_equal_python(width):
    for fill in (" ", "*"):
        assert strfn_np.ljust(TEXT, width, fill) == [s.ljust(width, fill) for s in TEXT]
        assert strfn_np.rjust(TEXT, width, fill) == [s.rjust(width, fill) for s in TEXT]
        assert strfn_np.center(TEXT, width, fill) == [s.center(width, fill) for s in TEXT]
        assert strfn_np.pad(TEXT, width, "left", fill) == strfn_np.rjust(TEXT, width, fill)
        assert strfn_np.pad(TEXT, width, "right", fill) == strfn_np.ljust(TEXT, width, fill)


def test_replace_equals_python():
    for pat in ("a", "aa", "ab", "f", "\0", "é", "zz-not-there", "aab"):
        for repl in ("", "X", "a", "longer than the pattern", "€"):
            for n in (-1, 0, 1, 2, 100):
                assert strfn_np.replace(TEXT, pat, repl, n) == [s.replace(pat, repl, n) for s in TEXT], (pat, repl, n)
    assert strfn_np.replace(["aaaa", "aaa"], "aa", "b") == ["bb", "ba"]  # leftmost, non-overlapping
    with pytest.raises(ValueError):
        strfn_np.replace(TEXT, "", "x")


def test_ascii_strip_sets_equal_python():
    for chars in ("a", "ab", "fx \x01", " ", "\x7f!", "z"):
        assert strfn_np.strip(TEXT, chars) == [s.strip(chars) for s in TEXT]
        assert strfn_np.lstrip(TEXT, chars) == [s.lstrip(chars) for s in TEXT]
        assert strfn_np.rstrip(TEXT, chars) == [s.rstrip(chars) for s in TEXT]
    assert strfn_np.strip(TEXT, "") == TEXT
    plain = [s for s in TEXT if not any(c in s for c in "\x1c\x1d\x1e\x1f\x85\xa0")]
    assert strfn_np.strip(plain) == [s.strip() for s in plain]
    with pytest.raises(NotImplementedError):
        strfn_np.strip(TEXT, "é")


def test_repeat_and_cat_equal_python():
    assert strfn_np.repeat(TEXT, 3) == [s * 3 for s in TEXT] and strfn_np.repeat(TEXT, 0) == [""] * len(TEXT)
    assert strfn_np.repeat(TEXT, -2) == [""] * len(TEXT)
    assert strfn_np.cat(TEXT, "_x") == [s + "_x" for s in TEXT] and strfn_np.cat("x_", TEXT) == ["x_" + s for s in TEXT]
    assert strfn_np.cat(TEXT, TEXT[::-1]) == [s + t for s, t in zip(TEXT, TEXT[::-1])]


# ---- where the reference's C++ is pinned instead -----------------------------------------------
def test_pinned_differences_from_python():
    # C isspace, not Unicode white space
    assert strfn_np.strip(["\x1c x \x1c", "\xa0x\xa0", "\x85x", " \t\n\v\f\rx\r\f\v\n\t "]) == ["\x1c x \x1c", "\xa0x\xa0", "\x85x", "x"]
    assert "\x1c x \x1c".strip() == "x" and "\xa0x\xa0".strip() == "x"
    # zfill is left padding with '0'
    assert strfn_np.zfill(["-5", "+5", "5", "12345"], 4) == ["00-5", "00+5", "0005", "12345"] and "-5".zfill(4) == "-005"
    # the fill is one ASCII byte
    for fill in ("é", "ab", ""):
        with pytest.raises(ValueError):
            strfn_np.pad(TEXT, 5, "left", fill)
    # CPython's center split
    assert strfn_np.center(["abc", "ab"], 6, "*") == ["*abc**", "**ab**"] and strfn_np.center(["ab"], 5, "*") == ["**ab*"]


# ---- the case-table builder ------------------------------------------------------------------------
@pytest.mark.parametrize("upper", [False, True])
def test_case_table_is_one_to_one_and_round_trips(upper):
    mapping = strings.case_mapping(upper)
    assert mapping == strfn_np.case_maps()[1 if upper else 0]
    assert len(mapping) == (1480 if upper else 1462)  # + the 26 ASCII letters the kernel maps inline
    assert all(0x80 <= k < 0x110000 and 0 <= v < 0x110000 and k != v for k, v in mapping.items())
    assert not any(0xD800 <= v < 0xE000 for v in mapping.values())
    table = strings.pack_case_table(mapping)
    assert table.dtype == np.uint32 and table.shape == (2 * len(mapping),) and len(mapping) <= strings.MAX_CASE_TABLE
    keys = table[0::2]
    assert (np.diff(keys.astype(np.int64)) > 0).all()  # sorted, no duplicates: the kernel searches it
    assert strings.unpack_case_table(table) == mapping
    assert strings.case_table(upper) is strings.case_table(upper)
    with pytest.raises(ValueError):
        strings.pack_case_table({0x41: 0x61})
    with pytest.raises(NotImplementedError):
        strings.pack_case_table({0x80 + k: 0x41 for k in range(strings.MAX_CASE_TABLE + 1)})


def test_case_table_without_pyarrow(monkeypatch):
    import sys
    monkeypatch.setitem(sys.modules, "pyarrow", None)  # `import pyarrow` raises ImportError
    for upper in (False, True):
        mapping = strings.case_mapping(upper)
        for cp in list(range(0x80, 0x3000)) + [0x10400, 0x10428, 0x1E9E]:
            t = chr(cp).upper() if upper else chr(cp).lower()
            assert mapping.get(cp, cp) == (ord(t) if len(t) == 1 else cp)


# ---- offsets of the result --------------------------------------------------------------------------
def test_offset_width_rule():
    for dt in (np.int32, np.int64):
        assert strings.take_offset_dtype(dt, 2 ** 31 - 1) == dt
        assert strings.take_offset_dtype(dt, 2 ** 31) == np.int64
    assert strings.take_offset_dtype(np.int32, 0) == np.int32


def test_transform_arguments_are_checked_without_a_device():
    ok = strings.transform_arguments
    assert ok("slice", 1, None) == dict(op="slice", a=1) and ok("slice", 0, -2) == dict(op="slice", a=0, b=-2, flags=1)
    assert ok("zfill", 4) == ok("pad", 4, "left", "0") == ok("rjust", 4, "0")
    assert ok("strip")["c0"] == b" \t\n\v\f\r" and ok("strip", "")["c0"] == b"" and ok("lstrip", "ab")["flags"] == 1
    assert ok("cat", "é")["c0"] == "é".encode() and ok("cat", "x", True)["flags"] == 1 and ok("cat", strings.COLUMN)["flags"] == 2
    assert ok("replace", "a", "bc", 2) == dict(op="replace", a=2, c0=b"a", c1=b"bc")
    assert ok("upper", True) == dict(op="upper", flags=1) and ok("repeat", -3) == dict(op="repeat", a=-3)
    for error, call in ((NotImplementedError, lambda: ok("replace", "a", "b", regex=True)),
                        (NotImplementedError, lambda: ok("replace", "a", "b", flags=2)),
                        (NotImplementedError, lambda: ok("strip", "é")), (NotImplementedError, lambda: ok("cat", "a" * 1025)),
                        (ValueError, lambda: ok("replace", "", "x")), (ValueError, lambda: ok("pad", 5, "left", "é")),
                        (ValueError, lambda: ok("center", 5, "ab")), (ValueError, lambda: ok("pad", 5, "middle")),
                        (ValueError, lambda: ok("repeat", 2 ** 63)), (TypeError, lambda: ok("repeat", 1.5)),
                        (TypeError, lambda: ok("slice", 0, 6, 2)), (TypeError, lambda: ok("zfill", True))):
        with pytest.raises(error):
            call()
    assert set(strings._ARGUMENTS) == set(strings.TRANSFORMS.values())


def test_transform_names_cover_the_model():
    assert set(strings.TRANSFORMS) == set(strfn_np.TRANSFORMS)
    assert set(strings.TRANSFORM_OPS) >= {"lower", "upper", "slice", "strip", "pad", "repeat", "cat", "replace"}
