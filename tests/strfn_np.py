"""The string transforms restated in plain Python: what the device kernels of csrc/strfn.hip
(vaex_amd/strings.py ``DeviceStringArray.lower`` ...) must produce, byte for byte.  It is the
oracle of the GPU tests; tests/test_strfn_np.py checks it against pyarrow and Python's ``str``.

Each transform is a function of one row's UTF-8 ``bytes`` (so that malformed input has a defined
answer too) and a column function over a list of ``str``.  Semantics are Python's ``str`` on valid
UTF-8 except where the reference's C++ differs, which is pinned here:

* lower / upper map one code point to one code point (``pyarrow.compute.utf8_lower`` /
  ``utf8_upper``; without pyarrow, Python's ``str.lower`` / ``str.upper`` where the result is one
  code point and the identity elsewhere).  A byte that starts no well-formed sequence (a stray
  continuation byte, a truncated or interrupted sequence, an overlong form, a value past
  U+10FFFF) is copied through.
* strip without an argument strips the six bytes of C ``isspace``, not Unicode whitespace: it
  keeps ``\\x1c`` .. ``\\x1f``, ``\\x85`` and ``\\xa0``, which ``str.strip`` removes.  With an argument it
  strips a set of ASCII bytes.
* pad widths count code points, the fill is one ASCII byte, and two-sided padding puts
  ``margin // 2 + (margin & width & 1)`` on the left (CPython's ``str.center``).
* zfill is left padding with ``'0'``: ``'-5'`` at width 4 is ``'00-5'`` (``str.zfill`` gives ``'-005'``).
* slice counts code points: a code point starts at every byte that is no continuation byte."""
import functools

import numpy as np

WHITESPACE = b" \t\n\v\f\r"


def _b(s):
    return s.encode("utf-8", "surrogatepass")


def _s(b):
    return b.decode("utf-8", "surrogatepass")


def column_bytes(col):
    """(offsets int64, data uint8) of a list of str: the Arrow layout the kernels write."""
    enc = [_b(s) for s in col]
    offsets = np.zeros(len(enc) + 1, np.int64)
    np.cumsum([len(e) for e in enc], out=offsets[1:])
    return offsets, np.frombuffer(b"".join(enc), dtype=np.uint8)


# ---- case ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_maps():
    """(lower, upper): dicts code point -> image over the code points >= 128 that change."""
    cps = [cp for cp in range(0x80, 0x110000) if not 0xD800 <= cp < 0xE000]
    try:
        import pyarrow as pa
        import pyarrow.compute as pc
        ar = pa.array([chr(cp) for cp in cps], type=pa.string())
        images = [pc.utf8_lower(ar).to_pylist(), pc.utf8_upper(ar).to_pylist()]
    except ImportError:
        images = [[chr(cp).lower() for cp in cps], [chr(cp).upper() for cp in cps]]
    out = []
    for im in images:
        out.append({cp: ord(t) for cp, t in zip(cps, im) if len(t) == 1 and ord(t) != cp})
    return tuple(out)


def _unit(b, i):
    """(size, code point or None) of the unit at the non-ASCII byte b[i]."""
    c = b[i]
    if 0xC0 <= c < 0xE0:
        size, v, least = 2, c & 0x1F, 0x80
    elif 0xE0 <= c < 0xF0:
        size, v, least = 3, c & 0x0F, 0x800
    elif 0xF0 <= c < 0xF8:
        size, v, least = 4, c & 0x07, 0x10000
    else:
        return 1, None
    if i + size > len(b):
        return 1, None
    for k in b[i + 1:i + size]:
        if k & 0xC0 != 0x80:
            return 1, None
        v = v << 6 | (k & 0x3F)
    if v < least or v > 0x10FFFF:
        return 1, None
    return size, v


def _case(b, upper, ascii):
    table = {} if ascii else case_maps()[1 if upper else 0]
    out = bytearray()
    i = 0
    while i < len(b):
        c = b[i]
        if c < 0x80:
            if upper and 0x61 <= c <= 0x7A:
                c -= 32
            elif not upper and 0x41 <= c <= 0x5A:
                c += 32
            out.append(c)
            i += 1
            continue
        size, cp = _unit(b, i)
        if cp is None or ascii:
            out += b[i:i + size]
        else:
            out += _b(chr(table.get(cp, cp)))
        i += size
    return bytes(out)


def lower_bytes(b):
    return _case(b, False, False)


def upper_bytes(b, ascii=False):
    return _case(b, True, ascii)


# ---- ranges --------------------------------------------------------------------------------------
def _starts(b):
    return [i for i, c in enumerate(b) if c & 0xC0 != 0x80]


def slice_bytes(b, start=0, stop=None):
    st = _starts(b)
    n = len(st)
    start, stop, _ = slice(start, stop).indices(n)

    def at(k):
        return 0 if k == 0 else (st[k] if k < n else len(b))
    b0, b1 = at(start), at(stop)
    return b[b0:b1] if b1 > b0 else b""


def _strip_set(to_strip):
    if to_strip is None:
        return WHITESPACE
    s = _b(to_strip)
    if any(c >= 0x80 for c in s):
        raise NotImplementedError("strip takes a set of ASCII characters")
    return s


def strip_bytes(b, to_strip=None, left=True, right=True):
    chars = _strip_set(to_strip)
    b0, b1 = 0, len(b)
    while left and b0 < b1 and b[b0] in chars:
        b0 += 1
    while right and b1 > b0 and b[b1 - 1] in chars:
        b1 -= 1
    return b[b0:b1]


def pad_bytes(b, width, side="left", fillchar=" "):
    fill = _b(fillchar)
    if len(fill) != 1 or fill[0] >= 0x80:
        raise ValueError("fillchar is one ASCII character")
    margin = max(0, width - len(_starts(b)))
    if side == "left":
        left = margin
    elif side == "right":
        left = 0
    elif side == "both":
        left = margin // 2 + (margin & width & 1)
    else:
        raise ValueError(f"side {side!r}")
    return fill * left + b + fill * (margin - left)


def repeat_bytes(b, repeats):
    return b * max(0, repeats)


def replace_bytes(b, pat, repl, n=-1):
    pat, repl = _b(pat), _b(repl)
    if not pat:
        raise ValueError("replace takes a pattern that is not empty")
    out = bytearray()
    i = 0
    while n != 0:
        f = b.find(pat, i)
        if f < 0:
            break
        out += b[i:f] + repl
        i = f + len(pat)
        n -= n > 0
    return bytes(out + b[i:])


# ---- columns (lists of str) ------------------------------------------------------------------
def _map(fn, col, *args, **kw):
    return [_s(fn(_b(s), *args, **kw)) for s in col]


def lower(col): return _map(lower_bytes, col)
def upper(col, ascii=False): return _map(upper_bytes, col, ascii)
def slice_(col, start=0, stop=None): return _map(slice_bytes, col, start, stop)
def strip(col, to_strip=None): return _map(strip_bytes, col, to_strip)
def lstrip(col, to_strip=None): return _map(strip_bytes, col, to_strip, True, False)
def rstrip(col, to_strip=None): return _map(strip_bytes, col, to_strip, False, True)
def pad(col, width, side="left", fillchar=" "): return _map(pad_bytes, col, width, side, fillchar)
def ljust(col, width, fillchar=" "): return pad(col, width, "right", fillchar)
def rjust(col, width, fillchar=" "): return pad(col, width, "left", fillchar)
def center(col, width, fillchar=" "): return pad(col, width, "both", fillchar)
def zfill(col, width): return pad(col, width, "left", "0")
def repeat(col, repeats): return _map(repeat_bytes, col, repeats)
def replace(col, pat, repl, n=-1): return _map(replace_bytes, col, pat, repl, n)


def cat(col, other):
    """``col + other``: other is a str constant or a second column; a str first argument with a
    column second is the constant-first form."""
    if isinstance(col, str):
        return [col + s for s in other]
    if isinstance(other, str):
        return [s + other for s in col]
    return [s + t for s, t in zip(col, other)]


TRANSFORMS = {"str_lower": lower, "str_upper": upper, "str_slice": slice_, "str_strip": strip, "str_lstrip": lstrip,
              "str_rstrip": rstrip, "str_pad": pad, "str_ljust": ljust, "str_rjust": rjust, "str_center": center,
              "str_zfill": zfill, "str_repeat": repeat, "str_cat": cat, "str_replace": replace}
