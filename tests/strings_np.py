"""The string functions restated in plain Python and NumPy: what the device string kernels
(vaex_amd/strings.py, csrc/strings.hip) must compute, bit for bit.  tests/test_strings_np.py
checks this restatement against pandas; the GPU tests compare the kernels with it.

Strings are Python ``str``; a column is a list or an object array of them.  Lengths are UTF-8
bytes (``byte_length``) or code points (``len``); predicates compare UTF-8 bytes, which for
literal patterns is what comparing code points gives."""
import numpy as np


def _b(s):
    return s.encode("utf-8", "surrogatepass")


# ---- the edge strings ---------------------------------------------------------------------------
def edge_strings():
    """The empty string; lengths 0 .. 17 placed so that every start alignment 0 .. 7 occurs in
    the concatenated bytes; prefixes of one another; embedded NULs; UTF-8 of 2, 3 and 4 bytes;
    one string of 70,000 bytes among short ones."""
    out = [""]
    cur = 0
    for length in range(18):
        for align in range(8):
            pad = (align - cur) % 8
            if pad:
                out.append("f" * pad)
                cur += pad
            s = "".join(chr(1 + (i * 7 + length * 13 + align) % 126) for i in range(length))
            out.append(s)
            cur += length
    out += ["a", "ab", "a\0", "a\0b", "\0", "\0\0\0", "", "aaab", "aab", "xxaab", "b"]
    out += ["é", "€", "\U0001d11e", "aé€\U0001d11ez", "éé", "é"]
    out += ["x" + "".join(chr(97 + (i * 31 + i // 251) % 26) for i in range(69999)), "short", "a"]
    return out


def long_strings(n, mean=300, seed=0):
    """n strings whose mean length is about ``mean`` bytes (the wave-per-row form), drawn from a
    small alphabet so that long common prefixes occur, with duplicates."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(mean - 40, mean + 41, size=n)
    base = "".join(chr(97 + k % 26) for k in range(mean + 41))
    out = []
    for i, ln in enumerate(lens.tolist()):
        k = int(rng.integers(0, 50))
        out.append(base[:ln - 2] + "%02d" % k)
    return out


# ---- element-wise ------------------------------------------------------------------------------
def byte_length(col):
    return np.array([len(_b(s)) for s in col], dtype=np.int64)


def length(col):
    return np.array([len(s) for s in col], dtype=np.int64)


def equals(col, pat):
    return np.array([s == pat for s in col], dtype=bool)


def notequals(col, pat):
    return ~equals(col, pat)


def startswith(col, pat):
    p = _b(pat)
    return np.array([_b(s)[:len(p)] == p for s in col], dtype=bool)


def endswith(col, pat):
    p = _b(pat)
    return np.array([len(_b(s)) >= len(p) and _b(s)[len(_b(s)) - len(p):] == p for s in col], dtype=bool)


def contains(col, pat):
    p = _b(pat)
    return np.array([_b(s).find(p) >= 0 for s in col], dtype=bool)


PREDICATES = {"str_equals": equals, "str_notequals": notequals, "str_startswith": startswith,
              "str_endswith": endswith, "str_contains": contains}


# ---- the encoder ---------------------------------------------------------------------------------
def encode(col, known=None):
    """(codes int32, dictionary list): first-appearance codes.  ``known``: a dictionary to go
    on from (a second ``update``)."""
    keys = list(known or [])
    index = {k: i for i, k in enumerate(keys)}
    codes = np.empty(len(col), np.int32)
    for i, s in enumerate(col):
        c = index.get(s)
        if c is None:
            c = index[s] = len(keys)
            keys.append(s)
        codes[i] = c
    return codes, keys


def map_ordinal(col, keys):
    index = {k: i for i, k in enumerate(keys)}
    return np.array([index.get(s, -1) for s in col], dtype=np.int32)


def bytewise_sorted(keys):
    return sorted(keys, key=_b)


def value_counts(col, ascending=False):
    """(keys, counts) in the numeric rule's order: the keys ascending bytewise, then a stable
    sort by count; descending is the exact reverse of that."""
    counts = {}
    for s in col:
        counts[s] = counts.get(s, 0) + 1
    keys = bytewise_sorted(counts)
    c = np.array([counts[k] for k in keys], dtype=np.int64)
    order = np.argsort(c, kind="stable")
    if not ascending:
        order = order[::-1]
    return [keys[i] for i in order], c[order]


def unique(col):
    return encode(col)[1]


# ---- sort ----------------------------------------------------------------------------------------
def argsort(col, ascending=True):
    """np.argsort(kind="stable") over the str objects (Python's str order is the code points',
    which is the UTF-8 bytes'); descending is the exact reverse."""
    order = np.argsort(np.array(list(col), dtype=object), kind="stable")
    return order if ascending else order[::-1]


def lexsort(cols, ascending=True):
    """np.lexsort with the first column the most significant; str columns as objects."""
    keys = [np.array(list(c), dtype=object) if len(c) and isinstance(c[0], str) else np.asarray(c) for c in cols]
    order = np.lexsort(keys[::-1])
    return order if ascending else order[::-1]
