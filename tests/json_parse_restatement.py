"""What the device JSON reader (csrc/json_parse.hip, dad_3dheads_amd/json_reader.py) must lift from a document, stated
as a walk over the tree `json.loads` returns, and the CPU entry of its number routine. Shared by tests/test_json_parse_host.py and
tests/test_gpu_json_parse.py."""
import ctypes
import math
import struct

import numpy as np

MIN_NORMAL = 2.2250738585072014e-308
FLAGS = {"grammar": 0x1, "digits": 0x2, "big_int": 0x4, "subnormal": 0x8, "overflow": 0x10, "ambiguous": 0x20}


def double_bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def _is_number(x):
    return isinstance(x, (int, float)) and not isinstance(x, bool)


def _device_number(x):
    """A number the routine converts: a finite double that is 0 or normal, an int up to 2^53."""
    if isinstance(x, int):
        return abs(x) <= 2 ** 53
    return math.isfinite(x) and (x == 0.0 or abs(x) >= MIN_NORMAL)


def _numeric(x):
    """A list that holds nothing but numbers and such lists: json.loads made it of the bytes `[ ] ,`, whitespace and number tokens
    (NaN and the infinities are spelled with letters)."""
    return isinstance(x, list) and all((_is_number(v) and (isinstance(v, int) or math.isfinite(v))) or _numeric(v) for v in x)


def _regular(x):
    """(shape, flat values) of a numeric list of shape (n,) or (r, c), else None."""
    if x and all(_is_number(v) for v in x):
        return (len(x),), list(x)
    if x and all(isinstance(v, list) and v and all(_is_number(w) for w in v) for v in x) and len({len(v) for v in x}) == 1:
        return (len(x), len(x[0])), [w for v in x for w in v]
    return None


def predict_lifted(tree, min_count=32):
    """[(shape, float64 bit patterns, is_int flags)] of the arrays the reader lifts, in document order: the maximal numeric arrays that
    are regular with at most two levels, hold at least `min_count` numbers, and only numbers the routine converts."""
    out = []

    def walk(x):
        if isinstance(x, list):
            if _numeric(x):
                reg = _regular(x)
                if reg and len(reg[1]) >= max(min_count, 1) and all(_device_number(v) for v in reg[1]):
                    out.append((reg[0], [double_bits(v) for v in reg[1]], [isinstance(v, int) for v in reg[1]]))
                return
            for v in x:
                walk(v)
        elif isinstance(x, dict):
            for v in x.values():
                walk(v)

    walk(tree)
    return out


def lifted_of(doc):
    """The same list from a json_reader.JsonDocument."""
    values = doc.values.cpu().numpy().view(np.uint64)
    is_int = doc.is_int.cpu().numpy()
    return [(a.shape, values[a.offset:a.offset + a.count].tolist(), [bool(k) for k in is_int[a.offset:a.offset + a.count]]) for a in doc.arrays]


def host_parse(lib, texts):
    """dad3d_json_parse_number_host on the tokens `texts` -> (bits uint64, is_int uint8, flags uint32)."""
    raw = [t.encode("ascii") for t in texts]
    lengths = np.array([len(r) for r in raw], dtype=np.int64)
    ends = np.cumsum(lengths)
    starts = ends - lengths
    blob = np.frombuffer(b"".join(raw) + b"#", dtype=np.uint8)
    n = len(raw)
    bits, is_int, flags = np.full(n, 0xAAAAAAAAAAAAAAAA, np.uint64), np.full(n, 7, np.uint8), np.full(n, 0xFFFF, np.uint32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    status = lib.dad3d_json_parse_number_host(p(blob), p(starts), p(ends), n, p(bits), p(is_int), p(flags))
    assert status == 0, lib.dad3d_last_error()
    return bits, is_int, flags
