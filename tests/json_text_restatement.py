"""Python-integer restatement of the number rule of csrc/json_number.hpp: the text `repr(float(np.float32(x)))`
from exact integer arithmetic, stated as the rule itself (the shortest decimal string inside the rounding interval of the double,
the nearest among the shortest) and not as the kernel's algorithm. Shared by tests/test_json_text_host.py and
tests/test_gpu_json_text.py, with the sample set both use.
"""
import ctypes
import json

import numpy as np

MAX_NUMBER_BYTES, MAX_LITERAL_BYTES, FLAG_NONFINITE = 23, 64, 0x1
_POW10 = [10 ** i for i in range(400)]


def _floor_log10(num, den):
    """floor(log10(num / den)) for positive integers."""
    k = ((num.bit_length() - den.bit_length()) * 1233) >> 12  # an estimate, then exact steps
    while (num >= den * _POW10[k + 1]) if k + 1 >= 0 else (num * _POW10[-k - 1] >= den):
        k += 1
    while (num < den * _POW10[k]) if k >= 0 else (num * _POW10[-k] < den):
        k -= 1
    return k


def shortest_digits(bits):
    """float32 bit pattern (finite, non-zero) -> (D, decpt): value = 0.D x 10^decpt, D the shortest digit string that reads back to
    the DOUBLE, the nearest such, an exact tie to the even last digit."""
    be, fr = (bits >> 23) & 0xff, bits & 0x7fffff
    m, e = (fr | 0x800000, be - 150) if be else (fr, -149)
    shift = 24 - m.bit_length()  # a float32 denormal is a normal double: bring the top bit to 2^23
    m, e = m << shift, e - shift
    # in units of 2^(e - 31), a quarter of the double's ulp 2^(e - 29): the value and the two ends of its rounding interval
    v = m << 31
    lo, hi = v - (1 if m == 0x800000 else 2), v + 2  # the lower neighbour of a power of two is half as far; both ends count
    if e - 31 >= 0:
        v, lo, hi, den = v << (e - 31), lo << (e - 31), hi << (e - 31), 1
    else:
        den = 1 << (31 - e)
    # the largest p such that a multiple of 10^p lies in [lo, hi] / den: the width is below 10^p0, so p0 or p0 - 1
    p0 = _floor_log10(hi - lo, den) + 1
    for p in (p0, p0 - 1):
        if p >= 0:
            unit, a, b, c = den * _POW10[p], lo, hi, v
        else:
            unit, a, b, c = den, lo * _POW10[-p], hi * _POW10[-p], v * _POW10[-p]
        t_lo, t_hi = -((-a) // unit), b // unit
        if t_lo > t_hi:
            continue
        down = c // unit
        cands = [t for t in (down, down + 1) if t_lo <= t <= t_hi]
        assert cands, bits
        if len(cands) == 2:
            r = 2 * (c - down * unit)  # twice the distance to `down`, against one unit
            t = down if r < unit or (r == unit and down % 2 == 0) else down + 1
        else:
            t = cands[0]
        while t % 10 == 0:  # only p0 can give one (10^p0 itself)
            t, p = t // 10, p + 1
        digits = str(t)
        return digits, len(digits) + p
    raise AssertionError(bits)


def layout(neg, digits, decpt):
    sign = "-" if neg else ""
    if -4 < decpt <= 16:
        if decpt <= 0:
            return sign + "0." + "0" * -decpt + digits
        if decpt >= len(digits):
            return sign + digits + "0" * (decpt - len(digits)) + ".0"
        return sign + digits[:decpt] + "." + digits[decpt:]
    e = decpt - 1
    return sign + digits[0] + ("." + digits[1:] if len(digits) > 1 else "") + "e" + ("-" if e < 0 else "+") + "%02d" % abs(e)


def number_text(bits):
    """The text of one float32 bit pattern, or None for NaN / +-inf."""
    bits = int(bits)
    if (bits >> 23) & 0xff == 0xff:
        return None
    if bits & 0x7fffffff == 0:
        return "-0.0" if bits >> 31 else "0.0"
    return layout(bits >> 31, *shortest_digits(bits))


def python_numbers(x):
    """What Python prints: repr of every value widened to double."""
    return [repr(v) for v in np.asarray(x, dtype=np.float32).astype(np.float64).tolist()]


EDGE_FRACTIONS = (0, 1, 2, 0x3fffff, 0x400000, 0x400001, 0x7ffffe, 0x7fffff)
NAMED = np.array([0.1, 1e-4, 1e-5, 1e16, 9.99999e15, 1e22, 2.0 ** -20, 2.0 ** 100, 2.0 ** -149, np.finfo(np.float32).max, 0.0, -0.0, 123.0,
                  16777216.0], dtype=np.float32)
NAMED_TEXT = {0.1: "0.10000000149011612", 1e-4: "9.999999747378752e-05", 1e16: "1.0000000272564224e+16", 9.99999e15: "9999989535145984.0",
              2.0 ** -149: "1.401298464324817e-45", float(np.finfo(np.float32).max): "3.4028234663852886e+38", 123.0: "123.0",
              16777216.0: "16777216.0"}


def sample_bits(n_random=4096, seed=20241017):
    """Every biased exponent 0 .. 254 and both signs x (the edge fractions + `n_random` seeded fractions): uint32 bit patterns."""
    rng = np.random.default_rng(seed)
    fr = np.concatenate([np.array(EDGE_FRACTIONS, dtype=np.uint32), rng.integers(0, 2 ** 23, n_random, dtype=np.uint64).astype(np.uint32)])
    be = np.arange(255, dtype=np.uint32)
    pos = ((be[:, None] << np.uint32(23)) | fr[None, :]).ravel()
    return np.concatenate([pos, pos | np.uint32(0x80000000)])


def host_numbers(lib, x):
    """dad3d_json_number_host on float32 `x` -> list of str (None for a non-finite value)."""
    x = np.ascontiguousarray(x, dtype=np.float32).ravel()
    stride = 24
    out = np.full((x.size, stride), 0x23, dtype=np.uint8)
    lengths = np.zeros(x.size, dtype=np.int32)
    status = lib.dad3d_json_number_host(x.ctypes.data_as(ctypes.c_void_p), x.size, out.ctypes.data_as(ctypes.c_void_p), stride,
                                        lengths.ctypes.data_as(ctypes.c_void_p))
    assert status == 0, lib.dad3d_last_error()
    raw, ln = out.tobytes(), lengths.tolist()
    assert all((out[i, max(n, 0):] == 0x23).all() for i, n in enumerate(ln[:2000]))  # nothing behind a number is touched
    return [None if n < 0 else raw[i * stride: i * stride + n].decode("ascii") for i, n in enumerate(ln)]


def one_list_json(values):
    """json.dumps of a flat list of the float32 `values` widened to double (NaN / Infinity as json.dumps prints them)."""
    return json.dumps(np.asarray(values, dtype=np.float32).astype(np.float64).tolist()).encode("ascii")
