"""CPU: the host side of the device JSON reader (csrc/json_parse_number.hpp, json_pow5_table.hpp, the C ABI of csrc/json_parse.hip). The
power table is recomputed with big integers; the kernels' own number routine, run on the CPU (`dad3d_json_parse_number_host`), gives
the bits of `float(text)` for every token it does not flag, flags exactly what DESIGN.md 4.14 lists and nothing a float32 or a
17-digit double can spell; the grammar rejects what `json.loads` rejects; the entries validate their arguments without a GPU."""
import ctypes
import importlib.util
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import json_parse_restatement as P
import json_text_restatement as R
from dad_3dheads_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "dad-3dheads_amd", "csrc")
F = P.FLAGS


def _want_bits(texts):
    return np.array([float(t) for t in texts], dtype=np.float64).view(np.uint64)


def test_power_table_equals_a_big_integer_recomputation():
    text = open(os.path.join(CSRC, "json_pow5_table.hpp")).read()
    q_min = int(re.search(r"#define DAD3D_JSON_POW5_MIN \((-?\d+)\)", text).group(1))
    q_max = int(re.search(r"#define DAD3D_JSON_POW5_MAX \((-?\d+)\)", text).group(1))
    rows = [(int(h, 16), int(lo, 16)) for h, lo in re.findall(r"\{0x([0-9a-f]{16})ull, 0x([0-9a-f]{16})ull\}", text)]
    assert (q_min, q_max) == (-342, 308) and len(rows) == 651
    for q, (hi, lo) in zip(range(q_min, q_max + 1), rows):
        t = (hi << 64) | lo
        assert 1 << 127 <= t < 1 << 128, q
        if q >= 0:  # the floor: the top 128 bits of 5^q
            p = 5 ** q
            shift = p.bit_length() - 128
            assert t == (p >> shift if shift >= 0 else p << -shift), q
        else:  # the reciprocal 2^b / 5^-q scaled into [2^127, 2^128): rounded up; past 5^27 computed wider and cut, within one of it
            p = 5 ** -q
            floor = (1 << (127 + (p - 1).bit_length())) // p
            assert t == floor + 1 if q >= -27 else floor <= t <= floor + 1, q
    spec = importlib.util.spec_from_file_location("gen_json_pow5", os.path.join(CSRC, "gen_json_pow5.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.render() == text
    assert subprocess.run([sys.executable, os.path.join(CSRC, "gen_json_pow5.py"), "--check"]).returncode == 0


def test_float32_values_are_never_flagged_and_exact():
    lib = _lib.load()
    x = np.concatenate([R.sample_bits().view(np.float32), R.NAMED]).astype(np.float64)
    texts = [repr(v) for v in x.tolist()]
    bits, is_int, flags = P.host_parse(lib, texts)
    assert not flags.any(), [(t, f) for t, f in zip(texts, flags.tolist()) if f][:10]  # float32 denormals are normal doubles
    assert np.array_equal(bits, x.view(np.uint64)) and not is_int.any()


def test_seeded_doubles_are_never_flagged_and_exact():
    lib = _lib.load()
    rng = np.random.default_rng(20241017)
    x = rng.uniform(1.0, 10.0, 200000) * 10.0 ** rng.integers(-300, 301, 200000) * rng.choice([-1.0, 1.0], 200000)
    texts = [repr(v) for v in x.tolist()]  # at most 17 significant digits, normal range
    bits, _, flags = P.host_parse(lib, texts)
    assert not flags.any(), [(t, f) for t, f in zip(texts, flags.tolist()) if f][:10]
    assert np.array_equal(bits, x.view(np.uint64))
    # the same values spelled otherwise: upper-case E, fixed 19 digits (the sign of the exponent is always written)
    other = [("%.18E" % v) if i % 2 else ("%.18e" % v).replace("e-", "E-") for i, v in enumerate(x[:20000].tolist())]
    bits, _, flags = P.host_parse(lib, other)
    assert not flags.any() and np.array_equal(bits, _want_bits(other))


def test_random_bit_patterns_flag_only_subnormals():
    lib = _lib.load()
    rng = np.random.default_rng(5)
    x = rng.integers(0, 2 ** 64, 100000, dtype=np.uint64).view(np.float64)
    x = x[np.isfinite(x)]
    texts = [repr(v) for v in x.tolist()]
    bits, _, flags = P.host_parse(lib, texts)
    subnormal = (np.abs(x) < P.MIN_NORMAL) & (x != 0)
    assert np.array_equal(flags != 0, subnormal) and set(flags[subnormal].tolist()) <= {F["subnormal"]}
    assert np.array_equal(bits[~subnormal], x.view(np.uint64)[~subnormal]) and not bits[subnormal].any()


def test_integers_and_named_tokens():
    lib = _lib.load()
    rng = np.random.default_rng(6)
    ints = [0, 1, -1, 7, 2 ** 24 + 1, 2 ** 53 - 1, 2 ** 53, -(2 ** 53)] + rng.integers(-2 ** 53, 2 ** 53, 5000).tolist()
    texts = [str(v) for v in ints]
    bits, is_int, flags = P.host_parse(lib, texts)
    assert not flags.any() and is_int.all() and np.array_equal(bits, _want_bits(texts))
    assert [int(np.uint64(b).view(np.float64)) for b in bits[:8]] == ints[:8]
    named = {"-0.0": 0, "0": 1, "-0": 1, "0.0": 0, "1E5": 0, "1e+5": 0, "1e-05": 0, "0e99999999999": 0, "0.000e-5": 0, "1234567890123456789e-5": 0,
             "0.0000000000000000000000001234567890123456789": 0, "123456789012345678.9": 0, "2.2250738585072014e-308": 0,
             "1.7976931348623157e308": 0, "17976931348623157e292": 0, "9007199254740993.0": 0, "9007199254740993e0": 0, "1e22": 0, "1e23": 0,
             "8.5e0": 0, "9007199254740993e-1": 0, "4503599627370496.5": 0, "4503599627370497.5": 0, "0.5e-0": 0}
    bits, is_int, flags = P.host_parse(lib, list(named))
    assert not flags.any() and is_int.tolist() == list(named.values()) and np.array_equal(bits, _want_bits(list(named)))
    assert bits[0] == 1 << 63 and bits[1] == 0 and bits[2] == 1 << 63  # the sign of a zero is kept; json.loads("-0") is the int 0


def test_flags_appear_exactly_where_listed():
    lib = _lib.load()
    cases = {
        "12345678901234567890": F["digits"], "1.2345678901234567890": F["digits"], "0.00012345678901234567890": F["digits"],
        "10000000000000000000": F["digits"], "1234567890123456789": F["big_int"], "9007199254740993": F["big_int"],
        "-9007199254740993": F["big_int"], "5e-324": F["subnormal"], "2.2250738585072011e-308": F["subnormal"], "1e-320": F["subnormal"],
        "1e-400": F["subnormal"], "1e-99999999999999999999": F["subnormal"], "1e309": F["overflow"], "1.8e308": F["overflow"],
        "1e99999999999999999999": F["overflow"], "1234567890123456789e291": F["overflow"],
    }
    bits, _, flags = P.host_parse(lib, list(cases))
    assert flags.tolist() == list(cases.values()) and not bits.any()
    for text in cases:  # what the host makes of them is still a number: the array goes to json.loads, not to an error
        json.loads(text)


@pytest.mark.parametrize("text", ["01", "1.", ".5", "-", "1e", "+1", "1e+", "--1", "", "-.5", "1.e5", "1e5.0", "1-2", "1e5e5", "00", "-01", "1..2",
                                  "e5", "1E", "1.5-", "0x10", "1e-", "-e", "."])
def test_grammar_rejects(text):
    lib = _lib.load()
    bits, is_int, flags = P.host_parse(lib, [text, "7"])
    assert flags.tolist() == [F["grammar"], 0] and bits[0] == 0
    with pytest.raises(ValueError):
        json.loads("[%s]" % text if text else "[,]")


def test_symbols_constants_and_validation_without_a_gpu():
    header = open(os.path.join(ROOT, "include", "dad3d.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("dad3d_json_parse_scratch_bytes", "dad3d_json_parse_index", "dad3d_json_parse_lists", "dad3d_json_parse_check_arrays",
                 "dad3d_json_parse_extract", "dad3d_json_parse_number_host"):
        assert re.search(r"DAD3D_EXPORT [a-z_0-9]+ " + name + r"\(", header), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert "benchmark.py:177-180" in header
    for name, value in {"TILE_BYTES": 4096, "RECORD_INTS": 6, **{"FLAG_" + k.upper(): v for k, v in F.items()}}.items():
        assert getattr(_lib, "JSON_PARSE_" + name) == value == int(re.search(r"#define DAD3D_JSON_PARSE_" + name + r" (\w+)", header).group(1), 0)
    lib = _lib.load()
    tile = _lib.JSON_PARSE_TILE_BYTES
    assert lib.dad3d_json_parse_scratch_bytes(1) == 16 + 20 and lib.dad3d_json_parse_scratch_bytes(tile) == tile + 20
    assert lib.dad3d_json_parse_scratch_bytes(tile + 1) == tile + 16 + 40 and lib.dad3d_json_parse_scratch_bytes(2 ** 31 - 1) == 2 ** 31 + 5 * 4 * 2 ** 19
    assert lib.dad3d_json_parse_scratch_bytes(0) == 0 and lib.dad3d_json_parse_scratch_bytes(-5) == 0 and lib.dad3d_json_parse_scratch_bytes(2 ** 31) == 0
    ptr = 0x10000  # never dereferenced: every call below is refused on the host
    for args in ((None, 64, ptr, 4096, ptr), (ptr, 0, ptr, 4096, ptr), (ptr, 2 ** 31, ptr, 2 ** 33, ptr), (ptr, 64, ptr, 83, ptr), (ptr + 8, 64, ptr, 4096, ptr)):
        lib.dad3d_clear_error()
        assert lib.dad3d_json_parse_index(*args, 0, None) == _lib.E_INVALID, args
        assert b"dad3d_json_parse_index" in lib.dad3d_last_error()
    assert lib.dad3d_json_parse_lists(ptr, 64, ptr, 4096, ptr, ptr, -1, ptr, ptr, ptr, ptr, 0, 0, None) == _lib.E_INVALID
    assert lib.dad3d_json_parse_lists(ptr, 64, ptr, 4096, ptr, None, 4, ptr, ptr, ptr, ptr, 0, 0, None) == _lib.E_INVALID
    assert lib.dad3d_json_parse_check_arrays(ptr, 64, ptr, ptr, 4, ptr, ptr, ptr, 4, ptr, ptr, None, 2, 0, None) == _lib.E_INVALID
    assert lib.dad3d_json_parse_check_arrays(ptr, 64, ptr, ptr, 4, ptr, ptr, ptr, 4, ptr, ptr, ptr, 0, 0, None) == _lib.OK  # nothing to do
    assert lib.dad3d_json_parse_extract(ptr, 64, ptr, 4, ptr, 1, 4, ptr, ptr, 3, 0, None) == _lib.E_INVALID
    assert lib.dad3d_json_parse_extract(ptr, 64, ptr, 4, ptr, 0, 0, ptr, ptr, 0, 0, None) == _lib.OK
    assert lib.dad3d_json_parse_number_host(None, None, None, 1, None, None, None) == _lib.E_INVALID
    assert lib.dad3d_json_parse_number_host(None, None, None, 0, None, None, None) == _lib.OK


def test_the_walk_that_predicts_lifted_arrays():
    """The prediction the GPU tests hold the reader to, on a tree small enough to read."""
    tree = {"a": [1, 2.5, 3], "b": [[1, 2], [3, 4]], "c": [[1, 2], [3]], "d": [1, [2]], "e": [], "f": [[[1, 2]]], "g": [1, True], "h": [float("nan"), 1],
            "i": [{"x": [5, 6]}, [7, 8]], "j": [2 ** 53 + 1, 1], "k": [5e-324, 1.0], "l": "[1,2]"}
    got = P.predict_lifted(tree, min_count=2)
    assert [g[0] for g in got] == [(3,), (2, 2), (2,), (2,)]
    assert got[0][1] == [P.double_bits(v) for v in (1.0, 2.5, 3.0)] and got[0][2] == [True, False, True]
    assert [g[0] for g in P.predict_lifted(tree, min_count=3)] == [(3,), (2, 2)]
