"""CPU: the inflate routine the decode kernels run (csrc/inflate.hpp through dad3d_inflate_host) against
`zlib.decompress`, and the plain-Python restatement of tests/png_decode_restatement.py pinned to zlib and PIL first. Valid streams of
every compressor setting and the hand-written ones zlib does not produce must inflate to zlib's bytes with flag 0, whole and cut into
ranges of 1 byte, 7 bytes and with empty ranges; a malformed stream must set a flag wherever zlib raises, and give zlib's bytes where
zlib does not; the guard bytes around the output stay intact in every call (png_decode_restatement.host_inflate)."""
import zlib

import numpy as np
import pytest

import png_decode_restatement as D
import png_restatement as R
from dad_3dheads_amd import _lib

SPLITS = (1, 7, "whole", "empties")


@pytest.fixture(scope="module")
def valid():
    return D.valid_streams()


def test_the_restatement_is_zlib_on_valid_streams(valid):
    for name, stream, data in valid:
        assert zlib.decompress(stream) == data, name
        if len(stream) < 30000:  # the long ones: test_compressor_settings_cover_what_the_table_says
            assert D.inflate(stream) == data, name
    rng = np.random.default_rng(3)
    for i in range(40):
        data = rng.integers(0, rng.integers(1, 257), rng.integers(0, 600), dtype=np.uint8).tobytes()
        for name, kw in D.SETTINGS:
            assert D.inflate(D.compress(data, **kw)) == data, (i, name)


def test_the_restatement_refuses_what_zlib_refuses():
    cases = D.malformed_streams() + [(f"cut at {k}", s) for k, s in enumerate(D.truncation_sweep())]
    cases += [(f"bit {i}", s) for i, s in enumerate(D.bit_flips())]
    refused = 0
    for name, stream in cases:
        want = D.zlib_says(stream)
        try:
            got = D.inflate(stream)
        except D.InflateError:
            got = None
        assert got == want, name
        refused += want is None
    assert refused > len(cases) // 2


def test_every_named_malformed_stream_is_refused_by_zlib():
    for name, stream in D.malformed_streams():
        assert D.zlib_says(stream) is None, name


def test_the_png_writer_is_read_by_pil():
    rng = np.random.default_rng(4)
    for c in (1, 2, 3, 4):
        img = rng.integers(0, 256, (7, 5, c), dtype=np.uint8)
        for types in ([0] * 7, [1] * 7, [2] * 7, [3] * 7, [4] * 7, [(7 * y + 3) % 5 for y in range(7)]):
            data = D.write_png(img, types=types, split=7, before=[(b"gAMA", b"\0\0\xb1\x8f")], after=[(b"tEXt", b"k\0v")], empties=True)
            mode, px = R.pil_pixels(data)
            assert mode == R.PIL_MODE[c] and np.array_equal(px, img)
            info = R.read_png(D.write_png(img, types=types, split=3))
            assert np.array_equal(R.unfilter(info["stream"], 7, 5, c), img)
            assert [k for k, _ in D.read_chunks(data)][:2] == [b"IHDR", b"gAMA"]


def test_compressor_settings_cover_what_the_table_says(valid):
    """What each zlib setting is in the list for, read off its stream by the restatement: block types 0 / 1 / 2, the largest
    distance, the longest match, the longest code."""
    seen = {}
    for name, stream, data in valid[:len(D.SETTINGS)]:
        seen[name] = {}
        assert D.inflate(stream, seen[name]) == data, name
    assert seen["level 0"]["kinds"] == {0}
    assert 1 in seen["fixed"]["kinds"] and 2 not in seen["fixed"]["kinds"]
    assert 2 in seen["huffman only"]["kinds"] and seen["huffman only"]["length"] == 0
    assert 2 in seen["rle"]["kinds"] and seen["rle"]["distance"] == 1
    for name in ("level 1", "level 6", "level 9"):
        assert 2 in seen[name]["kinds"] and seen[name]["distance"] > 8192 and seen[name]["code_bits"] >= 12, (name, seen[name])
    assert max(seen[name]["distance"] for name in ("level 1", "level 6", "level 9")) > 30000
    assert max(t["code_bits"] for t in seen.values()) == 14
    assert seen["wbits 9"]["distance"] <= 512 and 2 in seen["wbits 9"]["kinds"]
    for name in ("fixed", "rle", "level 1", "level 6", "level 9", "wbits 9"):
        assert seen[name]["length"] == 258, name


def test_valid_streams_whole_and_in_ranges(valid):
    for name, stream, data in valid:
        for rule in SPLITS:
            if rule == 1 and len(stream) > 20000:
                continue  # ranges of one byte: the short streams and the fuzz cover them
            flag, got = D.host_inflate(D.split_ranges(stream, rule), len(data))
            assert flag == 0, (name, rule)
            assert got == data, (name, rule)


def test_exact_capacity_and_overflow(valid):
    for name, stream, data in valid:
        if not data:
            continue
        flag, _ = D.host_inflate([stream], len(data) - 1)
        assert flag == _lib.PNG_DECODE_FLAG_OVERFLOW, name
    flag, got = D.host_inflate([], 16)
    assert flag == _lib.PNG_DECODE_FLAG_MALFORMED and got == b""


def test_fuzz_against_zlib():
    rng = np.random.default_rng(7)
    n_inputs, n_streams = 2400, 0
    for i in range(n_inputs):
        kind = i % 4
        n = int(rng.integers(0, 3000 if i % 16 < 4 else 250))  # every kind at both sizes; most inputs short, to stay quick
        if kind == 0:
            data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        elif kind == 1:
            data = rng.integers(0, int(rng.integers(1, 6)), n, dtype=np.uint8).tobytes()
        elif kind == 2:
            piece = rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8).tobytes()
            data = (piece * (n // len(piece) + 1))[:n]
        else:
            base = rng.integers(0, 256, max(n // 3, 1), dtype=np.uint8).tobytes()
            data = base + bytes(int(rng.integers(0, 300))) + base[::-1] + base
        for name, kw in D.SETTINGS:
            stream = D.compress(data, **kw)
            n_streams += 1
            for rule in SPLITS:
                flag, got = D.host_inflate(D.split_ranges(stream, rule), len(data) + int(rng.integers(0, 3)))
                assert flag == 0, (i, name, rule)
                assert got == data, (i, name, rule)
    assert n_streams == n_inputs * len(D.SETTINGS) and n_inputs >= 2000  # thousands of inputs, each through every setting


def check_against_zlib(name, stream, capacity=4096):
    want = D.zlib_says(stream)
    for rule in ("whole", 1):
        flag, got = D.host_inflate(D.split_ranges(stream, rule), capacity)
        if want is None:
            assert flag != 0, name
        else:
            assert flag == 0 and got == want, name
    return want is None


def test_malformed_streams(valid):
    # first: nothing of the valid list is flagged, so a fallback cannot hide a fault
    for name, stream, data in valid:
        assert D.host_inflate([stream], len(data))[0] == 0, name
    for name, stream in D.malformed_streams():
        assert check_against_zlib(name, stream), name


def test_truncation_at_every_length():
    for k, stream in enumerate(D.truncation_sweep()):
        assert check_against_zlib(f"cut at {k}", stream)


def test_every_single_bit_flip():
    refused = sum(check_against_zlib(f"bit {i}", stream) for i, stream in enumerate(D.bit_flips()))
    assert refused > 400
