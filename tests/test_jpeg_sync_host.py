"""CPU: the piece-wise entropy stage of the JPEG reader through dad3d_jpeg_decode_sync_host, which runs the
`__host__ __device__` routines of csrc/jpeg_sync.hpp that the kernels of csrc/jpeg_decode_sync.hip run. Held to PIL on the corpus of
tests/jpeg_cases.py, the demo image and two files chosen for the hand-over, at pieces of 16 and 128 bytes; held to
dad3d_jpeg_decode_host on every damaged file of tests/test_jpeg_host.py; and its (mode, pieces, groups) held to the second statement
of the rules in tests/jpeg_sync_restatement.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import jpeg_sync_restatement as S
from jpeg_cases import MALFORMED, corpus, demo_bytes, header_defects, host_decode, jpeg, pil_array, picture, refused
from jpeg_sync_cases import PIECES, damaged, host_decode_sync, three_groups, unverified
from dad_3dheads_amd import _lib


def all_files():
    return list(corpus()) + [("the demo image", demo_bytes()), ("three groups", three_groups()), ("not verified", unverified())]


@functools.lru_cache(maxsize=None)
def decoded(piece_bytes):
    """{name: (flag, pixels, info)} of every file, once for all tests."""
    return {name: host_decode_sync(f, piece_bytes) for name, f in all_files()}


@pytest.mark.parametrize("piece_bytes", PIECES)
def test_every_file_equals_pil_and_none_is_flagged(piece_bytes):
    got = decoded(piece_bytes)
    for name, f in all_files():
        flag, pixels, _ = got[name]
        assert flag == 0, name
        assert np.array_equal(pixels, pil_array(f)), name


@pytest.mark.parametrize("piece_bytes", PIECES)
def test_info_equals_the_restatement(piece_bytes):
    got = decoded(piece_bytes)
    for name, f in all_files():
        assert got[name][2] == S.info(f, piece_bytes), name


def test_the_corpus_holds_every_mode():
    small, large = decoded(16), decoded(128)
    assert small["three groups"][2] == (1, 620, 3) and small["not verified"][2][0] == 2 and small["not verified"][2][2] >= 3
    assert large["the demo image"][2][0] == 1 and large["the demo image"][2][2] >= 3
    with_markers = [name for name, f in corpus() if b"\xff\xdd" in f[:f.index(b"\xff\xda")]]
    assert len(with_markers) > 100 and all(small[n][2] == (0, 0, 0) and large[n][2] == (0, 0, 0) for n in with_markers)
    assert {v[2][0] for v in small.values()} == {0, 1, 2}
    # a condition, not a measurement: at pieces of 128 bytes no ordinary file (smooth content, photos, noise up to quality 95) is left
    # to the serial walk -- and here no file at all is
    assert [n for n, v in large.items() if v[2][0] == 2] == []
    # several groups and verified, at 128 bytes too: only the demo image is long enough
    assert sum(v[2][2] >= 2 for v in large.values()) >= 1 and sum(v[2][2] >= 3 and v[2][0] == 1 for v in small.values()) >= 10


def test_piece_sizes_between_give_the_same_pixels():
    for f in (three_groups(), unverified(), corpus()[5][1]):
        want = pil_array(f)
        for piece_bytes in (32, 64, 256):
            flag, pixels, info = host_decode_sync(f, piece_bytes)
            assert flag == 0 and np.array_equal(pixels, want) and info == S.info(f, piece_bytes)


def test_channel_conversion():
    for name, f in corpus()[::23]:
        for channels in (1, 3):
            flag, pixels, _ = host_decode_sync(f, 16, channels)
            assert flag == 0 and np.array_equal(pixels, pil_array(f, channels)), (name, channels)


@pytest.mark.parametrize("piece_bytes", PIECES)
def test_damaged_files_get_the_flag_and_the_pixels_of_the_serial_decoder(piece_bytes):
    flagged = 0
    for what, f in damaged():
        want_flag, want = host_decode(f)
        flag, pixels, info = host_decode_sync(f, piece_bytes)
        assert flag == want_flag, what
        flagged += bool(flag)
        if flag == 0:
            assert np.array_equal(pixels, want), what
    assert 0 < flagged < len(damaged())


def test_info_of_damaged_files_equals_the_restatement():
    """What the header walk or the segment table flags has (0, 0, 0); what the strict walk flags keeps its pieces and groups."""
    seen = set()
    for what, f in damaged()[::13]:
        flag, _, info = host_decode_sync(f, 16)
        assert info == S.info(f, 16), what
        seen.add((bool(flag), info[0]))
    assert {(True, 0), (True, 1), (False, 1)} <= seen


def test_files_outside_the_decoder_and_header_defects_keep_their_flags():
    for name, (f, flag) in list(refused().items()) + list(header_defects().items()):
        got, pixels, info = host_decode_sync(f, 128)
        assert got == flag and pixels is None and info == (0, 0, 0) == S.info(f, 128), name


def test_data_that_ends_in_front_of_the_last_block_is_flagged():
    """The strict walk of the file's last piece finds that blocks are missing, as the serial walk finds a bit beyond the end."""
    f = jpeg(picture((64, 64, 3), 5, "ramp"), quality=90)
    scan = f.index(b"\xff\xda") + 14
    for cut in (scan, scan + 1, scan + 15, scan + 16, scan + 17, (scan + len(f)) // 2):
        short = f[:cut] + b"\xff\xd9"
        assert host_decode(short)[0] == MALFORMED
        for piece_bytes in PIECES:
            assert host_decode_sync(short, piece_bytes)[0] == MALFORMED, (cut, piece_bytes)


def test_argument_contract():
    lib = _lib.load()
    f = jpeg(picture((8, 8, 3), 4), quality=90)
    buf = (C.c_uint8 * len(f)).from_buffer_copy(f)
    h, w, c, flag = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    info = (C.c_int32 * 4)()
    refs = (C.byref(h), C.byref(w), C.byref(c), C.byref(flag))
    out = np.empty(8 * 8 * 3, np.uint8)
    for piece_bytes in (0, 8, 15, 24, 100, 512, -16):
        assert lib.dad3d_jpeg_decode_sync_host(buf, len(f), 0, piece_bytes, out.ctypes.data, out.size, *refs, info) == _lib.E_INVALID
    assert lib.dad3d_jpeg_decode_sync_host(buf, len(f), 2, 16, out.ctypes.data, out.size, *refs, info) == _lib.E_INVALID
    assert lib.dad3d_jpeg_decode_sync_host(buf, len(f), 0, 16, out.ctypes.data, out.size, *refs, None) == _lib.E_INVALID
    assert lib.dad3d_jpeg_decode_sync_host(buf, -1, 0, 16, out.ctypes.data, out.size, *refs, info) == _lib.E_INVALID
    assert lib.dad3d_jpeg_decode_sync_host(buf, len(f), 0, 16, out.ctypes.data, out.size - 1, *refs, info) == _lib.E_INVALID  # too small
    assert lib.dad3d_jpeg_decode_sync_host(buf, len(f), 0, 16, out.ctypes.data, out.size, *refs, info) == _lib.OK and flag.value == 0
    assert tuple(info) == (1, -(-(len(f) - 2 - f.index(b"\xff\xda") - 14) // 16), 1, 0)

    rows = np.zeros(2 * _lib.JPEG_DECODE_SYNC_DESC_INTS, np.int64)
    rows[:24] = [0, len(f), 8, 8, 3, 0, 24, 3, 0, 0, 0, 0] + [1024, 70000, 130, 140, 1, 192, 140, 1, 0, 0, 0, 0]
    grid = np.zeros(_lib.JPEG_DECODE_SYNC_GRID_INTS, np.int32)
    for piece_bytes in (0, 8, 48, 512):
        assert lib.dad3d_jpeg_decode_sync_scratch_bytes(rows.ctypes.data, 2, grid.ctypes.data, piece_bytes) == 0
    assert lib.dad3d_jpeg_decode_sync_scratch_bytes(None, 2, grid.ctypes.data, 16) == 0
    assert lib.dad3d_jpeg_decode_sync_scratch_bytes(rows.ctypes.data, 0, grid.ctypes.data, 16) == 0
    plain = lib.dad3d_jpeg_decode_scratch_bytes(rows.ctypes.data, 2, grid.ctypes.data)
    total = lib.dad3d_jpeg_decode_sync_scratch_bytes(rows.ctypes.data, 2, grid.ctypes.data, 16)
    pieces = [-(-len(f) // 16), -(-70000 // 16)]
    groups = [-(-p // 256) for p in pieces]
    assert total == plain + 32 * (sum(pieces) + sum(groups)) and grid[3] == max(groups) and total % 16 == 0
    more = rows[24:].reshape(2, 4)
    assert more[:, 1].tolist() == pieces and more[:, 3].tolist() == groups and more[0, 0] == plain and (more[:, [0, 2]] % 16 == 0).all()
    rows[2] = 0  # a height of 0
    assert lib.dad3d_jpeg_decode_sync_scratch_bytes(rows.ctypes.data, 2, grid.ctypes.data, 16) == 0
    # the device entry refuses the piece size and null pointers before it touches a device
    for piece_bytes in (0, 8, 48, 512):
        assert lib.dad3d_jpeg_decode_sync(1, 16, rows.ctypes.data, 1, grid.ctypes.data, piece_bytes, 1, 16, 1, 1, 16, 1 << 20, 0, None) == _lib.E_INVALID
    assert lib.dad3d_jpeg_decode_sync(None, 16, rows.ctypes.data, 1, grid.ctypes.data, 16, 1, 16, 1, 1, 16, 1 << 20, 0, None) == _lib.E_INVALID
    assert lib.dad3d_jpeg_decode_sync(1, 16, rows.ctypes.data, 1, grid.ctypes.data, 16, 1, 16, 1, None, 16, 1 << 20, 0, None) == _lib.E_INVALID
    assert lib.dad3d_jpeg_decode_sync(1, 16, rows.ctypes.data, 0, grid.ctypes.data, 16, 1, 16, 1, 1, 16, 1 << 20, 0, None) == _lib.E_INVALID
    lib.dad3d_clear_error()


def test_python_arguments_are_checked_before_a_device_is_asked_for():
    from dad_3dheads_amd import jpeg_reader

    with pytest.raises(ValueError):
        jpeg_reader.JpegDecoder(entropy="pieces")
    with pytest.raises(ValueError):
        jpeg_reader.JpegDecoder(entropy="sync", piece_bytes=48)
    assert jpeg_reader.SYNC_PIECE_BYTES in (64, 128, 256)
