"""Shared by tests/test_jpeg_sync_host.py and tests/test_gpu_jpeg_decode_sync.py: dad3d_jpeg_decode_sync_host through ctypes, the two
files the piece-wise entropy stage is tried hardest on, and the damaged files of tests/test_jpeg_host.py."""
import ctypes as C
import functools

import numpy as np

from dad_3dheads_amd import _lib
from jpeg_cases import demo_bytes, jpeg, picture

PIECES = (16, 128)


def host_decode_sync(data, piece_bytes, channels=None):
    """(flag, uint8 [H,W,C] or None, (mode, pieces, groups)) from dad3d_jpeg_decode_sync_host."""
    lib = _lib.load()
    h, w, c, flag = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    info = (C.c_int32 * 4)()
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    args = (C.byref(h), C.byref(w), C.byref(c), C.byref(flag), info)
    _lib.check(lib.dad3d_jpeg_decode_sync_host(buf, len(data), channels or 0, piece_bytes, None, 0, *args))
    if flag.value:
        return flag.value, None, tuple(info[:3])
    out = np.empty((h.value, w.value, c.value), np.uint8)
    _lib.check(lib.dad3d_jpeg_decode_sync_host(buf, len(data), channels or 0, piece_bytes, out.ctypes.data, out.size, *args))
    assert info[3] == 0
    return flag.value, (None if flag.value else out), tuple(info[:3])


@functools.lru_cache(maxsize=None)
def three_groups():
    """64 x 64 x 3 noise at quality 95 and 4:4:4: three groups of 256 pieces of 16 bytes, and the hand-over is verified."""
    return jpeg(picture((64, 64, 3), 11), quality=95, subsampling=0)


@functools.lru_cache(maxsize=None)
def unverified():
    """128 x 128 noise at quality 100: with codes of up to 16 bits and values of up to 10 the walks meet too late for pieces of 16
    bytes, so the file is decoded serially inside the call (mode 2); pieces of 128 bytes make it one group."""
    return jpeg(picture((128, 128), 12), quality=100)


@functools.lru_cache(maxsize=None)
def damaged():
    """[(what, bytes)]: every truncation of three small files and of the first 4 KB of the demo image, and every single-bit flip of
    a small file -- the files of test_truncated_files and test_every_single_bit_flip_of_a_small_file."""
    out = []
    small = [jpeg(picture((8, 8, 3), 1), quality=90), jpeg(picture((17, 9, 3), 2), quality=75, subsampling=2, restart_marker_blocks=1),
             jpeg(picture((12, 20), 3), quality=50)]
    for k, f in enumerate([demo_bytes()[:4096]] + small):
        out += [((k, n), f[:n]) for n in range(len(f))]
    f = jpeg(picture((8, 8, 3), 4), quality=90)
    out += [((at, bit), f[:at] + bytes([f[at] ^ (1 << bit)]) + f[at + 1:]) for at in range(len(f)) for bit in range(8)]
    return out
