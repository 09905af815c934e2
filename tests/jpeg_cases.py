"""Shared by tests/test_jpeg_host.py and tests/test_gpu_jpeg_decode.py: JPEG files written by PIL, files the device must refuse,
hand-made header defects, and dad3d_jpeg_decode_host through ctypes."""
import ctypes as C
import functools
import io
import os
import warnings

import numpy as np
from PIL import Image

from dad_3dheads_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MALFORMED, UNSUPPORTED = _lib.JPEG_DECODE_FLAG_MALFORMED, _lib.JPEG_DECODE_FLAG_UNSUPPORTED


def picture(shape, seed, kind="noise"):
    """uint8 [h,w] or [h,w,3]: noise, a ramp, or flat 8x8 blocks."""
    rng = np.random.default_rng(seed)
    h, w = shape[:2]
    if kind == "noise":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == "ramp":
        y, x = np.mgrid[0:h, 0:w]
        base = ((3 * x + 5 * y + seed) % 256).astype(np.uint8)
    else:
        base = np.kron(rng.integers(0, 256, ((h + 7) // 8, (w + 7) // 8), dtype=np.uint8), np.ones((8, 8), np.uint8))[:h, :w]
    return base if len(shape) == 2 else np.stack([base, np.roll(base, 3, axis=1), 255 - base], axis=2)


def jpeg(img, **options):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", **options)
    return buf.getvalue()


def pil_array(data, channels=None):
    """What PIL makes of the bytes; warnings of libjpeg are PIL's own business."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        im = Image.open(io.BytesIO(data))
        im.load()
        if channels is not None:
            im = im.convert({1: "L", 3: "RGB"}[channels])
        arr = np.asarray(im)
    return arr[:, :, None] if arr.ndim == 2 else arr


def pil_raises(data):
    try:
        pil_array(data)
    except Exception:  # noqa: BLE001 -- PIL's own error, whatever its class
        return True
    return False


def demo_bytes():
    return np.load(os.path.join(ROOT, "tests", "golden", "demo_image.npz"))["jpeg"].tobytes()


def host_decode(data, channels=None):
    """(flag, uint8 [H,W,C] or None) from dad3d_jpeg_decode_host."""
    lib = _lib.load()
    h, w, c, flag = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    args = (C.byref(h), C.byref(w), C.byref(c), C.byref(flag))
    _lib.check(lib.dad3d_jpeg_decode_host(buf, len(data), channels or 0, None, 0, *args))
    if flag.value:
        return flag.value, None
    out = np.empty((h.value, w.value, c.value), np.uint8)
    _lib.check(lib.dad3d_jpeg_decode_host(buf, len(data), channels or 0, out.ctypes.data, out.size, *args))
    return flag.value, (None if flag.value else out)


@functools.lru_cache(maxsize=None)
def corpus():
    """[(name, bytes)]: a few hundred baseline files, none larger than 140 x 140."""
    files = []
    sizes = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33)
    for i, h in enumerate(sizes):
        for j, w in enumerate(sizes):
            img = picture((h, w, 3), 100 * i + j, ("noise", "ramp", "flat")[(i + j) % 3])
            for sub in (0, 1, 2):
                files.append((f"{h}x{w} sub {sub}", jpeg(img, quality=85, subsampling=sub)))
                files.append((f"{h}x{w} sub {sub} restart 1", jpeg(img, quality=85, subsampling=sub, restart_marker_blocks=1)))
    rng = np.random.default_rng(7)
    for k in range(24):
        h, w = (int(v) for v in rng.integers(1, 140, 2))
        q, sub, kind = (1, 50, 95, 100)[k % 4], k % 3, ("noise", "ramp", "flat")[(k // 4) % 3]
        files.append((f"random {h}x{w} q{q} sub {sub} {kind}", jpeg(picture((h, w, 3), k, kind), quality=q, subsampling=sub)))
        files.append((f"random grey {h}x{w} q{q}", jpeg(picture((h, w), k, kind), quality=q)))
    for sub in (0, 1, 2):
        img = picture((75, 131, 3), 40 + sub)
        files.append((f"optimize sub {sub}", jpeg(img, quality=90, subsampling=sub, optimize=True)))
        files.append((f"restart rows sub {sub}", jpeg(img, quality=90, subsampling=sub, restart_marker_rows=1)))
        files.append((f"restart 3 of 50 or 90 MCUs sub {sub}", jpeg(img, quality=75, subsampling=sub, restart_marker_blocks=7)))
        files.append((f"restart 4 optimize sub {sub}", jpeg(img, quality=30, subsampling=sub, restart_marker_blocks=4, optimize=True)))
    files.append(("grey restart 1", jpeg(picture((40, 41), 3), quality=90, restart_marker_blocks=1)))
    files.append(("grey restart rows", jpeg(picture((40, 41), 4, "ramp"), quality=90, restart_marker_rows=1)))
    return files


def markers(data):
    """[(marker, start, end)] of the segments in front of the entropy data: data[start:end] is FF xx and the segment."""
    out, pos = [], 2
    while data[pos + 1] != 0xDA:
        n = data[pos + 2] << 8 | data[pos + 3]
        out.append((data[pos + 1], pos, pos + 2 + n))
        pos += 2 + n
    n = data[pos + 2] << 8 | data[pos + 3]
    out.append((0xDA, pos, pos + 2 + n))
    return out


def patched(data, at, value):
    return data[:at] + bytes([value]) + data[at + 1:]


def refused():
    """{name: (bytes, flag)}: valid files outside the decoder."""
    img = picture((24, 20, 3), 5)
    base = jpeg(img, quality=90)
    sof = next(s for m, s, _ in markers(base) if m == 0xC0)
    cmyk = io.BytesIO()
    Image.fromarray(picture((9, 12, 3), 6)).convert("CMYK").save(cmyk, "JPEG")
    return {"progressive": (jpeg(img, quality=90, progressive=True), UNSUPPORTED), "CMYK": (cmyk.getvalue(), UNSUPPORTED),
            "SOF1": (patched(base, sof + 1, 0xC1), UNSUPPORTED)}


def header_defects():
    """{name: (bytes, flag)}: one defect each in a 4:2:0 file of PIL's."""
    base = jpeg(picture((24, 20, 3), 8), quality=90, subsampling=2)
    seg = {m: (s, e) for m, s, e in reversed(markers(base))}  # the first of each kind
    dqt, dht, sof, sos = seg[0xDB][0], seg[0xC4][0], seg[0xC0][0], seg[0xDA][0]
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01"
    dri3 = b"\xff\xdd\x00\x05\x00\x04\x00"
    rgb_ids = patched(patched(patched(base, sof + 10, ord("R")), sof + 13, ord("G")), sof + 16, ord("B"))
    rgb_ids = patched(patched(patched(rgb_ids, sos + 5, ord("R")), sos + 7, ord("G")), sos + 9, ord("B"))
    app0 = seg[0xE0]
    cases = {
        "no SOI": (patched(base, 1, 0xD9), MALFORMED),
        "16-bit quantisation table": (patched(base, dqt + 4, 0x10), UNSUPPORTED),
        "quantisation table 4": (patched(base, dqt + 4, 0x04), MALFORMED),
        "Huffman class 2": (patched(base, dht + 4, 0x20), MALFORMED),
        "a Huffman code that overflows its length": (patched(base, dht + 5, 3), MALFORMED),
        "12-bit samples": (patched(base, sof + 4, 12), UNSUPPORTED),
        "width 0": (patched(patched(base, sof + 7, 0), sof + 8, 0), MALFORMED),
        "sampling 4x1": (patched(base, sof + 11, 0x41), UNSUPPORTED),
        "a second SOF0": (base[:sos] + base[sof:seg[0xC0][1]] + base[sos:], MALFORMED),
        "Se = 62": (patched(base, seg[0xDA][1] - 2, 62), UNSUPPORTED),
        "a table nobody defined": (patched(base, sos + 6, 0x03), MALFORMED),
        "an Adobe APP14": (base[:sof] + adobe + base[sof:], UNSUPPORTED),
        "DRI of three bytes": (base[:sos] + dri3 + base[sos:], MALFORMED),
        "component ids R G B without JFIF": (rgb_ids[:app0[0]] + rgb_ids[app0[1]:], UNSUPPORTED),
        "fill bytes in front of EOI": (base[:-2] + b"\xff" + base[-2:], UNSUPPORTED),
        "no EOI": (base[:-2], MALFORMED),
    }
    return cases
