"""Shared by tests/test_jpeg_encode_host.py and tests/test_gpu_jpeg_encode.py: the corpus of images and options the JPEG encoder is
held to PIL on (built here, from seeds), PIL's own bytes for a case, and dad3d_jpeg_encode_host through ctypes."""
import ctypes as C
import functools
import io

import numpy as np
from PIL import Image

import jpeg_encode_restatement as R
from dad_3dheads_amd import _lib
from jpeg_cases import picture

SIDES = (1, 2, 7, 8, 9, 15, 16, 17, 31, 33)
QUALITIES = (1, 24, 50, 75, 95, 100)


def pil_bytes(img, quality=75, subsampling=None, restart_marker_rows=0, restart_marker_blocks=0):
    """The oracle: uint8 [H,W,1] is saved as mode L, [H,W,3] as RGB; `subsampling` None is PIL's own default."""
    options = {"quality": quality}
    if restart_marker_rows:
        options["restart_marker_rows"] = restart_marker_rows
    if restart_marker_blocks:
        options["restart_marker_blocks"] = restart_marker_blocks
    if img.shape[2] == 3 and subsampling is not None:
        options["subsampling"] = subsampling
    buf = io.BytesIO()
    Image.fromarray(img[:, :, 0] if img.shape[2] == 1 else img).save(buf, "JPEG", **options)
    return buf.getvalue()


def image(h, w, c, seed, kind):
    if kind in ("zeros", "ones"):
        return np.full((h, w, c), 0 if kind == "zeros" else 255, np.uint8)
    if kind == "constant":
        return np.full((h, w, c), 97, np.uint8)
    return picture((h, w, 3), seed, kind) if c == 3 else picture((h, w), seed, kind)[:, :, None]


def interval_of(img, options):
    """The restart interval in MCUs the C entry points take for a case."""
    h, w, c = img.shape
    sub = options.get("subsampling")
    sub = (2 if sub is None else sub) if c == 3 else 0
    if options.get("restart_marker_rows"):
        return R.restart_interval(h, w, c, sub, options["restart_marker_rows"])
    return options.get("restart_marker_blocks", 0)


@functools.lru_cache(maxsize=None)
def corpus():
    """[(name, image, options)]: about 120 cases, none above 140 x 140. Sides from SIDES (not their full square), both channel counts,
    the three samplings, QUALITIES, 0 / 1 / 2 restart rows; then the shapes the issue names."""
    cases = []

    def add(name, img, **options):
        cases.append((f"{name} {img.shape[0]}x{img.shape[1]}x{img.shape[2]} {options}", img, options))

    kinds = ("noise", "ramp", "flat")
    k = 0
    for i, h in enumerate(SIDES):
        for w in (SIDES[i], SIDES[(i + 3) % len(SIDES)]):
            add("grey", image(h, w, 1, k, kinds[k % 3]), quality=QUALITIES[k % 6], restart_marker_rows=k % 3)
            for sub in (0, 1, 2):
                k += 1
                add("rgb", image(h, w, 3, k, kinds[k % 3]), quality=QUALITIES[(k + sub) % 6], subsampling=sub, restart_marker_rows=(k // 3) % 3)
    # dummy luma blocks on the right and at the bottom
    for h, w in ((8, 8), (8, 17), (17, 8), (17, 17), (33, 33), (1, 33), (7, 31)):
        for kind in ("noise", "flat"):
            add(f"dummy blocks 4:2:0 {kind}", image(h, w, 3, h + w, kind), quality=95, subsampling=2)
    add("dummy blocks 4:2:0 restart", image(8, 17, 3, 5, "noise"), quality=75, subsampling=2, restart_marker_rows=1)
    add("PIL's default sampling", image(17, 9, 3, 6, "noise"), quality=75)
    for c in (1, 3):
        add("one pixel", image(1, 1, c, 7, "noise"), quality=75, subsampling=2)
    add("4:2:2", image(17, 9, 3, 8, "noise"), quality=75, subsampling=1)
    add("4:2:2", image(9, 17, 3, 9, "ramp"), quality=50, subsampling=1, restart_marker_rows=1)
    for c in (1, 3):  # dense in FF bytes and long codes
        add("noise at 100", image(33, 31, c, 10 + c, "noise"), quality=100, subsampling=0)
        add("noise at 100", image(33, 31, c, 20 + c, "noise"), quality=100, subsampling=2, restart_marker_rows=1)
    for kind in ("constant", "zeros", "ones"):  # EOB only: a few bytes per MCU row
        for c in (1, 3):
            add(kind, image(33, 33, c, 0, kind), quality=75, subsampling=2, restart_marker_rows=c // 3)
            add(kind, image(16, 16, c, 0, kind), quality=1 if kind == "zeros" else 100, subsampling=0)
    add("13 intervals: RSTn wraps", image(100, 9, 1, 30, "noise"), quality=75, restart_marker_rows=1)
    add("13 intervals: RSTn wraps", image(100, 17, 3, 31, "ramp"), quality=50, subsampling=1, restart_marker_rows=1)
    add("10 intervals: RSTn wraps", image(140, 33, 3, 32, "noise"), quality=24, subsampling=2, restart_marker_rows=1)
    assert len({name for name, _, _ in cases}) == len(cases)
    return cases


@functools.lru_cache(maxsize=None)
def corpus_pil():
    return [pil_bytes(img, **options) for _, img, options in corpus()]


@functools.lru_cache(maxsize=None)
def corpus_restated():
    return [R.encode(img, **options) for _, img, options in corpus()]


def host_encode(img, quality=75, subsampling=None, restart_marker_rows=0, restart_marker_blocks=0):
    """(flag, bytes) from dad3d_jpeg_encode_host; the bytes behind the file must be as they were."""
    lib = _lib.load()
    img = np.ascontiguousarray(img)
    h, w, c = img.shape
    options = {"subsampling": subsampling, "restart_marker_rows": restart_marker_rows, "restart_marker_blocks": restart_marker_blocks}
    sub = (2 if subsampling is None else subsampling) if c == 3 else 0
    cap = lib.dad3d_jpeg_max_bytes(h, w, c, sub)
    assert cap > 0
    out = np.full(cap + 8, 0x23, np.uint8)
    n, flag = C.c_int64(-1), C.c_int32(-1)
    _lib.check(lib.dad3d_jpeg_encode_host(img.ctypes.data, h, w, c, quality, sub, interval_of(img, options), out.ctypes.data, cap, C.byref(n),
                                          C.byref(flag)))
    assert 0 <= n.value <= cap and (out[n.value:] == 0x23).all()
    return flag.value, out[:n.value].tobytes()
