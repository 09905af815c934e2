"""What the PNG tests share, NumPy and the standard library only:

  * the filter rule of csrc/png_encode.hip restated: per row the five PNG filters, the one with the smallest sum of
    (v < 128 ? v : 256 - v) over its bytes, the lowest type on a tie; `filtered_stream` is type byte + filtered row per row;
  * a strict PNG reader (`read_png`): signature, IHDR fields, every chunk's CRC against `zlib.crc32`, chunk order, the IDATs joined
    and `zlib.decompress`ed (which checks the Adler-32) -- PIL alone loads a file with a damaged trailer without complaint;
  * the container of the encoder around any deflate (`container`), for pinning the two above to PIL and zlib;
  * a bitstream restatement of the segment encoder (`deflate_segment`, `zlib_stream`, `png_file`): the greedy parse over distances
    {1, second}, the block type choice and the bit packing in Python integers. The Huffman tables come from
    `dad3d_deflate_tables_host` (the routine the kernel runs, fuzzed on its own in tests/test_png_host.py), so the bytes are the
    bytes the device must produce.
"""
import bisect
import ctypes as C
import io
import os
import struct
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIGNATURE = b"\x89PNG\r\n\x1a\n"
COLOUR_TYPE = {1: 0, 2: 4, 3: 2, 4: 6}
PIL_MODE = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}


def fixture_images():
    """{name: uint8 [H,W,C]} of the committed fixtures the issue names."""
    out = {}
    with np.load(os.path.join(GOLDEN, "sim3dr_golden.npz")) as z:
        for k in ("head_image", "pncc_image", "soup_image", "tri8_image"):
            out[k] = np.ascontiguousarray(z[k])
    with np.load(os.path.join(GOLDEN, "demo_image.npz")) as z:
        out["photo"] = np.ascontiguousarray(z["resized"])
    with np.load(os.path.join(GOLDEN, "uv_texture_golden.npz")) as z:
        out["texture0"] = np.ascontiguousarray(z["textures"][0])
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# filter
# ---------------------------------------------------------------------------------------------------------------------------
def filter_rows(image):
    """uint8 [H,W,C] (or [H,W]) -> (types [H], filtered [H, W*C] uint8)."""
    img = np.asarray(image)
    if img.ndim == 2:
        img = img[:, :, None]
    h, w, c = img.shape
    x = img.reshape(h, w * c).astype(np.int64)
    a = np.zeros_like(x)
    a[:, c:] = x[:, :-c]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    cc = np.zeros_like(x)
    cc[1:, c:] = x[:-1, :-c]
    p = a + b - cc
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - cc)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, cc))
    cand = np.stack([x, x - a, x - b, x - (a + b) // 2, x - paeth]) & 255  # [5,H,WC]
    cost = np.where(cand < 128, cand, 256 - cand).sum(axis=2)  # [5,H]
    types = np.argmin(cost, axis=0)  # the first minimum: the lowest type on a tie
    rows = cand[types, np.arange(h)].astype(np.uint8)
    return types.astype(np.uint8), rows


def filtered_stream(image):
    types, rows = filter_rows(image)
    return np.concatenate([types[:, None], rows], axis=1).tobytes()


def unfilter(stream, h, w, c):
    """The inverse, byte by byte (slow, small images only): the pixels a decoder gets."""
    rb = w * c
    out = np.zeros((h, rb), dtype=np.int64)
    for y in range(h):
        t = stream[y * (rb + 1)]
        row = stream[y * (rb + 1) + 1:(y + 1) * (rb + 1)]
        for i in range(rb):
            a = out[y, i - c] if i >= c else 0
            b = out[y - 1, i] if y else 0
            cc = out[y - 1, i - c] if y and i >= c else 0
            if t == 4:
                p = a + b - cc
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - cc)
                pred = a if pa <= pb and pa <= pc else b if pb <= pc else cc
            else:
                pred = (0, a, b, (a + b) // 2)[t]
            out[y, i] = (row[i] + pred) & 255
    return out.astype(np.uint8).reshape(h, w, c)


# ---------------------------------------------------------------------------------------------------------------------------
# container and strict reader
# ---------------------------------------------------------------------------------------------------------------------------
def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def container(h, w, c, idat_payloads):
    """The encoder's file around the given IDAT payloads."""
    ihdr = struct.pack(">IIBBBBB", w, h, 8, COLOUR_TYPE[c], 0, 0, 0)
    return SIGNATURE + chunk(b"IHDR", ihdr) + b"".join(chunk(b"IDAT", p) for p in idat_payloads) + chunk(b"IEND", b"")


def reference_png(image):
    """filtered stream -> zlib.compress -> the container: a valid file from the standard library alone."""
    img = np.asarray(image)
    h, w, c = img.shape
    return container(h, w, c, [zlib.compress(filtered_stream(img), 6)])


class PngError(AssertionError):
    pass


def read_png(data):
    """Strict: returns {"width", "height", "channels", "idat": [payloads], "stream": the inflated filtered stream}."""
    data = bytes(data)
    if data[:8] != SIGNATURE:
        raise PngError("signature")
    at, chunks = 8, []
    while at < len(data):
        if at + 12 > len(data):
            raise PngError(f"a chunk header past the end at {at}")
        (n,) = struct.unpack(">I", data[at:at + 4])
        kind, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        if at + 12 + n > len(data):
            raise PngError(f"chunk {kind!r} at {at} runs past the end")
        (crc,) = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        if crc != zlib.crc32(kind + body):
            raise PngError(f"CRC of chunk {kind!r} at {at}: {crc:08x}, expected {zlib.crc32(kind + body):08x}")
        chunks.append((kind, body))
        at += 12 + n
    kinds = [k for k, _ in chunks]
    if kinds[0] != b"IHDR" or kinds[-1] != b"IEND" or chunks[-1][1] != b"" or set(kinds[1:-1]) != {b"IDAT"}:
        raise PngError(f"chunk order {kinds[:3]} .. {kinds[-2:]}")
    if len(chunks[0][1]) != 13:
        raise PngError("IHDR length")
    w, h, depth, ctype, comp, flt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    if depth != 8 or ctype not in COLOUR_TYPE.values() or (comp, flt, lace) != (0, 0, 0) or w < 1 or h < 1:
        raise PngError(f"IHDR fields {(w, h, depth, ctype, comp, flt, lace)}")
    c = {v: k for k, v in COLOUR_TYPE.items()}[ctype]
    idat = [body for _, body in chunks[1:-1]]
    inflater = zlib.decompressobj()
    try:
        stream = inflater.decompress(b"".join(idat)) + inflater.flush()
    except zlib.error as e:
        raise PngError(f"inflate: {e}")
    if not inflater.eof or inflater.unused_data:
        raise PngError("the zlib stream does not end with the last IDAT")
    if len(stream) != h * (1 + w * c):
        raise PngError(f"{len(stream)} bytes of filtered stream for {h} x {w} x {c}")
    return {"width": w, "height": h, "channels": c, "idat": idat, "stream": stream}


def pil_pixels(data):
    """(mode, uint8 [H,W,C]) as PIL decodes the file."""
    from PIL import Image

    im = Image.open(io.BytesIO(bytes(data)))
    im.load()
    arr = np.asarray(im)
    return im.mode, arr[:, :, None] if arr.ndim == 2 else arr


# ---------------------------------------------------------------------------------------------------------------------------
# the segment encoder, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
def tables(ll_hist, d_hist):
    """dad3d_deflate_tables_host -> dict of numpy arrays / ints."""
    from dad_3dheads_amd import _lib

    lib = _lib.load()
    ll = np.ascontiguousarray(ll_hist, dtype=np.uint32)
    dd = np.ascontiguousarray(d_hist, dtype=np.uint32)
    assert ll.shape == (286,) and dd.shape == (30,)
    out = {"ll_len": np.zeros(286, np.uint8), "d_len": np.zeros(30, np.uint8), "cl_len": np.zeros(19, np.uint8),
           "ll_code": np.zeros(286, np.uint16), "d_code": np.zeros(30, np.uint16), "cl_code": np.zeros(19, np.uint16),
           "header": np.zeros(_lib.DEFLATE_HEADER_BYTES, np.uint8)}
    hb, dyn, fix = C.c_int32(0), C.c_uint32(0), C.c_uint32(0)
    _lib.check(lib.dad3d_deflate_tables_host(ll.ctypes.data, dd.ctypes.data, *(out[k].ctypes.data for k in
                                             ("ll_len", "d_len", "cl_len", "ll_code", "d_code", "cl_code", "header")),
                                             C.addressof(hb), C.addressof(dyn), C.addressof(fix)))
    out.update(header_bits=hb.value, dynamic_bits=dyn.value, fixed_bits=fix.value)
    return out


LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0,) * 8 + (1,) * 4 + (2,) * 4 + (3,) * 4 + (4,) * 4 + (5,) * 4 + (0,)


def length_symbol(n):
    """match length 3..258 -> (symbol, extra bits, extra value): the table of RFC 1951 3.2.5."""
    i = bisect.bisect_right(LENGTH_BASE, n) - 1
    return 257 + i, LENGTH_EXTRA[i], n - LENGTH_BASE[i]


def reverse_bits(code, n):
    return int(format(code, f"0{n}b")[::-1], 2) if n else 0


def fixed_code(sym):
    if sym < 144:
        return 0x30 + sym, 8
    if sym < 256:
        return 0x190 + sym - 144, 9
    if sym < 280:
        return sym - 256, 7
    return 0xC0 + sym - 280, 8


def greedy_parse(x, lo, hi, second):
    """Tokens of x[lo:hi): (literal byte,) or (length, distance). Matches at distances 1 and `second`, may reach in front of lo,
    end at hi, 3..258 long; the longer wins, distance 1 on a tie."""
    xa = np.frombuffer(x, dtype=np.uint8)
    n = hi - lo
    runs = []
    for d in (1, second):
        eq = np.zeros(n + 1, dtype=bool)
        first = max(lo, d)
        if first < hi:
            eq[first - lo:n] = xa[first:hi] == xa[first - d:hi - d]
        # run[i] = ones from i on: distance to the next False
        idx = np.where(eq, n + 1, np.arange(n + 1))
        nxt = np.minimum.accumulate(idx[::-1])[::-1]
        runs.append(np.minimum(nxt - np.arange(n + 1), 258)[:n])
    l1, l2 = runs
    best = np.where(l1 >= l2, l1, l2).tolist()
    dist = np.where(l1 >= l2, 1, second).tolist()
    tokens, i = [], 0
    while i < n:
        if best[i] >= 3:
            tokens.append((best[i], dist[i]))
            i += best[i]
        else:
            tokens.append((x[lo + i],))
            i += 1
    return tokens


def deflate_segment(x, lo, hi, second):
    """The payload of the segment x[lo:hi): one block (stored / fixed / dynamic, the fewest bits, the simpler on a tie) and the empty
    stored block. Returns (bytes, kind)."""
    n = hi - lo
    tokens = greedy_parse(x, lo, hi, second)
    ll_hist, d_hist = np.zeros(286, np.uint32), np.zeros(30, np.uint32)
    ll_hist[256] = 1
    for t in tokens:
        if len(t) == 1:
            ll_hist[t[0]] += 1
        else:
            ll_hist[length_symbol(t[0])[0]] += 1
            d_hist[t[1] - 1] += 1
    tab = tables(ll_hist, d_hist)
    kind, bits = 0, 8 * (5 + n)
    if tab["fixed_bits"] < bits:
        kind, bits = 1, tab["fixed_bits"]
    if tab["dynamic_bits"] < bits:
        kind, bits = 2, tab["dynamic_bits"]
    if kind == 0:
        body = b"\x00" + struct.pack("<HH", n, n ^ 0xFFFF) + bytes(x[lo:hi])
        return body + b"\x00\x00\x00\xff\xff", 0
    if kind == 1:
        acc, pos = 2, 3
        ll = [fixed_code(s) for s in range(286)]
        dd = [(d, 5) for d in range(30)]
    else:
        acc, pos = int.from_bytes(tab["header"].tobytes(), "little"), tab["header_bits"]
        ll = list(zip(tab["ll_code"].tolist(), tab["ll_len"].tolist()))
        dd = list(zip(tab["d_code"].tolist(), tab["d_len"].tolist()))
    ll = [(reverse_bits(c, k), k) for c, k in ll]
    dd = [(reverse_bits(c, k), k) for c, k in dd]
    parts = []
    for t in tokens:
        if len(t) == 1:
            parts.append(ll[t[0]])
        else:
            sym, eb, extra = length_symbol(t[0])
            parts.append(ll[sym])
            if eb:
                parts.append((extra, eb))
            parts.append(dd[t[1] - 1])
    parts.append(ll[256])
    for v, k in parts:
        acc |= v << pos
        pos += k
    assert pos == bits, (pos, bits, kind)
    nbytes = (pos + 3 + 7) // 8
    return acc.to_bytes(nbytes, "little") + b"\x00\x00\xff\xff", kind


def segment_payloads(stream, second, segment_bytes):
    n = len(stream)
    return [deflate_segment(stream, lo, min(lo + segment_bytes, n), second) for lo in range(0, max(n, 1), segment_bytes)]


def trailer(stream):
    return b"\x03\x00" + struct.pack(">I", zlib.adler32(stream))


def zlib_stream(data, second, segment_bytes):
    """The bytes dad3d_zlib_compress must produce for `data`."""
    data = bytes(data)
    return b"\x78\x01" + b"".join(p for p, _ in segment_payloads(data, second, segment_bytes)) + trailer(data)


def png_file(image, segment_bytes):
    """The bytes dad3d_png_encode must produce for `image` -> (file, kinds of its segments)."""
    img = np.asarray(image)
    h, w, c = img.shape
    stream = filtered_stream(img)
    segs = segment_payloads(stream, c, segment_bytes)
    return container(h, w, c, [b"\x78\x01"] + [p for p, _ in segs] + [trailer(stream)]), [k for _, k in segs]
