"""The baseline JPEG encoder of csrc/jpeg_encode.hip restated in numpy and integers, header included: the file
`Image.fromarray(img).save(buf, "JPEG", quality=q, subsampling=s, restart_marker_rows=r)` writes, byte for byte. PIL (libjpeg-turbo)
is the authority: where libjpeg's code and the plain wording of a rule part (the DC of a dummy block in a bottom row, `coefficients`),
this file follows the bytes PIL writes."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62,
                   63])
# Annex K.1, in natural order
STD_QUANT = (
    np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
              18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
              103, 99]),
    np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
             + [99] * 32),
)
# Annex K.3: (the number of codes of each length 1 .. 16, the symbols in code order) for DC 0, AC 0, DC 1, AC 1
_AC0 = [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
        0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
        0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
        0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
        0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
        0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
        0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
        0xfa]
_AC1 = [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
        0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
        0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
        0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
        0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
        0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
        0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
        0xfa]
STD_HUFF = {
    (0, 0): ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    (1, 0): ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], _AC0),
    (0, 1): ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    (1, 1): ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], _AC1),
}


def quality_scale(quality):
    return 5000 // quality if quality < 50 else 200 - 2 * quality


def quant_table(which, quality):
    """jpeg_set_quality(quality, force_baseline): natural order, 1 .. 255."""
    return np.clip((STD_QUANT[which] * quality_scale(quality) + 50) // 100, 1, 255)


def huff_codes(cls, which):
    """{symbol: (code, length)} of a standard table: canonical codes in the order of the symbols."""
    bits, vals = STD_HUFF[(cls, which)]
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return out


class Geometry:
    def __init__(self, h, w, c, subsampling):
        self.h, self.w, self.comps = h, w, c
        self.hs, self.vs = ((1, 1), (2, 1), (2, 2))[subsampling] if c == 3 else (1, 1)
        if c == 1:  # a scan of one component is not interleaved: an MCU is one block, and nothing is padded to the sampling factors
            self.mcus_x, self.mcus_y = (w + 7) // 8, (h + 7) // 8
        else:
            self.mcus_x, self.mcus_y = (w + 8 * self.hs - 1) // (8 * self.hs), (h + 8 * self.vs - 1) // (8 * self.vs)
        self.blocks_per_mcu = 1 if c == 1 else self.hs * self.vs + 2


def restart_interval(h, w, c, subsampling, restart_marker_rows):
    g = Geometry(h, w, c, subsampling)
    interval = restart_marker_rows * g.mcus_x
    if not 0 <= interval <= 65535:
        raise ValueError(f"restart_marker_rows {restart_marker_rows} x {g.mcus_x} MCUs per row passes 65535")
    return interval


def header(h, w, c, quality, subsampling, interval):
    """SOI .. SOS in libjpeg's order."""
    g = Geometry(h, w, c, subsampling)
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    tables = 1 if c == 1 else 2
    for t in range(tables):
        out += b"\xff\xdb\x00\x43" + bytes([t]) + bytes(quant_table(t, quality)[ZIGZAG].tolist())
    out += b"\xff\xc0" + (8 + 3 * c).to_bytes(2, "big") + b"\x08" + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([c])
    for i in range(c):
        out += bytes([i + 1, (g.hs << 4 | g.vs) if i == 0 else 0x11, 0 if i == 0 else 1])
    for t in range(tables):
        for cls in (0, 1):
            bits, vals = STD_HUFF[(cls, t)]
            out += b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([cls << 4 | t]) + bytes(bits) + bytes(vals)
    if interval:
        out += b"\xff\xdd\x00\x04" + interval.to_bytes(2, "big")
    out += b"\xff\xda" + (6 + 2 * c).to_bytes(2, "big") + bytes([c])
    for i in range(c):
        out += bytes([i + 1, 0 if i == 0 else 0x11])
    return bytes(out + b"\x00\x3f\x00")


def ycbcr(rgb):
    """jccolor.c: 16-bit fixed point, three planes of int64."""
    r, g, b = (rgb[:, :, i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def component_plane(plane, hs, vs, blocks_x, blocks_y):
    """One component's samples padded to whole blocks: the columns of the input replicated to hs x 8 x blocks_x and the rows to a
    multiple of vs (jcprepct.c), the box filter with its alternating bias (jcsample.c), then the last row of the result replicated."""
    h, w = plane.shape
    rows = np.minimum(np.arange((h + vs - 1) // vs * vs), h - 1)
    cols = np.minimum(np.arange(blocks_x * 8 * hs), w - 1)
    p = plane[np.ix_(rows, cols)]
    if hs == 2 and vs == 2:
        bias = np.tile([1, 2], blocks_x * 4)
        p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
    elif hs == 2:
        bias = np.tile([0, 1], blocks_x * 4)
        p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
    return p[np.minimum(np.arange(blocks_y * 8), p.shape[0] - 1)]


def fdct(block):
    """jfdctint.c on a level-shifted 8 x 8 block: CONST_BITS 13, PASS1_BITS 2; the result is 8 times the DCT."""
    def descale(x, n):
        return (x + (1 << (n - 1))) >> n

    def one_pass(d, first):
        t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
        t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        o = [None] * 8
        if first:
            o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
        else:
            o[0], o[4] = descale(t10 + t11, 2), descale(t10 - t11, 2)
        n = 11 if first else 15
        z1 = (t12 + t13) * 4433
        o[2], o[6] = descale(z1 + t13 * 6270, n), descale(z1 - t12 * 15137, n)
        z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
        z5 = (z3 + z4) * 9633
        t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
        z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
        o[7], o[5], o[3], o[1] = descale(t4 + z1 + z3, n), descale(t5 + z2 + z4, n), descale(t6 + z2 + z3, n), descale(t7 + z1 + z4, n)
        return o

    rows = np.stack(one_pass([block[:, i] for i in range(8)], True), axis=1)  # along each row
    return np.stack(one_pass([rows[i, :] for i in range(8)], False), axis=0)  # along each column


def quantise(coef, table):
    """The division by 8 Q rounded half away from zero."""
    div = 8 * table.reshape(8, 8)
    mag = (np.abs(coef) + (div >> 1)) // div
    return np.where(coef < 0, -mag, mag)


class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, length):
        self.acc, self.n = self.acc << length | code, self.n + length
        while self.n >= 8:
            byte = self.acc >> (self.n - 8) & 255
            self.out.append(byte)
            if byte == 255:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def encode_block(bw, zz, pred, dc_codes, ac_codes):
    def value(v):
        n = int(abs(v)).bit_length()
        return n, (v if v >= 0 else v - 1) & ((1 << n) - 1)

    n, bits = value(int(zz[0]) - pred)
    bw.put(*dc_codes[n])
    if n:
        bw.put(bits, n)
    run = 0
    for k in range(1, 64):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            bw.put(*ac_codes[0xf0])
            run -= 16
        n, bits = value(v)
        bw.put(*ac_codes[run << 4 | n])
        bw.put(bits, n)
        run = 0
    if run:
        bw.put(*ac_codes[0])


def coefficients(img, quality, subsampling):
    """[(component, quantised block in zigzag order)] in the order of the scan, dummy blocks included."""
    h, w, c = img.shape
    g = Geometry(h, w, c, subsampling)
    if c == 1:
        planes = [component_plane(img[:, :, 0].astype(np.int64), 1, 1, g.mcus_x, g.mcus_y)]
    else:
        y, cb, cr = ycbcr(img)
        real_x, real_y = (w + 7) // 8, (h + 7) // 8
        planes = [component_plane(y, 1, 1, real_x, real_y)] + [component_plane(p, g.hs, g.vs, g.mcus_x, g.mcus_y) for p in (cb, cr)]
    tables = [quant_table(0, quality), quant_table(1, quality), quant_table(1, quality)]

    def block(comp, by, bx):
        p = planes[comp]
        return quantise(fdct(p[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] - 128), tables[comp]).reshape(64)[ZIGZAG]

    out = []
    for my in range(g.mcus_y):
        for mx in range(g.mcus_x):
            if c == 1:
                out.append((0, block(0, my, mx)))
                continue
            for v in range(g.vs):
                for u in range(g.hs):
                    by, bx = my * g.vs + v, mx * g.hs + u
                    real_x, real_y = planes[0].shape[1] // 8, planes[0].shape[0] // 8
                    # A dummy block has no AC. On the right it takes the DC of the block in front of it; in a dummy row at the
                    # bottom every block takes the DC of the LAST block of the MCU's row above (jccoefct.c reads MCU_buffer[blkn - 1]),
                    # not of the block above it: the one place where PIL's bytes and the issue's wording part.
                    src_x = bx if by < real_y else mx * g.hs + g.hs - 1
                    zz = block(0, min(by, real_y - 1), min(src_x, real_x - 1))
                    if by >= real_y or bx >= real_x:
                        zz = np.concatenate([zz[:1], np.zeros(63, zz.dtype)])
                    out.append((0, zz))
            out.append((1, block(1, my, mx)))
            out.append((2, block(2, my, mx)))
    return out


def encode(img, quality=75, subsampling=None, restart_marker_rows=0, restart_marker_blocks=0):
    """uint8 [H,W] or [H,W,1] (mode L) or [H,W,3] (RGB) -> the bytes of the file. `restart_marker_blocks` is PIL's name for an
    interval given in MCUs, which the C entry point takes; rows, where given, win, as in libjpeg."""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[:, :, None]
    h, w, c = img.shape
    assert img.dtype == np.uint8 and c in (1, 3) and 1 <= quality <= 100
    subsampling = (2 if subsampling is None else subsampling) if c == 3 else 0
    g = Geometry(h, w, c, subsampling)
    interval = restart_interval(h, w, c, subsampling, restart_marker_rows) if restart_marker_rows else restart_marker_blocks
    dc = [huff_codes(0, 0), huff_codes(0, 1), huff_codes(0, 1)]
    ac = [huff_codes(1, 0), huff_codes(1, 1), huff_codes(1, 1)]
    bw, pred, restarts = BitWriter(), [0, 0, 0], 0
    for i, (comp, zz) in enumerate(coefficients(img, quality, subsampling)):
        mcu, first = divmod(i, g.blocks_per_mcu)
        if interval and first == 0 and mcu and mcu % interval == 0:
            bw.flush()
            bw.out += bytes([0xff, 0xd0 + restarts % 8])
            pred, restarts = [0, 0, 0], restarts + 1
        encode_block(bw, zz, pred[comp], dc[comp], ac[comp])
        pred[comp] = int(zz[0])
    bw.flush()
    return header(h, w, c, quality, subsampling, interval) + bytes(bw.out) + b"\xff\xd9"
