"""The decode rules of DESIGN.md 4.19 for baseline JPEG in plain Python / numpy, flags included: a second statement of what
csrc/jpeg_entropy.hpp and csrc/jpeg_idct.hpp compute, written from the rules and not from that code, and held to PIL beside it
(tests/test_jpeg_host.py). `decode(data, channels)` -> (flag, uint8 [H,W,C] or None)."""
import numpy as np

MALFORMED, UNSUPPORTED = 0x1, 0x2

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


class Flag(Exception):
    def __init__(self, flag, why):
        super().__init__(why)
        self.flag = flag


def _huffman(counts, symbols, dc):
    """{code as a string of bits: symbol}; libjpeg's validity: no code reaches the all-ones code of its length."""
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            codes[format(code, "0%db" % length)] = symbols[k]
            code, k = code + 1, k + 1
        if counts[length - 1] and code >= 1 << length:
            raise Flag(MALFORMED, "a code overflows its length")
        code <<= 1
    if dc and any(s > 15 for s in symbols):
        raise Flag(MALFORMED, "a DC symbol above 15")
    return codes, sorted({len(c) for c in codes})


def parse(data):
    """The marker walk up to the entropy data."""
    if len(data) < 4 or data[:2] != b"\xff\xd8":
        raise Flag(MALFORMED, "no SOI")
    hd = {"quant": {}, "huff": {}, "interval": 0, "jfif": False, "adobe": False, "sof": None}
    pos = 2
    while True:
        if pos + 4 > len(data) or data[pos] != 0xFF:
            raise Flag(MALFORMED, "no marker where one must be")
        m, seg = data[pos + 1], data[pos + 2] << 8 | data[pos + 3]
        if seg < 2 or pos + 2 + seg > len(data):
            raise Flag(MALFORMED, "a segment's length")
        d = data[pos + 4:pos + 2 + seg]
        if 0xE0 <= m <= 0xEF or m == 0xFE:
            if m == 0xE0 and len(d) >= 14 and d[:5] == b"JFIF\0":
                hd["jfif"] = True
            if m == 0xEE and d[:5] == b"Adobe":
                hd["adobe"] = True
        elif m == 0xDB:
            while d:
                if len(d) < 65:
                    raise Flag(MALFORMED, "DQT length")
                if d[0] >> 4 == 1:
                    raise Flag(UNSUPPORTED, "16-bit table")
                if d[0] >> 4 or d[0] & 15 > 3:
                    raise Flag(MALFORMED, "DQT")
                table = np.zeros(64, np.int64)
                table[ZIGZAG] = np.frombuffer(d[1:65], np.uint8)
                hd["quant"][d[0] & 15] = table
                d = d[65:]
        elif m == 0xC4:
            while d:
                if len(d) < 17:
                    raise Flag(MALFORMED, "DHT length")
                tc, th, counts = d[0] >> 4, d[0] & 15, list(d[1:17])
                if tc > 1 or th > 3 or sum(counts) > 256 or len(d) < 17 + sum(counts):
                    raise Flag(MALFORMED, "DHT")
                hd["huff"][(tc, th)] = _huffman(counts, list(d[17:17 + sum(counts)]), tc == 0)
                d = d[17 + sum(counts):]
        elif m == 0xC0:
            if hd["sof"] is not None or len(d) < 6:
                raise Flag(MALFORMED, "SOF")
            precision, h, w, nc = d[0], d[1] << 8 | d[2], d[3] << 8 | d[4], d[5]
            if precision == 12 or nc in (2, 4) or (h == 0 and w > 0):
                raise Flag(UNSUPPORTED, "precision, components or DNL")
            if precision != 8 or nc not in (1, 3) or len(d) != 6 + 3 * nc or w == 0:
                raise Flag(MALFORMED, "SOF0")
            comps = []
            for c in range(nc):
                cid, hv, tq = d[6 + 3 * c:9 + 3 * c]
                if not (1 <= hv >> 4 <= 4 and 1 <= hv & 15 <= 4) or tq > 3:
                    raise Flag(MALFORMED, "component")
                allowed = (0x11, 0x21, 0x22) if nc == 3 and c == 0 else (0x11,)
                if hv not in allowed:
                    raise Flag(UNSUPPORTED, "sampling factors")
                comps.append({"id": cid, "h": hv >> 4, "v": hv & 15, "tq": tq})
            if len({c["id"] for c in comps}) != nc:
                raise Flag(MALFORMED, "component ids")
            hd["sof"] = (h, w, comps)
        elif m == 0xDD:
            if len(d) != 2:
                raise Flag(MALFORMED, "DRI")
            hd["interval"] = d[0] << 8 | d[1]
        elif m == 0xDA:
            if hd["sof"] is None:
                raise Flag(MALFORMED, "SOS without SOF")
            comps = hd["sof"][2]
            if len(d) != 4 + 2 * len(comps) or d[0] != len(comps):
                raise Flag(UNSUPPORTED if len(d) >= 1 and 1 <= d[0] < len(comps) else MALFORMED, "SOS")
            for c, comp in enumerate(comps):
                td, ta = d[2 + 2 * c] >> 4, d[2 + 2 * c] & 15
                if d[1 + 2 * c] != comp["id"] or (0, td) not in hd["huff"] or (1, ta) not in hd["huff"] or comp["tq"] not in hd["quant"]:
                    raise Flag(MALFORMED, "a missing table")
                comp["dc"], comp["ac"] = hd["huff"][(0, td)], hd["huff"][(1, ta)]
            if tuple(d[-3:]) != (0, 63, 0):
                raise Flag(UNSUPPORTED, "spectral selection")
            ids = [c["id"] for c in comps]
            if len(comps) == 3 and (hd["adobe"] or (not hd["jfif"] and ids != [1, 2, 3])):
                raise Flag(UNSUPPORTED, "colour space")
            hd["scan_at"] = pos + 2 + seg
            return hd
        elif m in (0xC1, 0xC2, 0xC3, 0xDC) or 0xC5 <= m <= 0xCF:
            raise Flag(UNSUPPORTED, "another process")
        else:
            raise Flag(MALFORMED, "an unknown marker")
        pos += 2 + seg


def segments(data, hd, mcus):
    """[(start, end)] of the entropy segments; the data ends at EOI."""
    n = hd["interval"]
    expected = -(-mcus // n) if n else 1
    out, start, p = [], hd["scan_at"], hd["scan_at"]
    while p + 1 < len(data):
        if data[p] != 0xFF or data[p + 1] == 0:
            p += 1
            continue
        b = data[p + 1]
        if 0xD0 <= b <= 0xD7:
            if b - 0xD0 != len(out) % 8 or len(out) + 1 >= expected:
                raise Flag(MALFORMED, "a restart marker out of sequence")
            out.append((start, p))
            start = p = p + 2
            continue
        if b != 0xD9:
            raise Flag(UNSUPPORTED, "fill bytes or another marker inside the scan")
        out.append((start, p))
        if len(out) != expected:
            raise Flag(MALFORMED, "the number of restart markers")
        return out
    raise Flag(MALFORMED, "no EOI")


class Bits:
    def __init__(self, raw):
        raw = raw.replace(b"\xff\x00", b"\xff")
        self.bits = format(int.from_bytes(raw, "big"), "0%db" % (8 * len(raw))) if raw else ""
        self.at = 0

    def take(self, n):
        if self.at + n > len(self.bits):
            raise Flag(MALFORMED, "a bit beyond the segment's last byte")
        v = int(self.bits[self.at:self.at + n], 2)
        self.at += n
        return v

    def symbol(self, table):
        codes, lengths = table
        for n in lengths:
            s = codes.get(self.bits[self.at:self.at + n])
            if s is not None:
                if self.at + n > len(self.bits):
                    break
                self.at += n
                return s
        if self.at + 16 > len(self.bits):
            raise Flag(MALFORMED, "a bit beyond the segment's last byte")
        raise Flag(MALFORMED, "a code no table assigns")


def _extend(v, s):
    return v - (1 << s) + 1 if v < 1 << (s - 1) else v


def _block(bits, comp, pred):
    out = np.zeros(64, np.int64)
    s = bits.symbol(comp["dc"])
    if s > 11:
        raise Flag(MALFORMED, "DC size")
    pred += _extend(bits.take(s), s) if s else 0
    if not -32768 <= pred <= 32767:
        raise Flag(MALFORMED, "DC beyond 16 bits")
    out[0] = pred
    k = 1
    while k < 64:
        rs = bits.symbol(comp["ac"])
        r, s = rs >> 4, rs & 15
        if s == 0:
            if r != 15:
                break
            k += 16
            continue
        k += r
        if s > 10 or k > 63:
            raise Flag(MALFORMED, "AC size or index")
        out[ZIGZAG[k]] = _extend(bits.take(s), s)
        k += 1
    return out, pred


def _pass(x):
    """The 1-D transform along the last axis, before the descale."""
    i0, i1, i2, i3, i4, i5, i6, i7 = (x[..., k] for k in range(8))
    z1 = (i2 + i6) * 4433
    t2, t3 = z1 - i6 * 15137, z1 + i2 * 6270
    t0, t1 = (i0 + i4) << 13, (i0 - i4) << 13
    a10, a13, a11, a12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = i7, i5, i3, i1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    return np.stack([a10 + t3, a11 + t2, a12 + t1, a13 + t0, a13 - t0, a12 - t1, a11 - t2, a10 - t3], axis=-1)


def idct(coefs, quant):
    """[n, 64] quantised coefficients -> [n, 8, 8] samples."""
    x = (coefs * quant[None]).reshape(-1, 8, 8)
    if x.size and (x.min() < -32768 or x.max() > 32767):
        raise Flag(UNSUPPORTED, "a dequantised coefficient beyond 16 bits")
    x = (_pass(x.transpose(0, 2, 1)) + 1024) >> 11  # the columns
    if x.size and (x.min() < -32768 or x.max() > 32767):
        raise Flag(UNSUPPORTED, "a first-pass result beyond 16 bits")
    x = (_pass(x.transpose(0, 2, 1)) + 131072) >> 18  # the rows
    if x.size and (x.min() < -512 or x.max() > 511):
        raise Flag(UNSUPPORTED, "a second-pass result outside the range table")
    return np.clip(x + 128, 0, 255)


def _h2v1(p):
    dw = p.shape[1]
    if dw <= 2:
        return np.repeat(p, 2, axis=1)
    out = np.empty((p.shape[0], 2 * dw), np.int64)
    out[:, 0], out[:, -1] = p[:, 0], p[:, -1]
    out[:, 1:-1:2] = (3 * p[:, :-1] + p[:, 1:] + 2) >> 2
    out[:, 2::2] = (3 * p[:, 1:] + p[:, :-1] + 1) >> 2
    return out


def _h2v2(p):
    dh, dw = p.shape
    if dw <= 2:
        return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
    above, below = np.vstack([p[:1], p[:-1]]), np.vstack([p[1:], p[-1:]])
    t = np.empty((2 * dh, dw), np.int64)
    t[0::2], t[1::2] = 3 * p + above, 3 * p + below
    out = np.empty((2 * dh, 2 * dw), np.int64)
    out[:, 0], out[:, -1] = (4 * t[:, 0] + 8) >> 4, (4 * t[:, -1] + 7) >> 4
    out[:, 2::2] = (3 * t[:, 1:] + t[:, :-1] + 8) >> 4
    out[:, 1:-1:2] = (3 * t[:, :-1] + t[:, 1:] + 7) >> 4
    return out


def decode_checked(data, channels=None):
    hd = parse(data)
    h, w, comps = hd["sof"]
    hmax, vmax = comps[0]["h"], comps[0]["v"]
    mx, my = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    segs = segments(data, hd, mx * my)
    n = hd["interval"] or mx * my
    blocks = [np.zeros((my * c["v"], mx * c["h"], 64), np.int64) for c in comps]
    for k, (start, end) in enumerate(segs):
        bits, preds = Bits(data[start:end]), [0] * len(comps)
        for m in range(k * n, min((k + 1) * n, mx * my)):
            row, col = divmod(m, mx)
            for c, comp in enumerate(comps):
                for v in range(comp["v"]):
                    for hh in range(comp["h"]):
                        blocks[c][row * comp["v"] + v, col * comp["h"] + hh], preds[c] = _block(bits, comp, preds[c])
        if len(bits.bits) - bits.at >= 8:
            raise Flag(MALFORMED, "a whole unread byte")
    planes = []
    for c, comp in enumerate(comps):
        bh, bw = blocks[c].shape[:2]
        px = idct(blocks[c].reshape(-1, 64), hd["quant"][comp["tq"]]).reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)
        dh, dw = -(-h * comp["v"] // vmax), -(-w * comp["h"] // hmax)
        px = px[:dh, :dw]
        if comp["h"] < hmax:
            px = _h2v2(px) if comp["v"] < vmax else _h2v1(px)
        planes.append(px[:h, :w])
    if len(comps) == 1:
        img = planes[0][:, :, None]
        if channels == 3:
            img = np.repeat(img, 3, axis=2)
    else:
        y, cb, cr = planes[0], planes[1] - 128, planes[2] - 128
        f = lambda x: int(np.floor(x * 65536 + 0.5))  # noqa: E731
        r = np.clip(y + ((f(1.402) * cr + 32768) >> 16), 0, 255)
        b = np.clip(y + ((f(1.772) * cb + 32768) >> 16), 0, 255)
        g = np.clip(y + ((-f(0.34414) * cb + 32768 - f(0.71414) * cr) >> 16), 0, 255)
        img = np.stack([r, g, b], axis=2)
        if channels == 1:
            img = ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16)[:, :, None]
    return img.astype(np.uint8)


def decode(data, channels=None):
    try:
        return 0, decode_checked(bytes(data), channels)
    except Flag as e:
        return e.flag, None
