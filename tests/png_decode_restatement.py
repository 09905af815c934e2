"""What the PNG / zlib decode tests share, the standard library and NumPy only:

  * `inflate`: RFC 1950 / 1951 in plain Python, bit by bit, with zlib's acceptance rules; `InflateError` for what zlib refuses;
  * `read_chunks`: the chunks of a PNG file with their CRCs checked;
  * `BitWriter` and the deflate *writer*: blocks with chosen code lengths, chosen (length, distance) tokens, stored blocks -- the
    streams zlib itself does not produce;
  * `write_png`: a PNG with forced per-row filter types, an IDAT split rule, extra chunks and any deflate;
  * the lists of valid and malformed zlib streams the host and the GPU tests both run;
  * `host_inflate`: dad3d_inflate_host over a list of ranges, with guard bytes around the output.
"""
import ctypes as C
import struct
import zlib

import numpy as np

import png_restatement as R

LENGTH_BASE = R.LENGTH_BASE
LENGTH_EXTRA = R.LENGTH_EXTRA
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 30
GUARD = 0x5A


class InflateError(Exception):
    pass


# ---------------------------------------------------------------------------------------------------------------------------
# inflate, plain
# ---------------------------------------------------------------------------------------------------------------------------
class _Bits:
    def __init__(self, data):
        self.data, self.at, self.buf, self.cnt = bytes(data), 0, 0, 0

    def take(self, n):
        while self.cnt < n:
            if self.at >= len(self.data):
                raise InflateError("truncated")
            self.buf |= self.data[self.at] << self.cnt
            self.at += 1
            self.cnt += 8
        v = self.buf & ((1 << n) - 1)
        self.buf >>= n
        self.cnt -= n
        return v

    def align(self):
        self.take(self.cnt & 7)


def _canonical(lengths, may_be_single):
    """{(length, code): symbol}; raises for an oversubscribed or (unless allowed) incomplete set."""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    if count[0] == len(lengths):
        return {}
    left = 1
    for n in range(1, 16):
        left = (left << 1) - count[n]
        if left < 0:
            raise InflateError("oversubscribed")
    if left > 0 and not (may_be_single and count[1] == 1 and sum(count[1:]) == 1):
        raise InflateError("incomplete")
    count[0] = 0
    code, nxt = 0, [0] * 16
    for n in range(1, 16):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    table = {}
    for sym, n in enumerate(lengths):
        if n:
            table[(n, nxt[n])] = sym
            nxt[n] += 1
    return table


def _symbol(bits, table):
    code = 0
    for n in range(1, 16):
        code = code << 1 | bits.take(1)
        if (n, code) in table:
            return table[(n, code)]
    raise InflateError("invalid code")


def inflate(data, trace=None):
    """zlib.decompress in plain Python (bytes behind the Adler-32 are ignored, as zlib.decompress ignores them). `trace`: a dict that
    receives the block types seen, the largest distance, the longest match and the longest code length."""
    trace = {} if trace is None else trace
    trace.update(kinds=set(), distance=0, length=0, code_bits=0)
    bits = _Bits(data)
    cmf, flg = bits.take(8), bits.take(8)
    if cmf & 15 != 8 or cmf >> 4 > 7 or (cmf << 8 | flg) % 31 or flg & 0x20:
        raise InflateError("header")
    out = bytearray()
    while True:
        last, kind = bits.take(1), bits.take(2)
        trace["kinds"].add(kind)
        if kind == 0:
            bits.align()
            n, nn = bits.take(16), bits.take(16)
            if n != nn ^ 0xFFFF:
                raise InflateError("LEN / NLEN")
            for _ in range(n):
                out.append(bits.take(8))
        elif kind == 3:
            raise InflateError("block type 3")
        else:
            if kind == 1:
                ll, dd = _canonical(FIXED_LL, False), _canonical(FIXED_D + [5, 5], False)
            else:
                nlen, ndist, ncode = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
                if nlen > 286 or ndist > 30:
                    raise InflateError("too many symbols")
                cl = [0] * 19
                for i in range(ncode):
                    cl[CL_ORDER[i]] = bits.take(3)
                if not any(cl):
                    raise InflateError("no code length code")
                clt = _canonical(cl, False)
                lengths = []
                while len(lengths) < nlen + ndist:
                    s = _symbol(bits, clt)
                    if s < 16:
                        lengths.append(s)
                        continue
                    if s == 16:
                        if not lengths:
                            raise InflateError("repeat with nothing in front")
                        val, rep = lengths[-1], 3 + bits.take(2)
                    elif s == 17:
                        val, rep = 0, 3 + bits.take(3)
                    else:
                        val, rep = 0, 11 + bits.take(7)
                    if len(lengths) + rep > nlen + ndist:
                        raise InflateError("repeat too long")
                    lengths += [val] * rep
                if lengths[256] == 0:
                    raise InflateError("no end of block")
                ll, dd = _canonical(lengths[:nlen], True), _canonical(lengths[nlen:], True)
                trace["code_bits"] = max(trace["code_bits"], max(lengths))
            while True:
                s = _symbol(bits, ll)
                if s < 256:
                    out.append(s)
                elif s == 256:
                    break
                else:
                    if s >= 286:
                        raise InflateError("length symbol")
                    n = LENGTH_BASE[s - 257] + bits.take(LENGTH_EXTRA[s - 257])
                    d = _symbol(bits, dd)
                    if d >= 30:
                        raise InflateError("distance symbol")
                    dist = DIST_BASE[d] + bits.take(DIST_EXTRA[d])
                    if dist > len(out):
                        raise InflateError("distance too far")
                    trace["distance"], trace["length"] = max(trace["distance"], dist), max(trace["length"], n)
                    for _ in range(n):
                        out.append(out[-dist])
        if last:
            break
    bits.align()
    want = 0
    for _ in range(4):
        want = want << 8 | bits.take(8)
    if want != zlib.adler32(bytes(out)):
        raise InflateError("Adler-32")
    return bytes(out)


def read_chunks(data):
    """[(type, body)] of a PNG file, every CRC checked."""
    data = bytes(data)
    assert data[:8] == R.SIGNATURE
    at, out = 8, []
    while at < len(data):
        (n,) = struct.unpack(">I", data[at:at + 4])
        kind, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body), kind
        out.append((kind, body))
        at += 12 + n
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the deflate writer
# ---------------------------------------------------------------------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, bits):  # low bit first
        self.acc |= value << self.n
        self.n += bits

    def code(self, code, bits):  # a Huffman code: high bit first
        for i in range(bits - 1, -1, -1):
            self.put((code >> i) & 1, 1)

    def align(self):
        self.n = (self.n + 7) & ~7

    def raw(self, data):
        assert self.n % 8 == 0
        for x in bytes(data):
            self.put(x, 8)

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def codes_of(lengths):
    """Canonical codes of RFC 1951 3.2.2 for any lengths (complete or not)."""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for n in range(1, 16):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = []
    for n in lengths:
        out.append(nxt[n])
        nxt[n] += n > 0
    return out


def length_code(n):
    return R.length_symbol(n)


def dist_code(d):
    for i in range(29, -1, -1):
        if d >= DIST_BASE[i]:
            return i, DIST_EXTRA[i], d - DIST_BASE[i]
    raise ValueError(d)


def put_tokens(w, tokens, ll_len, d_len):
    """tokens: ints (literals), (length, distance) pairs, or ("sym", ll symbol) / ("dsym", length, distance symbol, extra) raw."""
    llc, dc = codes_of(ll_len), codes_of(d_len)
    for t in tokens:
        if isinstance(t, int):
            w.code(llc[t], ll_len[t])
        elif t[0] == "sym":
            w.code(llc[t[1]], ll_len[t[1]])
        elif t[0] == "dsym":
            sym, eb, extra = length_code(t[1])
            w.code(llc[sym], ll_len[sym])
            w.put(extra, eb)
            w.code(dc[t[2]], d_len[t[2]])
        else:
            sym, eb, extra = length_code(t[0])
            assert ll_len[sym], sym
            w.code(llc[sym], ll_len[sym])
            w.put(extra, eb)
            d, deb, dextra = dist_code(t[1])
            assert d_len[d], d
            w.code(dc[d], d_len[d])
            w.put(dextra, deb)
    w.code(llc[256], ll_len[256])


def stored_block(w, data, last, nlen=None):
    w.put(last, 1)
    w.put(0, 2)
    w.align()
    w.put(len(data), 16)
    w.put(len(data) ^ 0xFFFF if nlen is None else nlen, 16)
    w.raw(data)


def fixed_block(w, tokens, last):
    w.put(last, 1)
    w.put(1, 2)
    put_tokens(w, tokens, FIXED_LL, FIXED_D + [5, 5])


def dynamic_header(w, last, ll_len, d_len, cl_len, cl_symbols, hlit=None, hdist=None):
    """cl_symbols: the run-length coded lengths as (symbol,) or (symbol, extra value)."""
    w.put(last, 1)
    w.put(2, 2)
    w.put((len(ll_len) if hlit is None else hlit) - 257, 5)
    w.put((len(d_len) if hdist is None else hdist) - 1, 5)
    ncode = 19
    while ncode > 4 and cl_len[CL_ORDER[ncode - 1]] == 0:
        ncode -= 1
    w.put(ncode - 4, 4)
    for i in range(ncode):
        w.put(cl_len[CL_ORDER[i]], 3)
    clc = codes_of(cl_len)
    for s in cl_symbols:
        w.code(clc[s[0]], cl_len[s[0]])
        if s[0] >= 16:
            w.put(s[1], {16: 2, 17: 3, 18: 7}[s[0]])


def plain_cl(lengths):
    """Every length written as itself with a 5-bit code for 0 .. 15 and 16 / 17 / 18 unused."""
    return [(n,) for n in lengths]


CL_FLAT = [4] * 16 + [0, 0, 0]  # 16 codes of 4 bits: complete


def dynamic_block(w, tokens, ll_len, d_len, last, cl_len=None, cl_symbols=None):
    cl_len = CL_FLAT if cl_len is None else cl_len
    cl_symbols = plain_cl(list(ll_len) + list(d_len)) if cl_symbols is None else cl_symbols
    dynamic_header(w, last, ll_len, d_len, cl_len, cl_symbols)
    put_tokens(w, tokens, ll_len, d_len)


def tokens_output(tokens):
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out)


def zlib_wrap(body, data=None, adler=None):
    tail = struct.pack(">I", zlib.adler32(data) if adler is None else adler)
    return b"\x78\x01" + body + tail


# ---- the hand-written streams ----
def hand_written():
    """{name: (stream, expected bytes)}: valid streams zlib's compressor does not make."""
    out = {}
    rng = np.random.default_rng(5)
    base = rng.integers(0, 256, 32768, dtype=np.uint8).tolist()

    tokens = base + [(258, 32768)]
    w = BitWriter()
    d_len = [0] * 30
    d_len[29], d_len[0] = 1, 1
    dynamic_block(w, tokens, _ll_with(285), d_len, 1)
    out["distance 32768, length 258"] = (zlib_wrap(w.bytes(), tokens_output(tokens)), tokens_output(tokens))

    # a 15-bit code: lengths 1, 2, .., 14, 15, 15 on sixteen symbols
    ll = [0] * 286
    chain = [256, 65, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 76, 77, 78, 79]
    for n, s in zip([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 15], chain):
        ll[s] = n
    tokens = [79, 78, 65, 79, 70]
    w = BitWriter()
    dynamic_block(w, tokens, ll, [0], 1)
    out["a 15-bit code"] = (zlib_wrap(w.bytes(), bytes(tokens)), bytes(tokens))

    tokens = [7, 8, 9, (20, 3), (5, 3)]
    w = BitWriter()
    dynamic_block(w, tokens, _ll_with(257, 258, 259, 260, 261, 262, 263, 264, 265, 266, 267, 268, 269), [0, 0, 1], 1)
    out["one distance code"] = (zlib_wrap(w.bytes(), tokens_output(tokens)), tokens_output(tokens))

    tokens = [1, 2, 3, 4]
    w = BitWriter()
    dynamic_block(w, tokens, _ll_with(), [0], 1)
    out["no distance code"] = (zlib_wrap(w.bytes(), bytes(tokens)), bytes(tokens))

    stream, data = _repeat_across()
    out["repeat-16 across the boundary"] = (stream, data)

    w = BitWriter()
    stored_block(w, b"", 0)
    stored_block(w, b"abc", 0)
    stored_block(w, b"", 1)
    out["stored blocks of length 0"] = (zlib_wrap(w.bytes(), b"abc"), b"abc")
    return out


def _ll_with(*extra):
    """A complete literal/length code: the 256 literals and the end of block, plus `extra` symbols. 9 bits for most, padded to
    completeness with 8-bit codes: k codes of 8 bits and m of 9 with 2 k + m = 512."""
    syms = list(range(257)) + list(extra)
    m = len(syms)
    k = 512 - m  # k + (m - k) / 2 = 256  ->  codes of 8 bits: k = 512 - m
    ll = [0] * 286
    for i, s in enumerate(syms):
        ll[s] = 8 if i < k else 9
    return ll


def _repeat_across():
    """HLIT = 259, HDIST = 4: the lengths are 64 x 8 (literals 0 .. 63), 192 x 0, then 2 for symbols 256 and 257 written out, and a
    repeat-16 of three that gives symbol 258 and the distance codes 0 and 1 their length 2; the distance codes 2 and 3 follow written
    out. Both codes are complete (64 / 256 + 3 / 4; 4 / 4), and so is the code-length code: 0, 2, 8 and 16 at 2 bits."""
    ll = [8] * 64 + [0] * 192 + [2, 2, 2]
    d_len = [2, 2, 2, 2]
    cl_len = [0] * 19
    for s in (0, 2, 8, 16):
        cl_len[s] = 2
    symbols = [(8,)] * 64 + [(0,)] * 192 + [(2,), (2,), (16, 0), (2,), (2,)]
    tokens = [5, 6, 7, (3, 2), (4, 3), 9]
    w = BitWriter()
    dynamic_block(w, tokens, ll, d_len, 1, cl_len, symbols)
    data = tokens_output(tokens)
    return zlib_wrap(w.bytes(), data), data


# ---- the lists ----
def mixed_data():
    """40 000 random bytes + their first 35 000 + 3 000 zeros + 20 000 bytes drawn from 0 .. 3."""
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, 40000, dtype=np.uint8).tobytes()
    return a + a[:35000] + bytes(3000) + rng.integers(0, 4, 20000, dtype=np.uint8).tobytes()


def compress(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    return c.compress(data) + c.flush()


SETTINGS = [("level 0", dict(level=0)), ("fixed", dict(strategy=zlib.Z_FIXED)), ("huffman only", dict(strategy=zlib.Z_HUFFMAN_ONLY)),
            ("rle", dict(strategy=zlib.Z_RLE)), ("level 1", dict(level=1)), ("level 6", dict(level=6)), ("level 9", dict(level=9)),
            ("wbits 9", dict(wbits=9))]


def valid_streams():
    """[(name, stream, expected bytes)]"""
    data = mixed_data()
    out = [(name, compress(data, **kw), data) for name, kw in SETTINGS]
    out.append(("empty", zlib.compress(b""), b""))
    out.append(("one byte", zlib.compress(b"x"), b"x"))
    big = np.random.default_rng(2).integers(0, 256, 70000, dtype=np.uint8).tobytes()
    out.append(("stored 65535", compress(big, level=0), big))
    out += [(name, s, d) for name, (s, d) in hand_written().items()]
    return out


def small_stream():
    """About 100 bytes: a dynamic block with matches."""
    data = (b"the quick brown fox jumps over the lazy dog; pack my box with five dozen liquor jugs; the quick brown fox jumps over the "
            b"lazy dog again, and the five dozen jugs again")
    s = compress(data, level=9)
    assert 80 <= len(s) <= 140, len(s)
    return s, data


def malformed_streams():
    """[(name, stream)]: every rejection case of inflate.hpp. zlib is asked about each one by the tests."""
    good, data = small_stream()
    out = [("truncated", good[:-5]), ("Adler mismatch", good[:-1] + bytes([good[-1] ^ 1])),
           ("CM = 7", bytes([0x77, 0x01 + (31 - (0x7701 % 31)) % 31]) + good[2:]), ("CINFO = 8", b"\x88\x1c" + good[2:]),
           ("FCHECK", bytes([good[0], good[1] ^ 1]) + good[2:]), ("FDICT", b"\x78\x20" + good[2:])]
    w = BitWriter()
    w.put(1, 1), w.put(3, 2)
    out.append(("block type 3", zlib_wrap(w.bytes(), b"")))
    w = BitWriter()
    stored_block(w, b"abc", 1, nlen=0x1234)
    out.append(("LEN / NLEN", zlib_wrap(w.bytes(), b"abc")))
    # oversubscribed: three codes of 1 bit
    ll = [0] * 257
    ll[0] = ll[1] = ll[256] = 1
    w = BitWriter()
    dynamic_header(w, 1, ll, [0], CL_FLAT, plain_cl(ll + [0]))
    out.append(("oversubscribed lengths", zlib_wrap(w.bytes() + bytes(4), b"")))
    # incomplete: two codes of 2 bits
    ll = [0] * 257
    ll[0] = ll[256] = 2
    w = BitWriter()
    dynamic_header(w, 1, ll, [0], CL_FLAT, plain_cl(ll + [0]))
    w.code(1, 2)
    out.append(("incomplete lengths", zlib_wrap(w.bytes() + bytes(4), b"")))
    # an incomplete code-length code: one code of 1 bit
    cl = [0] * 19
    cl[0] = 1
    w = BitWriter()
    dynamic_header(w, 1, [0] * 257, [0], cl, [(0,)] * 258)
    out.append(("incomplete code-length code", zlib_wrap(w.bytes() + bytes(4), b"")))
    # symbols 286 / 287 and distance codes 30 / 31 exist only in the fixed code
    for sym in (286, 287):
        w = BitWriter()
        fixed_block(w, [65, ("sym", sym)], 1)
        out.append((f"symbol {sym}", zlib_wrap(w.bytes() + bytes(4), b"A")))
    for d in (30, 31):
        w = BitWriter()
        fixed_block(w, [65, 66, 67, ("dsym", 3, d)], 1)
        out.append((f"distance code {d}", zlib_wrap(w.bytes() + bytes(4), b"ABC")))
    w = BitWriter()
    fixed_block(w, [65, 66, (3, 3)], 1)
    out.append(("distance in front of the output", zlib_wrap(w.bytes(), b"ABABA")))
    # HLIT = 287 (288 is not expressible with 286 lengths: the header field alone)
    w = BitWriter()
    dynamic_header(w, 1, _ll_with(), [0], CL_FLAT, plain_cl(_ll_with() + [0]), hlit=287)
    out.append(("HLIT above 286", zlib_wrap(w.bytes() + bytes(8), b"")))
    w = BitWriter()
    dynamic_header(w, 1, _ll_with(), [0] * 30, CL_FLAT, plain_cl(_ll_with() + [0] * 30), hdist=31)
    out.append(("HDIST above 30", zlib_wrap(w.bytes() + bytes(8), b"")))
    # no end of block code
    ll = [8] * 256 + [0]
    w = BitWriter()
    dynamic_header(w, 1, ll, [0], CL_FLAT, plain_cl(ll + [0]))
    out.append(("no end of block", zlib_wrap(w.bytes() + bytes(4), b"")))
    # a repeat-16 as the first code, and a repeat running past HLIT + HDIST
    cl = [0] * 19
    cl[0] = cl[8] = cl[16] = cl[18] = 2
    w = BitWriter()
    dynamic_header(w, 1, [0] * 257, [0], cl, [(16, 0)])
    out.append(("repeat-16 first", zlib_wrap(w.bytes() + bytes(8), b"")))
    w = BitWriter()
    dynamic_header(w, 1, [0] * 257, [0], cl, [(8,)] * 250 + [(18, 127)])
    out.append(("repeat past the tables", zlib_wrap(w.bytes() + bytes(8), b"")))
    return out


def truncation_sweep():
    good, _ = small_stream()
    return [good[:k] for k in range(len(good))]


def bit_flips():
    good, _ = small_stream()
    return [good[:i >> 3] + bytes([good[i >> 3] ^ (1 << (i & 7))]) + good[(i >> 3) + 1:] for i in range(8 * len(good))]


def zlib_says(stream):
    """bytes, or None where zlib.decompress raises."""
    try:
        return zlib.decompress(stream)
    except zlib.error:
        return None


def split_ranges(stream, rule):
    stream = bytes(stream)
    if rule == "whole":
        return [stream]
    if rule == "empties":
        third = len(stream) // 3
        return [b"", stream[:third], b"", b"", stream[third:], b""]
    return [stream[i:i + rule] for i in range(0, len(stream), rule)] or [b""]


def host_inflate(ranges, capacity):
    """dad3d_inflate_host -> (flag, bytes); asserts that nothing outside out[0, capacity) was written."""
    from dad_3dheads_amd import _lib

    lib = _lib.load()
    keep = [np.frombuffer(bytes(r) + b"\0", dtype=np.uint8) for r in ranges]
    ptrs = (C.c_void_p * max(len(ranges), 1))(*[k.ctypes.data for k in keep])
    lens = (C.c_int64 * max(len(ranges), 1))(*[len(r) for r in ranges])
    buf = np.full(capacity + 128, GUARD, dtype=np.uint8)
    length, flag = C.c_int64(-1), C.c_int32(-1)
    _lib.check(lib.dad3d_inflate_host(ptrs, lens, len(ranges), buf.ctypes.data + 64, capacity, C.addressof(length), C.addressof(flag)))
    assert (buf[:64] == GUARD).all() and (buf[64 + capacity:] == GUARD).all(), "guard bytes"
    assert 0 <= length.value <= capacity
    return flag.value, buf[64:64 + length.value].tobytes()


# ---------------------------------------------------------------------------------------------------------------------------
# the PNG writer
# ---------------------------------------------------------------------------------------------------------------------------
def filter_with(image, types):
    """The filtered stream of uint8 [H,W,C] with the given filter type per row."""
    img = np.asarray(image)
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
    cand = np.stack([x, x - a, x - b, x - (a + b) // 2, x - paeth]) & 255
    types = np.asarray(types, dtype=np.int64)
    rows = cand[np.minimum(types, 4), np.arange(h)].astype(np.uint8)
    return np.concatenate([types.astype(np.uint8)[:, None], rows], axis=1).tobytes()


def write_png(image, types=None, split=None, level=6, before=(), after=(), deflated=None, empties=False):
    """A PNG of uint8 [H,W,C]: `types` forces the filter type of every row (default: 0), `split` = bytes per IDAT (None: one),
    `before` / `after` = extra chunks (type, body) around the IDATs, `deflated` = the zlib stream to use instead of zlib's own,
    `empties` puts a zero-length IDAT between the others."""
    img = np.asarray(image)
    h, w, c = img.shape
    stream = filter_with(img, [0] * h if types is None else types)
    z = zlib.compress(stream, level) if deflated is None else deflated
    parts = [z] if split is None else [z[i:i + split] for i in range(0, len(z), split)]
    if empties:
        parts = [q for p in parts for q in (p, b"")]
    ihdr = struct.pack(">IIBBBBB", w, h, 8, R.COLOUR_TYPE[c], 0, 0, 0)
    return (R.SIGNATURE + R.chunk(b"IHDR", ihdr) + b"".join(R.chunk(k, v) for k, v in before) + b"".join(R.chunk(b"IDAT", p) for p in parts) +
            b"".join(R.chunk(k, v) for k, v in after) + R.chunk(b"IEND", b""))
