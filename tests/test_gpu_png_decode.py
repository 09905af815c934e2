"""GPU: PNG files and zlib streams read back on the device (csrc/png_decode.hip, dad_3dheads_amd/png_reader.py),
bit-equal to `PIL.Image.open` and `zlib.decompress`. Every case goes through the C ABI first, with guard bytes around every output
and the flags asserted before anything else (a host fallback must not be able to hide a kernel fault), then through `png_reader`.
The streams and files come from tests/png_decode_restatement.py, which tests/test_png_decode_host.py pins to zlib and PIL."""
import ctypes as C
import io
import struct
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import png_decode_restatement as D
import png_restatement as R
from dad_3dheads_amd import _lib, png_reader, writers

pytestmark = pytest.mark.gpu
S = _lib.PNG_SEGMENT_BYTES
GUARD = 0x23
MALFORMED, UNSUPPORTED, OVERFLOW = _lib.PNG_DECODE_FLAG_MALFORMED, _lib.PNG_DECODE_FLAG_UNSUPPORTED, _lib.PNG_DECODE_FLAG_OVERFLOW


def align(n):
    return (n + 15) // 16 * 16


# ---------------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------------
def capi_zlib(streams, caps):
    """dad3d_zlib_decompress -> (outputs, flags); the guard bytes behind every output are checked."""
    lib = _lib.load()
    rows, at, out_at = [], 0, 0
    for s, cap in zip(streams, caps):
        rows.append([at, len(s), out_at, cap])
        at += align(len(s)) + 16
        out_at += align(cap) + 16
    data = np.full(at, 0xEE, dtype=np.uint8)
    for row, s in zip(rows, streams):
        data[row[0]:row[0] + row[1]] = np.frombuffer(s, dtype=np.uint8)
    dev = torch.from_numpy(data).cuda()
    desc = torch.tensor(rows, dtype=torch.int64).cuda()
    out = torch.full((out_at,), GUARD, dtype=torch.uint8, device="cuda")
    lengths = torch.full((len(rows),), -1, dtype=torch.int64, device="cuda")
    flags = torch.full((len(rows),), -1, dtype=torch.int32, device="cuda")
    _lib.check(lib.dad3d_zlib_decompress(dev.data_ptr(), at, desc.data_ptr(), len(rows), out.data_ptr(), out_at, lengths.data_ptr(),
                                         flags.data_ptr(), 0, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    host, ln, fl = out.cpu().numpy(), lengths.cpu().tolist(), flags.cpu().tolist()
    outs = []
    for k, row in enumerate(rows):
        assert 0 <= ln[k] <= row[3], k
        end = rows[k + 1][2] if k + 1 < len(rows) else out_at
        if fl[k] == 0:
            assert (host[row[2] + ln[k]:end] == GUARD).all(), k  # nothing behind an item is touched
        else:
            assert ln[k] == 0 and (host[row[2] + row[3]:end] == GUARD).all(), k  # a refused item stays inside its room
        outs.append(host[row[2]:row[2] + ln[k]].tobytes())
    return outs, fl


def header_of(data):
    w, h, depth, colour = struct.unpack(">IIBB", data[16:26])
    return h, w, {0: 1, 4: 2, 2: 3, 6: 4, 3: 1}.get(colour, 1)


def capi_png(files, channels=None, force_general=False, pad=5, shapes=None):
    """dad3d_png_decode -> (images or None per file, flags, info). Rows lie `pad` bytes apart; every byte between the rows and between
    the images must stay as it was."""
    lib = _lib.load()
    rows, at, out_at = [], 0, 0
    for i, f in enumerate(files):
        h, w, c = header_of(f) if shapes is None or shapes[i] is None else shapes[i]
        oc = c if channels is None else channels
        stride = w * oc + pad
        rows.append([at, len(f), h, w, c, out_at, stride, oc, 0, 0, 0, 0])
        at += align(len(f)) + 16
        out_at += align(h * stride) + 16
    desc = np.asarray(rows, dtype=np.int64)
    most = C.c_int32(0)
    nbytes = lib.dad3d_png_decode_scratch_bytes(desc.ctypes.data, len(rows), C.addressof(most))
    assert nbytes > 0
    data = np.full(at, 0xEE, dtype=np.uint8)
    for row, f in zip(rows, files):
        data[row[0]:row[0] + row[1]] = np.frombuffer(f, dtype=np.uint8)
    dev = torch.from_numpy(data).cuda()
    out = torch.full((out_at,), GUARD, dtype=torch.uint8, device="cuda")
    flags = torch.full((len(rows),), -1, dtype=torch.int32, device="cuda")
    info = torch.full((len(rows),), -1, dtype=torch.int32, device="cuda")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    desc_dev = torch.from_numpy(desc).cuda()
    _lib.check(lib.dad3d_png_decode(dev.data_ptr(), at, desc_dev.data_ptr(), len(rows), most.value, out.data_ptr(), out_at,
                                    flags.data_ptr(), info.data_ptr(), scratch.data_ptr(), nbytes, int(force_general), 0,
                                    torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    host, fl, inf = out.cpu().numpy(), flags.cpu().tolist(), info.cpu().tolist()
    images = []
    for k, row in enumerate(rows):
        _, _, h, w, _, o, stride, oc = row[:8]
        end = rows[k + 1][5] if k + 1 < len(rows) else out_at
        block = host[o:o + h * stride].reshape(h, stride)
        assert (block[:, w * oc:] == GUARD).all() and (host[o + h * stride:end] == GUARD).all(), k
        images.append(block[:, :w * oc].reshape(h, w, oc).copy() if fl[k] == 0 else None)
    return images, fl, inf


def pil_array(data, channels=None):
    im = Image.open(io.BytesIO(data))
    im.load()
    if channels is not None:
        im = im.convert(R.PIL_MODE[channels])
    arr = np.asarray(im)
    return arr[:, :, None] if arr.ndim == 2 else arr


def pil_raises(data):
    try:
        pil_array(data)
    except Exception:  # noqa: BLE001 -- whatever PIL raises for the file
        return True
    return False


def decode_all(files, channels=None):
    """The C ABI and png_reader on the same files, both equal to PIL; returns info."""
    images, flags, info = capi_png(files, channels)
    assert flags == [0] * len(files)
    want = [pil_array(f, channels) for f in files]
    for k, (got, ref) in enumerate(zip(images, want)):
        assert got.shape == ref.shape and np.array_equal(got, ref), k
    res = png_reader.PngDecoder(0).decode(files, channels)
    assert res.flags.tolist() == [0] * len(files)
    for k, (got, ref) in enumerate(zip(res.tensors(), want)):
        assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), ref), k
    return info


# ---------------------------------------------------------------------------------------------------------------------------
# zlib streams
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def valid():
    return D.valid_streams()


def test_valid_streams_as_a_batch(valid):
    streams = [s for _, s, _ in valid]
    outs, flags = capi_zlib(streams, [len(d) + (k % 3) for k, (_, _, d) in enumerate(valid)])
    assert flags == [0] * len(valid)  # first
    for (name, _, data), got in zip(valid, outs):
        assert got == data, name
    outs, flags = capi_zlib(streams, [max(len(d) - 1, 0) for _, _, d in valid])
    assert [f for f, (_, _, d) in zip(flags, valid) if d] == [OVERFLOW] * sum(1 for _, _, d in valid if d)


def against_zlib(streams, capacity=4096):
    outs, flags = capi_zlib(streams, [capacity] * len(streams))
    refused = 0
    for k, (s, got, flag) in enumerate(zip(streams, outs, flags)):
        want = D.zlib_says(s)
        if want is None:
            assert flag != 0, k
            refused += 1
        else:
            assert flag == 0 and got == want, k
    return refused


def test_malformed_streams(valid):
    good, data = D.small_stream()
    outs, flags = capi_zlib([good], [len(data)])
    assert flags == [0] and outs == [data]  # first: the stream the sweeps damage is read without a flag
    named = D.malformed_streams()
    assert against_zlib([s for _, s in named]) == len(named)
    sweep = D.truncation_sweep()
    assert against_zlib(sweep) == len(sweep)  # one batch
    assert against_zlib(D.bit_flips()) > 400


def test_compress_then_decompress():
    rng = np.random.default_rng(11)
    rows = np.stack([rng.integers(0, 256, 20000, dtype=np.uint8), rng.integers(0, 3, 20000, dtype=np.uint8),
                     np.tile(rng.integers(0, 256, 40, dtype=np.uint8), 500), np.zeros(20000, np.uint8)])
    streams = writers.zlib_compress_batch(torch.from_numpy(rows).cuda())
    outs, flags = capi_zlib(streams, [20000] * 4)
    assert flags == [0] * 4
    assert outs == [r.tobytes() for r in rows]
    assert png_reader.zlib_decompress_batch(streams, 20000) == [r.tobytes() for r in rows]
    assert png_reader.zlib_decompress_batch(streams, [20000, 20001, 30000, 19999]) == [r.tobytes() for r in rows]  # the last: the host's
    with pytest.raises(zlib.error):
        png_reader.zlib_decompress_batch([streams[0][:-3]], 20000)


# ---------------------------------------------------------------------------------------------------------------------------
# files of other encoders
# ---------------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1), (1, 1, 2), (1, 1, 3), (1, 1, 4), (2, 3, 2), (3, 5, 3), (64, 1, 1), (65, 7, 3), (5, 700, 4), (3, 8292, 1), (130, 40, 3)]


def image_of(shape, seed):
    """Smooth ramps with noise on a tenth of the pixels: compressible, and every Paeth branch occurs."""
    h, w, c = shape
    rng = np.random.default_rng(seed)
    y, x, ch = np.meshgrid(np.arange(h), np.arange(w), np.arange(c), indexing="ij")
    img = (3 * x + 5 * y + 40 * ch) % 256
    noisy = rng.random((h, w, 1)) < 0.1
    return np.where(noisy, rng.integers(0, 256, (h, w, c)), img).astype(np.uint8)


def pil_png(img, level):
    buf = io.BytesIO()
    Image.fromarray(img[:, :, 0] if img.shape[2] == 1 else img, R.PIL_MODE[img.shape[2]]).save(buf, "PNG", compress_level=level)
    return buf.getvalue()


EXTRA = [(b"gAMA", struct.pack(">I", 45455)), (b"pHYs", struct.pack(">IIB", 2835, 2835, 1)), (b"tEXt", b"Comment\0a test file"),
         (b"tIME", struct.pack(">HBBBBB", 2024, 1, 2, 3, 4, 5))]


def test_shapes_and_encoders():
    files = []
    for k, shape in enumerate(SHAPES):
        img = image_of(shape, k)
        types = [(7 * y + 3) % 5 for y in range(shape[0])]
        files += [pil_png(img, level) for level in (0, 1, 6, 9)]
        files += [D.write_png(img, types, split=1), D.write_png(img, types, split=7), D.write_png(img, types),
                  D.write_png(img, types, split=7, empties=True), D.write_png(img, types, split=1000, before=EXTRA[:2], after=EXTRA[2:]),
                  D.write_png(img, types, before=EXTRA, after=EXTRA, level=0)]
    info = decode_all(files)
    assert not any(info)  # none of these has the layout of this library's encoder


@pytest.mark.parametrize("shape", [(3, 5, 3), (65, 7, 3), (5, 700, 4), (130, 40, 1), (70, 9, 2)], ids=lambda s: "x".join(map(str, s)))
def test_filters(shape):
    h, w, c = shape
    rng = np.random.default_rng(h * w)
    random = rng.integers(0, 256, shape, dtype=np.uint8)
    # ties of Paeth: a == b (left equals above), pa == pb, pb == pc -- from pixels drawn from two and three values
    ties = [rng.choice(np.array(v, dtype=np.uint8), shape) for v in ([10, 20], [0, 255], [5, 10, 15], [100, 101, 102])]
    files = []
    for img in [random] + ties:
        files += [D.write_png(img, [t] * h, split=4096) for t in range(5)]
        files.append(D.write_png(img, [(7 * y + 3) % 5 for y in range(h)]))
    decode_all(files)
    if h * w * c < 3000:  # the restated unfilter reads the writer's files too (byte by byte: the small cases)
        for f in files[:6]:
            assert np.array_equal(R.unfilter(R.read_png(f)["stream"], h, w, c), random)
    bad = [D.write_png(random, [0] * (h - 1) + [5]), D.write_png(random, [5] + [1] * (h - 1)), D.write_png(random, [4] * (h // 2) + [255] * (h - h // 2))]
    _, flags, _ = capi_png(bad)
    assert flags == [MALFORMED] * 3


def test_channel_conversion():
    rng = np.random.default_rng(21)
    files = [pil_png(rng.integers(0, 256, (9, 11, c), dtype=np.uint8), 6) for c in (1, 2, 3, 4)]
    for channels in (3, 1, 2, 4):  # 3 is what the predictor asks for
        images, flags, _ = capi_png(files, channels)
        assert flags == [0] * 4
        for f, got in zip(files, images):
            want = np.asarray(Image.open(io.BytesIO(f)).convert(R.PIL_MODE[channels]))
            assert np.array_equal(got, want.reshape(9, 11, channels)), (channels, header_of(f))
    for got, f in zip(png_reader.load_png_batch(files), files):
        assert np.array_equal(got.cpu().numpy(), np.asarray(Image.open(io.BytesIO(f)).convert("RGB")))


# ---------------------------------------------------------------------------------------------------------------------------
# the segmented path
# ---------------------------------------------------------------------------------------------------------------------------
def own_files():
    images = R.fixture_images()
    files = []
    for img in images.values():
        files += writers.png_batch(torch.from_numpy(img[None]).cuda())
    return list(images.values()), files


LEAD = 4  # kLead of csrc/png_decode.hip: how far a segment's distances may reach into the segment before


def inflates_alone(payload, lead=0):
    """zlib on one IDAT as a raw deflate stream with `lead` bytes of history: False where a distance reaches further back."""
    try:
        (zlib.decompressobj(-15, zdict=bytes(lead)) if lead else zlib.decompressobj(-15)).decompress(payload)
    except zlib.error:
        return False
    return True


def independent(data):
    return all(inflates_alone(p) for p in R.read_png(data)["idat"][1:-1])


def within_lead(data):
    """What the segmented path takes, decided by zlib: the first segment inflates alone, every other with LEAD bytes in front."""
    segments = R.read_png(data)["idat"][1:-1]
    return inflates_alone(segments[0]) and all(inflates_alone(p, LEAD) for p in segments[1:])


def test_own_files_on_both_paths():
    images, files = own_files()
    imgs, flags, info = capi_png(files)
    assert flags == [0] * len(files)
    for got, want in zip(imgs, images):
        assert np.array_equal(got, want)
    general, flags, forced = capi_png(files, force_general=True)
    assert flags == [0] * len(files) and forced == [0] * len(files)
    for got, want in zip(general, images):
        assert np.array_equal(got, want)
    # both kinds of file are here, which zlib decides: every IDAT inflating on its own, and IDATs that copy from the one before
    alone = [independent(f) for f in files]
    assert any(alone) and not all(alone) and all(within_lead(f) for f in files)
    assert all(info)
    res = png_reader.PngDecoder(0).decode(files)
    assert res.segmented.tolist() == [bool(i) for i in info] and res.flags.tolist() == [0] * len(files)
    for got, want in zip(res.tensors(), images):
        assert np.array_equal(got.cpu().numpy(), want)
    small = [R.png_file(image_of(s, 3), S)[0] for s in SHAPES]  # the encoder's bytes from its restatement: one segment, and up to four
    assert all(within_lead(f) for f in small) and all(decode_all(small))


def test_own_files_report_the_segmented_bit():
    """Every file of `writers.png_batch` reports the segmented bit. The encoder lets a match at a segment's first bytes reach up to C
    bytes in front of the segment (png_encode.hip reads the four bytes before it): counted with zlib on every IDAT alone, 7 of the
    head render's 25 segments are independent, 7 of 25 of the PNCC map, 12 of 25 of the UV texture, all of the RGBA soup, the 8 x 8
    triangle and the photo. The segmented path inflates the dependent ones a second time with their true last four bytes of history."""
    _, files = own_files()
    _, flags, info = capi_png(files)
    assert flags == [0] * len(files)
    assert info == [_lib.PNG_DECODE_INFO_SEGMENTED] * len(files)


def flushed_png(img, mode, cuts=None):
    """The filtered stream (filter 0) deflated with a flush of `mode` behind every piece, cut into IDATs at the flushes: header |
    pieces ending in 00 00 FF FF | 03 00 + Adler-32, the layout of this library's files."""
    h, w, c = img.shape
    stream = D.filter_with(img, [0] * h)
    cuts = cuts or list(range(S, len(stream), S)) + [len(stream)]
    comp = zlib.compressobj(6)
    parts, lo = [], 0
    for hi in cuts:
        parts.append(comp.compress(stream[lo:hi]) + comp.flush(mode))
        lo = hi
    tail = comp.flush()
    assert parts[0][:2] == b"\x78\x9c" and tail[:2] == b"\x03\x00" and len(tail) == 6 and all(p[-4:] == b"\x00\x00\xff\xff" for p in parts)
    parts = [parts[0][:2], parts[0][2:]] + parts[1:] + [tail]
    ihdr = struct.pack(">IIBBBBB", w, h, 8, R.COLOUR_TYPE[c], 0, 0, 0)
    return R.SIGNATURE + R.chunk(b"IHDR", ihdr) + b"".join(R.chunk(b"IDAT", p) for p in parts) + R.chunk(b"IEND", b"")


def test_files_that_only_look_segmented():
    rng = np.random.default_rng(31)
    period = rng.integers(0, 256, (1, 1023, 1), dtype=np.uint8)
    img = np.tile(period, (32, 1, 1))  # 32 rows of 1 + 1023 bytes: four segments, every row a copy of the one above
    sync, full = flushed_png(img, zlib.Z_SYNC_FLUSH), flushed_png(img, zlib.Z_FULL_FLUSH)
    uneven = flushed_png(img, zlib.Z_FULL_FLUSH, cuts=[S, 2 * S - 1, 3 * S, 4 * S])  # 8192, 8191, 8193, 8192
    images, flags, info = capi_png([sync, full, uneven])
    assert flags == [0, 0, 0]
    for got in images:
        assert np.array_equal(got, img)
    assert info[0] == 0  # the history crosses the IDATs: only the serial inflate reads it
    assert info[1] in (0, _lib.PNG_DECODE_INFO_SEGMENTED)
    assert info[2] == 0
    decode_all([sync, full, uneven])


def test_short_distances_across_flushes():
    """Flushed streams whose history crosses the IDATs by no more than LEAD bytes, which is what the segmented path allows: one run
    of zeros through the whole stream (every segment's last bytes are copies of the bytes in front of it, back to the first
    segment), and noise with runs of zeros over the cuts. Right pixels, and the bit wherever zlib takes every IDAT with LEAD bytes
    of history."""
    rng = np.random.default_rng(37)
    run = np.zeros((40, 1023, 1), dtype=np.uint8)
    noisy = []
    for runs in ([(3 * S - 2, 3 * S + 300)], [(S - 700, S + 900), (3 * S - 2, 3 * S + 300)]):
        stream = rng.integers(1, 256, (40, 1024), dtype=np.uint8)
        stream[:, 0] = 0  # the filter bytes
        for lo, hi in runs:
            stream.reshape(-1)[lo:hi] = 0
        noisy.append(stream[:, 1:].reshape(40, 1023, 1).copy())
    originals = [run] + noisy
    files = [flushed_png(img, zlib.Z_SYNC_FLUSH) for img in originals]
    expected = [within_lead(f) for f in files]
    assert expected[:2] == [True, True] and not any(independent(f) for f in files)
    images, flags, info = capi_png(files)
    assert flags == [0, 0, 0]
    for got, img in zip(images, originals):
        assert np.array_equal(got, img)
    assert [bool(i) for i in info] == expected
    decode_all(files)


# ---------------------------------------------------------------------------------------------------------------------------
# unsupported and malformed files
# ---------------------------------------------------------------------------------------------------------------------------
def saved(im, **kw):
    buf = io.BytesIO()
    im.save(buf, "PNG", **kw)
    return buf.getvalue()


def test_unsupported_files_go_to_pil():
    rng = np.random.default_rng(41)
    palette = Image.fromarray(rng.integers(0, 256, (6, 7, 3), dtype=np.uint8), "RGB").quantize(16)
    sixteen = Image.fromarray(rng.integers(0, 65536, (6, 7), dtype=np.uint16))
    bilevel = Image.fromarray(rng.integers(0, 2, (6, 7), dtype=np.uint8) * 255, "L").convert("1")
    ihdr = struct.pack(">IIBBBBB", 1, 1, 8, 2, 0, 0, 1)  # Adam7 of one pixel: one pass, one row
    adam7 = R.SIGNATURE + R.chunk(b"IHDR", ihdr) + R.chunk(b"IDAT", zlib.compress(b"\x00\x0a\x14\x1e")) + R.chunk(b"IEND", b"")
    files = [saved(palette), saved(sixteen), saved(bilevel), adam7]
    assert files[0][25] == 3 and files[1][24] == 16 and files[2][24] == 1 and files[3][28] == 1 and not any(pil_raises(f) for f in files)
    _, flags, _ = capi_png(files)
    assert flags == [UNSUPPORTED] * 4
    good = pil_png(image_of((4, 4, 3), 1), 6)
    res = png_reader.PngDecoder(0).decode(files + [good], channels=3)
    assert res.flags.tolist() == [-1, -1, -1, UNSUPPORTED, 0]  # the host's look at the IHDR keeps the first three off the device
    for got, f in zip(res.tensors(), files + [good]):
        assert np.array_equal(got.cpu().numpy(), pil_array(f, 3))


def test_malformed_files():
    img = image_of((20, 30, 3), 5)
    good = D.write_png(img, [(7 * y + 3) % 5 for y in range(20)], split=200)
    _, flags, _ = capi_png([good])
    assert flags == [0]  # first
    stream = D.filter_with(img, [1] * 20)
    chunks = D.read_chunks(good)
    idat_at = good.index(b"IDAT")

    def flip(data, at):
        return data[:at] + bytes([data[at] ^ 0x40]) + data[at + 1:]

    z = zlib.compress(stream)
    cases = {
        "signature": flip(good, 1),
        "CRC of IHDR": flip(good, 8 + 8 + 13 + 1),
        "CRC of an IDAT": flip(good, idat_at + 4 + len(chunks[1][1]) + 2),
        "a byte of an IDAT": flip(good, idat_at + 20),
        "Adler-32": D.write_png(img, [1] * 20, deflated=z[:-1] + bytes([z[-1] ^ 1])),
        "an IDAT cut short": D.write_png(img, [1] * 20, deflated=z[:-9]),
        "a stream one byte short": D.write_png(img, [1] * 20, deflated=zlib.compress(stream[:-1])),
        "a stream one byte long": D.write_png(img, [1] * 20, deflated=zlib.compress(stream + b"\0")),
        "no IEND": good[:-12],
        "cut inside a chunk": good[:len(good) // 2],
        "an unknown critical chunk": D.write_png(img, before=[(b"ABCD", b"xyz")]),
        "IDATs apart": _idats_apart(img),
    }
    names = list(cases)
    files = [cases[k] for k in names]
    _, flags, _ = capi_png(files, shapes=[(20, 30, 3)] * len(files))
    for name, flag in zip(names, flags):
        assert flag == MALFORMED, name
    _, flags, _ = capi_png([good, good, good], shapes=[(20, 31, 3), (21, 30, 3), (20, 30, 4)])  # IHDR against the descriptor
    assert flags == [MALFORMED] * 3
    decoder = png_reader.PngDecoder(0)
    for name, f in zip(names, files):
        if pil_raises(f):
            with pytest.raises(Exception):  # noqa: B017, PT011 -- PIL's own error, whatever its class
                decoder.decode([f])
        else:  # the device is stricter than PIL: the pixels are then PIL's
            res = decoder.decode([f])
            assert res.flags.tolist() != [0], name
            assert np.array_equal(res.tensors()[0].cpu().numpy(), pil_array(f)), name
    assert pil_raises(cases["signature"]) and pil_raises(cases["CRC of IHDR"])


def _idats_apart(img):
    data = D.write_png(img, split=100)
    chunks = D.read_chunks(data)
    chunks.insert(3, (b"tEXt", b"k\0v"))  # behind the second IDAT
    return R.SIGNATURE + b"".join(R.chunk(k, v) for k, v in chunks)


def test_truncated_files_stay_in_bounds():
    good = pil_png(image_of((40, 40, 3), 9), 6)
    files = [good[:k] for k in range(0, len(good), 97)]
    _, flags, _ = capi_png(files, shapes=[(40, 40, 3)] * len(files))
    assert all(f == MALFORMED for f in flags)


# ---------------------------------------------------------------------------------------------------------------------------
# the predictor
# ---------------------------------------------------------------------------------------------------------------------------
class Stub(torch.nn.Module):
    """Fixed parameters and landmarks, moved by the mean colour of the input so that a wrong pixel shows."""

    def __init__(self):
        super().__init__()
        from dad_3dheads_amd import synthetic

        self.register_buffer("base", torch.from_numpy(synthetic.synthetic_params(1, seed=8))[0])
        self.register_buffer("ramp", torch.linspace(0.2, 0.9, 68)[None, :, None])

    def forward(self, x):
        feat = x.double().mean(dim=(2, 3)).float()
        p = self.base[None] + 0.01 * torch.tanh(feat).sum(1, keepdim=True)
        lm = torch.sigmoid(feat[:, :2])[:, None, :].expand(-1, 68, -1) * self.ramp
        return {"OUTPUT_3DMM_PARAMS": p, "OUTPUT_2D_LANDMARKS": lm}


def test_predict_files_equals_predict_batch(flame_model, monkeypatch):
    from dad_3dheads_amd.config import load_default_config
    from dad_3dheads_amd.predictor import FaceMeshPredictor

    pred = FaceMeshPredictor(load_default_config(), cuda_id=0, model=Stub(), flame_model=flame_model)
    photo = R.fixture_images()["photo"]
    arrays = [photo, image_of((90, 120, 3), 1), image_of((130, 40, 4), 2)[:, :, :3].copy(), image_of((33, 47, 1), 3)]
    files = [writers.png_batch(torch.from_numpy(arrays[0][None]).cuda())[0], pil_png(arrays[1], 6),
             pil_png(image_of((130, 40, 4), 2), 9), pil_png(arrays[3], 1)]  # own file, RGB, RGBA and grey: four sizes in one call
    arrays = [np.array(pil_array(f, 3)) for f in files]
    assert np.array_equal(arrays[0], photo) and np.array_equal(arrays[2], image_of((130, 40, 4), 2)[:, :, :3])
    staged = []
    launch = pred._preprocess_launch

    def spy(sources):
        out = launch(sources)
        staged.append(out.clone())
        return out

    monkeypatch.setattr(pred, "_preprocess_launch", spy)
    want = pred.predict_batch(arrays)
    got = pred.predict_files(files)
    assert len(staged) == 2 and torch.equal(staged[0], staged[1])  # the preprocessed tensor, bit for bit
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        assert set(g) == set(w) == {"points", "projected_vertices", "3d_vertices", "3dmm_params"}
        assert np.array_equal(g["points"], w["points"])
        for k in ("projected_vertices", "3d_vertices", "3dmm_params"):
            assert torch.equal(g[k], w[k]), k
    dev = pred.predict_files(files[:2], device_outputs=True)
    assert dev[0]["3d_vertices"].is_cuda
