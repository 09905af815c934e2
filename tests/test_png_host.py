"""CPU: the parts of the PNG encoder that need no GPU.

  * tests/png_restatement.py pins itself: its filter rule on hand-computed rows (each of the five types, and the tie rule), its
    container and strict reader against PIL and zlib on every fixture image, its bitstream restatement against zlib's inflate;
  * `dad3d_deflate_tables_host` -- the single-lane table routine of csrc/deflate_tables.hpp, the code the kernel runs -- fuzzed over
    seeded histograms: lengths within the limits, Kraft sums, canonical codes, and a block assembled from its header bits and codes
    inflates to the intended symbols;
  * the argument validation of the C ABI, which happens before any device work.
"""
import zlib

import numpy as np
import pytest

import png_restatement as R
from dad_3dheads_amd import _lib, writers


@pytest.fixture(scope="module")
def images():
    return R.fixture_images()


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------
HAND_ROWS = [
    # (rows of a one-channel image, expected types, expected filtered rows): worked by hand from the PNG specification
    # costs None 4, Sub 7, Up 4 (the row above is zeros): a tie of None and Up goes to type 0
    ([[1, 255, 1, 255]], [0], [[1, 255, 1, 255]]),
    # Sub 40 against None 100, Up 100, Average 70, Paeth 40 (no row above: Paeth predicts the left byte): a tie goes to type 1
    ([[10, 20, 30, 40]], [1], [[10, 10, 10, 10]]),
    # Up: the row repeats the one above, Up and Paeth both give zeros: a tie goes to type 2
    ([[10, 200, 30, 77], [10, 200, 30, 77]], [0, 2], [[10, 200, 30, 77], [0, 0, 0, 0]]),
    # Average: every byte is floor((left + above) / 2): 50 = 100 // 2, 50 = (50 + 50) // 2, 125 = (50 + 200) // 2, 72 = (125 + 20) // 2
    ([[100, 50, 200, 20], [50, 50, 125, 72]], [0, 3], [[100, 50, 200, 20], [0, 0, 0, 0]]),
    # Paeth 56 + 7 + 85 + 73 = 221 against None 269, Sub 312, Up 309, Average 368; predictors: above 158, upper left 158, above 235, above 1
    ([[158, 70, 235, 1], [214, 165, 64, 184]], [0, 4], [[158, 70, 235, 1], [56, 7, 85, 183]]),
]


@pytest.mark.parametrize("rows, types, filtered", HAND_ROWS)
def test_filter_rule_on_hand_computed_rows(rows, types, filtered):
    img = np.array(rows, dtype=np.uint8)[:, :, None]
    got_types, got_rows = R.filter_rows(img)
    assert got_types.tolist() == types
    assert got_rows.tolist() == filtered
    assert np.array_equal(R.unfilter(R.filtered_stream(img), *img.shape), img)


def test_filter_rule_with_channels_looks_one_pixel_back():
    img = np.array([[[10, 200], [12, 190], [14, 180]], [[10, 200], [12, 190], [14, 180]]], dtype=np.uint8)
    types, rows = R.filter_rows(img)
    assert types.tolist() == [1, 2]
    assert rows.tolist() == [[10, 200, 2, 246, 2, 246], [0] * 6]  # 12 - 10, 190 - 200, ...: the byte two places back


def test_container_and_reader_against_pil_and_zlib(images):
    for name, img in images.items():
        data = R.reference_png(img)
        info = R.read_png(data)
        assert (info["height"], info["width"], info["channels"]) == img.shape, name
        assert info["stream"] == R.filtered_stream(img), name
        mode, px = R.pil_pixels(data)
        assert mode == R.PIL_MODE[img.shape[2]] and np.array_equal(px, img), name
    small = images["tri8_image"]
    assert np.array_equal(R.unfilter(R.filtered_stream(small), *small.shape), small)


def test_reader_is_strict():
    img = R.fixture_images()["tri8_image"]
    good = R.reference_png(img)
    R.read_png(good)
    for at in (0, 17, 30, len(good) - 20, len(good) - 14, len(good) - 1):  # signature, IHDR, IHDR CRC, Adler-32, IDAT CRC, IEND CRC
        bad = bytearray(good)
        bad[at] ^= 0x01
        with pytest.raises(R.PngError):
            R.read_png(bytes(bad))
    with pytest.raises(R.PngError):
        R.read_png(good[:-12])
    with pytest.raises(R.PngError):
        R.read_png(good + b"\x00")


def test_bitstream_restatement_inflates(images):
    s = _lib.PNG_SEGMENT_BYTES
    for name in ("tri8_image", "soup_image", "pncc_image"):
        data, kinds = R.png_file(images[name], s)
        info = R.read_png(data)
        assert info["stream"] == R.filtered_stream(images[name]), name
        assert len(info["idat"]) == len(kinds) + 2 and info["idat"][0] == b"\x78\x01", name
        assert np.array_equal(R.pil_pixels(data)[1], images[name]), name
    rng = np.random.default_rng(5)
    noise = rng.integers(0, 256, 3 * s + 5, dtype=np.uint8).tobytes()
    assert [k for _, k in R.segment_payloads(noise, 4, s)][:3] == [0, 0, 0]  # stored; the five bytes behind them are cheaper as a fixed block
    for data in (noise, bytes(s + 2), bytes(1), b"ab" * 300, bytes(rng.integers(0, 3, 2 * s, dtype=np.uint8))):
        assert zlib.decompress(R.zlib_stream(data, _lib.ZLIB_SECOND_DISTANCE, s)) == data


# ---------------------------------------------------------------------------------------------------------------------------
# dad3d_deflate_tables_host
# ---------------------------------------------------------------------------------------------------------------------------
def kraft(lengths):
    used = [int(x) for x in lengths if x]
    return sum(2.0 ** -x for x in used), len(used)


def canonical(lengths):
    """RFC 1951 3.2.2."""
    lengths = [int(x) for x in lengths]
    count = [0] * 17
    for x in lengths:
        count[x] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = []
    for x in lengths:
        out.append(nxt[x] if x else 0)
        nxt[x] += 1 if x else 0
    return out


def check_tables(ll_hist, d_hist, rng):
    t = R.tables(ll_hist, d_hist)
    for key, hist, limit in (("ll", ll_hist, 15), ("d", d_hist, 15), ("cl", None, 7)):
        lengths = t[key + "_len"]
        assert lengths.max() <= limit, (key, lengths)
        total, used = kraft(lengths)
        if hist is not None:
            assert np.array_equal(lengths > 0, np.asarray(hist) > 0), key  # a code for every used symbol and for no other
        assert total <= 1.0, (key, total)
        if used >= 2:
            assert total == 1.0, (key, total, lengths)
        if used == 1:
            assert lengths.max() == 1, key
        assert t[key + "_code"].tolist() == canonical(lengths), key
    # the cost the block type is chosen by
    ll_extra = np.array([R.LENGTH_EXTRA[s - 257] if s >= 257 else 0 for s in range(286)])
    want = t["header_bits"] + int((np.asarray(ll_hist, np.int64) * (t["ll_len"] + ll_extra)).sum()) + sum(
        int(d_hist[s]) * (int(t["d_len"][s]) + (0 if s < 4 else s // 2 - 1)) for s in range(30))
    assert t["dynamic_bits"] == want
    # a block of the header and a seeded symbol sequence inflates to that sequence
    lits = [s for s in range(256) if ll_hist[s]]
    lens = [s for s in range(257, 286) if ll_hist[s]]
    dists = [s for s in range(30) if d_hist[s]]
    acc, pos = int.from_bytes(t["header"].tobytes(), "little"), t["header_bits"]
    assert acc >> pos == 0 and acc & 7 == 4
    expect = bytearray(b"\x07" * 40000 if dists else b"")  # history for the distances: a preset dictionary's worth of bytes
    prefix = bytes(expect)
    symbols = []
    for _ in range(60):
        if lens and dists and rng.random() < 0.4:
            symbols.append((lens[rng.integers(len(lens))], dists[rng.integers(len(dists))]))
        elif lits:
            symbols.append((lits[rng.integers(len(lits))],))
    for sym in symbols:
        code, n = int(t["ll_code"][sym[0]]), int(t["ll_len"][sym[0]])
        acc |= R.reverse_bits(code, n) << pos
        pos += n
        if len(sym) == 1:
            expect.append(sym[0])
            continue
        i = sym[0] - 257
        eb, extra = R.LENGTH_EXTRA[i], 0
        if eb:
            extra = int(rng.integers(1 << eb))
            acc |= extra << pos
            pos += eb
        length = R.LENGTH_BASE[i] + extra
        d = sym[1]
        code, n = int(t["d_code"][d]), int(t["d_len"][d])
        acc |= R.reverse_bits(code, n) << pos
        pos += n
        deb = 0 if d < 4 else d // 2 - 1
        dbase = d + 1 if d < 4 else (2 + (d & 1)) * (1 << deb) + 1
        dextra = int(rng.integers(1 << deb)) if deb else 0
        if deb:
            acc |= dextra << pos
            pos += deb
        dist = dbase + dextra
        for _ in range(length):
            expect.append(expect[-dist])
    code, n = int(t["ll_code"][256]), int(t["ll_len"][256])
    acc |= R.reverse_bits(code, n) << pos
    pos += n
    acc |= 3 << pos  # the empty final fixed block: 1, 01, then seven zero bits
    pos += 10
    raw = acc.to_bytes((pos + 7) // 8, "little")
    # the history in front: a stored block of the prefix (32 768 bytes is the window, 40 000 spans it)
    front = b""
    for lo in range(0, len(prefix), 65535):
        part = prefix[lo:lo + 65535]
        front += b"\x00" + len(part).to_bytes(2, "little") + (len(part) ^ 0xFFFF).to_bytes(2, "little") + part
    inflater = zlib.decompressobj(-15)
    got = inflater.decompress(front + raw) + inflater.flush()
    assert inflater.eof
    assert got == bytes(expect)
    return t


def seeded_histograms():
    rng = np.random.default_rng(20260101)
    cases = []

    def hist(ll, d):
        ll = np.asarray(ll, dtype=np.uint32).copy()
        ll[256] = max(int(ll[256]), 1)
        cases.append((ll, np.asarray(d, dtype=np.uint32)))

    fib = [1, 1]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    for trial in range(2400):
        kind = trial % 8
        ll, d = np.zeros(286, np.int64), np.zeros(30, np.int64)
        n_d = (0, 1, 2, int(rng.integers(3, 31)))[trial % 4]  # zero, one, two and more used distance codes
        d_syms = rng.choice(30, n_d, replace=False)
        if kind == 0:  # uniform over a random subset
            syms = rng.choice(286, int(rng.integers(2, 287)), replace=False)
            ll[syms] = rng.integers(1, 50)
            d[d_syms] = rng.integers(1, 50)
        elif kind == 1:  # geometric
            syms = rng.choice(286, int(rng.integers(2, 287)), replace=False)
            ll[syms] = rng.geometric(rng.uniform(0.002, 0.5), len(syms))
            d[d_syms] = rng.geometric(0.05, n_d)
        elif kind == 2:  # Fibonacci weights on 18..29 symbols: an unlimited code would be 17..28 bits deep
            k = int(rng.integers(18, 30))
            ll[rng.choice(286, k, replace=False)] = fib[:k]
            if n_d >= 18:
                d[d_syms[:n_d]] = fib[:n_d]
            else:
                d[d_syms] = rng.integers(1, 9, n_d)
        elif kind == 3:  # one used literal and the end of block
            ll[int(rng.integers(256))] = int(rng.integers(1, 9000))
            d[:] = 0
            n_d = 0
        elif kind == 4:  # uniform over everything: long runs of equal lengths in the header
            ll[:] = int(rng.integers(1, 100))
            d[d_syms] = int(rng.integers(1, 100))
        elif kind == 5:  # lengths whose code-length histogram is Fibonacci-like: the code-length code wants more than 7 bits
            groups = rng.permutation(np.arange(1, 15))
            at = 0
            for i, g in enumerate(groups[:12]):
                count = fib[i] if at + fib[i] <= 286 else 0
                ll[at:at + count] = 1 << int(g)
                at += count
            ll = ll[rng.permutation(286)]  # scattered: few runs for the repeat symbols to absorb
            d[d_syms] = rng.integers(1, 1 << 12, n_d)
        elif kind == 6:  # sparse: a few symbols far apart, runs of zero lengths of every size
            syms = rng.choice(286, int(rng.integers(2, 12)), replace=False)
            ll[syms] = rng.integers(1, 5000, len(syms))
            d[d_syms] = rng.integers(1, 5000, n_d)
        else:  # what a filtered image gives: two-sided geometric around zero, a few matches
            v = np.round(rng.laplace(0, rng.uniform(0.5, 20), 8192)).astype(np.int64) & 255
            ll[:256] = np.bincount(v, minlength=256)
            ll[257 + rng.integers(0, 29, 5)] += rng.integers(1, 40, 5)
            d[d_syms[:4] % 4] = rng.integers(1, 40, min(n_d, 4))
        hist(ll, d)
    return cases


def test_deflate_tables_fuzz():
    rng = np.random.default_rng(7)
    cases = seeded_histograms()
    assert len(cases) >= 2000
    deep = limited_cl = one_lit = 0
    n_dist = set()
    for ll, d in cases:
        t = check_tables(ll, d, rng)
        deep += int(t["ll_len"].max() == 15)
        limited_cl += int(t["cl_len"].max() == 7)
        one_lit += int((ll > 0).sum() == 2)
        n_dist.add(min(int((d > 0).sum()), 3))
    assert deep >= 100 and limited_cl >= 50 and one_lit >= 100 and n_dist == {0, 1, 2, 3}, (deep, limited_cl, one_lit, n_dist)


def test_deflate_tables_match_an_unlimited_huffman_code_when_none_is_deeper_than_the_limit():
    """Where no code needs clamping the lengths are a minimum-redundancy code: the same total as heapq's Huffman."""
    import heapq

    rng = np.random.default_rng(11)
    for _ in range(200):
        ll = np.zeros(286, np.uint32)
        syms = rng.choice(286, int(rng.integers(2, 200)), replace=False)
        ll[syms] = rng.integers(1, 200, len(syms))
        ll[256] = max(int(ll[256]), 1)
        t = R.tables(ll, np.zeros(30, np.uint32))
        heap = [(int(c), i, (i,)) for i, c in enumerate(ll) if c]
        depth = dict.fromkeys([i for _, i, _ in heap], 0)
        heapq.heapify(heap)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for s in a[2] + b[2]:
                depth[s] += 1
            heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
        if max(depth.values()) <= 15:
            assert int((ll.astype(np.int64) * t["ll_len"]).sum()) == sum(int(ll[s]) * k for s, k in depth.items())


def test_deflate_tables_host_validates():
    lib = _lib.load()
    ll = np.zeros(286, np.uint32)
    ll[256] = 1
    assert lib.dad3d_deflate_tables_host(ll.ctypes.data, *([None] * 11)) == _lib.E_INVALID
    assert b"null" in lib.dad3d_last_error()
    big = ll.copy()
    big[0] = 1 << 22
    with pytest.raises(_lib.Dad3dError, match="count"):
        R.tables(big, np.zeros(30, np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------
# C ABI: validation before any device work
# ---------------------------------------------------------------------------------------------------------------------------
def test_size_queries():
    lib = _lib.load()
    s = _lib.PNG_SEGMENT_BYTES
    assert lib.dad3d_png_max_bytes(256, 256, 3) == 47 + 256 * 769 + 22 * 25 + 30
    assert lib.dad3d_png_max_bytes(1, 1, 1) == 47 + 2 + 22 + 30
    assert lib.dad3d_zlib_max_bytes(s) == 2 + s + 10 + 6 and lib.dad3d_zlib_max_bytes(s + 1) == 2 + s + 1 + 20 + 6
    for bad in ((0, 4, 3), (4, 0, 3), (4, 4, 0), (4, 4, 5), (-1, 4, 3), (1 << 15, 1 << 15, 2)):
        assert lib.dad3d_png_max_bytes(*bad) == 0, bad
        assert lib.dad3d_png_scratch_bytes(1, *bad) == 0, bad
    assert lib.dad3d_png_scratch_bytes(0, 4, 4, 3) == 0 and lib.dad3d_png_scratch_bytes(2, 4, 4, 3) > 0
    assert lib.dad3d_zlib_max_bytes(0) == 0 and lib.dad3d_zlib_max_bytes(1 << 31) == 0 and lib.dad3d_zlib_scratch_bytes(0, 5) == 0
    assert lib.dad3d_png_scratch_bytes(3, 8, 8, 3) >= 3 * (8 * 25 + s)


def test_png_encode_validates_before_device_work():
    lib = _lib.load()
    a = 0x1000  # an aligned non-null address: never dereferenced, every call fails validation first
    stride = (lib.dad3d_png_max_bytes(8, 8, 3) + 15) // 16 * 16
    need = lib.dad3d_png_scratch_bytes(2, 8, 8, 3)

    def call(images=a, batch=2, h=8, w=8, c=3, out=a, out_stride=stride, lengths=a, flags=a, scratch=a, scratch_bytes=need):
        return lib.dad3d_png_encode(images, batch, h, w, c, out, out_stride, lengths, flags, scratch, scratch_bytes, 0, None)

    cases = [(dict(images=None), b"null"), (dict(out=None), b"null"), (dict(lengths=None), b"null"), (dict(flags=None), b"null"),
             (dict(scratch=None), b"null"), (dict(c=0), b"channels"), (dict(c=5), b"channels"), (dict(h=0), b"image of"),
             (dict(w=-3), b"image of"), (dict(out_stride=stride - 16), b"out_stride"), (dict(out_stride=stride + 8), b"aligned"),
             (dict(out=a + 4), b"aligned"), (dict(scratch_bytes=need - 1), b"scratch"), (dict(batch=0), b"batch"),
             (dict(batch=65536), b"batch"), (dict(h=1 << 15, w=1 << 15, c=2, out_stride=1 << 40), b"2^31")]
    for kwargs, word in cases:
        lib.dad3d_clear_error()
        assert call(**kwargs) == _lib.E_INVALID, kwargs
        assert word in lib.dad3d_last_error(), (kwargs, lib.dad3d_last_error())


def test_zlib_compress_validates_before_device_work():
    lib = _lib.load()
    a = 0x1000
    stride = (lib.dad3d_zlib_max_bytes(100) + 15) // 16 * 16
    need = lib.dad3d_zlib_scratch_bytes(2, 100)

    def call(data=a, batch=2, n=100, out=a, out_stride=stride, lengths=a, flags=a, scratch=a, scratch_bytes=need):
        return lib.dad3d_zlib_compress(data, batch, n, out, out_stride, lengths, flags, scratch, scratch_bytes, 0, None)

    for kwargs, word in [(dict(data=None), b"null"), (dict(n=0), b"stream of"), (dict(n=1 << 31), b"stream of"), (dict(batch=0), b"batch"),
                         (dict(out_stride=stride - 16), b"out_stride"), (dict(scratch_bytes=0), b"scratch"), (dict(lengths=a + 4), b"misaligned")]:
        lib.dad3d_clear_error()
        assert call(**kwargs) == _lib.E_INVALID, kwargs
        assert word in lib.dad3d_last_error(), (kwargs, lib.dad3d_last_error())


def test_image_saver_writes_a_numpy_image(tmp_path, images):
    saver = writers.ImageSaver()
    assert saver.extension == ".png"
    for name in ("head_image", "soup_image"):
        path = str(tmp_path / (name + saver.extension))
        saver(images[name], path)
        data = open(path, "rb").read()
        info = R.read_png(data)
        assert (info["height"], info["width"], info["channels"]) == images[name].shape
        assert np.array_equal(R.pil_pixels(data)[1], images[name])  # the array's own channel order
    grey = images["head_image"][:, :, 0]
    saver(grey, str(tmp_path / "grey.png"))
    assert np.array_equal(R.pil_pixels(open(tmp_path / "grey.png", "rb").read())[1][:, :, 0], grey)
    with pytest.raises(ValueError, match="image"):
        saver(images["head_image"].astype(np.float32), str(tmp_path / "bad.png"))


def test_host_paths_of_the_batch_calls(tmp_path, images):
    batch = np.stack([images["head_image"], images["pncc_image"]])
    files = writers.png_batch(batch)
    assert [np.array_equal(R.pil_pixels(f)[1], img) for f, img in zip(files, batch)] == [True, True]
    paths = [str(tmp_path / f"{i}.png") for i in range(2)]
    writers.save_png_batch(batch, paths)
    assert [open(p, "rb").read() for p in paths] == files
    with pytest.raises(ValueError, match="encoder"):
        writers.save_png_batch(batch, paths, encoder="gpu")
