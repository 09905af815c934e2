"""GPU: the PNG encoder (csrc/png_encode.hip, writers.PngEncoder) and its deflate on plain byte rows (writers.zlib_compress_batch),
DESIGN.md 4.15. A file must pass the strict reader of tests/png_restatement.py (every CRC, the Adler-32 through zlib's inflate),
inflate to the restated filtered stream byte for byte -- filter types included -- and decode with PIL to the input pixels; and its
bytes are those of the CPU bitstream restatement of the encoder, which shares nothing with the kernels but the table routine."""
import zlib

import numpy as np
import pytest
import torch

import png_restatement as R
from dad_3dheads_amd import _lib, writers

pytestmark = pytest.mark.gpu
S = _lib.PNG_SEGMENT_BYTES
GUARD = 0x23
# file bytes against zlib level 1 on the same filtered stream. The CPU bitstream restatement of this parse is at most
# 1.062 x zlib level 1 on the fixture images (the photo), + 5 %; the chunk framing zlib does not have is added apart.
SIZE_MARGIN = 1.062 + 0.05


@pytest.fixture(scope="module")
def images():
    return R.fixture_images()


@pytest.fixture(scope="module")
def expected(images):
    """{name: (the restatement's file, kinds of its segments)}: computed once."""
    return {name: R.png_file(img, S) for name, img in images.items()}


def capi_png(batch):
    """dad3d_png_encode on uint8 [B,H,W,C] -> (files, lengths, flags), straight through ctypes; checks the guard bytes."""
    lib = _lib.load()
    b, h, w, c = batch.shape
    dev = torch.from_numpy(np.ascontiguousarray(batch)).cuda()
    stride = (lib.dad3d_png_max_bytes(h, w, c) + 15) // 16 * 16
    out = torch.full((b, stride), GUARD, dtype=torch.uint8, device="cuda")
    lengths = torch.full((b,), -1, dtype=torch.int64, device="cuda")
    flags = torch.full((b,), -1, dtype=torch.int32, device="cuda")
    nbytes = lib.dad3d_png_scratch_bytes(b, h, w, c)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _lib.check(lib.dad3d_png_encode(dev.data_ptr(), b, h, w, c, out.data_ptr(), stride, lengths.data_ptr(), flags.data_ptr(),
                                    scratch.data_ptr(), nbytes, 0, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    host, ln, fl = out.cpu().numpy(), lengths.cpu().numpy(), flags.cpu().numpy()
    return host, ln, fl


def files_of(host, ln, fl):
    assert fl.tolist() == [0] * len(fl)  # first: a host fallback must not be able to hide a kernel fault
    for i in range(len(ln)):
        assert 0 < ln[i] <= host.shape[1], i
        assert (host[i, ln[i]:] == GUARD).all(), i  # nothing behind a file is touched
    return [host[i, :ln[i]].tobytes() for i in range(len(ln))]


def capi_zlib(rows):
    lib = _lib.load()
    b, n = rows.shape
    dev = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    stride = (lib.dad3d_zlib_max_bytes(n) + 15) // 16 * 16
    out = torch.full((b, stride), GUARD, dtype=torch.uint8, device="cuda")
    lengths = torch.full((b,), -1, dtype=torch.int64, device="cuda")
    flags = torch.full((b,), -1, dtype=torch.int32, device="cuda")
    nbytes = lib.dad3d_zlib_scratch_bytes(b, n)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _lib.check(lib.dad3d_zlib_compress(dev.data_ptr(), b, n, out.data_ptr(), stride, lengths.data_ptr(), flags.data_ptr(),
                                       scratch.data_ptr(), nbytes, 0, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return files_of(out.cpu().numpy(), lengths.cpu().numpy(), flags.cpu().numpy())


def check_file(data, img, want=None):
    info = R.read_png(data)
    assert (info["height"], info["width"], info["channels"]) == img.shape
    stream = R.filtered_stream(img)
    if info["stream"] != stream:
        rb = 1 + img.shape[1] * img.shape[2]
        got_types = [info["stream"][y * rb] for y in range(img.shape[0])]
        assert got_types == [stream[y * rb] for y in range(img.shape[0])], "filter types"
        assert info["stream"] == stream
    assert info["idat"][0] == b"\x78\x01" and info["idat"][-1][:2] == b"\x03\x00" and len(info["idat"]) == 2 + -(-len(stream) // S)
    for payload in info["idat"][1:-1]:
        assert payload[-4:] == b"\x00\x00\xff\xff"  # every segment ends on a byte
    mode, px = R.pil_pixels(data)
    assert mode == R.PIL_MODE[img.shape[2]]
    assert np.array_equal(px, img)
    if want is not None:
        assert data == want


def test_fixtures_through_the_c_abi(images, expected):
    for name, img in images.items():
        (data,) = files_of(*capi_png(img[None]))
        check_file(data, img, expected[name][0])


def seeded_image(h, w, c, seed):
    """Smooth ramps, flat runs and some noise: rows that pick different filters, matches at both distances."""
    rng = np.random.default_rng(seed)
    y, x, ch = np.meshgrid(np.arange(h), np.arange(w), np.arange(c), indexing="ij")
    img = (3 * x + 5 * y + 40 * ch) % 256
    img[:, w // 3: w // 2] = 77
    noisy = rng.random((h, w, 1)) < 0.1
    img = np.where(noisy, rng.integers(0, 256, (h, w, c)), img)
    return img.astype(np.uint8)


SHAPES = [(1, 1, 1), (1, 1, 2), (1, 1, 3), (1, 1, 4), (2, 3, 2), (8, 8, 3),
          (1, S - 2, 1), (8, S // 8 - 1, 1), (1, S, 1),  # L = S - 1, S, S + 1
          (5, 700, 4),  # rows of 2801 bytes across the boundaries at 8192
          (3, S + 100, 1)]  # a row longer than a segment


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes(shape):
    h, w, c = shape
    if (h, c) == (8, 1):
        assert h * (1 + w * c) == S
    batch = np.stack([seeded_image(h, w, c, 1), seeded_image(h, w, c, 2)[::-1].copy()])
    files = files_of(*capi_png(batch))
    for data, img in zip(files, batch):
        check_file(data, img, R.png_file(img, S)[0])


def test_all_zero_and_noise_images():
    rng = np.random.default_rng(9)
    zero = np.zeros((64, 67, 3), np.uint8)
    noise = rng.integers(0, 256, (64, 67, 3), dtype=np.uint8)
    files = files_of(*capi_png(np.stack([zero, noise])))
    check_file(files[0], zero, R.png_file(zero, S)[0])
    check_file(files[1], noise, R.png_file(noise, S)[0])
    n = 64 * (1 + 67 * 3)
    nseg = -(-n // S)
    assert len(files[0]) < 77 + 22 * nseg + 64 * nseg  # a segment of zeros is a handful of maximal matches
    assert len(files[1]) <= n + 77 + 22 * nseg  # the stored path: the stream, the block and chunk words, nothing more


ZERO_LENGTHS = [1, 2, 3, 4, 257, 258, 259, 260, 261, 516, 517, S, S + 1, S + 2]


def test_zlib_zeros():
    """Remainders of 1 and 2 behind a maximal match, segment tails shorter than a match."""
    for n in ZERO_LENGTHS:
        rows = np.zeros((2, n), np.uint8)
        rows[1, n // 2] = 1 if n > 4 else 0
        for got, row in zip(capi_zlib(rows), rows):
            assert zlib.decompress(got) == row.tobytes(), n
            assert got == R.zlib_stream(row.tobytes(), _lib.ZLIB_SECOND_DISTANCE, S), n


def seeded_streams():
    """64 lengths in 1..3S x 4 kinds of content = 256 streams, grouped by length (the C ABI compresses rows of one length)."""
    rng = np.random.default_rng(2026)
    lengths = [1, 2, 5, S - 1, S, S + 1, 2 * S, 2 * S + 1, 3 * S - 1, 3 * S] + [int(v) for v in rng.integers(1, 3 * S + 1, 54)]
    fib = np.array([1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181, 6765], dtype=np.float64)
    out = []
    for i, n in enumerate(lengths):
        rows = np.zeros((4, n), np.uint8)
        rows[0] = rng.integers(0, 256, n)  # uniform noise
        rows[1] = np.minimum(rng.geometric(rng.uniform(0.05, 0.6), n) - 1, 255)  # geometric
        rows[2] = rng.choice(len(fib), n, p=fib / fib.sum()) * 11  # Fibonacci-weighted: a deep code
        rows[3] = rng.integers(0, 1 + i % 2, n) * 200 + 3  # a one- or two-symbol alphabet
        out.append(rows)
    return out


def test_zlib_seeded_streams():
    total = 0
    for i, rows in enumerate(seeded_streams()):
        got = capi_zlib(rows)
        for k in range(4):
            assert zlib.decompress(got[k]) == rows[k].tobytes(), (rows.shape, k)
        if i % 8 == 0:  # and the restatement's bytes, for every eighth length
            for k in range(4):
                assert got[k] == R.zlib_stream(rows[k].tobytes(), _lib.ZLIB_SECOND_DISTANCE, S), (rows.shape, k)
        total += 4
    assert total == 256


def test_zlib_compress_batch(images):
    rows = torch.from_numpy(np.stack([np.frombuffer(R.filtered_stream(images["soup_image"]), np.uint8)] * 3).copy()).cuda()
    rows[1] = 0
    got = writers.zlib_compress_batch(rows)
    assert [zlib.decompress(g) for g in got] == [r.cpu().numpy().tobytes() for r in rows]
    assert len(got[1]) < 200 and got[0] == got[2]
    assert writers.zlib_compress_batch(rows[:0]) == []
    for bad in (rows.cpu(), rows.int(), rows[:, ::2], rows[0]):
        with pytest.raises(ValueError, match="data"):
            writers.zlib_compress_batch(bad)


def test_batch_invariance(images, expected):
    names = ["head_image", "pncc_image", "texture0"]
    alone = {n: expected[n][0] for n in names}
    three = np.stack([images[n] for n in names])
    assert files_of(*capi_png(three)) == [alone[n] for n in names]
    rng = np.random.default_rng(4)
    order = [names[i] for i in rng.integers(0, 3, 64)]
    many = np.stack([images[n] for n in order])
    first = files_of(*capi_png(many))
    assert first == [alone[n] for n in order]
    assert files_of(*capi_png(many)) == first  # deterministic


def test_size_against_zlib_level_1(images):
    ratios = {}
    for name, img in images.items():
        (data,) = files_of(*capi_png(img[None]))
        stream = R.filtered_stream(img)
        z1 = len(zlib.compress(stream, 1))
        nseg = -(-len(stream) // S)
        ratios[name] = len(data) / z1
        print(f"{name}: {len(data)} bytes, zlib level 1 {z1}, ratio {ratios[name]:.3f}")
        assert len(data) <= SIZE_MARGIN * z1 + 77 + 12 * nseg, (name, len(data), z1)
    assert ratios["head_image"] <= 1.2 and ratios["pncc_image"] <= 1.2, ratios


@pytest.fixture()
def host_calls(monkeypatch):
    """Counts the calls of the host encoder: the GPU path must take none for an unflagged image."""
    calls = []
    real = writers._png_host

    def counted(image):
        calls.append(np.asarray(image).shape)
        return real(image)

    monkeypatch.setattr(writers, "_png_host", counted)
    return calls


def test_save_png_batch_of_a_cuda_batch(tmp_path, images, expected, host_calls):
    names = ["head_image", "pncc_image", "texture0", "head_image"]
    batch = torch.from_numpy(np.stack([images[n] for n in names])).cuda()
    paths = [str(tmp_path / f"{i}.png") for i in range(4)]
    writers.save_png_batch(batch, paths)
    assert host_calls == []
    for path, name in zip(paths, names):
        data = open(path, "rb").read()
        assert data == expected[name][0]
        assert np.array_equal(R.pil_pixels(data)[1], images[name])
    assert writers.png_batch(batch) == [expected[n][0] for n in names] and host_calls == []
    writers.save_png_batch(batch, paths, encoder="host")
    assert len(host_calls) == 4
    writers.save_png_batch(batch.cpu().numpy(), paths)
    assert len(host_calls) == 8
    assert np.array_equal(R.pil_pixels(open(paths[2], "rb").read())[1], images["texture0"])
    assert writers.png_batch(batch[:0]) == []


def test_flagged_item_falls_back_to_the_host(images, expected, host_calls):
    enc = writers.PngEncoder(256, 256, 3, device=0)
    batch = torch.from_numpy(np.stack([images["head_image"], images["pncc_image"], images["texture0"]])).cuda()
    data = enc.encode(batch)
    torch.cuda.synchronize()
    assert data.flags.cpu().tolist() == [0, 0, 0] and data.batch == 3 and enc.stride % 16 == 0
    assert [bytes(x) for x in data.to_host()] == [expected[n][0] for n in ("head_image", "pncc_image", "texture0")]
    assert host_calls == []
    flagged = enc.encode(batch, extra_flags=torch.tensor([0, 1, 0], dtype=torch.int32, device="cuda"))
    files = [bytes(x) for x in flagged.to_host()]
    assert host_calls == [(256, 256, 3)]  # that item alone
    assert files[0] == expected["head_image"][0] and files[2] == expected["texture0"][0]
    assert files[1] != expected["pncc_image"][0] and np.array_equal(R.pil_pixels(files[1])[1], images["pncc_image"])


def test_encoder_refuses_what_the_kernel_cannot_read(images):
    enc = writers.PngEncoder(48, 64, 4, device=0)
    good = torch.from_numpy(images["soup_image"][None].copy()).cuda()
    enc.encode(good)
    strided = good.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    assert not strided.is_contiguous()
    for bad in (strided, good.float(), good.cpu(), good[:, :, :, :3], good[0], good.cpu().numpy()):
        with pytest.raises(ValueError, match="images"):
            enc.encode(bad)
    with pytest.raises(ValueError, match="PngEncoder"):
        writers.PngEncoder(4, 4, 5, device=0)


def test_graph_replay_gives_the_same_files(images, expected):
    enc = writers.PngEncoder(256, 256, 3, device=0)
    enc.reserve(2)
    src = torch.zeros((2, 256, 256, 3), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        enc.encode(src)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        data = enc.encode(src)  # no allocation, no sync: capturable
    src.copy_(torch.from_numpy(np.stack([images["head_image"], images["pncc_image"]])).cuda())
    graph.replay()
    torch.cuda.synchronize()
    assert [bytes(x) for x in data.to_host()] == [expected["head_image"][0], expected["pncc_image"][0]]
