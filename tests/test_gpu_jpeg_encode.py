"""GPU: the JPEG encoder (csrc/jpeg_encode.hip, writers.JpegEncoder), DESIGN.md 4.20. The device's files are, byte for byte, those of
the CPU restatement (tests/jpeg_encode_restatement.py) and of PIL, with every flag zero -- a host fallback must never be what makes a
case pass -- and nothing behind a file touched. Small shapes, chosen where the kernels can go wrong: a batch past 64 images, a scan
of several chunks of 256 blocks with and without restart intervals, intervals that end at, in front of and behind chunk borders and
the last MCU, dummy blocks, the longest and the shortest scans side by side."""
import numpy as np
import pytest
import torch

import jpeg_encode_restatement as R
from jpeg_cases import pil_array
from jpeg_encode_cases import corpus, corpus_pil, corpus_restated, image, interval_of, pil_bytes
from dad_3dheads_amd import _lib, jpeg_reader, writers

pytestmark = pytest.mark.gpu
GUARD = 0x23


def capi_jpeg(batch, quality=75, subsampling=None, restart_marker_rows=0, restart_marker_blocks=0):
    """dad3d_jpeg_encode on uint8 [B,H,W,C] straight through ctypes -> the files; the flags must be zero and the bytes behind a file
    as they were."""
    lib = _lib.load()
    b, h, w, c = batch.shape
    options = {"subsampling": subsampling, "restart_marker_rows": restart_marker_rows, "restart_marker_blocks": restart_marker_blocks}
    sub = (2 if subsampling is None else subsampling) if c == 3 else 0
    dev = torch.from_numpy(np.ascontiguousarray(batch)).cuda()
    stride = (lib.dad3d_jpeg_max_bytes(h, w, c, sub) + 15) // 16 * 16
    out = torch.full((b, stride), GUARD, dtype=torch.uint8, device="cuda")
    lengths = torch.full((b,), -1, dtype=torch.int64, device="cuda")
    flags = torch.full((b,), -1, dtype=torch.int32, device="cuda")
    nbytes = lib.dad3d_jpeg_encode_scratch_bytes(b, h, w, c, sub)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _lib.check(lib.dad3d_jpeg_encode(dev.data_ptr(), b, h, w, c, quality, sub, interval_of(batch[0], options), out.data_ptr(), stride,
                                     lengths.data_ptr(), flags.data_ptr(), scratch.data_ptr(), nbytes, 0,
                                     torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    host, ln, fl = out.cpu().numpy(), lengths.cpu().numpy(), flags.cpu().numpy()
    assert fl.tolist() == [0] * b  # first: a host fallback must not be able to hide a kernel fault
    for i in range(b):
        assert 0 < ln[i] <= stride, i
        assert (host[i, ln[i]:] == GUARD).all(), i
    return [host[i, :ln[i]].tobytes() for i in range(b)]


def test_corpus_through_the_c_abi():
    for (name, img, options), pil, restated in zip(corpus(), corpus_pil(), corpus_restated()):
        (got,) = capi_jpeg(img[None], **options)
        assert got == restated, name
        assert got == pil, name


def test_batch_of_65_images():
    """Past one wave of images, and past 64 workgroups of the packing kernel."""
    batch = np.stack([image(17, 15, 3, k, ("noise", "ramp", "flat")[k % 3]) for k in range(65)])
    got = capi_jpeg(batch, quality=75, subsampling=2, restart_marker_rows=1)
    for k in range(65):
        assert got[k] == pil_bytes(batch[k], quality=75, subsampling=2, restart_marker_rows=1), k
    for k in (0, 1, 2, 63, 64):
        assert got[k] == R.encode(batch[k], 75, 2, 1), k


@pytest.fixture(scope="module")
def square():
    """136 x 136 at 4:4:4: 17 x 17 x 3 = 867 blocks, four chunks of the packing kernel; an interval of a row is 51 blocks, so intervals
    end in front of, at no and behind chunk borders (256 = 5 x 51 + 1)."""
    return np.stack([image(136, 136, 3, 1, "noise"), image(136, 136, 3, 2, "ramp")])


@pytest.mark.parametrize("rows", [0, 1])
def test_a_scan_of_several_chunks(square, rows):
    got = capi_jpeg(square, quality=90, subsampling=0, restart_marker_rows=rows)
    for k in range(2):
        assert got[k] == R.encode(square[k], 90, 0, rows), k
        assert got[k] == pil_bytes(square[k], quality=90, subsampling=0, restart_marker_rows=rows), k


def test_intervals_against_chunk_borders_and_the_last_mcu():
    """Grey 128 x 136: 16 rows of 17 MCUs of one block, 272 blocks, two chunks. 17: PIL's row, and 16: the last interval ends at the
    last MCU; 255 / 256 / 257: the marker in lane 254, in the chunk's last lane, in the next chunk's first; 271, 272, 300: a last
    interval of one MCU, none, an interval longer than the scan; 1: a marker behind every block."""
    img = image(128, 136, 1, 3, "noise")
    for blocks in (1, 16, 17, 255, 256, 257, 271, 272, 300):
        (got,) = capi_jpeg(img[None], quality=50, restart_marker_blocks=blocks)
        assert got == pil_bytes(img, quality=50, restart_marker_blocks=blocks), blocks
    (got,) = capi_jpeg(img[None], quality=50, restart_marker_blocks=17)
    assert got == R.encode(img, 50, restart_marker_blocks=17)
    colour = image(33, 140, 3, 4, "ramp")  # 3 x 9 MCUs of 6 blocks: 162 blocks; 43 MCUs = 258 blocks would pass a chunk
    for blocks in (4, 9, 26, 27):
        (got,) = capi_jpeg(colour[None], quality=75, subsampling=2, restart_marker_blocks=blocks)
        assert got == pil_bytes(colour, quality=75, subsampling=2, restart_marker_blocks=blocks), blocks


def test_the_longest_and_the_shortest_scan_side_by_side():
    dense, flat = image(33, 31, 3, 5, "noise"), image(33, 31, 3, 0, "constant")
    batch = np.stack([dense, flat, dense[::-1].copy(), flat])
    for options in ({"quality": 100, "subsampling": 0}, {"quality": 100, "subsampling": 2, "restart_marker_rows": 1}):
        got = capi_jpeg(batch, **options)
        assert got == [R.encode(img, **options) for img in batch]
        assert got == [pil_bytes(img, **options) for img in batch]
        head = got[0].index(b"\xff\xda") + 14  # SOS of three components; the header is the same for all four
        assert got[0].count(b"\xff\x00") >= 10 and len(got[1]) - head < (len(got[0]) - head) // 8  # the scans: long and short


def test_graph_replay_gives_the_eager_files():
    enc = writers.JpegEncoder(40, 56, 3, quality=85, subsampling=1, restart_marker_rows=1, device=0)
    enc.reserve(2)
    first = torch.from_numpy(np.stack([image(40, 56, 3, 1, "noise"), image(40, 56, 3, 2, "ramp")])).cuda()
    second = torch.from_numpy(np.stack([image(40, 56, 3, 3, "flat"), image(40, 56, 3, 4, "noise")])).cuda()
    eager = []
    for pixels in (first, second):
        data = enc.encode(pixels)
        assert data.flags.cpu().tolist() == [0, 0]
        eager.append([bytes(x) for x in data.to_host()])
    src = torch.zeros_like(first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        enc.encode(src)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        data = enc.encode(src)  # no allocation, no sync: capturable
    for pixels, want in zip((first, second), eager):
        src.copy_(pixels)
        graph.replay()
        torch.cuda.synchronize()
        replayed = writers.JpegData(enc, src, 2)  # `data` remembers its first copy to the host: a fresh view of the same buffers
        assert replayed.text.data_ptr() == data.text.data_ptr() and replayed.flags.cpu().tolist() == [0, 0]
        assert [bytes(x) for x in replayed.to_host()] == want
    assert eager[0] == [pil_bytes(img, quality=85, subsampling=1, restart_marker_rows=1) for img in first.cpu().numpy()]


def test_round_trip_through_the_device_decoder():
    batch = np.stack([image(75, 131, 3, k, ("noise", "ramp", "flat")[k % 3]) for k in range(6)])
    decoder = jpeg_reader.JpegDecoder(0)
    for options in ({"quality": 90, "subsampling": 2, "restart_marker_rows": 1}, {"quality": 75, "subsampling": 0, "restart_marker_rows": 1},
                    {"quality": 75, "subsampling": 1}):
        files = capi_jpeg(batch, **options)
        got = decoder.decode(files)
        assert got.flags.tolist() == [0] * 6  # the device's own path, restart markers or none
        for t, f in zip(got.tensors(), files):
            assert np.array_equal(t.cpu().numpy(), pil_array(f))
    grey = batch[:, :, :, :1].copy()
    files = capi_jpeg(grey, quality=60, restart_marker_rows=1)
    got = decoder.decode(files)
    assert got.flags.tolist() == [0] * 6 and all(np.array_equal(t.cpu().numpy(), pil_array(f)) for t, f in zip(got.tensors(), files))


@pytest.fixture()
def host_calls(monkeypatch):
    """Counts the calls of the host encoder: the GPU path must take none for an unflagged image."""
    calls = []
    real = writers._jpeg_host

    def counted(image, **options):
        calls.append(np.asarray(image).shape)
        return real(image, **options)

    monkeypatch.setattr(writers, "_jpeg_host", counted)
    return calls


def test_save_jpeg_batch_of_a_cuda_batch(tmp_path, host_calls):
    pixels = np.stack([image(33, 47, 3, k, ("noise", "ramp", "flat")[k % 3]) for k in range(4)])
    batch = torch.from_numpy(pixels).cuda()
    paths = [str(tmp_path / f"{i}.jpg") for i in range(4)]
    for options in ({}, {"quality": 92, "subsampling": 0, "restart_marker_rows": 2}):
        want = [pil_bytes(img, **options) for img in pixels]
        writers.save_jpeg_batch(batch, paths, **options)
        assert host_calls == []
        assert [open(p, "rb").read() for p in paths] == want
        assert writers.jpeg_batch(batch, **options) == want and host_calls == []
    assert writers._jpeg_encoder_for(batch) is writers._jpeg_encoder_for(batch, quality=75, subsampling=2)  # one encoder per option set
    assert writers._jpeg_encoder_for(batch) is not writers._jpeg_encoder_for(batch, quality=76)
    grey = batch[:, :, :, :1].contiguous()
    assert writers.jpeg_batch(grey, quality=50) == [pil_bytes(img, quality=50) for img in pixels[:, :, :, :1]] and host_calls == []
    writers.save_jpeg_batch(batch, paths, encoder="host")
    assert len(host_calls) == 4
    assert writers.jpeg_batch(batch[:, :, ::2]) == [pil_bytes(img) for img in pixels[:, :, ::2]]  # not contiguous: the host path
    assert len(host_calls) == 8
    assert writers.jpeg_batch(batch[:0]) == []


def test_flagged_item_falls_back_to_the_host_with_the_same_bytes(host_calls):
    pixels = np.stack([image(24, 40, 3, k, "noise") for k in range(3)])
    enc = writers.JpegEncoder(24, 40, 3, quality=80, device=0)
    batch = torch.from_numpy(pixels).cuda()
    want = [pil_bytes(img, quality=80) for img in pixels]
    data = enc.encode(batch)
    assert data.flags.cpu().tolist() == [0, 0, 0] and enc.stride % 16 == 0 and (enc.subsampling, enc.restart_interval) == (2, 0)
    assert [bytes(x) for x in data.to_host()] == want and host_calls == []
    flagged = enc.encode(batch, extra_flags=torch.tensor([0, 1, 0], dtype=torch.int32, device="cuda"))
    assert [bytes(x) for x in flagged.to_host()] == want
    assert host_calls == [(24, 40, 3)]  # that item alone
    for bad in (batch.float(), batch.cpu(), batch[:, :, :, :1], batch[0], pixels, batch.permute(0, 2, 1, 3)):
        with pytest.raises(ValueError, match="images"):
            enc.encode(bad)
    with pytest.raises(ValueError, match="JPEG"):
        writers.JpegEncoder(8, 8, 4, device=0)
    with pytest.raises(ValueError, match="65535"):
        writers.JpegEncoder(8, 65535, 3, subsampling=0, restart_marker_rows=8, device=0)


def test_the_argument_contract():
    """Every invalid call returns DAD3D_E_INVALID before any device work: the output, lengths and flags stay as they were."""
    lib = _lib.load()
    h, w, c, sub, b = 16, 24, 3, 2, 2
    stride = (lib.dad3d_jpeg_max_bytes(h, w, c, sub) + 15) // 16 * 16
    nbytes = lib.dad3d_jpeg_encode_scratch_bytes(b, h, w, c, sub)
    dev = torch.zeros((b, h, w, c), dtype=torch.uint8, device="cuda")
    out = torch.full((b, stride + 16), GUARD, dtype=torch.uint8, device="cuda")
    lengths = torch.full((b + 1,), -1, dtype=torch.int64, device="cuda")
    flags = torch.full((b + 1,), -1, dtype=torch.int32, device="cuda")
    scratch = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
    good = dict(images=dev.data_ptr(), batch=b, h=h, w=w, c=c, quality=75, subsampling=sub, interval=0, out=out.data_ptr(), stride=stride,
                lengths=lengths.data_ptr(), flags=flags.data_ptr(), scratch=scratch.data_ptr(), scratch_bytes=nbytes)
    bad = [{"images": None}, {"out": None}, {"lengths": None}, {"flags": None}, {"scratch": None}, {"c": 2}, {"c": 4}, {"h": 0}, {"h": 65536},
           {"w": 0}, {"w": 65536}, {"batch": 0}, {"batch": 65536}, {"quality": 0}, {"quality": 101}, {"subsampling": -1}, {"subsampling": 3},
           {"interval": -1}, {"interval": 65536}, {"stride": stride - 16}, {"stride": stride + 8}, {"scratch_bytes": nbytes - 1},
           {"out": out.data_ptr() + 8}, {"scratch": scratch.data_ptr() + 8}, {"lengths": lengths.data_ptr() + 4}, {"flags": flags.data_ptr() + 2},
           {"subsampling": 0}]  # 4:4:4 needs more of both buffers than 4:2:0 was given
    for change in bad:
        a = {**good, **change}
        status = lib.dad3d_jpeg_encode(*a.values(), 0, torch.cuda.current_stream().cuda_stream)
        assert status == _lib.E_INVALID, change
    torch.cuda.synchronize()
    assert (out == GUARD).all() and (lengths == -1).all() and (flags == -1).all()  # nothing was launched
    assert lib.dad3d_jpeg_encode(*good.values(), 0, torch.cuda.current_stream().cuda_stream) == _lib.OK
    torch.cuda.synchronize()
    assert flags[:b].tolist() == [0, 0] and int(lengths[0]) == len(pil_bytes(np.zeros((h, w, c), np.uint8), quality=75, subsampling=2))
