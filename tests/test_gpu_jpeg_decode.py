"""GPU: baseline JPEG files read back on the device (csrc/jpeg_decode.hip, dad_3dheads_amd/jpeg_reader.py),
bit-equal to `PIL.Image.open`. Every case goes through the C ABI first, with guard bytes around every output and the flags asserted
before anything else (a host fallback must not be able to hide a kernel fault), then through `jpeg_reader`. The files come from
tests/jpeg_cases.py; tests/test_jpeg_host.py holds the same routines to PIL on a CPU, and the damaged files run here are only those
it shows dad3d_jpeg_decode_host to flag."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

from jpeg_cases import MALFORMED, UNSUPPORTED, demo_bytes, header_defects, host_decode, jpeg, pil_array, picture, refused
from dad_3dheads_amd import _lib, jpeg_reader

pytestmark = pytest.mark.gpu
GUARD = 0x23


def align(n):
    return (n + 15) // 16 * 16


def capi_jpeg(files, channels=None, pad=5, shapes=None):
    """dad3d_jpeg_decode -> (images or None per file, flags). Rows lie `pad` bytes apart; every byte between the rows and between
    the images must stay as it was."""
    lib = _lib.load()
    rows, at, out_at = [], 0, 0
    for i, f in enumerate(files):
        h, w, c = jpeg_reader._header(f) if shapes is None or shapes[i] is None else shapes[i]
        oc = c if channels is None else channels
        stride = w * oc + pad
        rows.append([at, len(f), h, w, c, out_at, stride, oc, 0, 0, 0, 0])
        at += align(len(f)) + 16
        out_at += align(h * stride) + 16
    desc = np.asarray(rows, dtype=np.int64)
    grid = np.zeros(_lib.JPEG_DECODE_GRID_INTS, dtype=np.int32)
    nbytes = lib.dad3d_jpeg_decode_scratch_bytes(desc.ctypes.data, len(rows), grid.ctypes.data)
    assert nbytes > 0
    data = np.full(at, 0xEE, dtype=np.uint8)
    for row, f in zip(rows, files):
        data[row[0]:row[0] + row[1]] = np.frombuffer(f, dtype=np.uint8)
    dev = torch.from_numpy(data).cuda()
    out = torch.full((out_at,), GUARD, dtype=torch.uint8, device="cuda")
    flags = torch.full((len(rows),), -1, dtype=torch.int32, device="cuda")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    desc_dev = torch.from_numpy(desc).cuda()
    _lib.check(lib.dad3d_jpeg_decode(dev.data_ptr(), at, desc_dev.data_ptr(), len(rows), grid.ctypes.data, out.data_ptr(), out_at,
                                     flags.data_ptr(), scratch.data_ptr(), nbytes, 0, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    host, fl = out.cpu().numpy(), flags.cpu().tolist()
    images = []
    for k, row in enumerate(rows):
        _, _, h, w, _, o, stride, oc = row[:8]
        end = rows[k + 1][5] if k + 1 < len(rows) else out_at
        block = host[o:o + h * stride].reshape(h, stride)
        assert (block[:, w * oc:] == GUARD).all() and (host[o + h * stride:end] == GUARD).all(), k
        images.append(block[:, :w * oc].reshape(h, w, oc).copy() if fl[k] == 0 else None)
    return images, fl


def decode_all(files, channels=None):
    """The C ABI and jpeg_reader on the same files, both equal to PIL with every flag 0."""
    images, flags = capi_jpeg(files, channels)
    assert flags == [0] * len(files)
    want = [pil_array(f, channels) for f in files]
    for k, (got, ref) in enumerate(zip(images, want)):
        assert got.shape == ref.shape and np.array_equal(got, ref), k
    res = jpeg_reader.JpegDecoder(0).decode(files, channels)
    assert res.flags.tolist() == [0] * len(files) and len(res) == len(files)
    assert res.shapes == [w.shape for w in want]
    for k, (got, ref) in enumerate(zip(res.tensors(), want)):
        assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), ref), k


def small_files():
    files = [jpeg(picture((1, 1, 3), 1), quality=90), jpeg(picture((1, 9, 3), 2), quality=90), jpeg(picture((9, 1, 3), 3), quality=90),
             jpeg(picture((8, 8, 3), 4), quality=90, subsampling=0)]
    for sub in (0, 1, 2):
        files.append(jpeg(picture((16, 16, 3), 10 + sub), quality=85, subsampling=sub))  # one MCU at 4:2:0
        files.append(jpeg(picture((17, 17, 3), 20 + sub, "ramp"), quality=85, subsampling=sub))  # and a pixel more
    for w in (1, 2, 3, 4):
        files.append(jpeg(picture((11, w, 3), 30 + w), quality=90, subsampling=2))  # chroma of two samples or fewer across: replicated
        files.append(jpeg(picture((11, w, 3), 40 + w), quality=90, subsampling=1))
    files.append(jpeg(picture((33, 47, 3), 50), quality=75, subsampling=2))
    files.append(jpeg(picture((33, 47), 51), quality=75))
    files.append(jpeg(picture((33, 47, 3), 52, "flat"), quality=100, subsampling=1, optimize=True))
    return files


def test_small_shapes():
    decode_all(small_files())


@pytest.mark.parametrize("channels", [1, 3])
def test_channel_conversion(channels):
    decode_all(small_files()[3:9] + [jpeg(picture((33, 47), 51), quality=75)], channels)
    with pytest.raises(ValueError):
        jpeg_reader.JpegDecoder(0).decode(small_files()[:1], channels=4)


def test_restart_markers():
    every = jpeg(picture((72, 72, 3), 60), quality=85, subsampling=0, restart_marker_blocks=1)
    assert every.count(b"\xff\xd0") + every.count(b"\xff\xd7") > 0 and sum(every.count(bytes([0xFF, 0xD0 + k])) for k in range(8)) == 80
    rows = [jpeg(picture((72, 100, 3), 61 + sub, "ramp"), quality=85, subsampling=sub, restart_marker_rows=1) for sub in (0, 1, 2)]
    uneven = jpeg(picture((40, 56, 3), 65), quality=85, subsampling=2, restart_marker_blocks=5)  # 12 MCUs: 5, 5, 2
    grey = jpeg(picture((40, 41), 66), quality=90, restart_marker_blocks=1)
    decode_all([every] + rows + [uneven, grey])  # 81 segments: more than a wave's lanes


def test_seventy_mixed_files_in_one_call():
    rng = np.random.default_rng(70)
    files = []
    for k in range(70):
        h, w = (int(v) for v in rng.integers(1, 40, 2))
        shape = (h, w) if k % 5 == 4 else (h, w, 3)
        options = {"restart_marker_blocks": 2} if k % 7 == 3 else {}
        files.append(jpeg(picture(shape, k, ("noise", "ramp", "flat")[k % 3]), quality=(30, 75, 95)[k % 3], **({} if len(shape) == 2 else {"subsampling": k % 3}),
                          **options))
    decode_all(files)  # more than 64 files on the one-lane-per-file path


def test_demo_image():
    decode_all([demo_bytes()])


def test_refused_kinds_beside_good_files():
    good = small_files()[4]
    kinds = refused()
    names = sorted(kinds)
    files = [good] + [kinds[n][0] for n in names] + [good]
    shapes = [None] + [pil_array(f).shape[:2] + (3,) for f in files[1:-1]] + [None]  # a row for each, whatever the file states
    images, flags = capi_jpeg(files, shapes=shapes)
    assert flags == [0] + [kinds[n][1] for n in names] + [0]
    assert np.array_equal(images[0], pil_array(good)) and np.array_equal(images[-1], pil_array(good))
    res = jpeg_reader.JpegDecoder(0).decode(files, channels=3)
    assert res.flags.tolist() == [0, -1, -1, -1, 0]  # the host walks the markers up to SOF0 and finds another frame: PIL gets the file as it is
    for got, f in zip(res.tensors(), files):
        assert np.array_equal(got.cpu().numpy(), pil_array(f, 3))
    odd = header_defects()["Se = 62"][0]  # libjpeg warns and goes on: the device's flag, PIL's pixels
    res = jpeg_reader.JpegDecoder(0).decode([good, odd, good])
    assert res.flags.tolist() == [0, UNSUPPORTED, 0]
    for got, f in zip(res.tensors(), [good, odd, good]):
        assert np.array_equal(got.cpu().numpy(), pil_array(f))


def test_header_defects():
    cases = header_defects()
    names = sorted(cases)
    files = [cases[n][0] for n in names]
    _, flags = capi_jpeg(files, shapes=[(24, 20, 3)] * len(files))
    assert flags == [cases[n][1] for n in names]
    good = jpeg(picture((24, 20, 3), 8), quality=90, subsampling=2)
    _, flags = capi_jpeg([good, good, good, good], shapes=[None, (24, 21, 3), (25, 20, 3), (24, 20, 1)])  # SOF0 against the row
    assert flags == [0] + [MALFORMED] * 3


def test_damaged_files_are_flagged():
    """A dozen files dad3d_jpeg_decode_host flags, beside good ones: the flag path, with the pixels then PIL's or the error PIL's."""
    good = jpeg(picture((17, 9, 3), 2), quality=75, subsampling=2, restart_marker_blocks=1)
    scan = good.index(b"\xff\xda")
    damaged = [good[:n] for n in (scan + 14, scan + 30, len(good) - 2, len(good) - 1)]
    for at in range(scan + 14, len(good) - 2, 3):
        f = good[:at] + bytes([good[at] ^ 0x10]) + good[at + 1:]
        if len(damaged) < 12 and host_decode(f)[0]:
            damaged.append(f)
    assert len(damaged) == 12 and all(host_decode(f)[0] for f in damaged)
    files = [good] + damaged + [good]
    images, flags = capi_jpeg(files, shapes=[(17, 9, 3)] * len(files))
    assert flags[0] == 0 and flags[-1] == 0 and all(flags[1:-1])
    assert np.array_equal(images[0], pil_array(good)) and np.array_equal(images[-1], pil_array(good))
    decoder = jpeg_reader.JpegDecoder(0)
    for f in damaged:
        try:
            want = pil_array(f)
        except Exception:  # noqa: BLE001 -- PIL's own error, whatever its class
            with pytest.raises(Exception):  # noqa: B017, PT011
                decoder.decode([f])
            continue
        res = decoder.decode([f])
        assert res.flags.tolist() != [0] and np.array_equal(res.tensors()[0].cpu().numpy(), want)


def test_decode_packed():
    files = [jpeg(picture((20, 31, 3), 80), quality=85, subsampling=2), b"", jpeg(picture((9, 9), 81), quality=85)]
    offsets, at = [], 0
    for f in files:
        offsets.append(at)
        at += align(len(f))
    buffer = torch.zeros(at, dtype=torch.uint8)
    for o, f in zip(offsets, files):
        buffer[o:o + len(f)] = torch.from_numpy(np.frombuffer(f, dtype=np.uint8).copy()) if f else buffer[o:o]
    decoder = jpeg_reader.JpegDecoder(0)
    keep = [0, 2]
    res = decoder.decode_packed(buffer, [offsets[i] for i in keep], [len(files[i]) for i in keep])
    assert res.flags.tolist() == [0, 0]
    heads = [jpeg_reader._header(files[i]) for i in keep]
    on_device = decoder.decode_packed(buffer.cuda(), [offsets[i] for i in keep], [len(files[i]) for i in keep], channels=3, heads=heads)
    assert on_device.flags.tolist() == [0, 0]
    for k, i in enumerate(keep):
        assert np.array_equal(res.tensors()[k].cpu().numpy(), pil_array(files[i]))
        assert np.array_equal(on_device.tensors()[k].cpu().numpy(), pil_array(files[i], 3))
    with pytest.raises(Exception):  # noqa: B017, PT011 -- a file of no bytes beside the others (same offset as its neighbour): PIL's error
        decoder.decode_packed(buffer, offsets, [len(f) for f in files])
    neighbours = decoder.decode_packed(buffer, [offsets[0], offsets[2]], [len(files[0]), len(files[2])], channels=1)
    assert np.array_equal(neighbours.tensors()[0].cpu().numpy(), pil_array(files[0], 1))


def png_file():
    buf = io.BytesIO()
    Image.fromarray(picture((8, 8, 3), 4)).save(buf, "PNG")
    return buf.getvalue()


@pytest.mark.parametrize("kind", ["jpeg", "png"])
def test_decode_packed_contract_errors_raise_before_any_launch(kind):
    from dad_3dheads_amd import png_reader

    f, decoder, no_mode = {"jpeg": (jpeg(picture((8, 8, 3), 4), quality=90), jpeg_reader.JpegDecoder(0), 2),
                           "png": (png_file(), png_reader.PngDecoder(0), 5)}[kind]
    buffer = torch.zeros(align(len(f)) + 16, dtype=torch.uint8)
    buffer[:len(f)] = torch.from_numpy(np.frombuffer(f, dtype=np.uint8).copy())
    for bad in (lambda: decoder.decode_packed(buffer, [8], [len(f)]),  # an offset that is no multiple of 16
                lambda: decoder.decode_packed(buffer, [16], [len(f) + 16]),  # past the end
                lambda: decoder.decode_packed(buffer, [0, 16], [len(f)]),  # offsets and sizes of different lengths
                lambda: decoder.decode_packed(buffer, [-16], [len(f)]),
                lambda: decoder.decode_packed(buffer.to(torch.int8), [0], [len(f)]),
                lambda: decoder.decode_packed(buffer.view(2, -1), [0], [len(f)]),
                lambda: decoder.decode_packed(buffer, [0], [len(f)], channels=no_mode),
                lambda: decoder.decode_packed(buffer, [0], [len(f)], heads=[]),
                lambda: decoder.decode_packed(buffer.numpy(), [0], [len(f)])):  # not a tensor
        with pytest.raises(ValueError):
            bad()
    assert decoder.decode_packed(buffer, [0], [len(f)]).flags.tolist() == [0]  # and the call the bad ones are one step away from


def test_load_jpeg_batch():
    files = small_files()[3:6] + [jpeg(picture((33, 47), 51), quality=75)]
    for got, f in zip(jpeg_reader.load_jpeg_batch(files), files):
        assert np.array_equal(got.cpu().numpy(), pil_array(f, 3))


def test_replay_in_a_captured_graph_with_new_files():
    lib = _lib.load()
    first = jpeg(picture((40, 56, 3), 90), quality=85, subsampling=2, restart_marker_blocks=2)
    second = jpeg(picture((40, 56, 3), 91, "ramp"), quality=85, subsampling=2, restart_marker_blocks=2)
    room = align(max(len(first), len(second)))
    rows = [[0, len(first), 40, 56, 3, 0, 56 * 3, 3, 0, 0, 0, 0]]
    desc = np.asarray(rows, dtype=np.int64)
    grid = np.zeros(_lib.JPEG_DECODE_GRID_INTS, dtype=np.int32)
    nbytes = lib.dad3d_jpeg_decode_scratch_bytes(desc.ctypes.data, 1, grid.ctypes.data)
    assert nbytes > 0
    data = torch.zeros(room, dtype=torch.uint8, device="cuda")
    desc_dev = torch.from_numpy(desc).cuda()
    out = torch.zeros(40 * 56 * 3, dtype=torch.uint8, device="cuda")
    flags = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def load(f):
        data.zero_()
        data[:len(f)] = torch.from_numpy(np.frombuffer(f, dtype=np.uint8).copy()).cuda()
        desc_dev[0, 1] = len(f)

    def launch():
        _lib.check(lib.dad3d_jpeg_decode(data.data_ptr(), room, desc_dev.data_ptr(), 1, grid.ctypes.data, out.data_ptr(), out.numel(),
                                         flags.data_ptr(), scratch.data_ptr(), nbytes, 0, torch.cuda.current_stream().cuda_stream))

    load(first)
    launch()  # the warm-up
    torch.cuda.synchronize()
    assert flags.tolist() == [0] and np.array_equal(out.cpu().numpy().reshape(40, 56, 3), pil_array(first))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    load(second)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert flags.tolist() == [0] and np.array_equal(out.cpu().numpy().reshape(40, 56, 3), pil_array(second))


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


def test_predict_files_on_jpeg_and_png_equals_predict_batch(flame_model, monkeypatch):
    from dad_3dheads_amd.config import load_default_config
    from dad_3dheads_amd.predictor import FaceMeshPredictor

    pred = FaceMeshPredictor(load_default_config(), cuda_id=0, model=Stub(), flame_model=flame_model)
    png = io.BytesIO()
    Image.fromarray(picture((90, 120, 3), 1)).save(png, "PNG")
    files = [jpeg(picture((130, 40, 3), 2, "ramp"), quality=85, subsampling=2), png.getvalue(),
             jpeg(picture((33, 47), 3), quality=85, restart_marker_blocks=3)]  # colour JPEG, PNG, grey JPEG: three sizes in one call
    arrays = [np.array(np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))) for f in files]
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
    assert len(got) == len(want) == 3
    for g, w in zip(got, want):
        assert set(g) == set(w) == {"points", "projected_vertices", "3d_vertices", "3dmm_params"}
        assert np.array_equal(g["points"], w["points"])
        for k in ("projected_vertices", "3d_vertices", "3dmm_params"):
            assert torch.equal(g[k], w[k]), k
    only = pred.predict_files(files[::2], device_outputs=True)  # JPEG alone
    assert only[0]["3d_vertices"].is_cuda and torch.equal(only[1]["3dmm_params"].cpu(), want[2]["3dmm_params"])
