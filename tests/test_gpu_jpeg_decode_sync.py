"""GPU: the piece-wise entropy stage of the JPEG reader (csrc/jpeg_decode_sync.hip): `JpegDecoder(entropy="sync")` and
dad3d_jpeg_decode_sync give PIL's pixels, the flags of the one-lane-per-segment decoder and the modes of dad3d_jpeg_decode_sync_host,
which tests/test_jpeg_sync_host.py holds to PIL and to the restatement on a CPU. The C entry runs with the scratch and the output
pre-filled with FF and with guard bytes between the rows and behind the items."""
import numpy as np
import pytest
import torch

from jpeg_cases import MALFORMED, demo_bytes, jpeg, pil_array, pil_raises, picture, refused
from jpeg_sync_cases import host_decode_sync, three_groups, unverified
from test_gpu_jpeg_decode import Stub, align, capi_jpeg
from dad_3dheads_amd import _lib, jpeg_reader

pytestmark = pytest.mark.gpu
GUARD = 0xFF
PIECES = (16, None)  # None: the default


def piece_bytes_of(p):
    return jpeg_reader.SYNC_PIECE_BYTES if p is None else p


def mixed():
    """[(name, bytes)]: the shapes and the kinds of file the stage must take; the last two never give pixels on the device."""
    whole = jpeg(picture((40, 56, 3), 65), quality=85, subsampling=2)
    return [("1 x 1", jpeg(picture((1, 1, 3), 1), quality=90)), ("7 x 9 grey", jpeg(picture((7, 9), 2), quality=90)),
            ("17 x 33 at 4:2:2", jpeg(picture((17, 33, 3), 3), quality=85, subsampling=1)),
            ("120 x 136 at 4:2:0", jpeg(picture((120, 136, 3), 4, "ramp"), quality=85, subsampling=2)),
            ("three groups", three_groups()), ("not verified", unverified()),
            ("restart markers", jpeg(picture((40, 56, 3), 5), quality=85, subsampling=2, restart_marker_blocks=5)),
            ("progressive", refused()["progressive"][0]), ("truncated", whole[:len(whole) * 2 // 3])]


def capi_sync(files, piece_bytes, channels=None, pad=5, shapes=None, spoil=None):
    """dad3d_jpeg_decode_sync -> (images or None per file, flags, info rows). `spoil(more, nbytes)` may change the four table columns
    of every file behind dad3d_jpeg_decode_sync_scratch_bytes."""
    lib = _lib.load()
    rows, at, out_at = [], 0, 0
    for i, f in enumerate(files):
        h, w, c = jpeg_reader._header(f) if shapes is None or shapes[i] is None else shapes[i]
        oc = c if channels is None else channels
        stride = w * oc + pad
        rows.append([at, len(f), h, w, c, out_at, stride, oc, 0, 0, 0, 0])
        at += align(len(f)) + 16
        out_at += align(h * stride) + 16
    n = len(rows)
    desc = np.concatenate([np.asarray(rows, dtype=np.int64).ravel(), np.zeros(4 * n, np.int64)])
    grid = np.zeros(_lib.JPEG_DECODE_SYNC_GRID_INTS, dtype=np.int32)
    nbytes = lib.dad3d_jpeg_decode_sync_scratch_bytes(desc.ctypes.data, n, grid.ctypes.data, piece_bytes)
    assert nbytes > 0
    if spoil is not None:
        spoil(desc[12 * n:].reshape(n, 4), nbytes)
    data = np.full(at, 0xEE, dtype=np.uint8)
    for row, f in zip(rows, files):
        data[row[0]:row[0] + row[1]] = np.frombuffer(f, dtype=np.uint8)
    dev = torch.from_numpy(data).cuda()
    out = torch.full((out_at,), GUARD, dtype=torch.uint8, device="cuda")
    flags = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    info = torch.full((n, 4), -1, dtype=torch.int32, device="cuda")
    scratch = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    desc_dev = torch.from_numpy(desc).cuda()
    _lib.check(lib.dad3d_jpeg_decode_sync(dev.data_ptr(), at, desc_dev.data_ptr(), n, grid.ctypes.data, piece_bytes, out.data_ptr(), out_at,
                                          flags.data_ptr(), info.data_ptr(), scratch.data_ptr(), nbytes, 0, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    host, fl = out.cpu().numpy(), flags.cpu().tolist()
    images = []
    for k, row in enumerate(rows):
        _, _, h, w, _, o, stride, oc = row[:8]
        end = rows[k + 1][5] if k + 1 < n else out_at
        block = host[o:o + h * stride].reshape(h, stride)
        assert (block[:, w * oc:] == GUARD).all() and (host[o + h * stride:end] == GUARD).all(), k
        images.append(block[:, :w * oc].reshape(h, w, oc).copy() if fl[k] == 0 else None)
    return images, fl, info.cpu().numpy()


@pytest.mark.parametrize("channels", [None, 1, 3])
@pytest.mark.parametrize("pieces", PIECES)
def test_mixed_batch_through_the_c_entry(pieces, channels):
    p = piece_bytes_of(pieces)
    names, files = zip(*mixed())
    shapes = [None if jpeg_reader._header(f) else pil_array(f).shape[:2] + (3,) for f in files[:-1]] + [(40, 56, 3)]
    images, flags, info = capi_sync(files, p, channels, shapes=shapes)
    _, want_flags = capi_jpeg(files, channels, shapes=shapes)
    assert flags == want_flags and flags[:7] == [0] * 7 and all(flags[7:])
    modes = []
    for k, f in enumerate(files):
        host_flag, _, host_info = host_decode_sync(f, p, channels)
        assert tuple(info[k]) == host_info + (0,) and bool(host_flag) == bool(flags[k]), names[k]
        modes.append(host_info[0])
        if flags[k] == 0:
            assert np.array_equal(images[k], pil_array(f, channels)), names[k]
    assert modes[:7] == ([1, 1, 1, 1, 1, 2, 0] if p == 16 else [1, 1, 1, 1, 1, 1, 0])
    assert p != 16 or tuple(info[4][:3]) == (1, 620, 3)


@pytest.mark.parametrize("channels", [None, 1, 3])
@pytest.mark.parametrize("pieces", PIECES)
def test_mixed_batch_through_the_reader(pieces, channels):
    names, files = zip(*mixed()[:-1])  # PIL refuses the truncated file: below
    sync = jpeg_reader.JpegDecoder(0, entropy="sync", piece_bytes=pieces).decode(files, channels)
    plain = jpeg_reader.JpegDecoder(0).decode(files, channels)
    assert sync.flags.tolist() == plain.flags.tolist() == [0] * 7 + [-1]
    for name, got, f in zip(names, sync.tensors(), files):
        assert got.is_cuda and torch.equal(got.cpu(), torch.from_numpy(np.array(pil_array(f, channels)))), name
    want = [host_decode_sync(f, piece_bytes_of(pieces), channels)[2][0] for f in files[:-1]] + [-1]
    assert sync.modes.dtype == np.int32 and sync.modes.tolist() == want
    assert plain.modes.tolist() == [0] * 7 + [-1]
    truncated = mixed()[-1][1]
    assert pil_raises(truncated)
    with pytest.raises(Exception):  # noqa: B017, PT011 -- PIL's own error
        jpeg_reader.JpegDecoder(0, entropy="sync", piece_bytes=pieces).decode([truncated], channels)


def test_demo_image():
    f = demo_bytes()
    for pieces in PIECES:
        images, flags, info = capi_sync([f], piece_bytes_of(pieces))
        assert flags == [0] and info[0, 0] == 1 and info[0, 2] >= 3
        assert np.array_equal(images[0], pil_array(f))
    res = jpeg_reader.JpegDecoder(0, entropy="sync").decode([f], 3)
    assert res.flags.tolist() == [0] and res.modes.tolist() == [1] and np.array_equal(res.tensors()[0].cpu().numpy(), pil_array(f, 3))
    assert np.array_equal(jpeg_reader.load_jpeg_batch([f], entropy="sync")[0].cpu().numpy(), pil_array(f, 3))


def test_more_files_than_a_wave():
    rng = np.random.default_rng(71)
    files = []
    for k in range(70):
        h, w = (int(v) for v in rng.integers(1, 60, 2))
        shape = (h, w) if k % 5 == 4 else (h, w, 3)
        options = {"restart_marker_blocks": 2} if k % 7 == 3 else {}
        files.append(jpeg(picture(shape, k, ("noise", "ramp", "flat")[k % 3]), quality=(30, 75, 95)[k % 3], **({} if len(shape) == 2 else {"subsampling": k % 3}),
                          **options))
    images, flags, info = capi_sync(files, 16)
    assert flags == [0] * 70
    for k, f in enumerate(files):
        assert np.array_equal(images[k], pil_array(f)), k
        assert tuple(info[k][:3]) == host_decode_sync(f, 16)[2], k


def test_a_row_whose_tables_do_not_fit_is_a_flag_not_an_access():
    good = three_groups()
    files = [good] * 5

    def spoil(more, nbytes):
        more[1, 0] = nbytes - 32  # a piece table that ends behind the scratch
        more[2, 1] = 619          # room for one piece less than the file has
        more[3, 2] += 8           # a group table off its alignment
        more[4, 3] = 2            # and one with a group too few

    images, flags, info = capi_sync(files, 16, spoil=spoil)
    assert flags == [0] + [MALFORMED] * 4 and np.array_equal(images[0], pil_array(good))
    assert info.tolist() == [[1, 620, 3, 0]] + [[0, 0, 0, 0]] * 4


@pytest.mark.parametrize("pieces", PIECES)
def test_replay_in_a_captured_graph_with_new_files(pieces):
    lib, p = _lib.load(), piece_bytes_of(pieces)
    first = jpeg(picture((64, 64, 3), 90), quality=95, subsampling=0)
    second = jpeg(picture((64, 64, 3), 91, "ramp"), quality=95, subsampling=0)
    room = align(max(len(first), len(second)))
    desc = np.asarray([0, room, 64, 64, 3, 0, 64 * 3, 3, 0, 0, 0, 0] + [0] * 4, dtype=np.int64)  # tables for the longest file the room holds
    grid = np.zeros(_lib.JPEG_DECODE_SYNC_GRID_INTS, dtype=np.int32)
    nbytes = lib.dad3d_jpeg_decode_sync_scratch_bytes(desc.ctypes.data, 1, grid.ctypes.data, p)
    assert nbytes > 0
    data = torch.zeros(room, dtype=torch.uint8, device="cuda")
    desc_dev = torch.from_numpy(desc).cuda()
    out = torch.zeros(64 * 64 * 3, dtype=torch.uint8, device="cuda")
    flags = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    info = torch.full((1, 4), -1, dtype=torch.int32, device="cuda")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def load(f):
        data.zero_()
        data[:len(f)] = torch.from_numpy(np.frombuffer(f, dtype=np.uint8).copy()).cuda()
        desc_dev[1] = len(f)

    def launch():
        _lib.check(lib.dad3d_jpeg_decode_sync(data.data_ptr(), room, desc_dev.data_ptr(), 1, grid.ctypes.data, p, out.data_ptr(), out.numel(),
                                              flags.data_ptr(), info.data_ptr(), scratch.data_ptr(), nbytes, 0, torch.cuda.current_stream().cuda_stream))

    load(first)
    launch()  # the warm-up
    torch.cuda.synchronize()
    assert flags.tolist() == [0] and np.array_equal(out.cpu().numpy().reshape(64, 64, 3), pil_array(first))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for f in (second, first):
        load(f)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert flags.tolist() == [0] and np.array_equal(out.cpu().numpy().reshape(64, 64, 3), pil_array(f))
        assert tuple(info[0].tolist()) == host_decode_sync(f, p)[2] + (0,)


def test_predict_files_with_sync_returns_what_the_default_returns(flame_model):
    from dad_3dheads_amd.config import load_default_config
    from dad_3dheads_amd.predictor import FaceMeshPredictor

    pred = FaceMeshPredictor(load_default_config(), cuda_id=0, model=Stub(), flame_model=flame_model)
    files = [jpeg(picture((130, 40, 3), 2, "ramp"), quality=85, subsampling=2), three_groups(),
             jpeg(picture((33, 47), 3), quality=85, restart_marker_blocks=3)]
    want = pred.predict_files(files)
    got = pred.predict_files(files, jpeg_entropy="sync")
    assert len(got) == len(want) == 3
    for g, w in zip(got, want):
        assert set(g) == set(w) and np.array_equal(g["points"], w["points"])
        for k in ("projected_vertices", "3d_vertices", "3dmm_params"):
            assert torch.equal(g[k], w[k]), k
    with pytest.raises(ValueError):
        pred.predict_files(files, jpeg_entropy="pieces")
