"""GPU: the heads of a frame from bounding boxes -- csrc/preprocess_boxes.hip (`dad3d_preprocess_boxes`,
`dad3d_flame_readjust_params_frame`, `dad3d_points_readjust_frame`), `FaceMeshPredictor.predict_boxes` and the overlays' `image_index`.

The box rule is held to `dataset.extend_bbox` / `ensure_bbox_boundaries` (pinned to the reference's goldens by
test_train_batch_host.py), the geometry to `resize_geometry`, the pixels to the preprocessing oracle on the host crop
(oracle/preprocess_ref.py), and the mapping into the frame to the reference's float32 sequence on `predict_batch`'s results:
integers equal, floats bit for bit. Frames are uniform random bytes, so a tap outside the crop changes the result."""
import ctypes as C

import numpy as np
import pytest
import torch

from dad_3dheads_amd import _lib, resize_geometry
from dad_3dheads_amd.dataset import ensure_bbox_boundaries, extend_bbox
from oracle import preprocess_ref as pp

pytestmark = pytest.mark.gpu

E, CO, R = _lib.BOX_FLAG_EMPTY, _lib.BOX_FLAG_COLLAPSED, _lib.BOX_FLAG_RANGE
NAN, INF = float("nan"), float("inf")
SHAPES = [(97, 131), (300, 200), (64, 64), (520, 1010)]  # (h, w); the fourth holds the 512-high strips and the 1 x 1000 crop
FOUR = (0.05, 0.2, 0.1, 0.3)  # (left, right, top, bottom), all different
# offset -> [((x, y, w, h), frame, expected flags)]
CASES = {
    None: [
        ((10, 5, 30, 20), 0, 0),         # 20 x 30, up-scaled
        ((10, 5, 180, 290), 1, 0),       # 290 x 180, down-scaled
        ((50, 20, 100, 256), 1, 0),      # long side exactly 256: the copy branch
        ((0, 0, 131, 97), 0, 0),         # the frame itself
        ((0, 0, 64, 64), 2, 0),
        ((111, 77, 20, 20), 0, 0),       # the frame's last pixel is the crop's
        ((0, 0, 17, 13), 0, 0),
        ((3, 4, 5, 512), 3, 0),          # 5 * 0.5 = 2.5 -> 2
        ((20, 4, 7, 512), 3, 0),         # 7 * 0.5 = 3.5 -> 4
        ((30, 30, 1, 1), 2, 0),          # 1 x 1
        ((-10, 20, 40, 30), 0, 0),       # over the left edge
        ((110, 20, 40, 30), 0, 0),       # right
        ((20, -8, 30, 40), 0, 0),        # top
        ((20, 80, 30, 40), 0, 0),        # bottom
        ((-5, -7, 40, 30), 0, 0),        # two edges at once
        ((120, 90, 40, 30), 0, 0),
        ((-3.7, -2.2, 40.9, 30.5), 1, 0),  # toward zero: (-3, -2), not (-4, -3)
        ((40, 50, 60, 70), 1, 0),        # wholly inside, untouched
        ((200, 200, 10, 10), 0, E),      # outside the frame
        ((50, 50, -10, 10), 0, E),       # a negative width
        ((5, 100, 1000, 1), 3, CO),      # 1 x 1000: py3round(0.256) = 0
        ((NAN, 0, 10, 10), 0, R),
        ((0, 0, 10, INF), 0, R),
        ((0, 0, 2 ** 30, 10), 0, R),
        ((5, 5, 10, 10), 4, R),          # image_index == M
        ((5, 5, 10, 10), -1, R),
    ],
    0.1: [
        ((3, -2, 15, 17), 0, 0),         # extend_bbox -> [1, -3, 18, 20]: -3.7 goes to -3
        ((30, 40, 50, 60), 1, 0),
        ((0, 0, 131, 97), 0, 0),         # grows over all four edges
        ((-4.5, -6.5, 33.3, 21.7), 0, 0),
        ((150, 250, 60, 60), 1, 0),
        ((10, 10, 40, 40), 2, 0),
        ((0, 0, 64, 64), 2, 0),
        ((60, 2, 6, 470), 3, 0),
        ((700, 300, 100, 120), 3, 0),
        ((2 ** 30 - 64, 0, 10, 10), 0, E),  # still in range (and a float32), far outside
        ((0, 0, 2 ** 30 - 1, 10), 0, R),    # w * 1.2 leaves the range
    ],
    FOUR: [
        ((20, 30, 40, 50), 0, 0),
        ((100, 100, 80, 90), 1, 0),
        ((5.5, 6.5, 20.25, 30.75), 2, 0),
        ((0, 0, 200, 300), 1, 0),
        ((-3, -2, 15, 17), 0, 0),
        ((500, 200, 333, 211), 3, 0),
    ],
}
NP_DTYPES = {"int32": np.int32, "int64": np.int64, "float32": np.float32, "float64": np.float64}
BOX_DTYPE = {"int32": _lib.BOX_DTYPE_I32, "int64": _lib.BOX_DTYPE_I64, "float32": _lib.BOX_DTYPE_F32, "float64": _lib.BOX_DTYPE_F64}
F32, F16, BF16 = _lib.PREPROCESS_OUT_F32_NCHW, _lib.PREPROCESS_OUT_F16_NHWC, _lib.PREPROCESS_OUT_BF16_NHWC
OUT_DTYPE = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}


def _factors(offset):
    return None if offset is None else offset if isinstance(offset, tuple) else (offset,) * 4


def _cases(offset, dtype):
    """(boxes [N,4] of dtype, image_index int32 [N], expected flags [N]); a non-finite value has no integer form."""
    rows = [c for c in CASES[offset] if np.dtype(dtype).kind == "f" or all(np.isfinite(c[0]))]
    boxes = np.array([c[0] for c in rows], dtype=np.float64).astype(dtype)  # an integer dtype truncates: still a valid box
    return boxes, np.array([c[1] for c in rows], np.int32), np.array([c[2] for c in rows], np.int32)


def _expected(boxes, index, flags, offset, size):
    """crops int32 [N,4] and geometry float64 [N,5] from dataset.py and resize_geometry.py, given the hand-derived flags."""
    crops, geometry = np.zeros((len(boxes), 4), np.int32), np.zeros((len(boxes), 5), np.float64)
    geometry[:, 2] = 1.0
    for i, (box, image, flag) in enumerate(zip(boxes, index, flags)):
        if flag == R:
            continue
        v = box.astype(np.float64)
        grown = extend_bbox(v, _factors(offset)) if offset is not None else v.astype(np.int32)
        crops[i] = ensure_bbox_boundaries(grown, SHAPES[image])
        x, y, w, h = (int(c) for c in crops[i])
        assert (w <= 0 or h <= 0) == (flag == E), (box, crops[i], flag)
        if flag:
            continue
        new_h, new_w, top, left = resize_geometry.longest_max_size(h, w, size)
        assert new_h > 0 and new_w > 0
        geometry[i] = [left, top, size / float(max(h, w)), x, y]
    return crops, geometry


@pytest.fixture(scope="module")
def frames():
    rng = np.random.default_rng(2024)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SHAPES]


@pytest.fixture(scope="module")
def dev_frames(frames):
    """The second frame is a view into a wider image: a row stride larger than 3 * w, neighbours that are not zero."""
    out = [torch.from_numpy(f).cuda() for f in frames]
    wide = torch.randint(0, 256, (300, 260, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
    wide[:, 30:230] = out[1]
    out[1] = wide[:, 30:230]
    assert out[1].stride(0) == 780 and not out[1].is_contiguous()
    return out


def _launch(dev_frames, boxes, index, offset, fmt=F32, size=256):
    lib = _lib.load()
    n = len(boxes)
    table = torch.tensor([[t.data_ptr(), t.shape[0], t.shape[1], t.stride(0)] for t in dev_frames], dtype=torch.int64).cuda()
    d_boxes, d_index = torch.from_numpy(np.ascontiguousarray(boxes)).cuda(), torch.from_numpy(np.ascontiguousarray(index)).cuda()
    layout = torch.contiguous_format if fmt == F32 else torch.channels_last
    out = torch.full((n, 3, size, size), 7.0, dtype=OUT_DTYPE[fmt], device="cuda").contiguous(memory_format=layout)
    crops = torch.full((n, 4), -1, dtype=torch.int32, device="cuda")
    geometry = torch.full((n, 5), -1.0, dtype=torch.float64, device="cuda")
    flags = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    mean, std = (C.c_float * 3)(*pp.MEAN), (C.c_float * 3)(*pp.STD)
    off = None if offset is None else (C.c_double * 4)(*_factors(offset))
    _lib.check(lib.dad3d_preprocess_boxes(table.data_ptr(), len(dev_frames), d_boxes.data_ptr(), BOX_DTYPE[str(boxes.dtype)], d_index.data_ptr(), n, off,
                                          size, mean, std, fmt, out.data_ptr(), crops.data_ptr(), geometry.data_ptr(), flags.data_ptr(), 0, None))
    torch.cuda.synchronize()
    return out, crops.cpu().numpy(), geometry.cpu().numpy(), flags.cpu().numpy()


# ---- 1. the box rule and the geometry ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(NP_DTYPES))
@pytest.mark.parametrize("offset", list(CASES), ids=["none", "tenth", "four"])
def test_box_rule_and_geometry_bit_for_bit(dev_frames, offset, dtype):
    boxes, index, want_flags = _cases(offset, NP_DTYPES[dtype])
    want_crops, want_geometry = _expected(boxes, index, want_flags, offset, 256)
    _, crops, geometry, flags = _launch(dev_frames, boxes, index, offset)
    assert flags.tolist() == want_flags.tolist()
    assert np.array_equal(crops, want_crops), np.flatnonzero((crops != want_crops).any(1))
    assert geometry.tobytes() == want_geometry.tobytes(), np.flatnonzero((geometry != want_geometry).any(1))


# ---- 2. the pixels -------------------------------------------------------------------------------------------------------------
_oracle_cache = {}


def _oracle(frames, offset, size):
    """float32 [N,3,S,S]: the preprocessing oracle on every host crop, normalised zeros for a flagged row. Computed once."""
    key = (offset, size)
    if key not in _oracle_cache:
        boxes, index, flags = _cases(offset, np.float64)
        crops, _ = _expected(boxes, index, flags, offset, size)
        zero = pp.transform(np.zeros((2, 2, 3), np.uint8), size=size)
        assert len(np.unique(zero[0])) == 1
        rows = [zero if f else pp.transform(frames[i][y:y + h, x:x + w], size=size) for (x, y, w, h), i, f in zip(crops, index, flags)]
        _oracle_cache[key] = (boxes, index, flags, np.stack(rows))
    return _oracle_cache[key]


@pytest.mark.parametrize("offset", list(CASES), ids=["none", "tenth", "four"])
def test_pixels_equal_the_oracle_on_the_host_crop(frames, dev_frames, offset):
    boxes, index, flags, want = _oracle(frames, offset, 256)
    out, _, _, got_flags = _launch(dev_frames, boxes, index, offset)
    assert got_flags.tolist() == flags.tolist()
    got = out.cpu().numpy()
    for k in range(len(boxes)):
        assert np.array_equal(got[k], want[k]), (k, boxes[k], int((got[k] != want[k]).sum()))


@pytest.mark.parametrize("size", [255, 300])  # an odd row (2-byte stores), and a row of more than one workgroup
def test_pixels_at_other_sizes(frames, dev_frames, size):
    boxes, index, flags, want = _oracle(frames, None, size)
    out, _, geometry, got_flags = _launch(dev_frames, boxes, index, None, size=size)
    assert got_flags.tolist() == flags.tolist()
    assert np.array_equal(out.cpu().numpy(), want)
    assert geometry.tobytes() == _expected(boxes, index, flags, None, size)[1].tobytes()
    half, _, _, _ = _launch(dev_frames, boxes, index, None, fmt=BF16, size=size)
    assert torch.equal(half, out.to(torch.bfloat16).contiguous(memory_format=torch.channels_last))


@pytest.mark.parametrize("fmt", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("offset", [None, 0.1], ids=["none", "tenth"])
def test_half_formats_equal_the_cast_and_layout_of_the_float32_result(dev_frames, offset, fmt):
    boxes, index, _ = _cases(offset, np.float64)
    full, _, _, _ = _launch(dev_frames, boxes, index, offset)
    half, _, _, _ = _launch(dev_frames, boxes, index, offset, fmt=fmt)
    want = full.to(OUT_DTYPE[fmt]).contiguous(memory_format=torch.channels_last)
    assert half.dtype == OUT_DTYPE[fmt] and half.is_contiguous(memory_format=torch.channels_last) and half.stride() == want.stride()
    assert torch.equal(half.view(torch.int16), want.view(torch.int16))


def test_refusals_before_device_work():
    lib = _lib.load()
    one = torch.zeros(64, dtype=torch.int64, device="cuda")
    mean, std = (C.c_float * 3)(*pp.MEAN), (C.c_float * 3)(*pp.STD)

    def call(n_images=1, box_dtype=0, n=1, offset=None, size=256, fmt=F32, out=None, null=False):
        p = one.data_ptr()
        return lib.dad3d_preprocess_boxes(None if null else p, n_images, p, box_dtype, p, n, offset, size, mean, std, fmt,
                                          p if out is None else out, p, p, p, 0, None)

    assert call(n=0) == _lib.OK
    for kw in ({"box_dtype": 4}, {"fmt": 3}, {"n": 65536}, {"size": 0}, {"n_images": 0}, {"null": True}, {"out": one.data_ptr() + 2},
               {"offset": (C.c_double * 4)(0.1, NAN, 0.1, 0.1)}):
        assert call(**kw) == _lib.E_INVALID, kw


# ---- 3. the mapping into the frame ---------------------------------------------------------------------------------------------
class Stub(torch.nn.Module):
    """A small deterministic float32 model: an 8 x 8 average pool, then fixed seeded matrices to the 413-vector, the 136 landmark
    values and a [68,32,32] heatmap. `outputs` picks the heads it has."""

    def __init__(self, outputs=("params", "landmarks", "heatmap")):
        super().__init__()
        from dad_3dheads_amd import synthetic

        g = torch.Generator().manual_seed(5)
        self.register_buffer("w_params", torch.randn(3072, 413, generator=g) * 0.02)
        self.register_buffer("w_lmk", torch.randn(3072, 136, generator=g) * 0.02)
        self.register_buffer("w_heat", torch.randn(68, 3, generator=g))
        self.register_buffer("heat", 3.0 * torch.randn(68, 32, 32, generator=g))
        self.register_buffer("base", torch.from_numpy(synthetic.synthetic_params(1, seed=8))[0])
        self.outputs = outputs

    def forward(self, x):
        pooled = torch.nn.functional.avg_pool2d(x.float(), 8)  # [B,3,32,32]
        flat = pooled.flatten(1)
        out = {"OUTPUT_3DMM_PARAMS": self.base[None] + 0.05 * torch.tanh(flat @ self.w_params)}
        if "landmarks" in self.outputs:
            out["OUTPUT_2D_LANDMARKS"] = 0.5 + 0.6 * torch.tanh(flat @ self.w_lmk)  # reaches below 0 and above 1: the clip works
        if "heatmap" in self.outputs:
            out["OUTPUT_LANDMARKS_HEATMAP"] = self.heat[None] + torch.einsum("kc,bchw->bkhw", self.w_heat, pooled)
        return out


def _predictor(flame_model, outputs):
    from dad_3dheads_amd.config import load_default_config
    from dad_3dheads_amd.predictor import FaceMeshPredictor

    return FaceMeshPredictor(load_default_config(), cuda_id=0, model=Stub(outputs), flame_model=flame_model)


@pytest.fixture(scope="module")
def scene(frames):
    """Frames, host boxes per frame and the crops they become with offset 0.1; the last frame is 2100 x 3100 with a box whose
    crop starts at (3001, 1999), so the float32 addition of the origin rounds."""
    rng = np.random.default_rng(7)
    big = rng.integers(0, 256, (2100, 3100, 3), dtype=np.uint8)
    fr = [frames[0], frames[1], big]
    boxes = [np.array([[3, -2, 15, 17], [40, 30, 60, 50]], np.int32), np.array([[30.5, 40.25, 50, 60]], np.float64),
             np.array([[3008, 2007, 70, 80], [100, 200, 300, 400]], np.int64)]
    crops, index = [], []
    for i, b in enumerate(boxes):
        for row in b:
            crops.append(ensure_bbox_boundaries(extend_bbox(row.astype(np.float64), 0.1), fr[i].shape[:2]))
            index.append(i)
    assert crops[3].tolist()[:2] == [3001, 1999]
    return fr, boxes, np.stack(crops), np.array(index, np.int32)


@pytest.mark.parametrize("outputs", [("params", "landmarks", "heatmap"), ("params", "heatmap"), ("params",)],
                         ids=["landmarks", "heatmap", "params-only"])
def test_predict_boxes_equals_predict_batch_on_host_crops_moved_into_the_frame(flame_model, scene, outputs):
    from dad_3dheads_amd.predictor import find_3dmm_idx

    fr, boxes, crops, index = scene
    pred = _predictor(flame_model, outputs)
    got = pred.predict_boxes(fr, boxes)
    host_crops = [np.ascontiguousarray(fr[i][y:y + h, x:x + w]) for (x, y, w, h), i in zip(crops, index)]
    ref = pred.predict_batch(host_crops)
    assert len(got) == len(ref) == 5
    t0 = find_3dmm_idx("translation", pred.flame_constants)
    wanted_params = []
    for k, (g, r) in enumerate(zip(got, ref)):
        x, y = int(crops[k][0]), int(crops[k][1])
        assert g["bbox"].dtype == np.int32 and g["bbox"].tolist() == crops[k].tolist()
        assert g["image_index"] == index[k] and g["flags"] == 0
        # readjust_3dmm_to_the_input_image is predict_batch's; then adjust_3dmm_to_paddings(params, [y, _, x, _]) (head_mesh.py:48-60)
        p = r["3dmm_params"].clone()
        p[:, t0:t0 + 3] = p[:, t0:t0 + 3] + torch.Tensor([[x, y, 0]]) * 2 / 256
        wanted_params.append(p)
        assert torch.equal(g["3dmm_params"], p), (k, (g["3dmm_params"] != p).nonzero().tolist())
        if outputs == ("params",):
            assert set(g) == {"3dmm_params", "bbox", "image_index", "flags"}
            continue
        assert set(g) == {"points", "projected_vertices", "3d_vertices", "3dmm_params", "bbox", "image_index", "flags"}
        assert torch.equal(g["3d_vertices"], r["3d_vertices"])
        assert g["points"].dtype == r["points"].dtype and np.array_equal(g["points"], r["points"] + np.array([[x, y]]))
        assert g["projected_vertices"].shape == (1, 5023, 2)
    if outputs != ("params",):
        dec = pred.head_mesh.decode(torch.cat(wanted_params).cuda(), verts3d=True, proj=True, to_2d=True, landmarks=False, mutate=True)
        proj = dec["proj"].cpu()
        for k, g in enumerate(got):
            assert torch.equal(g["projected_vertices"], proj[k:k + 1]), k
        # and they are the crop's vertices moved by the origin, to float32's accuracy at that magnitude
        for k, (g, r) in enumerate(zip(got, ref)):
            shift = torch.tensor([float(crops[k][0]), float(crops[k][1])])
            assert (g["projected_vertices"] - (r["projected_vertices"] + shift)).abs().max() < 0.01


def test_flat_boxes_with_index_and_files_give_the_same_results(flame_model, scene, tmp_path):
    from PIL import Image

    fr, boxes, crops, index = scene
    pred = _predictor(flame_model, ("params", "landmarks"))
    small, small_boxes = fr[:2], boxes[:2]
    want = pred.predict_boxes(small, small_boxes, offset=(0.1, 0.1))
    flat = np.concatenate([b.astype(np.float64) for b in small_boxes])
    got = pred.predict_boxes([torch.from_numpy(f).cuda() for f in small], flat, image_index=[0, 0, 1], offset=(0.1, 0.1, 0.1, 0.1))
    paths = []
    for i, f in enumerate(small):
        paths.append(str(tmp_path / f"{i}.png"))
        Image.fromarray(f).save(paths[-1])
    files = pred.predict_files(paths, boxes=small_boxes, offset=0.1)
    for other in (got, files):
        for a, b in zip(want, other):
            assert a["bbox"].tolist() == b["bbox"].tolist() and a["image_index"] == b["image_index"]
            assert torch.equal(a["3dmm_params"], b["3dmm_params"]) and np.array_equal(a["points"], b["points"])
            assert torch.equal(a["projected_vertices"], b["projected_vertices"])
    with pytest.raises(ValueError, match="box 1 "):
        pred.predict_boxes(small, [np.array([[5, 5, 20, 20], [500, 5, 20, 20]]), np.zeros((0, 4))])


def test_half_input_goes_to_an_inference_net_where_it_lies(flame_model, scene, monkeypatch):
    """With an InferenceNet of bf16 the launch writes its input format, and the cast and layout pass of its forward are no-ops."""
    from dad_3dheads_amd.network import InferenceNet

    fr, boxes, crops, index = scene
    pred = _predictor(flame_model, ("params", "landmarks"))
    assert pred._input_format() == F32
    seen = []

    class Net(InferenceNet):
        def __init__(self, inner):
            torch.nn.Module.__init__(self)
            self.net, self.dtype = inner, torch.bfloat16

        def forward(self, x):
            y = x.to(self.dtype).contiguous(memory_format=torch.channels_last)  # network.py: InferenceNet.forward's first line
            seen.append((x.dtype, x.is_contiguous(memory_format=torch.channels_last), y.data_ptr() == x.data_ptr()))
            return self.net(y)

    full = pred.predict_boxes(fr[:2], boxes[:2])
    pred.model = Net(pred.model)
    assert pred._input_format() == BF16
    half = pred.predict_boxes(fr[:2], boxes[:2])
    assert seen == [(torch.bfloat16, True, True)]
    for a, b in zip(full, half):  # the stub computes in float32 from the bf16 input: close, not equal
        assert a["bbox"].tolist() == b["bbox"].tolist()
        assert (a["3dmm_params"] - b["3dmm_params"]).abs().max() < 0.05


def test_variant_entries_with_origin_zero_return_the_bits_of_the_existing_entries(flame_model):
    from dad_3dheads_amd import synthetic
    from dad_3dheads_amd.heatmap_points import points_from_landmarks

    pred = _predictor(flame_model, ("params",))
    lib, handle = _lib.load(), pred.head_mesh.flame._handle
    b = 70  # more than one workgroup of 64 rows
    rng = np.random.default_rng(3)
    geo5 = np.zeros((b, 5))
    geo5[:, 0], geo5[:, 1] = rng.integers(0, 100, b), rng.integers(0, 100, b)
    geo5[:, 2] = 256 / rng.integers(1, 3000, b).astype(np.float64)
    params = torch.from_numpy(synthetic.synthetic_params(b, seed=4)).cuda()
    old, new = params.clone(), params.clone()
    pads_scale = torch.tensor(geo5[:, :3], dtype=torch.float32).cuda()
    d_geo5 = torch.from_numpy(geo5).cuda()
    _lib.check(lib.dad3d_flame_readjust_params(handle, old.data_ptr(), b, pads_scale.data_ptr(), 0.0, 0.0, 1.0, None))
    _lib.check(lib.dad3d_flame_readjust_params_frame(handle, new.data_ptr(), b, d_geo5.data_ptr(), None))
    assert torch.equal(old.view(torch.int32), new.view(torch.int32))
    lm = torch.from_numpy(rng.uniform(-0.3, 1.3, (b, 68, 2)).astype(np.float32)).cuda()
    three = points_from_landmarks(lm, torch.from_numpy(geo5[:, :3].copy()).cuda(), 256)
    assert torch.equal(three, points_from_landmarks(lm, d_geo5, 256))
    geo5[:, 3], geo5[:, 4] = rng.integers(0, 4000, b), rng.integers(0, 4000, b)
    moved = points_from_landmarks(lm, torch.from_numpy(geo5).cuda(), 256)
    assert torch.equal(moved, three + torch.from_numpy(geo5[:, None, 3:]).cuda().to(torch.int32))


# ---- 4. no host wait -----------------------------------------------------------------------------------------------------------
def test_device_boxes_make_no_host_wait(flame_model, scene, monkeypatch):
    fr, boxes, crops, index = scene
    pred = _predictor(flame_model, ("params", "landmarks", "heatmap"))
    flat = np.concatenate([b.astype(np.float64) for b in boxes])
    flagged = np.concatenate([flat, [[5000, 5000, 10, 10], [NAN, 0, 1, 1]]])  # two flagged rows: they come back, with their flags
    flagged_index = np.concatenate([index, [0, 1]]).astype(np.int32)
    want = pred.predict_boxes(fr, boxes, device_outputs=True, points_on_device=True)
    d_frames = [torch.from_numpy(f).cuda() for f in fr]
    d_boxes, d_index = torch.from_numpy(flat).cuda(), torch.from_numpy(index).cuda()
    d_flagged, d_flagged_index = torch.from_numpy(flagged).cuda(), torch.from_numpy(flagged_index).cuda()
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError("a host wait")

    with monkeypatch.context() as m:
        for name in ("cpu", "item", "tolist", "numpy"):
            m.setattr(torch.Tensor, name, refuse)
        m.setattr(torch.cuda, "synchronize", refuse)
        got = pred.predict_boxes(d_frames, d_boxes, d_index, device_outputs=True, points_on_device=True)
        more = pred.predict_boxes(d_frames, d_flagged, d_flagged_index, device_outputs=True, points_on_device=True)
    keys = ("points", "projected_vertices", "3d_vertices", "3dmm_params", "bbox", "image_index", "flags")
    assert len(got) == len(want) == 5
    for g, w in zip(got, want):  # the same batch through the same kernels: the same bits
        for key in keys:
            assert g[key].is_cuda and torch.equal(g[key], w[key]), key
    assert [int(g["flags"]) for g in more] == [0, 0, 0, 0, 0, E, R]
    for g, w in zip(more, want):
        assert torch.equal(g["bbox"], w["bbox"]) and torch.equal(g["points"], w["points"])
    for g in more[5:]:
        for key in keys[:4]:
            assert bool(torch.isfinite(g[key].float()).all()), key


# ---- 5. the overlays -----------------------------------------------------------------------------------------------------------
def test_overlays_with_image_index_equal_sequential_single_head_calls(flame_model):
    from dad_3dheads_amd import overlay

    rng = np.random.default_rng(11)
    fr = [rng.integers(0, 256, (240, 320, 3), dtype=np.uint8), rng.integers(0, 256, (256, 208, 3), dtype=np.uint8)]
    boxes = [np.array([[10, 20, 100, 120], [150, 40, 140, 150], [60, 90, 90, 80]]), np.array([[30, 50, 120, 160]])]
    pred = _predictor(flame_model, ("params", "landmarks"))
    res = pred.predict_boxes(fr, boxes)
    index = [r["image_index"] for r in res]
    assert index == [0, 0, 0, 1]
    images = [torch.from_numpy(f).cuda() for f in fr]
    edges = overlay.mesh_edges()
    draws = {"landmarks": lambda p, im, **kw: overlay.draw_landmarks(p, im, **kw),
             "3d_landmarks": lambda p, im, **kw: overlay.draw_3d_landmarks(p, im, subset="191", **kw),
             "mesh": lambda p, im, **kw: overlay.draw_mesh(p, im, edges, **kw),
             "pose": lambda p, im, **kw: overlay.draw_pose(p, im, **kw)}
    for name, draw in draws.items():
        got = draw(res, images, image_index=index)
        running = [t.clone() for t in images]
        for r, i in zip(res, index):  # a loop over the reference's demo_utils: one head at a time on the running image
            running[i] = draw([r], [running[i]])[0]
        assert isinstance(got, list) and len(got) == 2
        for g, w, src in zip(got, running, images):
            assert torch.equal(g, w), name
            assert name not in ("landmarks", "pose") or not torch.equal(g, src), name  # something was drawn
    assert torch.equal(images[0], torch.from_numpy(fr[0]).cuda())  # the inputs stay as they were
