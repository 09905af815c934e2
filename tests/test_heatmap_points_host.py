"""CPU: the restatement the GPU tests of csrc/heatmap_points.hip are held to (tests/heatmap_points_restatement.py) is itself
held to np.argmax / torch.argmax with the reference's `// H, % H` unravel and to the literal numpy lines of predictor.py:132-152;
and the two entry points refuse bad arguments before any device work, so the refusals need no GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import heatmap_points_restatement as rs
from dad_3dheads_amd import _lib

NAN, INF = float("nan"), float("inf")


def _unravel_reference(x):
    """model_training/model/utils.py:49-52, literally."""
    B, C_, H, W = x.shape
    max_tensor = x.view(B, C_, -1).argmax(-1).view(-1, 1)
    return torch.cat((torch.div(max_tensor, H, rounding_mode="trunc"), max_tensor % H), dim=1).reshape(B, C_, 2)


PLANES = {
    "single": [3.0],
    "ties": [1.0, 5.0, 5.0, 2.0, 5.0],
    "first_is_max": [9.0, 1.0, 9.0],
    "nan_behind_larger": [1.0, 100.0, NAN, 200.0],
    "two_nans": [INF, NAN, 0.0, NAN],
    "nan_first": [NAN, 1.0],
    "minus_zero_first": [-1.0, -0.0, 0.0, -0.0],
    "plus_zero_first": [-1.0, 0.0, -0.0],
    "all_minus_inf": [-INF] * 6,
    "all_equal": [2.5] * 7,
    "inf_and_max": [3.0e38, INF, INF],
    "negatives": [-3.0, -2.0, -2.0, -5.0],
}


@pytest.mark.parametrize("name", sorted(PLANES))
def test_flat_peak_is_numpy_and_torch_argmax(name):
    v = np.array(PLANES[name], dtype=np.float32)
    k = rs.flat_peak(v)
    assert k == int(np.argmax(v)), (name, k)
    assert k == int(torch.from_numpy(v).argmax()), (name, k)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16, torch.uint8])
@pytest.mark.parametrize("hw", [(1, 1), (1, 2), (3, 5), (5, 3), (8, 8)])
def test_peaks_are_the_reference_unravel(dtype, hw):
    h, w = hw
    g = torch.Generator().manual_seed(h * 100 + w)
    x = torch.randint(0, 6, (2, 3, h, w), generator=g)  # few distinct values: ties in every plane
    x = x.to(dtype) if dtype == torch.uint8 else (x.to(torch.float32) - 2.5).to(dtype)
    if dtype != torch.uint8 and h * w > 2:
        x[0, 1].view(-1)[h * w - 1] = NAN
        x[1, 2].view(-1)[1] = NAN
        x[1, 2].view(-1)[2] = NAN
    want = _unravel_reference(x).numpy()
    vals = x.to(torch.float32).numpy() if dtype in (torch.bfloat16, torch.float16) else x.numpy()  # exact widening keeps order and ties
    got = rs.peaks(vals.reshape(2, 3, h * w), h)
    assert got.shape == (2, 3, 2) and np.array_equal(got, want)


def test_unravel_divides_by_h_where_h_differs_from_w():
    x = torch.zeros(1, 1, 3, 5)
    x[0, 0, 2, 4] = 1.0  # flat 14 -> (14 // 3, 14 % 3) = (4, 2), not (2, 4)
    assert rs.peaks(x.numpy().reshape(1, 1, 15), 3).tolist() == [[[4, 2]]]
    assert _unravel_reference(x).tolist() == [[[4, 2]]]


def _predictor_lines(landmarks, img_size, paddings, scale):
    """predictor.py:132-133 and 150-152, literally."""
    landmarks = landmarks.clip(min=0, max=img_size)
    landmarks = landmarks - np.array([[paddings[2], paddings[0]]])
    landmarks = (landmarks / scale).astype(int)
    return landmarks


GEOMETRIES = [  # (paddings = [top, bottom, left, right], scale)
    ([0, 0, 32, 32], 256 / float(683)),
    ([37, 36, 0, 0], 256 / float(911)),
    ([0, 1, 0, 0], 256 / float(257)),
    ([13, 14, 0, 0], 256 / float(100)),
    ([0, 0, 0, 0], 1.0),
]


@pytest.mark.parametrize("geo", GEOMETRIES)
def test_points_regressed_are_the_predictor_lines(geo):
    paddings, scale = geo
    rng = np.random.default_rng(5)
    lm = rng.uniform(-0.2, 1.2, size=(1, 68, 2)).astype(np.float32)  # below 0 and above 256 after the product
    lm[0, :6] = [[0.0, 1.0], [1.0, 0.0], [-0.0, 0.5], [0.999999, 1.000001], [INF, -INF], [0.25, 0.75]]
    want = _predictor_lines(lm[0] * 256.0, 256, paddings, scale)  # predictor.py:107: float32 array * python float
    got = rs.points(lm, 0, 256.0, 256, (paddings[2], paddings[0], scale))
    assert want.dtype == np.int64 and np.array_equal(got[0], want)


@pytest.mark.parametrize("geo", GEOMETRIES)
@pytest.mark.parametrize("stride", [2, 4])
def test_points_from_peaks_are_the_predictor_lines(geo, stride):
    paddings, scale = geo
    rng = np.random.default_rng(6)
    yx = rng.integers(0, 256 // stride + 3, size=(1, 68, 2)).astype(np.int32)  # a few beyond the image: clipped
    xy = yx[0, :, ::-1]
    want = _predictor_lines(float(stride) * xy.astype(np.int64), 256, paddings, scale)  # predictor.py:111-112
    got = rs.points(yx, 1, float(stride), 256, (paddings[2], paddings[0], scale))
    assert np.array_equal(got[0], want)


def test_points_per_image_geometry_and_nan():
    lm = np.array([[[0.5, 0.5], [NAN, 0.25]], [[0.5, 0.5], [2.0, -1.0]]], dtype=np.float32)
    geo = np.array([[32, 0, 256 / 683.0], [0, 37, 256 / 911.0]])
    got = rs.points(lm, 0, 256.0, 256, geo)
    assert got[0, 0].tolist() == [int((128.0 - 32) / (256 / 683.0)), int(128.0 / (256 / 683.0))]
    assert got[0, 1].tolist() == [rs.INT32_MIN, int(64.0 / (256 / 683.0))]
    assert got[1, 1].tolist() == [int(256.0 / (256 / 911.0)), int(-37 / (256 / 911.0))]


# -- the refusals: validation comes before any device work -------------------------------------------------------------------
def _argmax(heatmap=0x1000, dtype=0, batch=1, channels=1, h=2, w=2, layout=0, sigmoid=0, yx=0x2000, peak=None):
    return _lib.load().dad3d_heatmap_argmax(heatmap, dtype, batch, channels, h, w, layout, sigmoid, yx, peak, 0, None)


def _readjust(src=0x1000, kind=0, batch=1, n=1, geometry=None, scale=1.0, out=0x2000):
    return _lib.load().dad3d_points_readjust(src, kind, batch, n, 256.0, 256.0, geometry, 0, 0, scale, out, 0, None)


@pytest.mark.parametrize("kw,word", [
    (dict(heatmap=None), b"null"), (dict(yx=None), b"null"),
    (dict(batch=0), b"bad size"), (dict(channels=0), b"bad size"), (dict(h=0), b"bad size"), (dict(w=-1), b"bad size"),
    (dict(h=4097, w=4096), b"2^24"), (dict(batch=65536, channels=65536), b"launch grid"),
    (dict(dtype=4), b"unknown dtype"), (dict(dtype=-1), b"unknown dtype"),
    (dict(layout=2), b"unknown layout"), (dict(layout=-1), b"unknown layout"),
    (dict(dtype=_lib.HEATMAP_DTYPE_U8, sigmoid=1), b"uint8"),
    (dict(heatmap=0x1002, dtype=_lib.DTYPE_F32), b"aligned"), (dict(heatmap=0x1001, dtype=_lib.DTYPE_BF16), b"aligned"),
])
def test_heatmap_argmax_refuses_before_device_work(kw, word):
    assert _argmax(**kw) == _lib.E_INVALID
    assert word in _lib.load().dad3d_last_error()


def test_heatmap_argmax_takes_a_plane_of_exactly_2_pow_24_positions_up_to_validation():
    # 4096 x 4096 passes the size check: the next refusal in line is the null pointer's
    assert _argmax(heatmap=None, h=4096, w=4096) == _lib.E_INVALID
    assert b"null" in _lib.load().dad3d_last_error()


@pytest.mark.parametrize("kw,word", [
    (dict(src=None), b"null"), (dict(out=None), b"null"),
    (dict(batch=0), b"bad size"), (dict(n=0), b"bad size"), (dict(batch=-3), b"bad size"),
    (dict(batch=1 << 20, n=1 << 11), b"launch grid"),
    (dict(kind=2), b"unknown src_kind"), (dict(kind=-1), b"unknown src_kind"),
    (dict(scale=0.0), b"scale"), (dict(scale=-1.0), b"scale"), (dict(scale=float("nan")), b"scale"), (dict(scale=float("inf")), b"scale"),
])
def test_points_readjust_refuses_before_device_work(kw, word):
    assert _readjust(**kw) == _lib.E_INVALID
    assert word in _lib.load().dad3d_last_error()


def test_signatures_are_bound():
    lib = _lib.load()
    assert lib.dad3d_points_readjust.argtypes[9] is C.c_double  # the scale travels as the float64 it is
    assert len(lib.dad3d_heatmap_argmax.argtypes) == 12
