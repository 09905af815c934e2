"""GPU: csrc/heatmap_points.hip (`dad3d_heatmap_argmax`, `dad3d_points_readjust`) and its callers -- heatmap_points.py, the
predictor's `points`, StepMetrics' heatmap branch -- against the CPU restatement (tests/heatmap_points_restatement.py, itself
held to np.argmax and the reference's lines by test_heatmap_points_host.py) and against torch on the device. Everything is
exact equality of integers.

Seams of the kernels the planted positions straddle: a 16-byte vector (4, 8 or 16 elements), a wave's sweep (64 lanes: 256, 512,
1024 elements), a 256-thread workgroup's sweep (1024, 2048, 4096), the scalar head and tail of a plane that is not 16-byte
aligned (65 x 63), and for channels-last with 68 channels the 30 pixel slots of a workgroup, its four loads in flight (120) and the
runs of pixels a split launch gives its workgroups (multiples of 256 at 64 x 64, of 273 at 65 x 63)."""
import numpy as np
import pytest
import torch

import heatmap_points_restatement as rs
import train_objective_restatement as tor
from dad_3dheads_amd import _lib, heatmap_points as hp

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
DTYPES = [torch.float32, torch.float16, torch.bfloat16, torch.uint8]
NCHW, NHWC = _lib.LAYOUT_NCHW, _lib.LAYOUT_NHWC
INT_VIEW = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}


def argmax_raw(x, layout, sigmoid=False, peak=False):
    """The C entry on the values of `x` ([B,C,H,W], any device) laid out as `layout` says, whatever the sizes: a tensor of one
    channel or one pixel is contiguous both ways, so `heatmap_peaks` alone could not choose the layout for it."""
    x = x.cuda()
    b, c, h, w = x.shape
    buf = x.contiguous() if layout == NCHW else x.permute(0, 2, 3, 1).contiguous()
    yx = torch.full((b, c, 2), -7, dtype=torch.int32, device="cuda")
    pk = torch.full((b, c), -7.0, dtype=torch.float32, device="cuda") if peak else None
    _lib.check(_lib.load().dad3d_heatmap_argmax(buf.data_ptr(), hp._DTYPE[x.dtype], b, c, h, w, layout, int(sigmoid), yx.data_ptr(),
                                                None if pk is None else pk.data_ptr(), 0, torch.cuda.current_stream().cuda_stream))
    return (yx, pk) if peak else yx


def torch_peaks(x, sigmoid=False):
    """unravel_index (model/utils.py:49-52) on the device; a uint8 heatmap is widened first (exact, keeps order and ties)."""
    x = x.cuda()
    v = torch.sigmoid(x) if sigmoid else (x.float() if x.dtype == torch.uint8 else x)
    h = x.shape[2]
    k = v.flatten(2).argmax(-1)
    return torch.stack((torch.div(k, h, rounding_mode="trunc"), k % h), dim=-1).to(torch.int32), v.flatten(2).gather(2, k[..., None])[..., 0].float()


# ---- shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [NCHW, NHWC])
@pytest.mark.parametrize("dtype", DTYPES)
def test_shapes_equal_torch_on_the_device(dtype, layout):
    g = torch.Generator().manual_seed(31)
    for h, w in [(1, 1), (1, 2), (3, 5), (8, 8), (65, 63), (64, 64)]:
        for c in (1, 3, 68, 70):
            for b in (1, 2, 5):
                # few distinct values: ties in every plane; +-20 is beyond every dtype's sigmoid saturation (6.25, 8.32, 16.64)
                x = torch.randint(0, 41, (b, c, h, w), generator=g)
                x = x.to(torch.uint8) if dtype == torch.uint8 else (x - 20).to(dtype)
                if dtype != torch.uint8 and h * w >= 15:
                    x[0, 0].view(-1)[h * w - 2] = NAN  # a NaN wins over every number
                    x[-1, -1].view(-1)[7] = NAN
                    x[-1, -1].view(-1)[11] = NAN  # the first NaN wins
                for sig in ([False] if dtype == torch.uint8 else [False, True]):
                    want, want_peak = torch_peaks(x, sig)
                    got, got_peak = argmax_raw(x, layout, sig, peak=True)
                    assert torch.equal(got, want), (h, w, c, b, sig, (got != want).nonzero()[:4].tolist())
                    torch.testing.assert_close(got_peak, want_peak, rtol=0, atol=0, equal_nan=True)


def test_heatmap_peaks_picks_the_layout_from_the_strides():
    g = torch.Generator().manual_seed(32)
    x = torch.randn(3, 68, 17, 16, generator=g).cuda()
    want, want_peak = torch_peaks(x)
    cl = x.contiguous(memory_format=torch.channels_last)
    assert not cl.is_contiguous()
    assert torch.equal(hp.heatmap_peaks(x), want) and torch.equal(hp.heatmap_peaks(cl), want)
    yx, peak = hp.heatmap_peaks(cl, return_peak=True)
    assert yx.dtype == torch.int32 and torch.equal(yx, want) and torch.equal(peak, want_peak)
    wide = torch.randn(3, 70, 17, 40, generator=g).cuda()
    view = wide[:, 1:69, :, 3:19]  # neither contiguous nor channels-last: made contiguous first
    assert torch.equal(hp.heatmap_peaks(view), torch_peaks(view.contiguous())[0])
    off = torch.randn(2 * 68 * 15 * 15 + 1, generator=g).cuda()[1:].view(2, 68, 15, 15)  # 4-byte aligned only
    assert torch.equal(hp.heatmap_peaks(off), torch_peaks(off)[0])
    off_cl = off.contiguous(memory_format=torch.channels_last)
    assert torch.equal(hp.heatmap_peaks(off_cl), torch_peaks(off)[0])
    with pytest.raises(ValueError):
        hp.heatmap_peaks(x[0])
    with pytest.raises(ValueError):
        hp.heatmap_peaks(x.cpu())
    with pytest.raises(_lib.Dad3dError):
        hp.heatmap_peaks(x.to(torch.uint8), sigmoid=True)


def test_channels_last_with_an_output_that_is_only_4_byte_aligned():
    """A split launch keeps its packed pairs in yx_out, which needs 8-byte alignment; without it one workgroup takes the image."""
    g = torch.Generator().manual_seed(33)
    x = torch.randint(-20, 21, (2, 68, 64, 64), generator=g).float().cuda()
    buf = x.permute(0, 2, 3, 1).contiguous()
    yx = torch.full((2 * 68 * 2 + 1,), -7, dtype=torch.int32, device="cuda")[1:]
    assert yx.data_ptr() % 8 == 4
    _lib.check(_lib.load().dad3d_heatmap_argmax(buf.data_ptr(), _lib.DTYPE_F32, 2, 68, 64, 64, NHWC, 1, yx.data_ptr(), None, 0,
                                                torch.cuda.current_stream().cuda_stream))
    assert torch.equal(yx.view(2, 68, 2), torch_peaks(x, sigmoid=True)[0])


# ---- planted cases ---------------------------------------------------------------------------------------------------------
SEAMS = [0, 1, 3, 4, 7, 8, 15, 16, 29, 30, 31, 32, 59, 60, 63, 64, 119, 120, 127, 128, 255, 256, 272, 273, 274, 509, 510, 511, 512,
         545, 546, 547, 1023, 1024, 2047, 2048]
_planted_cache = {}


def planted(hw, dtype):
    """(values [P, hw] of `dtype` on the CPU, expected flat index [P] from the restatement, which must agree with the index every
    case was planted at by hand). Built once per (hw, dtype) and left unchanged."""
    if (hw, dtype) in _planted_cache:
        return _planted_cache[hw, dtype]
    last = hw - 1
    pos = sorted({p for p in SEAMS + [last - 1, last] if 0 <= p <= last})
    is_u8 = dtype == torch.uint8
    lo, hi = (1, 200) if is_u8 else (-1.0, 5.0)
    rows, by_hand = [], []

    def plane(fill=lo):
        return torch.full((hw,), fill, dtype=dtype)

    for p in pos:  # the maximum alone at p
        v = plane()
        v[p] = hi
        rows.append(v), by_hand.append(p)
    for p in pos[1:]:  # equal maxima on both sides of the seam in front of p: the lower index wins
        v = plane()
        v[p - 1] = v[p] = hi
        rows.append(v), by_hand.append(p - 1)
    for p in pos[:-1]:  # and far apart
        v = plane()
        v[p] = v[last] = hi
        rows.append(v), by_hand.append(p)
    rows.append(plane(hi)), by_hand.append(0)  # an all-equal plane
    rng = torch.Generator().manual_seed(hw)
    if is_u8:
        rows.append(plane(0)), by_hand.append(0)
        for _ in range(4):  # random planes, the top value several times
            v = torch.randint(0, 250, (hw,), generator=rng).to(torch.uint8)
            at = torch.randperm(hw, generator=rng)[:6]
            v[at] = torch.tensor([251, 255, 253, 255, 254, 255], dtype=torch.uint8)
            rows.append(v), by_hand.append(int(at[[1, 3, 5]].min()))
    else:
        a, b_ = 700 % hw, 5
        v = plane()
        v[b_], v[a] = 100.0, NAN  # a NaN behind a larger number
        rows.append(v), by_hand.append(a)
        v = plane()
        v[300 % hw], v[900 % hw], v[5] = NAN, NAN, INF  # two NaNs: the first
        rows.append(v), by_hand.append(min(300 % hw, 900 % hw))
        v = plane()
        v[10], v[20] = -0.0, 0.0  # -0.0 == +0.0: the first
        rows.append(v), by_hand.append(10)
        v = plane()
        v[10], v[20] = 0.0, -0.0
        rows.append(v), by_hand.append(10)
        rows.append(plane(-INF)), by_hand.append(0)  # an all -inf plane
        v = plane()
        v[5], v[77] = 3.0e4, INF
        rows.append(v), by_hand.append(77)
        top = int(torch.tensor([1.0], dtype=dtype).view(INT_VIEW[dtype])[0])
        for _ in range(4):  # random planes with a 4-ulp cluster at the top, its largest member twice
            v = torch.rand(hw, generator=rng).to(dtype)
            at = torch.randperm(hw, generator=rng)[:6]
            v.view(INT_VIEW[dtype])[at] = top + torch.tensor([1, 4, 3, 4, 0, 2]).to(INT_VIEW[dtype])
            rows.append(v), by_hand.append(int(at[[1, 3]].min()))
    vals = torch.stack(rows)
    wide = vals.float().numpy()  # exact for all four dtypes
    expect = np.array([rs.flat_peak(r) for r in wide], dtype=np.int64)
    hand = np.array(by_hand, dtype=np.int64)
    assert np.array_equal(expect, hand), (expect != hand).nonzero()  # the restatement agrees with every index planted by hand
    _planted_cache[hw, dtype] = (vals, expect)
    return _planted_cache[hw, dtype]


@pytest.mark.parametrize("layout", [NCHW, NHWC])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw", [(64, 64), (65, 63)])
def test_planted_cases_equal_the_restatement_and_torch(hw, dtype, layout):
    h, w = hw
    vals, expect = planted(h * w, dtype)
    c = 68
    b = -(-vals.shape[0] // c)
    x = vals[0][None].repeat(b * c, 1)  # the planes behind the last case repeat the first one
    x[: vals.shape[0]] = vals
    x = x.view(b, c, h, w)
    k = np.concatenate([expect, np.full(b * c - len(expect), expect[0])]).reshape(b, c)
    want = np.stack((k // h, k % h), axis=-1)
    got = argmax_raw(x, layout)
    assert np.array_equal(got.cpu().numpy(), want), (got.cpu().numpy() != want).any(-1).nonzero()
    assert torch.equal(got, torch_peaks(x)[0])
    if dtype != torch.uint8:  # with the sigmoid in front: torch on the device (the planted maxima saturate in bf16 and fp16 only)
        assert torch.equal(argmax_raw(x, layout, sigmoid=True), torch_peaks(x, sigmoid=True)[0])


@pytest.mark.parametrize("layout", [NCHW, NHWC])
@pytest.mark.parametrize("dtype,first,larger", [(torch.float32, 18.0, 25.0), (torch.bfloat16, 7.0, 9.0), (torch.float16, 9.0, 12.0)])
def test_sigmoid_first_saturated_position_wins(dtype, first, larger, layout):
    x = torch.full((1, 1, 8, 8), -30.0, dtype=dtype)
    x[0, 0, 1, 2], x[0, 0, 5, 5] = first, larger
    assert float(torch.sigmoid(x)[0, 0, 1, 2]) == 1.0  # saturated on the CPU as well
    (yx, peak), (yx0, peak0) = argmax_raw(x, layout, sigmoid=True, peak=True), argmax_raw(x, layout, sigmoid=False, peak=True)
    assert yx.tolist() == [[[1, 2]]] and yx0.tolist() == [[[5, 5]]]
    assert peak.tolist() == [[1.0]] and peak0.tolist() == [[larger]]
    assert torch.equal(yx, torch_peaks(x, sigmoid=True)[0]) and torch.equal(yx0, torch_peaks(x)[0])
    x = x.repeat(2, 68, 1, 1).cuda()  # the module's entry, 68 channels, both memory formats
    x = x if layout == NCHW else x.contiguous(memory_format=torch.channels_last)
    assert hp.heatmap_peaks(x, sigmoid=True).unique(dim=1).tolist() == [[[1, 2]]] * 2
    assert hp.heatmap_peaks(x).unique(dim=1).tolist() == [[[5, 5]]] * 2


# ---- the sigmoid's bits ----------------------------------------------------------------------------------------------------
def _pair_disagreements(a, b, layout):
    """Planes [a_i, b_i] (H = 1, W = 2): the kernel's index against torch.sigmoid(x).flatten(2).argmax(-1) on the device."""
    x = torch.stack((a, b), dim=-1)
    n = x.shape[0]
    bsz = 4096 if n % 4096 == 0 else 1
    x = x.view(bsz, n // bsz, 1, 2)
    want = torch.sigmoid(x).flatten(2).argmax(-1)
    got = argmax_raw(x, layout, sigmoid=True)
    assert int(got[..., 1].abs().max()) == 0  # k % 1
    bad = (got[..., 0] != want).flatten().nonzero().flatten()
    ties = int((want == 0).sum())
    return bad, ties


def test_sigmoid_sweep_float32_every_adjacent_pair_in_2_to_18():
    """Every float32 a in [2, 18) with b the next float after it: 26 214 400 pairs, in chunks of 2^22 planes. The answer is 0 exactly
    where sigmoid(a) == sigmoid(b), so one disagreement with the framework's kernel in the last bit of any of them shows here."""
    lo = int(torch.tensor([2.0]).view(torch.int32)[0])
    hi = int(torch.tensor([18.0]).view(torch.int32)[0])
    assert hi - lo == 26214400
    n_bad, n_ties, first = 0, 0, None
    chunk = 1 << 22
    for start in range(lo, hi, chunk):
        bits = torch.arange(start, min(start + chunk, hi), dtype=torch.int32, device="cuda")
        if bits.numel() % 4096:  # the last chunk: pad with its last pair
            bits = torch.cat((bits, bits[-1:].expand(4096 - bits.numel() % 4096)))
        a, b = bits.view(torch.float32), (bits + 1).view(torch.float32)
        bad, ties = _pair_disagreements(a, b, NCHW)
        n_ties += ties
        if bad.numel() and first is None:
            first = (float(a[bad[0]]), float(b[bad[0]]))
        n_bad += int(bad.numel())
    print(f"float32 sweep: {hi - lo} pairs, {n_ties} with equal sigmoids, {n_bad} disagreements, first {first}")
    assert n_bad == 0, (n_bad, first)
    assert n_ties > 0  # from 16.636066 up every pair is a tie


@pytest.mark.parametrize("layout", [NCHW, NHWC])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_sigmoid_sweep_every_adjacent_finite_pair_of_16_bit_patterns(dtype, layout):
    allp = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dtype)
    fin = allp[torch.isfinite(allp.float())]
    order = torch.sort(fin.float(), stable=True).indices  # by value; -0.0 and +0.0 stay a pair
    s = fin[order].cuda()
    a, b = s[:-1], s[1:]
    assert a.numel() == fin.numel() - 1 and a.numel() > 63000
    bad, ties = _pair_disagreements(a, b, layout)
    first = (float(a[bad[0]]), float(b[bad[0]])) if bad.numel() else None
    print(f"{dtype} sweep, layout {layout}: {a.numel()} pairs, {ties} with equal sigmoids, {bad.numel()} disagreements, first {first}")
    assert bad.numel() == 0, (int(bad.numel()), first)


# ---- points_readjust -------------------------------------------------------------------------------------------------------
GEO = [(32, 0, 256 / float(683)), (0, 37, 256 / float(911)), (0, 0, 256 / float(257)), (0, 13, 256 / float(100)), (7, 0, 1.0)]


@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("b,n", [(1, 1), (1, 68), (5, 1), (5, 68)])
def test_points_readjust_equals_the_restatement(b, n, kind, per_image):
    rng = np.random.default_rng(100 * b + n + kind)
    if kind == 0:
        src = rng.uniform(-0.2, 1.2, (b, n, 2)).astype(np.float32)
        flat = src.reshape(-1)
        flat[0] = INF
        flat[1 % flat.size] = -INF
        flat[-1] = NAN
        if flat.size > 8:
            flat[3:8] = [0.0, 1.0, -0.0, 0.99999994, 1.0000001]
        mul = 256.0
    else:
        src = rng.integers(0, 70, (b, n, 2)).astype(np.int32)  # stride 4: up to 276, beyond the clip
        mul = 4.0
    geo = [GEO[i % len(GEO)] for i in range(b)] if per_image else GEO[1]
    got = hp._readjust(torch.from_numpy(src).cuda(), kind, mul, 256, geo)
    assert got.dtype == torch.int32 and got.shape == (b, n, 2)
    want = rs.points(src, kind, mul, 256, np.array(geo))
    assert np.array_equal(got.cpu().numpy(), want)
    if kind == 0:
        assert got.flatten()[-1] == rs.INT32_MIN  # the NaN: pinned as this project's choice
        as_tensor = hp.points_from_landmarks(torch.from_numpy(src.reshape(b, -1)).cuda(), torch.tensor(np.array(geo).reshape(-1, 3)).expand(b, 3), 256)
        assert torch.equal(as_tensor, got)  # [B,2n] landmarks and a float64 tensor of triples: the same launch


# ---- the predictor ---------------------------------------------------------------------------------------------------------
class Regressor(torch.nn.Module):
    """{"OUTPUT_3DMM_PARAMS": [B,413], "OUTPUT_2D_LANDMARKS": [B,68,2]}; the landmarks reach below 0 and above 1."""

    def __init__(self):
        super().__init__()
        from dad_3dheads_amd import synthetic

        self.register_buffer("w", torch.randn(3, 413, generator=torch.Generator().manual_seed(0)) * 0.5)
        self.register_buffer("base", torch.from_numpy(synthetic.synthetic_params(1, seed=8))[0])

    def params(self, x):
        feat = x.mean(dim=(2, 3))
        return feat, self.base[None] + 0.05 * torch.tanh(feat @ self.w)

    def forward(self, x):
        feat, p = self.params(x)
        lm = torch.sigmoid(feat[:, :2])[:, None, :] * torch.linspace(-0.3, 2.2, 68, device=x.device)[None, :, None]
        return {"OUTPUT_3DMM_PARAMS": p, "OUTPUT_2D_LANDMARKS": lm}


class HeatmapOnly(Regressor):
    """A model without the landmark head: the params and the [B,68,64,64] heatmap, contiguous or channels-last. Some logits are
    beyond the float32 sigmoid's saturation, so the first saturated position differs from the largest logit."""

    def __init__(self, channels_last):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        hm = 4.0 * torch.randn(68, 64, 64, generator=g)
        at = torch.randint(0, 64 * 64, (68, 3), generator=g)
        hm.view(68, -1).scatter_(1, at, torch.tensor([[17.0, 30.0, 18.5]]).expand(68, 3))
        self.register_buffer("hm", hm)
        self.channels_last = channels_last

    def forward(self, x):
        feat, p = self.params(x)
        hm = self.hm[None] + torch.roll(self.hm, 5, -1)[None] * feat[:, :1, None, None]  # differs from image to image
        if self.channels_last:
            hm = hm.contiguous(memory_format=torch.channels_last)
        return {"OUTPUT_3DMM_PARAMS": p, "OUTPUT_LANDMARKS_HEATMAP": hm}


def _predictor(model, flame_model):
    from dad_3dheads_amd.config import load_default_config
    from dad_3dheads_amd.predictor import FaceMeshPredictor

    return FaceMeshPredictor(load_default_config(), cuda_id=0, model=model, flame_model=flame_model)


def _network_output(pred, images):
    staged = [torch.from_numpy(im).cuda() for im in images]
    batch = pred._preprocess_launch([(t.data_ptr(), t.shape[0], t.shape[1], t.shape[1] * 3) for t in staged])
    return pred.process(batch)


@pytest.mark.parametrize("hw", [(100, 180), (300, 211)])
def test_predict_tensor_regressed_points_equal_the_torch_chain_they_replace(flame_model, hw):
    pred = _predictor(Regressor(), flame_model)
    rng = np.random.default_rng(hw[0])
    images = rng.integers(0, 256, (3, hw[0], hw[1], 3), dtype=np.uint8)
    pads, scale, _ = pred._geometry(hw)
    assert pads[0] + pads[2] > 0  # a non-zero pad
    got = pred.predict_tensor(torch.from_numpy(images).cuda())["points"]
    out = _network_output(pred, list(images))
    # the expression predict_tensor had before the kernel
    pts = (out["OUTPUT_2D_LANDMARKS"].detach().float() * 256.0).clamp_(0, 256).double()
    pts = (pts - torch.tensor([pads[2], pads[0]], device="cuda", dtype=torch.float64)) / scale
    want = pts.to(torch.int32)
    assert got.dtype == torch.int32 and got.shape == (3, 68, 2)
    assert torch.equal(got, want), (got != want).nonzero()[:4].tolist()
    assert int((pts == 0).sum()) > 0 or int(want.min()) < 0  # the clip was at work


def _reference_points(heatmap_sigmoid_cpu, stride, img_size, paddings, scale):
    """predictor.py:111-112,132-133,150-152 on one image's sigmoid(heatmap) [1,C,H,W], literally."""
    x = heatmap_sigmoid_cpu
    B, C_, H, W = x.shape
    max_tensor = x.view(B, C_, -1).argmax(-1).view(-1, 1)
    keypoints = torch.cat((torch.div(max_tensor, H, rounding_mode="trunc"), max_tensor % H), dim=1).reshape(B, C_, 2)
    landmarks = float(stride) * keypoints.flip(-1)[0].cpu().numpy()
    landmarks = landmarks.clip(min=0, max=img_size)
    landmarks = landmarks - np.array([[paddings[2], paddings[0]]])
    return (landmarks / scale).astype(int)


@pytest.mark.parametrize("channels_last", [False, True])
def test_predictor_with_a_heatmap_only_model(flame_model, channels_last):
    pred = _predictor(HeatmapOnly(channels_last), flame_model)
    rng = np.random.default_rng(9)
    images = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in [(100, 180), (300, 211), (100, 180)]]
    out = _network_output(pred, images)
    hm = out["OUTPUT_LANDMARKS_HEATMAP"]
    assert hm.is_contiguous() != channels_last
    sig = torch.sigmoid(hm).cpu().contiguous()
    want = []
    for i, im in enumerate(images):
        pads, scale, _ = pred._geometry(im.shape[:2])
        want.append(_reference_points(sig[i : i + 1], 4, 256, pads, scale))
    assert len({w.tobytes() for w in want}) == 3  # the points differ from image to image
    res = pred.predict_batch(images)
    for r, w in zip(res, want):
        assert set(r) == {"points", "projected_vertices", "3d_vertices", "3dmm_params"}
        assert isinstance(r["points"], np.ndarray) and r["points"].dtype == w.dtype and r["points"].shape == (68, 2)
        assert np.array_equal(r["points"], w)
    dev = pred.predict_batch(images, device_outputs=True, points_on_device=True)
    for r, w in zip(dev, want):
        assert r["points"].is_cuda and r["points"].dtype == torch.int32 and r["points"].shape == (68, 2)
        assert r["3d_vertices"].is_cuda and np.array_equal(r["points"].cpu().numpy(), w)
    same = np.stack([images[0], images[2]])
    t = pred.predict_tensor(torch.from_numpy(same).cuda())
    assert "points" in t and t["points"].dtype == torch.int32
    assert np.array_equal(t["points"].cpu().numpy(), np.stack([want[0], want[2]]))


# ---- StepMetrics -----------------------------------------------------------------------------------------------------------
def test_step_metrics_heatmap_only_outputs(flame_model, static, flame_consts):
    from dad_3dheads_amd import landmarks, metrics, synthetic
    from dad_3dheads_amd.head_mesh import HeadMesh
    from oracle import flame_ref

    hm = HeadMesh(flame_model=flame_model, landmarks=landmarks.canonical("445", static), static=static, device=0)
    b, c, stride = 3, 68, 4
    face = np.arange(0, 5023, 3)
    params = torch.from_numpy(synthetic.synthetic_params(b, seed=120)).cuda()
    tgt3d = flame_ref.vertices_3d(flame_consts, torch.from_numpy(synthetic.synthetic_params(b, seed=121)), zero_rotation=True)
    tgt2d = flame_ref.reprojected_vertices(flame_consts, torch.from_numpy(synthetic.synthetic_params(b, seed=122)))
    logits, t8 = tor.iou_inputs(123, b, c, 64, 64)  # plane (0, 0) is +-60: saturated under a sigmoid, a tie of raw logits
    rng = np.random.default_rng(124)
    lmk, lmk_t = rng.uniform(0.1, 0.9, (b, c, 2)).astype(np.float32), rng.uniform(0.1, 0.9, (b, c, 2)).astype(np.float32)
    pres = (rng.random((b, c)) < 0.8).astype(np.float32)
    bbox = np.stack([np.zeros(b), np.zeros(b), rng.integers(150, 250, b), rng.integers(150, 250, b)], 1).astype(np.int64)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    targets = {"TARGET_LANDMARKS_HEATMAP": cu(t8), "TARGET_2D_LANDMARKS": cu(lmk_t), "TARGET_2D_LANDMARKS_PRESENCE": cu(pres),
               "TARGET_2D_FULL_LANDMARKS": tgt2d.cuda(), "TARGET_3D_MODEL_VERTICES": tgt3d.cuda(), "INPUT_BBOX_KEY": cu(bbox)}
    yx = rs.peaks(logits.reshape(b, c, -1), 64)  # the raw logits: no sigmoid on the training step
    pred = (float(stride) * yx[..., ::-1]).astype(np.float32)
    for memory_format in (torch.contiguous_format, torch.channels_last):
        outputs = {"OUTPUT_LANDMARKS_HEATMAP": cu(logits).contiguous(memory_format=memory_format), "OUTPUT_3DMM_PARAMS": params}
        sm = metrics.StepMetrics(hm, {"face": face}, 256, stride)
        got = sm(outputs, targets)
        assert {"heatmap_iou", "fr_2d_005", "fr_2d_01", "nme_2d"} <= set(got)
        out, _ = metrics.keypoint_errors(cu(pred), cu(lmk_t), cu(bbox), presence=cu(pres), pred_scale=1.0, target_scale=256,
                                         thresholds=(0.05, 0.1))
        assert float(got["fr_2d_005"]) == float(out[1]) and float(got["fr_2d_01"]) == float(out[2])
        assert float(got["nme_2d"]) == float(100 * out[0])
        e, n = tor.keypoint_errors(pred, lmk_t, bbox, presence=pres, pred_scale=1.0, target_scale=256)
        nme, rates = tor.nme_and_rates(e, n)
        assert abs(float(got["nme_2d"]) - 100 * nme) <= 1e-6 * 100 * nme
        assert [float(got["fr_2d_005"]), float(got["fr_2d_01"])] == rates
    assert metrics.StepMetrics(hm, {"face": face}, 256).stride == 2  # config["train"].get("stride", 2)
    # with the regressed landmarks present the heatmap is not consulted for the points: the results are the regressed branch's
    both = dict(outputs, OUTPUT_2D_LANDMARKS=cu(lmk))
    got = metrics.StepMetrics(hm, {"face": face}, 256, stride)(both, targets)
    out, _ = metrics.keypoint_errors(cu(lmk), cu(lmk_t), cu(bbox), presence=cu(pres), pred_scale=256, target_scale=256, thresholds=(0.05, 0.1))
    assert float(got["fr_2d_005"]) == float(out[1]) and float(got["fr_2d_01"]) == float(out[2]) and float(got["nme_2d"]) == float(100 * out[0])
