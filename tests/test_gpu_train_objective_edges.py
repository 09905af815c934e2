"""GPU: the training-objective kernels (csrc/train_objective.hip) at their seams and ties, on the cases of
tests/train_objective_cases.py -- inputs on dyadic grids whose float64 sums are exact in any order, certified on the CPU by
tests/test_train_objective_cases_host.py. Sums, per-channel IoUs, errors, rates, the visibility loss and every gradient are compared
to the bit; the means of ratios (the IoU loss, the NME) to half a float32 spacing plus the derived float64 bound (`tc.mean_bar`).

Reached here and nowhere else in the suite: the encode's chunk that crosses into the next channel and its scalar tail (S = 3, 5, 9, 25),
the scalar IoU forms at hw % 4 == 0 behind a pointer that is not aligned, the per-channel `iou` output and `accum` of the C entry, the
thread-stride seams of every kernel, `below=False`, eight thresholds, and the strict comparisons at a tie.
Not reached: the encode's grid-stride cap of 2^20 blocks, which needs a 4 GB output."""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import train_objective_cases as tc
import train_objective_restatement as rs
from dad_3dheads_amd import _lib, metrics
from dad_3dheads_amd.coder import HeatmapCoder
from dad_3dheads_amd.losses import IoULoss, LandmarksLossWVisibility, heatmap_iou_terms

pytestmark = pytest.mark.gpu
F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_objective_edges_golden.npz")
CANARY, PAD = 0xA5, 64


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(got, want):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want, dtype=got.dtype).reshape(got.shape)
    nan = np.isnan(want)  # a NaN is a NaN, whatever its payload
    return np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


def _within(name, got32, exact, bar):
    """|got - exact| <= bar in rational arithmetic; the distance is printed next to its bar."""
    dist = abs(Fraction(float(got32)) - exact)
    print(f"MEASURED {name}: distance {float(dist):.3e} bar {bar:.3e}")
    return dist <= Fraction(bar)


# ---- heatmap encode ------------------------------------------------------------------------------------------------------------------
def _between_canaries(shape, dtype):
    """A 16-byte-aligned contiguous view in the middle of a larger buffer of 0xA5 bytes."""
    nbytes = int(np.prod(shape)) * (1 if dtype == torch.uint8 else 4)
    buf = torch.full((PAD + nbytes + PAD,), CANARY, dtype=torch.uint8, device="cuda")
    view = buf[PAD:PAD + nbytes].view(dtype).view(shape)
    assert view.data_ptr() % 16 == 0 and view.is_contiguous()
    return buf, view


def _canaries_intact(buf):
    host = buf.cpu().numpy()
    return (host[:PAD] == CANARY).all() and (host[-PAD:] == CANARY).all()


def test_encode_odd_sizes_are_the_reference_coder_byte_for_byte():
    with np.load(GOLDEN) as z:
        golden = {k: z[k] for k in z.files}
    for name, img, stride, radius in (c.split(":") for c in golden["coder_cases"]):
        radius = radius if radius == "pointwise" else int(radius)
        kp, pr = golden[f"coder_{name}_keypoints"], golden[f"coder_{name}_presence"]
        assert 28 <= kp.shape[1] <= 32
        coder = HeatmapCoder({"img_size": int(img), "stride": int(stride), "radius": radius}, kp.shape[1])
        for form in ("raw", "uint8", "float"):
            got = coder.encode(_cu(kp), _cu(pr), form=form).cpu().numpy()
            ref = golden[f"coder_{name}_{form}"]
            assert got.dtype == ref.dtype and got.tobytes() == ref.tobytes(), (name, form)
        assert int(coder.invalid_points.item()) == 0  # the NaN points are absent
        item = coder(kp[0], pr[0])
        assert item.dtype == np.float32 and item.tobytes() == golden[f"coder_{name}_raw"][0].tobytes()


@pytest.mark.parametrize("size", [5, 3])
def test_encode_crossing_chunks_and_tails_between_canaries(size):
    """Every B*C*S*S of the list ends in another remainder of a 16-byte chunk: the scalar tail writes 1..15 bytes (uint8) and 1..3 floats,
    and at S = 3 one uint8 chunk spans three channels."""
    stride, radius = tc.ENCODE_STRIDE[size], tc.ENCODE_RADIUS[size]
    for k, (b, c) in enumerate(tc.ENCODE_BATCHES[size]):
        kp, pr = tc.encode_batch(size, stride, b, c, 50 * size + k)
        coder = HeatmapCoder({"img_size": size * stride, "stride": stride, "radius": radius}, c)
        for form in ("uint8", "float", "raw"):
            want = rs.encode(kp, pr, size, stride, radius, form)
            assert want.reshape(-1)[-1] != 0 and (b * c == 1 or want.reshape(-1)[0] != 0)  # the ends of the output carry a stamp
            buf, view = _between_canaries((b, c, size, size), torch.uint8 if form == "uint8" else torch.float32)
            out = coder.encode(_cu(kp), _cu(pr), form=form, out=view)
            assert out.data_ptr() == view.data_ptr() and _canaries_intact(buf), (b, c, form)
            assert view.cpu().numpy().tobytes() == want.tobytes(), (b, c, form)


@pytest.mark.parametrize("size", [5, 3])
def test_invalid_points_are_counted_once_wherever_their_channel_starts(size):
    """A channel's point is looked at by the chunk that starts the channel, or by the one that crosses into it: once, never twice."""
    stride, radius = tc.ENCODE_STRIDE[size], tc.ENCODE_RADIUS[size]
    kp, pr, bad = tc.encode_invalid_case(size, stride)
    good = [ch for ch in range(40) if ch not in bad and pr.reshape(-1)[ch]]
    for form in ("uint8", "float", "raw"):
        coder = HeatmapCoder({"img_size": size * stride, "stride": stride, "radius": radius}, 20)
        out = coder.encode(_cu(kp), _cu(pr), form=form).cpu().numpy().reshape(40, -1)
        assert int(coder.invalid_points.item()) == len(bad), form
        assert not out[list(bad)].any() and not out[~pr.reshape(-1)].any() and out[good].any(1).all()
        coder.encode(_cu(kp), _cu(pr), form=form)
        assert int(coder.invalid_points.item()) == 2 * len(bad), form
        with pytest.raises(ValueError):
            coder.encode(_cu(kp), _cu(pr), form=form, strict=True)
        assert int(coder.invalid_points.item()) == 2 * len(bad)  # strict counts on its own


# ---- heatmap IoU -----------------------------------------------------------------------------------------------------------------------
def _offset_by_one(t):
    """The same values as a contiguous view one element into its storage: not 16-byte (float) / 4-byte (uint8) aligned."""
    v = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % (16 if t.dtype == torch.float32 else 4) != 0
    return v


def _layouts(x, t, hw):
    """aligned; at hw % 4 == 0 (the vector form's sizes) also the prediction, then the target, one element into its storage."""
    yield "aligned", x, t
    if hw % 4 == 0:
        yield "pred+1", _offset_by_one(x), t
        yield "target+1", x, _offset_by_one(t)


def _loss_bars(name, out, n, d):
    exact, count = tc.exact_ratio_mean(n, d), len(n)
    assert _within(f"{name} mean IoU", out[1], exact, tc.mean_bar(count, out[1]))
    assert _within(f"{name} loss", out[0], 1 - exact, tc.mean_bar(count, out[0]))


def test_the_three_sigmoids_the_exact_logits_lean_on():
    x = _cu(tc.LOGITS.reshape(1, 5, 1, 1))
    sums = heatmap_iou_terms(x, torch.ones_like(x), sigmoid=True)[3].cpu().numpy()
    assert np.array_equal(sums[:, 0], [0.5, 1, 0, 1, 0]) and np.array_equal(sums[:, 2], [0.25, 1, 0, 1, 0])


@pytest.mark.parametrize("k", range(len(tc.IOU_SHAPES)), ids=[f"bc{b * c}-hw{hw}" for (b, c), hw in tc.IOU_SHAPES])
def test_iou_of_probabilities_is_exact_in_every_form_and_layout(k):
    bc, hw = tc.IOU_SHAPES[k]
    case = tc.iou_case(bc, hw, False, 1000 + k)
    lib = _lib.load()
    for t_np, t256 in ((case["t_f"], case["tf256"]), (case["t_u8"], case["tu256"])):
        want = tc.iou_sums(case["s256"], t256)
        n, d, iou32 = tc.iou_channels(want)
        for layout, x, t in _layouts(_cu(case["x"]), _cu(t_np), hw):
            name = f"iou {bc} hw {hw} {t_np.dtype} {layout}"
            p, tt, u8, sums, out = heatmap_iou_terms(x, t, sigmoid=False)
            assert p.data_ptr() == x.data_ptr() and tt.data_ptr() == t.data_ptr()  # the wrapper hands the view over, no copy
            assert _same_bits(sums, want), name
            _loss_bars(name, out.cpu().numpy(), n, d)
            # the C entry with its per-channel output and the metric's running sums, launched twice
            sums2 = torch.empty_like(sums)
            iou = torch.full((len(want),), -1.0, dtype=torch.float32, device="cuda")
            loss, accum = torch.empty(2, dtype=torch.float32, device="cuda"), _cu(np.array([0.25, 3.0], F))
            for _ in range(2):
                _lib.check(lib.dad3d_heatmap_iou(x.data_ptr(), t.data_ptr(), u8, bc[0], bc[1], hw, 0, sums2.data_ptr(), iou.data_ptr(),
                                                 loss.data_ptr(), accum.data_ptr(), 0, torch.cuda.current_stream().cuda_stream))
            assert _same_bits(sums2, want) and _same_bits(iou, iou32) and torch.equal(loss, out), name
            mean32 = loss.cpu().numpy()[1]
            assert _same_bits(accum, [F(F(0.25) + mean32) + mean32, 5.0]), name
        assert float(metrics.soft_iou(_cu(case["x"]), _cu(t_np))) == float(out[1]) == float(IoULoss.iou_metric(_cu(case["x"]), _cu(t_np)))


@pytest.mark.parametrize("k", range(len(tc.IOU_SHAPES)), ids=[f"bc{b * c}-hw{hw}" for (b, c), hw in tc.IOU_SHAPES])
def test_iou_loss_on_exact_logits_forward_and_backward(k):
    bc, hw = tc.IOU_SHAPES[k]
    case = tc.iou_case(bc, hw, True, 1100 + k)
    want = tc.iou_sums(case["s256"], case["tu256"])
    n, d, _ = tc.iou_channels(want)
    s32, t32 = (case["s256"] / 256.0).astype(F), (case["tu256"] / 256.0).astype(F)
    at_zero = case["x"] == 0
    t_u8 = _cu(case["t_u8"])
    for g in (1.0, 3.0):
        replay = tc.iou_grad_replay(s32, t32, want, g).reshape(case["x"].shape)
        assert np.all(replay[at_zero] != 0) and np.all(replay[~at_zero] == 0)
        for layout, x0, t in _layouts(_cu(case["x"]), t_u8, hw):
            name = f"iou logits {bc} hw {hw} {layout} g {g}"
            res = []
            for tgt in (t, _offset_by_one(t.float() / 255.0) if layout == "target+1" else t.float() / 255.0):
                assert _same_bits(heatmap_iou_terms(x0, tgt, sigmoid=True)[3], want), name
                x = x0.detach().requires_grad_(True)
                assert x.data_ptr() == x0.data_ptr()
                loss = IoULoss()(x, tgt)
                (loss * g).backward() if g != 1.0 else loss.backward()
                grad = x.grad.cpu().numpy()
                assert np.isfinite(grad).all() and np.all(grad[~at_zero] == 0), name  # +-200, +-inf: s (1 - s) is 0, not NaN
                assert _same_bits(grad[at_zero], replay[at_zero]), name
                res.append((loss.detach(), x.grad))
            assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), name
            exact = tc.exact_ratio_mean(n, d)
            assert _within(name, res[0][0].cpu().numpy(), 1 - exact, tc.mean_bar(len(n), res[0][0].cpu().numpy()))


def test_iou_loss_on_ordinary_logits_behind_unaligned_pointers():
    """The scalar forms at hw % 4 == 0 on seeded ordinary logits, at the bars of tests/test_gpu_train_objective.py."""
    from test_gpu_train_objective import _check_iou, _iou64, _torch_iou

    logits, t8 = rs.iou_inputs(611, 2, 3, 32, 32)
    x0, t = _cu(logits), _cu(t8)
    ref_loss, ref_iou, ref_grad = _iou64(x0, t)
    for layout, xl, tl in _layouts(x0, t, 1024):
        for tgt in (tl, _offset_by_one(t.float() / 255.0) if layout == "target+1" else t.float() / 255.0):
            x = xl.detach().requires_grad_(True)
            loss = IoULoss()(x, tgt)
            loss.backward()
            sums = heatmap_iou_terms(xl, tgt, sigmoid=True)[3]
            nn_, dd = sums[:, 0] + 1e-6, sums[:, 1] + sums[:, 2] - sums[:, 0] + 1e-6
            _check_iou(loss.detach(), (nn_ / dd).view_as(ref_iou), x.grad, ref_loss, ref_iou, ref_grad)
    x = x0.clone().requires_grad_(True)  # the torch fp32 statement meets the same bars
    tl_, ti = _torch_iou(x, t.float() / 255.0)
    tl_.backward()
    _check_iou(tl_.detach(), ti.detach(), x.grad, ref_loss, ref_iou, ref_grad)


# ---- landmark loss with visibility -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", tc.VIS_SHAPES, ids=[f"B{b}-N{n}" for b, n in tc.VIS_SHAPES])
def test_visibility_loss_and_gradient_to_the_bit(shape):
    for k, pattern in enumerate(tc.VIS_PATTERNS):
        case = tc.vis_case(*shape, pattern, 2000 + k)
        pp, t, tp = _cu(case["pp"]), _cu(case["target"]), _cu(case["tp"])
        for crit in tc.CRITERIA:
            for g in (1.0, 3.0):
                want_loss, want_grad = tc.vis_expected(case, crit, g)
                x = _cu(case["pred"]).requires_grad_(True)
                loss = LandmarksLossWVisibility(crit)([x, pp], [t, tp])
                (loss * g).backward() if g != 1.0 else loss.backward()
                assert _same_bits(loss.detach(), want_loss), (shape, pattern, crit)
                grad = x.grad.cpu().numpy()
                assert _same_bits(grad, want_grad), (shape, pattern, crit, g)
                assert np.all(grad[case["pp"] == 0] == 0)
            with torch.no_grad():  # grad_pred == nullptr
                assert _same_bits(LandmarksLossWVisibility(crit)([_cu(case["pred"]), pp], [t, tp]), want_loss)


def test_visibility_loss_nan_under_presence_zero_stays_the_references():
    """The reference multiplies, so the loss is NaN. Its gradient (tests/golden/train_objective_golden.npz, vis_*_grad[0, 0]) is NaN at
    that element only under l2 and smooth_l1, and 0 under l1: torch's sign(NaN) is 0, and 0 * presence 0 is 0."""
    case = tc.vis_case(3, 683, "alternating", 2100)
    pred = case["pred"].copy()
    assert case["pp"][1, 340] == 0
    pred[1, 340, 1] = np.nan
    for crit in tc.CRITERIA:
        _, clean = tc.vis_expected(case, crit)
        x = _cu(pred).requires_grad_(True)
        loss = LandmarksLossWVisibility(crit)([x, _cu(case["pp"])], [_cu(case["target"]), _cu(case["tp"])])
        loss.backward()
        grad = x.grad.cpu().numpy()
        nan = np.zeros(pred.shape, bool)
        nan[1, 340, 1] = crit != "l1"
        assert torch.isnan(loss) and np.array_equal(np.isnan(grad), nan), crit
        assert grad[1, 340, 1] == 0 or crit != "l1"
        nan[1, 340, 1] = True
        assert _same_bits(grad[~nan], clean[~nan]), crit


# ---- keypoint errors -------------------------------------------------------------------------------------------------------------------
def _launch(case, cube=False, thresholds=(0.05, 0.1), below=True, accum=None):
    opt = lambda a: None if a is None else _cu(a)  # noqa: E731
    return metrics.keypoint_errors(_cu(case["pred"]), _cu(case["target"]), opt(case["bbox"]), index=case["index"],
                                   presence=opt(case["presence"]), pred_scale=case["scale"], target_scale=case["scale"], cube=cube,
                                   thresholds=thresholds, below=below, accum=accum)


def _check_launch(case, cube, name, thresholds=(0.05, 0.1), below=True):
    out, err = _launch(case, cube, thresholds, below)
    out, err = out.cpu().numpy(), err.cpu().numpy()
    assert _same_bits(err[:, 0], case["err"]) and _same_bits(err[:, 1], case["norm"]), name
    nme, rates = tc.kp_finish(case["err"], case["norm"], thresholds, below)
    assert _same_bits(out[1:], rates), (name, out[1:], rates)
    if isinstance(nme, Fraction):
        count = len(case["err"])
        assert _within(f"nme {name}", out[0], nme, tc.mean_bar(count, out[0]))
    else:
        assert np.isnan(out[0]), name
    return out


@pytest.mark.parametrize("n", tc.KP_POINTS)
def test_keypoint_errors_rates_and_nme_at_the_stride_seams(n):
    for b in tc.KP_BATCHES:
        for k, (dims, indexed, presence) in enumerate((d, i, p) for d in (2, 3) for i in (False, True) for p in (False, True)):
            case = tc.kp_case(b, n, dims, indexed, presence, 3000 + 10 * b + k)
            _check_launch(case, False, f"B {b} n {n} dims {dims} index {indexed} presence {presence}")
            if b == 257:
                _check_launch(case, False, f"B {b} n {n} dims {dims} above", below=False)
        for k, (indexed, presence) in enumerate((i, p) for i in (False, True) for p in (False, True)):
            case = tc.kp_cube_case(b, n, indexed, presence, 4000 + 10 * b + k)
            _check_launch(case, True, f"B {b} n {n} cube index {indexed} presence {presence}")


@pytest.mark.parametrize("kind", ["bbox", "plain"])
def test_a_tie_counts_under_neither_comparison(kind):
    case = tc.kp_tie_case(kind)
    b = len(case["err"])
    for below in (True, False):
        out = _check_launch(case, False, f"ties {kind} below {below}", case["thresholds"], below)
        for k, thr in enumerate(case["thresholds"]):
            lim = thr * case["norm"][0]
            mine = case["limit"] == lim
            want = np.count_nonzero((case["side"] < 0) & mine) + np.count_nonzero(case["limit"] < lim) if below else \
                np.count_nonzero((case["side"] > 0) & mine) + np.count_nonzero(case["limit"] > lim)
            assert out[1 + k] == F(want / b)  # the neighbours fall on their sides, the tie on neither
    # eight thresholds in one launch (the first one ties), and none
    eight = case["thresholds"] + tc.THRESHOLDS_8[len(case["thresholds"]):]
    for below in (True, False):
        assert len(_check_launch(case, False, f"ties {kind} eight", eight, below)) == 9
    assert len(_check_launch(case, False, f"ties {kind} none", ())) == 1
    # through the class
    thr = case["thresholds"][0]
    gts = {"keypoints": _cu(case["target"] * F(case["scale"]))}
    if case["bbox"] is not None:
        gts["bboxes"] = _cu(case["bbox"])
    for below in (True, False):
        fr = metrics.FailureRate(threshold=thr, below=below)
        rate = tc.kp_finish(case["err"], case["norm"], (thr,), below)[1][0]
        for step in (1, 2):
            assert float(fr(_cu(case["pred"] * F(case["scale"])), gts)) == rate
            assert float(fr.states["total"]) == step and float(fr.compute()) == F(F(rate * step) / F(step))


def test_cube_path_non_finite_input_poisons_its_item_only():
    case = tc.kp_cube_case(4, 65, False, False, 4500)
    clean = _check_launch(case, True, "cube clean")
    for value in (np.nan, np.inf, -np.inf):
        for side in ("pred", "target"):
            bad = dict(case, **{side: case[side].copy()}, err=case["err"].copy())
            bad[side][2, 17, 1] = value
            bad["err"][2] = np.nan  # the reference gives NaN in all six cases
            for below in (True, False):
                out = _check_launch(bad, True, f"cube {value} in {side}", below=below)  # the other three items keep their bits
                assert np.isnan(out[0])
                rest = case["err"][[0, 1, 3]]  # the NaN item counts under neither: the counts are those of the other three
                cnt = [np.count_nonzero(rest < t * 2.0 if below else rest > t * 2.0) for t in (0.05, 0.1)]
                assert np.array_equal(out[1:], F(cnt) * F(0.25))
    same = dict(case, pred=case["pred"].copy(), err=case["err"].copy())
    same["pred"][1] = same["pred"][1, :1]  # all points equal: pscale == 0, 0 / 0
    same["err"][1] = np.nan
    _check_launch(same, True, "cube degenerate")
    assert clean[0] > 0
