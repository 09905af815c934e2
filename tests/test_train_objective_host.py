"""CPU: the float64 restatement of the training objective (tests/train_objective_restatement.py) against the reference's
own results (tests/golden/train_objective_golden.npz), the host stamp tables, numpy's float32 floor_divide rule,
`LossModule.from_config` and the metric state semantics. The HIP results are checked on the GPU
(tests/test_gpu_train_objective.py)."""
import os

import numpy as np
import pytest
import torch

import train_objective_restatement as rs
from dad_3dheads_amd import coder, loss_module, losses, metrics
from oracle import reference_runner

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_objective_golden.npz")
EDGES_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_objective_edges_golden.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def edges_golden():
    with np.load(EDGES_GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _cases(g, key):
    return [c.split(":") for c in g[key]]


def test_restated_encode_is_the_reference_coder_byte_for_byte(golden, edges_golden):
    sizes = set()
    for g in (golden, edges_golden):  # the second file: planes that are no multiple of a 16-byte chunk (S = 3, 5, 9, 25)
        for name, img, stride, radius in _cases(g, "coder_cases"):
            radius = radius if radius == "pointwise" else int(radius)
            size = int(img) // int(stride)
            sizes.add(size)
            kp, pr = g[f"coder_{name}_keypoints"], g[f"coder_{name}_presence"]
            for form in ("raw", "uint8", "float"):
                ref = g[f"coder_{name}_{form}"]
                got = rs.encode(kp, pr, size, int(stride), radius, form)
                assert got.dtype == ref.dtype and got.tobytes() == ref.tobytes(), (name, form)
            assert np.count_nonzero(g[f"coder_{name}_raw"]) > 0
    assert {3, 5, 9, 25} <= sizes


@pytest.mark.parametrize("radius", [0, 1, 2, 3, 5, 8, "pointwise"])
def test_host_tables_match_the_reference_draw_gaussian(radius):
    """The stamp of a centred point, drawn by the reference's expressions (restated in coder._stamp), in every form."""
    r = 1 if radius == "pointwise" else radius
    raw = coder.stamp_table(radius, "raw")
    assert raw.dtype == np.float32 and raw.shape == (2 * r + 1, 2 * r + 1)
    if radius != "pointwise":
        d = 2 * r + 1
        y, x = np.ogrid[-r: r + 1, -r: r + 1]
        h = np.exp(-(x * x + y * y) / (2 * (d / 6) ** 2))
        h[h < np.finfo(h.dtype).eps * h.max()] = 0
        assert np.array_equal(raw, h.astype(np.float32))
    u8 = coder.stamp_table(radius, "uint8")
    assert u8.dtype == np.uint8 and np.array_equal(u8, (np.float32(255.0) * raw).astype(np.uint8))
    f = coder.stamp_table(radius, "float")
    assert f.dtype == np.float32 and np.array_equal(f, torch.from_numpy(u8).div(255.0).numpy())


def test_floor_divide_rule_is_numpys():
    rng = np.random.default_rng(5)
    a = np.concatenate([rng.uniform(-1e4, 1e4, 200000), rng.integers(-3000, 3000, 20000) * 3.0, [0.0, -0.0, 1e30, -1e30,
                                                                                               np.inf, -np.inf, np.nan]]).astype(np.float32)
    for stride in (1, 2, 3, 4, 5, 6, 7, 12):
        with np.errstate(all="ignore"):
            ref = a // np.float32(stride)
        got = coder.floor_divide_f32(a, stride)
        assert np.array_equal(ref, got, equal_nan=True), stride
        assert np.array_equal(np.signbit(ref), np.signbit(got))
    below = np.nextafter(np.arange(1, 20000, dtype=np.float32) * np.float32(3), np.float32(-np.inf))  # just below multiples
    assert np.array_equal(below // np.float32(3), coder.floor_divide_f32(below, 3))


def test_restated_iou_meets_the_reference(golden):
    for name, seed, b, c, h, w in _cases(golden, "iou_cases"):
        logits, t8 = rs.iou_inputs(int(seed), int(b), int(c), int(h), int(w))
        for tgt in (t8, t8.astype(np.float32) / np.float32(255.0)):  # the dataset's bytes read as get_input reads them
            loss, iou, grad = rs.iou_loss(logits, tgt)
            assert abs(loss - float(golden[f"iou_{name}_loss"])) <= 2e-7
            assert abs(rs.soft_iou(rs.sigmoid64(logits), tgt) - float(golden[f"iou_{name}_soft_iou"])) <= 2e-7
            assert np.abs(grad - golden[f"iou_{name}_grad"]).max() <= 2e-6 * np.abs(grad).max()
        assert golden[f"iou_{name}_grad"][0, 0].max() == 0.0  # saturated logits: s (1 - s) = 0 in fp32


def test_restated_visibility_loss_meets_the_reference(golden):
    pred, pp, tgt, tp = rs.visibility_inputs(81, 3, 68)
    for crit in rs.CRITERIA:
        val, grad = rs.visibility_loss(pred, pp, tgt, tp, crit)
        assert np.isnan(val) and np.isnan(golden[f"vis_{crit}_loss"])  # multiply, not select: NaN * 0 is NaN
        assert np.array_equal(np.isnan(grad), np.isnan(golden[f"vis_{crit}_grad"]))
        finite = ~np.isnan(grad)
        assert np.abs(grad[finite] - golden[f"vis_{crit}_grad"][finite]).max() <= 1e-6 * np.abs(grad[finite]).max()
        clean = pred.copy()
        clean[0, 0, 1] = 0.25
        val, grad = rs.visibility_loss(clean, pp, tgt, tp, crit)
        assert abs(val - float(golden[f"vis_clean_{crit}_loss"])) <= 1e-6 * abs(val)
        assert np.abs(grad - golden[f"vis_clean_{crit}_grad"]).max() <= 1e-6 * np.abs(grad).max()


def test_restated_keypoint_metrics_meet_the_reference(golden):
    for name, seed, b, n, dims, spread in _cases(golden, "kp_cases"):
        p, q, pres, bbox = rs.keypoint_inputs(int(seed), int(b), int(n), int(dims), float(spread))
        if int(dims) == 2:
            err, norm = rs.keypoint_errors(p, q, bbox, presence=pres, pred_scale=256, target_scale=256)
        else:
            err, norm = rs.keypoint_errors(p, q, None, index=golden[f"{name}_index"], cube=True)
        nme, rates = rs.nme_and_rates(err, norm)
        assert abs(nme - float(golden[f"{name}_nme"])) <= 1e-6 * nme
        assert np.allclose(err / norm, golden[f"{name}_nme_items"], rtol=1e-6, atol=0)
        assert rates == [float(golden[f"{name}_fr_0.05"]), float(golden[f"{name}_fr_0.1"])]
        assert 0 < rates[1] and rates[0] < 1  # the cases exercise the thresholds


TRAIN_LOSS = {  # config/loss/train_loss.yaml, resolved (${batch_size}, ${constants}, ${train.*} filled in)
    "reduction": "sum",
    "criterions": [
        {"name": "heatmap_loss", "target_key": "TARGET_LANDMARKS_HEATMAP", "output_key": "OUTPUT_LANDMARKS_HEATMAP", "weight": 1.,
         "loss": {"_target_": "model_training.losses.IoULoss"}},
        {"name": "vertices3d_loss", "target_key": "TARGET_3D_MODEL_VERTICES", "output_key": "OUTPUT_3DMM_PARAMS", "weight": 50.,
         "loss": {"_target_": "model_training.losses.Vertices3DLoss", "criterion": "l2", "batch_size": 4, "consts": None,
                  "weights_and_indices": None}},
        {"name": "reprojection_loss", "target_key": "TARGET_2D_FULL_LANDMARKS", "output_key": "OUTPUT_3DMM_PARAMS", "weight": 0.05,
         "loss": {"_target_": "model_training.losses.ReprojectionLoss", "criterion": "smooth_l1", "batch_size": 4, "consts": None,
                  "img_size": 256, "weights_and_indices": None}},
        {"name": "landmarks_loss", "target_key": ["TARGET_2D_LANDMARKS", "TARGET_2D_LANDMARKS_PRESENCE"],
         "output_key": ["OUTPUT_2D_LANDMARKS", "TARGET_2D_LANDMARKS_PRESENCE"], "weight": 100.,
         "loss": {"_target_": "model_training.losses.LandmarksLossWVisibility", "criterion": "smooth_l1"}},
    ],
}


def test_from_config_builds_the_train_loss_block(monkeypatch):
    built = []

    class FakeMesh(torch.nn.Module):  # the mesh criteria need a GPU; record their arguments instead
        def __init__(self, *args, **kw):
            super().__init__()
            built.append((type(self).__name__, args, kw))

    V = type("Vertices3DLoss", (FakeMesh,), {})
    P = type("ReprojectionLoss", (FakeMesh,), {})
    monkeypatch.setitem(loss_module.CRITERIA, "model_training.losses.Vertices3DLoss", V)
    monkeypatch.setitem(loss_module.CRITERIA, "model_training.losses.ReprojectionLoss", P)
    monkeypatch.setattr(loss_module, "_MESH_CRITERIA", (V, P))
    regions = {"weights": {"head": .5, "face_w_ears": .75, "face": 1.}, "flame_indices": {"folder": "/x", "files": {"face": "face.npy"}}}
    cfg = {**TRAIN_LOSS, "criterions": [dict(c, loss=dict(c["loss"])) for c in TRAIN_LOSS["criterions"]]}
    for c in cfg["criterions"]:
        if "weights_and_indices" in c["loss"]:
            c["loss"]["weights_and_indices"] = regions
    m = loss_module.LossModule.from_config(cfg, head_mesh_kwargs={"device": 0})
    assert m.names == ["heatmap_loss", "vertices3d_loss", "reprojection_loss", "landmarks_loss"]
    assert m.weights == [1.0, 50.0, 0.05, 100.0] and m.schedule == [0, 0, 0, 0] and m.reduction == "sum"
    assert isinstance(m.criterions[0], losses.IoULoss) and isinstance(m.criterions[3], losses.LandmarksLossWVisibility)
    assert isinstance(m.criterions[3].criterion, torch.nn.SmoothL1Loss)
    assert [b[0] for b in built] == ["Vertices3DLoss", "ReprojectionLoss"]
    assert built[0][2] == {"criterion": "l2", "batch_size": 4, "consts": None, "weights_and_indices": regions, "device": 0}
    assert built[1][2]["img_size"] == 256 and built[1][2]["criterion"] == "smooth_l1"
    assert m.output_keys[3] == ["OUTPUT_2D_LANDMARKS", "TARGET_2D_LANDMARKS_PRESENCE"]
    with pytest.raises(ValueError, match="no HIP criterion"):
        loss_module.LossModule.from_config({"criterions": [{"name": "x", "target_key": "k", "loss": {"_target_": "a.B"}}]})
    with pytest.raises(ValueError, match="Unsupported discrepancy loss type"):
        losses.LandmarksLossWVisibility("huber")


def test_loss_module_schedule_and_reductions_on_plain_criteria():
    """forward's gating, weighting and reductions (loss_module.py:42-70) with CPU stand-in criteria."""
    mse = torch.nn.MSELoss()

    class Masked(torch.nn.Module):
        def forward(self, x, y):
            return mse(x[0] * x[1], y[0])

    m = loss_module.LossModule(["a", "b", "c"], ["p", "p", ["p", "q"]], ["t", "t", ["t", "q"]],
                               [mse, torch.nn.L1Loss(), Masked()], [2.0, 0.5, 3.0], [0, 5, 1], "sum")
    d = {"p": torch.tensor([1.0, 2.0]), "t": torch.tensor([0.0, 0.0]), "q": torch.tensor([1.0, 0.0])}
    total, terms = m(d, {}, 1)
    assert list(terms) == ["a", "c"] and float(terms["a"]) == 2.0 * 2.5 and float(terms["c"]) == 3.0 * 0.5
    assert float(total) == 6.5
    m.reduction = "mean"
    assert float(m(d, {}, 7)[0]) == pytest.approx((5.0 + 0.75 + 1.5) / 3)
    m.reduction = "none"
    assert m(d, {}, 0)[0].shape == (1,)
    m.reduction = "max"
    with pytest.raises(ValueError, match="Unsupported reduction"):
        m(d, {}, 0)


def test_metric_state_semantics_over_three_steps():
    """compute_on_step=True: the call returns the batch value, the state accumulates, compute() is the running value and
    reset() clears it (torchmetrics' Metric, restated in metrics._Metric). A CPU stand-in update fills the state the way
    the kernels do (value, 1)."""

    class Mean(metrics._Metric):
        _value_name = "value"

        def _update(self, x):
            acc = self._state(x.device)
            v = x.mean()
            acc[0] += v
            acc[1] += 1
            return v

        def compute(self):
            return self._acc[0] / self._acc[1]

    m = Mean()
    vals = [m(torch.tensor([float(i), float(i) + 2.0])) for i in range(3)]
    assert [float(v) for v in vals] == [1.0, 2.0, 3.0]
    assert float(m.compute()) == 2.0 and float(m.states["total"]) == 3.0 and float(m.states["value"]) == 6.0
    m.reset()
    assert float(m.states["total"]) == 0.0
    m.compute_on_step = False
    assert m(torch.tensor([4.0])) is None and float(m.compute()) == 4.0
    # the reference's finishes: FailureRate fr / total, KeypointsNME weight * nme / total, SoftIoU mean(ious / total)
    nme = metrics.KeypointsNME(weight=100)
    nme._acc = torch.tensor([0.3, 3.0])
    assert float(nme.compute()) == pytest.approx(10.0)
    fr = metrics.FailureRate(threshold=0.1)
    fr._acc = torch.tensor([1.5, 3.0])
    assert float(fr.compute()) == 0.5 and set(fr.states) == {"failure_rate", "total"}
    assert set(metrics.SoftIoUMetric().states) == {"ious", "total"}


def test_gpu_only_surfaces_refuse_cpu_tensors():
    x = torch.zeros((1, 2, 4, 4))
    with pytest.raises(ValueError, match="GPU"):
        losses.IoULoss()(x, x)
    with pytest.raises(ValueError, match="GPU"):
        losses.LandmarksLossWVisibility("l1")([torch.zeros(1, 2, 2), torch.ones(1, 2)], [torch.zeros(1, 2, 2), torch.ones(1, 2)])
    with pytest.raises(ValueError, match="GPU"):
        metrics.keypoints_nme(torch.zeros(1, 3, 2), torch.zeros(1, 3, 2))


@pytest.mark.skipif(not reference_runner.reference_available(), reason="reference tree not present on this machine")
def test_committed_golden_is_what_the_reference_produces_here(tmp_path):
    """Authoring container only: re-run the generator (the reference's own code) and compare every array."""
    import subprocess
    import sys

    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    out = tmp_path / "train_objective_golden.npz"
    subprocess.run([sys.executable, os.path.join(here, "make_train_objective_golden.py"), str(out)], check=True, capture_output=True,
                   timeout=600)
    with np.load(out) as fresh, np.load(GOLDEN) as committed:
        assert sorted(fresh.files) == sorted(committed.files)
        for k in fresh.files:
            assert np.array_equal(fresh[k], committed[k], equal_nan=fresh[k].dtype.kind == "f"), k


@pytest.mark.skipif(not reference_runner.reference_available(), reason="reference tree not present on this machine")
def test_committed_edges_golden_is_what_the_reference_produces_here(tmp_path):
    """Authoring container only: re-run the odd-size generator (the reference's own coder) and compare every array."""
    import subprocess
    import sys

    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    out = tmp_path / "train_objective_edges_golden.npz"
    subprocess.run([sys.executable, os.path.join(here, "make_train_objective_edges_golden.py"), str(out)], check=True,
                   capture_output=True, timeout=600)
    with np.load(out) as fresh, np.load(EDGES_GOLDEN) as committed:
        assert sorted(fresh.files) == sorted(committed.files)
        for k in fresh.files:
            assert fresh[k].dtype == committed[k].dtype, k
            assert np.array_equal(fresh[k], committed[k], equal_nan=fresh[k].dtype.kind == "f"), k  # the absent NaN keypoints
    assert os.path.getsize(EDGES_GOLDEN) < os.path.getsize(GOLDEN) and os.path.getsize(EDGES_GOLDEN) < 100_000
