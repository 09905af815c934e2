"""GPU: csrc/head_pose.hip -- `dad3d_head_pose` and `dad3d_procrustes` against their host entries (the same routines on the CPU, which
tests/test_pose_host.py holds to scipy and to `evaluation.procrustes`), and the callers that reach them: `draw_pose(angles="device")`,
`predict_batch(pose=True)`, `HeadTracker(pose=True)` and `evaluate_batch(procrustes="device")`."""
import numpy as np
import pytest
import torch

import pose_restatement as pr
from dad_3dheads_amd import _lib, evaluation, overlay, pose

pytestmark = pytest.mark.gpu

NF, DG, GB, IX = _lib.POSE_FLAG_NONFINITE, _lib.POSE_FLAG_DEGENERATE, _lib.POSE_FLAG_GIMBAL, _lib.POSE_FLAG_INDEX
ROW_COUNTS = (1, 63, 64, 65, 130, 257)
SIZES = [(480, 640), (200, 333), (1081, 1919)]


def _rows(n):
    return pr.rot6_rows(n, seed=pr.SEED + 10 + n).copy()


def _check(got: pose.HeadPose, host: pose.HeadPose, sizes, what):
    rotation, rpy, points, flags = (None if t is None else t.cpu().numpy() for t in got)
    assert np.array_equal(flags, host.flags), what
    good = (host.flags & (NF | DG)) == 0
    assert np.array_equal(rotation[good].view(np.uint32), host.rotation[good].view(np.uint32)), what  # bit for bit
    assert np.array_equal(np.isnan(rotation), np.isnan(host.rotation)), what
    assert np.isnan(rpy[~good]).all() and np.isfinite(rpy[good]).all(), what
    diff = np.abs(rpy[good] - host.rpy[good]).max() if good.any() else 0.0
    print(f"{what}: rpy device vs host max {diff:.3g} degrees")
    assert diff <= pr.RPY_TOL_DEG, what
    # points: equal to the host's except heads with a coordinate at an edge (by the statement's values), at most 1 %
    live = np.flatnonzero(((host.flags & IX) == 0) & good)
    sizes = [sizes] * len(flags) if isinstance(sizes[0], int) else sizes
    raw = pr.raw_points(host.rpy[live], [sizes[i] for i in live])
    skip = pr.near_edge(raw)
    assert skip.mean() <= pr.EDGE_CAP, (what, skip.mean())
    assert np.array_equal(points[live][~skip], host.points[live][~skip]), what
    assert np.all(points[(host.flags & IX) != 0] == 0), what


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_head_pose_matches_the_host_entry_uniform_size(n):
    rows = _rows(n)
    host = pose.head_pose_host(rows, size=(480, 640))
    got = pose.head_pose(torch.from_numpy(rows).cuda(), size=(480, 640), want=("rotation", "rpy", "points"))
    _check(got, host, (480, 640), f"bare [{n},6]")
    # the same rows inside every second row of a [2n,413] tensor: a strided view, read where it lies
    big = torch.randn((2 * n, pose.N_PARAMS), generator=torch.Generator().manual_seed(n)).cuda()
    big[::2, pose.ROTATION_OFFSET:pose.ROTATION_OFFSET + 6] = torch.from_numpy(rows).cuda()
    view = big[::2]
    assert n == 1 or not view.is_contiguous()
    _check(pose.head_pose(view, size=(480, 640), want=("rotation", "rpy", "points")), host, (480, 640), f"view [{n},413]")
    only = pose.head_pose(view, want=("rpy",))
    assert only.rotation is None and only.points is None and torch.equal(only.flags, got.flags)
    assert torch.equal(only.rpy.nan_to_num(7.0), got.rpy.nan_to_num(7.0))


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_head_pose_matches_the_host_entry_frame_table(n):
    """Three frames of different sizes; the index holds -1 and one index beyond the table (INDEX: zero points, the rest written)."""
    rows = _rows(n)
    index = np.random.default_rng(n).integers(0, 3, n).astype(np.int32)
    if n >= 63:
        index[1], index[n - 2] = -1, 3
    host = pose.head_pose_host(rows, frame_sizes=SIZES, image_index=index)
    if n >= 63:
        assert host.flags[1] & IX and host.flags[n - 2] & IX
    frames = [torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda") for h, w in SIZES[:2]] + [SIZES[2]]  # tensors and a bare size
    dev_index = torch.from_numpy(index).cuda()
    got = pose.head_pose(torch.from_numpy(rows).cuda(), frames=frames, image_index=dev_index, want=("rotation", "rpy", "points"))
    sizes = [SIZES[min(max(int(i), 0), 2)] for i in index]
    _check(got, host, sizes, f"frame list, n = {n}")
    table = torch.tensor([[t.data_ptr(), t.shape[0], t.shape[1], t.stride(0)] for t in frames[:2]] + [[1, *SIZES[2], 0]], dtype=torch.int64).cuda()
    _check(pose.head_pose(torch.from_numpy(rows).cuda(), frames=table, image_index=dev_index, want=("rotation", "rpy", "points")), host, sizes,
           f"frame table, n = {n}")


def test_head_pose_flags_of_bad_and_lock_rows():
    """NaN, Inf, a zero v1, v2 parallel to v1 and the exact-lock matrices among ordinary rows: the device's flags are the host's, a
    NONFINITE or DEGENERATE row has NaN angles and all ten points at its frame's centre, a lock row its angles."""
    lock = pr.lock_rows()
    rows = pr.rot6_rows(100, seed=pr.SEED + 9).copy()
    rows[-len(lock):] = lock
    rows[3, 1], rows[4, 5] = np.nan, -np.inf
    rows[5, :3] = 0.0
    rows[6] = [1.5, 1.5, 1.5, -3.0, -3.0, -3.0]
    host = pose.head_pose_host(rows, size=(300, 400))
    assert list(host.flags[3:7]) == [NF, NF, DG, DG] and np.all(host.flags[-len(lock):] == GB)
    got = pose.head_pose(torch.from_numpy(rows).cuda(), size=(300, 400), want=("rotation", "rpy", "points"))
    flags, rpy, points = got.flags.cpu().numpy(), got.rpy.cpu().numpy(), got.points.cpu().numpy()
    assert np.array_equal(flags, host.flags)
    bad = (flags & (NF | DG)) != 0
    assert np.isnan(rpy[bad]).all() and np.all(points[bad] == np.array([200.0, 150.0], np.float32))
    assert np.abs(rpy[~bad] - host.rpy[~bad]).max() <= pr.RPY_TOL_DEG
    assert np.array_equal(got.rotation.cpu().numpy()[~bad].view(np.uint32), host.rotation[~bad].view(np.uint32))


def test_head_pose_argument_errors():
    rows = torch.from_numpy(pr.rot6_rows(4).copy()).cuda()
    with pytest.raises(ValueError):
        pose.head_pose(rows.cpu())
    with pytest.raises(ValueError):
        pose.head_pose(rows, want=("points",))  # no frame size
    with pytest.raises(ValueError):
        pose.head_pose(rows, want=("angles",))
    with pytest.raises(ValueError):
        pose.head_pose(rows[:, :5])
    empty = pose.head_pose(rows[:0], size=(10, 10), want=("rotation", "rpy", "points"))
    assert empty.rotation.shape == (0, 3, 3) and empty.points.shape == (0, 10, 2) and empty.flags.shape == (0,)


# ---- draw_pose ---------------------------------------------------------------------------------------------------------------------
def _steady_rows(n, h, w, seed):
    """Rows whose arrow coordinates keep 0.01 px from every truncation and rounding edge: the host path's angles come from the
    framework's 6-D rule, whose matrix differs by an ulp or two from the device's (about 1e-5 degrees, 1e-5 px at most)."""
    rows = pr.rot6_rows(40 * n, seed=seed)
    rpy, flags = pose.rpy_rows(rows)
    gap = pr.edge_gap(pr.raw_points(rpy, (h, w)))
    keep = np.flatnonzero((gap >= 0.01) & (flags == 0) & (np.abs(np.abs(rpy[:, 2]) - 90.0) >= 1.0))
    assert len(keep) >= n
    return rows[keep[:n]]


def _params_with(rows):
    params = torch.randn((len(rows), pose.N_PARAMS), generator=torch.Generator().manual_seed(len(rows)))
    params[:, pose.ROTATION_OFFSET:pose.ROTATION_OFFSET + 6] = torch.from_numpy(rows)
    return params.cuda()


def test_draw_pose_device_angles_draw_the_host_paths_bytes():
    h, w = 200, 260
    params = _params_with(_steady_rows(2, h, w, seed=77))
    images = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (2, h, w, 3), dtype=np.uint8)).cuda()
    host = overlay.draw_pose({"3dmm_params": params}, images)
    dev = overlay.draw_pose({"3dmm_params": params}, images, angles="device")
    assert torch.equal(host, dev) and not torch.equal(dev, images)
    # frames of two sizes as a list, several heads per frame through image_index
    frames = [images[0], torch.from_numpy(np.random.default_rng(3).integers(0, 256, (240, 200, 3), dtype=np.uint8)).cuda()]
    rows = np.concatenate([_steady_rows(2, 200, 260, seed=78), _steady_rows(1, 240, 200, seed=79)])
    p3 = _params_with(rows)
    dicts = [{"3dmm_params": p3[i:i + 1]} for i in range(3)]
    host = overlay.draw_pose(dicts, frames, image_index=[0, 0, 1])
    dev = overlay.draw_pose(dicts, frames, image_index=[0, 0, 1], angles="device")
    assert all(torch.equal(a, b) for a, b in zip(host, dev))
    with pytest.raises(ValueError):
        overlay.draw_pose({"3dmm_params": params}, images, angles="gpu")


# ---- the predictor and the tracker -------------------------------------------------------------------------------------------------
POSE_KEYS = ("rotation_matrix", "rpy", "pose_flags")


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and a.device == b.device and torch.equal(a, b)
    return np.array_equal(np.asarray(a), np.asarray(b)) and np.asarray(a).dtype == np.asarray(b).dtype


def _assert_pose_keys(with_pose, without, on_device):
    assert len(with_pose) == len(without)
    for r, plain in zip(with_pose, without):
        assert set(r) == set(plain) | set(POSE_KEYS)
        for key in plain:
            assert _same(r[key], plain[key]), key  # every other key byte-equal
        want = pose.head_pose(r["3dmm_params"].cuda())
        rot, rpy, flags = r["rotation_matrix"], r["rpy"], r["pose_flags"]
        assert rot.dtype == torch.float32 and tuple(rot.shape) == (3, 3) and rpy.dtype == torch.float64 and tuple(rpy.shape) == (3,)
        assert rot.is_cuda == on_device and rpy.is_cuda == on_device
        assert torch.equal(rot.cuda(), want.rotation[0]) and torch.equal(rpy.cuda(), want.rpy[0]) and int(flags) == int(want.flags[0]) == 0
        assert bool(torch.isfinite(rpy).all())


@pytest.fixture(scope="module")
def predictor(flame_model):
    from test_gpu_predict_boxes import _predictor

    return _predictor(flame_model, ("params", "landmarks", "heatmap"))


def test_predict_batch_pose_keys(predictor):
    rng = np.random.default_rng(12)
    images = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((97, 131), (300, 200), (64, 64))]
    for on_device in (False, True):
        plain = predictor.predict_batch(images, device_outputs=on_device, points_on_device=on_device)
        posed = predictor.predict_batch(images, device_outputs=on_device, points_on_device=on_device, pose=True)
        _assert_pose_keys(posed, plain, on_device)
    batch = torch.from_numpy(np.stack([images[2]] * 2)).cuda()
    plain, posed = predictor.predict_tensor(batch), predictor.predict_tensor(batch, pose=True)
    assert all(torch.equal(plain[k], posed[k]) for k in plain) and set(posed) == set(plain) | set(POSE_KEYS)
    want = pose.head_pose(posed["3dmm_params"])
    assert torch.equal(posed["rotation_matrix"], want.rotation) and torch.equal(posed["rpy"], want.rpy)


def test_predict_boxes_pose_keys_and_the_move_into_the_frame_keeps_the_rotation(predictor):
    rng = np.random.default_rng(13)
    frames = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((97, 131), (300, 200))]
    boxes = [np.array([[10, 5, 60, 70]], np.int32), np.array([[30, 40, 120, 150], [5, 5, 90, 100]], np.int32)]
    plain = predictor.predict_boxes(frames, boxes)
    posed = predictor.predict_boxes(frames, boxes, pose=True)
    _assert_pose_keys(posed, plain, False)
    # adjust_3dmm_to_paddings moves scale and translation, never the rotation: the six floats keep their bits
    params = torch.randn((3, pose.N_PARAMS), generator=torch.Generator().manual_seed(3)).cuda()
    moved = params.clone()
    geometry = torch.tensor([[3.0, 4.0, 0.5, 10.0, 20.0], [0.0, 7.0, 1.25, 5.0, 0.0], [2.0, 0.0, 2.0, 0.0, 9.0]], dtype=torch.float64).cuda()
    predictor._readjust(moved, geometry)
    sl = slice(pose.ROTATION_OFFSET, pose.ROTATION_OFFSET + 6)
    assert torch.equal(moved[:, sl], params[:, sl]) and not torch.equal(moved, params)


def test_head_tracker_pose_keys(flame_model):
    from dad_3dheads_amd.config import load_default_config
    from dad_3dheads_amd.predictor import FaceMeshPredictor
    from dad_3dheads_amd.tracking import HeadTracker
    from test_gpu_track_boxes import FRAME_SHAPES, START, Stub

    pred = FaceMeshPredictor(load_default_config(), cuda_id=0, model=Stub(), flame_model=flame_model)
    rng = np.random.default_rng(31)
    frames = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda() for h, w in FRAME_SHAPES]
    steps = {}
    for with_pose in (False, True):
        pred.model.calls, pred.model.off = 0, None
        tracker = HeadTracker(pred, pose=with_pose)
        tracker.start(frames, START)
        steps[with_pose] = [tracker.step(frames) for _ in range(2)]
    for plain, posed in zip(steps[False], steps[True]):
        _assert_pose_keys(posed, plain, True)


# ---- Procrustes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_points", pr.PROCRUSTES_COUNTS)
def test_procrustes_matches_the_host_entry(n_points):
    x, y = pr.procrustes_inputs(n_points, items=65)
    dx, dy = torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(np.array(y)).cuda()
    whole = None
    for items in (1, 3, 65):
        got = tuple(t.cpu().numpy() for t in pose.procrustes_batch(dx[:items], dy[:items]))
        host = pose.procrustes_host(x[:items], y[:items])
        pr.assert_procrustes(got, x[:items], y[:items], ref=host[:3], what=f"n = {n_points}, {items} items vs host entry")
        pr.assert_procrustes(got, x[:items], y[:items], what=f"n = {n_points}, {items} items vs evaluation.procrustes")
        whole = got
    for i in (0, 7, 64):  # one item alone and inside the batch of 65: the same bits
        one = tuple(t.cpu().numpy() for t in pose.procrustes_batch(dx[i:i + 1], dy[i:i + 1]))
        assert all(np.array_equal(a[i:i + 1], b) for a, b in zip(whole, one)), (n_points, i)


def test_procrustes_degenerate_items_are_flagged():
    rng = np.random.default_rng(8)
    other = rng.standard_normal((3, 7, 3))
    same = np.tile(rng.standard_normal((3, 1, 3)), (1, 7, 1))
    bad = other.copy()
    bad[1, 3, 0] = np.inf
    for x, y, want in ((same, other, [DG] * 3), (other, same, [DG] * 3), (bad, other, [0, DG, 0]), (other[:, :1], other[:, :1] + 1, [DG] * 3)):
        b, t, c, flags = pose.procrustes_batch(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
        assert flags.tolist() == want == list(pose.procrustes_host(x, y)[3])
        lost = torch.tensor(want, device="cuda") != 0
        assert bool(torch.isnan(b[lost]).all() and torch.isnan(t[lost]).all() and torch.isnan(c[lost]).all())
        assert bool(torch.isfinite(b[~lost]).all() and torch.isfinite(t[~lost]).all())


# ---- the scorer --------------------------------------------------------------------------------------------------------------------
# |chamfer(device) - chamfer(host)| / chamfer(host), measured on the MI355X over the golden items: 0. The two alignments agree to
# a few float64 roundings (1e-16), and on these items none of them moved a float32 entry of the similarity handed to `nearest` (a
# move needs a float64 value within 1e-16 of a float32 rounding boundary, spacing 6e-8). Twice the measured value is allowed.
CHAMFER_DEVICE_VS_HOST = 0.0


def test_evaluate_batch_with_the_alignment_on_the_device(static):
    import eval_restatement as er
    from test_gpu_eval import _batch_inputs, _kw

    golden = er.load_golden()
    items = [0, 1, 2, 4]
    kw = _kw(golden, static)
    host = evaluation.evaluate_batch(*_batch_inputs(golden, items, static), **kw)
    dev = evaluation.evaluate_batch(*_batch_inputs(golden, items, static), **kw, procrustes="device")
    for key in ("pose_error", "nme", "z5"):
        assert torch.equal(host[key], dev[key]), key
    rel = ((dev["chamfer"] - host["chamfer"]).abs() / host["chamfer"].abs()).max().item()
    print(f"chamfer, alignment on the device vs on the host: max relative difference {rel:.3g}")
    assert rel <= 2 * CHAMFER_DEVICE_VS_HOST
    with pytest.raises(ValueError):
        evaluation.evaluate_batch(*_batch_inputs(golden, items, static), **kw, procrustes="gpu")
