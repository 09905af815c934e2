"""GPU: matrix projection (flame_dataset.py:115-141, visualize.py:10-22) against goldens produced by the reference's own
`visualize.get_2d_keypoints`, against the numpy restatement, and to the bit against the kernel's own fp32 order as
tests/train_batch_restatement.py states it (`world`, `project`: k = 0..3 in order, no fused multiply-add)."""
import itertools
import os

import numpy as np
import pytest
import torch

from dad_3dheads_amd import projection
import train_batch_restatement as tbr
from oracle import projection_ref

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "projection_golden.npz")
TOL_PX = 1e-3  # fp32 at image scale (coordinates up to ~1e3 px): numpy's sgemm may fuse / reorder the 4-term sums


def annotations():
    with np.load(GOLDEN) as z:
        for i in range(3):
            yield ({"vertices": z[f"vertices_{i}"].tolist(), "model_view_matrix": z[f"model_view_{i}"].tolist(),
                    "projection_matrix": z[f"projection_{i}"].tolist()}, int(z[f"height_{i}"]), z[f"keypoints_{i}"])


def test_keypoints_match_reference_goldens():
    for data, h, want in annotations():
        got = projection.get_2d_keypoints(data, h)
        assert got.shape == want.shape == (5023, 2)
        # float results agree to TOL_PX; `.astype(int)` can therefore only differ where the value sits on an integer
        _, world, proj = projection_ref.load_mesh(data)
        exact = projection_ref.project_vertices_onto_image(world.astype(np.float64), proj.astype(np.float64), h, 0, 0)
        near_integer = np.abs(exact - np.round(exact)) < 2 * TOL_PX
        assert np.array_equal(got[~near_integer], want[~near_integer])
        assert np.abs(got - want).max() <= 1 and (got != want).mean() < 1e-3


def test_batched_projection_matches_numpy_restatement():
    items = list(annotations())
    v = torch.tensor(np.stack([np.array(d["vertices"], np.float32) for d, _, _ in items])).cuda()
    mv = torch.tensor(np.stack([np.array(d["model_view_matrix"], np.float32) for d, _, _ in items])).cuda()
    pm = torch.tensor(np.stack([np.array(d["projection_matrix"], np.float32) for d, _, _ in items])).cuda()
    heights = torch.tensor([float(h) for _, h, _ in items])
    crop = torch.tensor([[10.0, 20.0], [0.0, 0.0], [-5.0, 7.0]])
    out = projection.project_batch(v, mv, pm, heights, crop, want_world=True, want_int=True)
    for i, (data, h, _) in enumerate(items):
        _, world, proj = projection_ref.load_mesh(data)
        ref = projection_ref.project_vertices_onto_image(world, proj, h, int(crop[i, 0]), int(crop[i, 1]))
        assert np.abs(out["world"][i].cpu().numpy() - world).max() < 1e-6
        assert np.abs(out["xy"][i].cpu().numpy() - ref).max() < TOL_PX
        assert torch.equal(out["xy_int"][i], out["xy"][i].to(torch.int32))
        single = projection.project_vertices_onto_image(world, proj, h, int(crop[i, 0]), int(crop[i, 1]))
        assert np.abs(single - ref).max() < TOL_PX


# ---- to the bit ----------------------------------------------------------------------------------------------------------
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def to_int(xy):
    """The kernel's (int) xy as include/dad3d.h states it: truncation toward zero, NaN -> 0, saturating at the int32 ends."""
    v = np.nan_to_num(xy.astype(np.float64), nan=0.0, posinf=INT_MAX, neginf=INT_MIN)
    return np.trunc(np.clip(v, INT_MIN, INT_MAX)).astype(np.int64).astype(np.int32)


def restated(v, mv, pm, height, crop):
    """(world [B,N,4], xy [B,N,2]) of a batch, one item at a time."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        world = [tbr.world(v[i], mv[i]) for i in range(len(v))]
        xy = [tbr.project(world[i], pm[i], int(height[i]), int(crop[i, 0]), int(crop[i, 1])) for i in range(len(v))]
    return np.stack(world), np.stack(xy)


def assert_projection_bits(v, mv, pm, height, crop, subsets=((True, True),)):
    world, xy = restated(v, mv, pm, height, crop)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()  # noqa: E731
    for want_world, want_int in subsets:
        out = projection.project_batch(dev(v), dev(mv), dev(pm), dev(height), dev(crop), want_world=want_world, want_int=want_int)
        assert set(out) == {"xy"} | ({"world"} if want_world else set()) | ({"xy_int"} if want_int else set())
        assert np.array_equal(out["xy"].cpu().numpy(), xy, equal_nan=True)
        if want_world:
            assert np.array_equal(out["world"].cpu().numpy(), world)
        if want_int:
            assert np.array_equal(out["xy_int"].cpu().numpy(), to_int(xy))
    return xy


def test_goldens_to_the_bit():
    items = list(annotations())
    v = np.stack([np.array(d["vertices"], np.float32) for d, _, _ in items])
    mv = np.stack([np.array(d["model_view_matrix"], np.float32) for d, _, _ in items])
    pm = np.stack([np.array(d["projection_matrix"], np.float32) for d, _, _ in items])
    height = np.array([h for _, h, _ in items], np.float32)
    crop = np.array([[10, 20], [0, 0], [-5, 7]], np.float32)
    xy = assert_projection_bits(v, mv, pm, height, crop)
    assert np.isfinite(xy).all()


@pytest.mark.parametrize("nver", [1, 255, 256, 257, 5023])
def test_seeded_cameras_to_the_bit_with_and_without_world_and_int(nver, static):
    """All four combinations of the two outputs `project_batch` makes optional (it always asks for xy). B = 4: four matrix pairs, heights and crop corners (two of them negative, one far enough that coordinates turn
    negative: the truncation is toward zero, not floor)."""
    sizes = [(480, 640), (1080, 1920), (333, 257), (720, 1280)]
    cams = [tbr.camera(100 + i, h, w, 150.0 + 60 * i, (w / 2 + 7 * i, h / 2 - 5 * i)) for i, (h, w) in enumerate(sizes)]
    v = np.stack([tbr.mesh(200 + i, static["template_geo"])[:nver] for i in range(4)])
    mv, pm = np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams])
    height = np.array([h for h, _ in sizes], np.float32)
    crop = np.array([[-13, -40], [2000, 1200], [0, -7], [31, 17]], np.float32)
    xy = assert_projection_bits(v, mv, pm, height, crop, subsets=list(itertools.product((False, True), repeat=2)))
    assert np.isfinite(xy).all() and np.abs(xy).max() < 2 ** 20
    if nver > 1:
        frac = xy[1] != np.trunc(xy[1])
        assert (xy[1] < 0).all() and frac.any()  # item 1 lies left of and above its crop corner
        assert np.array_equal(to_int(xy[1])[frac], np.ceil(xy[1][frac]).astype(np.int32))  # toward zero: up, on negatives


def test_points_behind_and_on_the_camera_plane():
    """Identity rotation, z translation -1: clip w = -(z - 1) exactly. w < 0 mirrors the point, w = 0 divides by zero (+-inf,
    NaN for 0 / 0), a tiny w overflows int32: xy to the bit, xy_int by the header's conversion rule."""
    mv, pm = tbr.camera(7, 480, 640, 200.0, (320, 240))
    mv[:3, :3] = np.eye(3, dtype=np.float32)
    mv[:3, 3] = (0, 0, -1)
    tiny = np.float32(1) - np.float32(2.0 ** -23)
    v = np.array([[0.05, 0.02, 0.0],      # in front: w = 1
                  [0.05, 0.02, 1.5],      # behind: w = -0.5
                  [0.05, -0.02, 1.0],     # on the plane: (+inf, -inf before the flip)
                  [-0.05, 0.0, 1.0],      # on the plane: (-inf, NaN)
                  [0.0, 0.0, 1.0],        # on the plane, on the axis: (NaN, NaN)
                  [1.0, -1.0, tiny],      # w = 2^-23: beyond int32 on both sides
                  [-1.0, 1.0, tiny]], np.float32)
    height, crop = np.array([480], np.float32), np.array([[-3, 4]], np.float32)
    xy = assert_projection_bits(v[None], mv[None], pm[None], height, crop)[0]
    w = tbr.world(v, mv)[:, 2] * -1
    assert w.tolist() == [1.0, -0.5, 0.0, 0.0, 0.0, 2.0 ** -23, 2.0 ** -23]
    assert np.isfinite(xy[:2]).all() and np.isinf(xy[2]).all() and np.isneginf(xy[3, 0]) and np.isnan(xy[3, 1]) and np.isnan(xy[4]).all()
    got = projection.project_batch(*(torch.from_numpy(a[None]).cuda() for a in (v, mv, pm)), 480.0,
                                   torch.tensor([[-3.0, 4.0]]), want_int=True)["xy_int"][0].cpu().numpy()
    assert got[2].tolist() == [INT_MAX, INT_MIN if xy[2, 1] < 0 else INT_MAX] and got[3].tolist() == [INT_MIN, 0] and got[4].tolist() == [0, 0]
    assert sorted(got[5].tolist() + got[6].tolist()) == [INT_MIN, INT_MIN, INT_MAX, INT_MAX]
