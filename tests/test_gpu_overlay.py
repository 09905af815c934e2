"""GPU: the overlay kernels (csrc/overlay.hip) and dad_3dheads_amd.overlay, bit-equal to tests/overlay_restatement.py (which
tests/test_overlay_host.py pins by hand). Batches of three images with their own point tables, 40 x 56 and 70 x 33 pixels: no tile
size divides them, both have more than one tile each way."""
import numpy as np
import pytest
import torch

import overlay_restatement as R
from dad_3dheads_amd import overlay

pytestmark = pytest.mark.gpu

SIZES = [(40, 56), (70, 33)]
B = 3
COLOR = (39, 48, 218)


def noise(h, w, seed, b=B):
    return np.random.default_rng(seed).integers(0, 256, (b, h, w, 3), dtype=np.uint8)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_segments(images, points, edges, color=COLOR, colors=None, thickness=0):
    """draw_segments on the GPU against the restatement, image by image; also that the input stays as it was."""
    src = cuda(images)
    got = overlay.draw_segments(src, cuda(points), np.asarray(edges, dtype=np.int32).reshape(-1, 2), color=color, colors=colors,
                                thickness=thickness)
    assert got.data_ptr() != src.data_ptr() and np.array_equal(src.cpu().numpy(), images)
    got = got.cpu().numpy()
    for b in range(len(images)):
        want = R.draw_segments(images[b].copy(), points[b], edges, color=color, colors=colors, thickness=thickness)
        assert np.array_equal(got[b], want), (b, np.argwhere((got[b] != want).any(2))[:8])
    return got


def check_discs(images, points, radius, index=None):
    src = cuda(images)
    got = overlay.draw_points(src, cuda(points), radius=radius, index=None if index is None else cuda(np.asarray(index, np.int32)))
    assert np.array_equal(src.cpu().numpy(), images)
    got = got.cpu().numpy()
    for b in range(len(images)):
        want = R.draw_discs(images[b].copy(), points[b], radius, overlay.POINT_COLOR, index=index)
        assert np.array_equal(got[b], want), (b, np.argwhere((got[b] != want).any(2))[:8])
    return got


def random_points(h, w, n, seed, margin=12):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-margin, w + margin, (B, n)), rng.uniform(-margin, h + margin, (B, n))], -1).astype(np.float32)


@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("thickness", [0, 1, 2, 4, 7])
def test_segments_across_tile_borders(hw, thickness):
    h, w = hw
    pts = random_points(h, w, 24, seed=1)
    got = check_segments(noise(h, w, 2), pts, [(i, i + 1) for i in range(0, 24, 2)] + [(0, 5), (7, 2)], thickness=thickness)
    assert (got != noise(h, w, 2)).any()


@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("thickness", [0, 2])
def test_segments_off_the_image_at_the_coordinate_limit_and_beyond(hw, thickness):
    h, w = hw
    # 0, 1: inside; 2 .. 5: the limits (8192.9 and -8192.9 truncate onto them); 6 .. 9: just beyond, skipped; 10, 11: off the image
    one = np.array([[5, 6], [w - 4, h - 7], [8192, 11], [-8192, h - 3], [8192.9, -8192.9], [13, 8192], [8193, 5], [3, -8193], [-8193.5, 9],
                    [9000, 9000], [-30, -25], [w + 40, h + 9]], np.float32)
    pts = np.stack([one, one[:, ::-1] * np.float32(1), one + np.float32(0.75)])
    pts[1, :2], pts[2, 6:10] = one[:2], one[6:10]
    edges = [(0, 2), (1, 3), (0, 4), (5, 1), (2, 3), (4, 5), (0, 6), (7, 1), (8, 0), (1, 9), (10, 11), (10, 0), (11, 1), (2, 4), (0, 1)]
    check_segments(noise(h, w, 3), pts, edges, thickness=thickness)


@pytest.mark.parametrize("hw", SIZES)
def test_non_finite_coordinates_skip_the_primitive_only(hw):
    h, w = hw
    pts = random_points(h, w, 10, seed=4, margin=0)
    pts[0, 3, 0], pts[1, 4, 1], pts[2, 5, 0], pts[2, 6, 1] = np.nan, np.inf, -np.inf, np.nan
    edges = [(0, 1), (2, 3), (4, 5), (6, 7), (8, 9), (3, 4), (1, 2)]
    for thickness in (0, 3):
        got = check_segments(noise(h, w, 5), pts, edges, thickness=thickness)
        assert (got != noise(h, w, 5)).any(3).any(2).any(1).all()  # the rest is still drawn, in every image
    check_discs(noise(h, w, 5), pts, 3)


@pytest.mark.parametrize("hw", SIZES)
def test_zero_length_segments(hw):
    h, w = hw
    pts = random_points(h, w, 6, seed=6, margin=0)
    pts[:, 5] = [w - 1, h - 1]
    edges = [(0, 0), (1, 1), (2, 2), (5, 5), (3, 4), (3, 3)]
    for thickness in (0, 1, 2, 5):
        check_segments(noise(h, w, 7), pts, edges, thickness=thickness)


@pytest.mark.parametrize("n_edges", [300, 513])
def test_many_segments_through_one_neighbourhood_fold_in_order_across_chunks(n_edges):
    h, w = SIZES[0]
    rng = np.random.default_rng(8)
    pts = np.stack([rng.uniform(27, 37, (B, 64)), rng.uniform(28, 36, (B, 64))], -1).astype(np.float32)  # round the tile corner (32, 32)
    edges = rng.integers(0, 64, (n_edges, 2))
    colors = rng.integers(0, 256, (n_edges, 3), dtype=np.uint8)
    got = check_segments(noise(h, w, 9), pts, edges, colors=colors)
    # the order matters here: the reversed list gives another picture
    back = overlay.draw_segments(cuda(noise(h, w, 9)), cuda(pts), edges[::-1].copy(), colors=colors[::-1].copy()).cpu().numpy()
    assert not np.array_equal(got, back)
    check_segments(noise(h, w, 9), pts, edges, colors=colors, thickness=2)


@pytest.mark.parametrize("hw", SIZES)
def test_per_segment_colour_table(hw):
    h, w = hw
    pts = random_points(h, w, 16, seed=10)
    edges = [(i, (i * 5 + 3) % 16) for i in range(16)]
    colors = np.random.default_rng(11).integers(0, 256, (16, 3), dtype=np.uint8)
    check_segments(noise(h, w, 12), pts, edges, colors=colors)
    check_segments(noise(h, w, 12), pts, edges, colors=colors, thickness=4)


@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("radius", [1, 3, 5])
def test_discs_at_corners_and_off_the_image(hw, radius):
    h, w = hw
    one = np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1], [-radius, 5], [w + radius - 1, h // 2], [w // 2, -radius - 1], [31.9, 32.1],
                    [w // 2, h + radius], [8192, 8192], [8193, 3], [-5000, 7], [np.nan, 3], [16.5, 15.5]], np.float32)
    pts = np.stack([one, one + np.float32(0.5), one - np.float32(0.5)])
    check_discs(noise(h, w, 13), pts, radius)
    check_discs(noise(h, w, 13), pts, radius, index=[13, 0, 3, 7, 7, 12, 99, -1])


def test_out_of_place_leaves_the_source_and_equals_in_place():
    h, w = SIZES[1]
    images, pts = noise(h, w, 14), random_points(h, w, 12, seed=15)
    edges = np.array([(i, (i + 5) % 12) for i in range(12)], np.int32)
    for draw in (lambda src, **k: overlay.draw_segments(src, cuda(pts), edges, **k),
                 lambda src, **k: overlay.draw_segments(src, cuda(pts), edges, thickness=3, **k),
                 lambda src, **k: overlay.draw_points(src, cuda(pts), radius=2, **k)):
        src = cuda(images)
        apart = draw(src)
        assert np.array_equal(src.cpu().numpy(), images) and not np.array_equal(apart.cpu().numpy(), images)
        other = torch.zeros_like(src)
        assert draw(src, out=other) is other and torch.equal(other, apart) and np.array_equal(src.cpu().numpy(), images)
        assert draw(src, out=src) is src and torch.equal(src, apart)
    one = cuda(images[0])  # a single [H,W,3] image comes back as one
    assert torch.equal(overlay.draw_points(one, cuda(pts[0]), radius=2), overlay.draw_points(cuda(images), cuda(pts), radius=2)[0])


def test_full_size_image_with_the_mesh_sized_edge_list():
    """954 x 766, 10 938 edges over 5023 points: the demo's head mesh in size. The points are a seeded walk, so that the edges
    (between points a few steps apart) are as short as a mesh's."""
    h, w, n, e = 954, 766, 5023, 10938
    rng = np.random.default_rng(16)
    walk = np.cumsum(rng.uniform(-9, 9, (n, 2)), 0)
    walk = (walk - walk.min(0)) / (walk.max(0) - walk.min(0)) * [w + 40, h + 40] - 20  # a little over the border
    pts = walk.astype(np.float32)[None]
    first = rng.integers(0, n, e)
    edges = np.stack([first, np.clip(first + rng.integers(-3, 4, e), 0, n - 1)], 1)
    images = noise(h, w, 17, b=1)
    got = check_segments(images, pts, edges)
    assert ((got != images).any(3).sum()) > 20000
    check_discs(images, pts, 4, index=rng.integers(0, n, 565))


# -- the public functions on a predictor's results ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def predicted(flame_model):
    from dad_3dheads_amd.predictor import FaceMeshPredictor

    pred = FaceMeshPredictor.random_init(cuda_id=0, flame_model=flame_model)
    rng = np.random.default_rng(18)
    photos = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in [(240, 200), (210, 260), (240, 200)]]
    results = pred.predict_batch(photos, device_outputs=True)
    assert all(r["projected_vertices"].is_cuda and r["3dmm_params"].is_cuda for r in results)
    return photos, results


def host_dicts(results):
    return [{k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in r.items()} for r in results]


def reference_overlays(photos, results, edges):
    """What every public function must return, from the restatement fed the same tensors."""
    out = {k: [] for k in ("68", "191", "445", "565", "mesh", "pose")}
    for photo, r in zip(photos, results):
        h, w = photo.shape[:2]
        verts = r["projected_vertices"].cpu().numpy().reshape(-1, 2)
        radius = max(1, int(min(h, w) * 0.005))
        out["68"].append(R.draw_discs(photo.copy(), np.asarray(r["points"], np.float32), radius, (255, 0, 0)))
        for subset in ("191", "445", "565"):
            out[subset].append(R.draw_discs(photo.copy(), verts, radius, (255, 0, 0), index=overlay.landmark_indices(subset)))
        out["mesh"].append(R.draw_segments(photo.copy(), verts, edges, color=(39, 48, 218)))
        out["pose"].append(R.draw_pose(photo.copy(), R.calculate_rpy(r["3dmm_params"].cpu().numpy()[0, 403:409])))
    return out


def test_public_functions_equal_the_restatement_in_every_input_form(predicted, static):
    photos, results = predicted
    edges = overlay.mesh_edges(static["faces"][:1500])
    want = reference_overlays(photos, results, edges)
    calls = {"68": lambda p, im: overlay.draw_landmarks(p, im), "191": lambda p, im: overlay.draw_3d_landmarks(p, im, "191"),
             "445": lambda p, im: overlay.draw_3d_landmarks(p, im, "445"), "565": lambda p, im: overlay.draw_3d_landmarks(p, im, "565"),
             "mesh": lambda p, im: overlay.draw_mesh(p, im, edges), "pose": lambda p, im: overlay.draw_pose(p, im)}
    mixed = [cuda(p) for p in photos]
    same = [0, 2]  # the two photos of one size, as a batch tensor
    batch = torch.stack([mixed[i] for i in same])
    for name, call in calls.items():
        got = call(results, mixed)  # a mixed-size list, device dicts
        assert isinstance(got, list) and len(got) == 3
        for i in range(3):
            assert np.array_equal(got[i].cpu().numpy(), want[name][i]), (name, i)
            assert np.array_equal(mixed[i].cpu().numpy(), photos[i])  # the inputs stay as they were
            assert torch.equal(call(results[i], mixed[i]), got[i]), (name, i)  # one image, its own dict
        from_host = call(host_dicts(results), mixed)  # host dicts are uploaded
        assert all(torch.equal(a, b) for a, b in zip(from_host, got)), name
        as_batch = call([results[i] for i in same], batch)  # a batch tensor
        assert as_batch.shape == batch.shape and all(torch.equal(as_batch[k], got[i]) for k, i in enumerate(same)), name
    # the batched dict of predict_tensor's form
    stacked = {"points": np.stack([results[i]["points"] for i in same]),
               "projected_vertices": torch.cat([results[i]["projected_vertices"] for i in same]),
               "3dmm_params": torch.cat([results[i]["3dmm_params"] for i in same])}
    for name, call in calls.items():
        assert all(np.array_equal(call(stacked, batch)[k].cpu().numpy(), want[name][i]) for k, i in enumerate(same)), name
    assert all((want["pose"][i] != photos[i]).any() for i in range(3))  # the arrows start at the centre, whatever the network says


def test_draw_landmarks_with_points_inside_the_images():
    """An untrained network may put every landmark off the image; here they lie inside, as integers on the host like `predict_batch`'s."""
    rng = np.random.default_rng(19)
    photos = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in [(240, 200), (210, 260), (240, 200)]]
    preds = [{"points": np.stack([rng.integers(0, p.shape[1], 68), rng.integers(0, p.shape[0], 68)], 1)} for p in photos]
    got = overlay.draw_landmarks(preds, [cuda(p) for p in photos])
    for g, photo, pred in zip(got, photos, preds):
        want = R.draw_discs(photo.copy(), pred["points"].astype(np.float32), 1, (255, 0, 0))
        assert np.array_equal(g.cpu().numpy(), want) and 60 <= (want != photo).any(2).sum() <= 68 * 5
