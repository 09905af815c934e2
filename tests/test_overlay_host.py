"""CPU: pins tests/overlay_restatement.py (the stroke rules the overlay kernels are held to) to facts countable by hand, and the host
side of dad_3dheads_amd.overlay (angles, arrow geometry, edge lists, argument checks) to a line-by-line restatement of the reference."""
import numpy as np
import pytest
import torch
from PIL import Image, ImageDraw

import overlay_restatement as R
from dad_3dheads_amd import _lib, overlay

RED = (255, 0, 0)


def blank(h=41, w=41):
    return np.zeros((h, w, 3), dtype=np.uint8)


def painted(img):
    return {(int(x), int(y)) for y, x in zip(*np.nonzero(img.any(2)))}


# -- discs --------------------------------------------------------------------------------------------------------------------------
def test_disc_radius_one_is_the_five_pixel_plus():
    img = R.draw_discs(blank(), np.array([[20.9, 20.2]], np.float32), 1, RED)
    assert painted(img) == {(20, 20), (19, 20), (21, 20), (20, 19), (20, 21)}
    assert (img[20, 20] == RED).all()


@pytest.mark.parametrize("r, half_widths", [(1, [1, 0]), (2, [2, 1, 0]), (3, [3, 2, 2, 0]), (4, [4, 3, 3, 2, 0]), (5, [5, 4, 4, 4, 3, 0])])
def test_disc_row_half_widths(r, half_widths):
    mask = R.disc_mask(41, 41, (20, 20), r)
    for dy in range(-r - 1, r + 2):
        row = np.flatnonzero(mask[20 + dy])
        if abs(dy) > r:
            assert row.size == 0
        else:
            hw = half_widths[abs(dy)]
            assert row.tolist() == list(range(20 - hw, 20 + hw + 1)), (r, dy)


# -- anti-aliased segments ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p0, p1", [((5, 9), (30, 9)), ((30, 9), (5, 9)), ((7, 3), (7, 33)), ((4, 6), (29, 31)), ((29, 6), (4, 31)), ((12, 12), (12, 12))])
def test_axis_aligned_and_diagonal_aa_segments_write_the_exact_colour_on_n_plus_one_pixels(p0, p1):
    color = (39, 48, 218)
    img = blank()
    img[:] = 77
    R.draw_aa(img, p0, p1, color)
    n = max(abs(p1[0] - p0[0]), abs(p1[1] - p0[1]))
    changed = (img != 77).any(2)
    assert changed.sum() == n + 1
    assert (img[changed] == color).all()
    assert changed[p0[1], p0[0]] and changed[p1[1], p1[0]]


def test_aa_weights_of_every_step_sum_to_256_and_follow_the_formula():
    rng = np.random.default_rng(3)
    for _ in range(300):
        p0, p1 = (int(v) for v in rng.integers(-60, 60, 2)), (int(v) for v in rng.integers(-60, 60, 2))
        p0, p1 = tuple(p0), tuple(p1)
        steps = R.aa_steps(p0, p1)
        n = max(abs(p1[0] - p0[0]), abs(p1[1] - p0[1]))
        assert steps.shape == (2 * (n + 1), 3)
        assert (steps[0::2, 2] + steps[1::2, 2] == 256).all()
        assert ((steps[:, 2] >= 0) & (steps[:, 2] <= 256)).all()
        assert len({(x, y) for x, y, _ in steps.tolist()}) == len(steps)  # no pixel twice
        # the first and the last step sit on the end points with the full weight
        assert steps[0].tolist() == [p0[0], p0[1], 256] and steps[-2].tolist() == [p1[0], p1[1], 256]
        # Python integers, one step at a time
        x_major = abs(p1[0] - p0[0]) >= abs(p1[1] - p0[1])
        d_minor = p1[1] - p0[1] if x_major else p1[0] - p0[0]
        minor0 = p0[1] if x_major else p0[0]
        for i in range(n + 1):
            q = 256 * minor0 + ((2 * i * d_minor * 256 + n) // (2 * n) if n else 0)
            assert steps[2 * i][1 if x_major else 0] == q >> 8 and steps[2 * i + 1][2] == q & 255


def scalar_fold(img, points, edges, color):
    for i0, i1 in edges:
        for x, y, a in R.aa_steps(tuple(points[i0]), tuple(points[i1])).tolist():
            R.blend(img, x, y, color, a)
    return img


def test_order_of_crossing_aa_segments_matters_and_matches_the_sequential_fold():
    pts = np.array([[3, 5], [36, 19], [4, 30], [35, 2]], np.float32)
    ipts = pts.astype(int)
    colors = np.array([[255, 0, 0], [0, 255, 0]], np.uint8)
    ab = R.draw_segments(blank(), pts, [[0, 1], [2, 3]], colors=colors)
    ba = R.draw_segments(blank(), pts, [[2, 3], [0, 1]], colors=colors[::-1])
    assert not np.array_equal(ab, ba)
    only_a, only_b = R.draw_segments(blank(), pts, [[0, 1]], color=RED), R.draw_segments(blank(), pts, [[2, 3]], color=RED)
    overlap = only_a.any(2) & only_b.any(2)
    assert overlap.any() and np.array_equal(ab[~overlap], ba[~overlap])
    # each equals its own pixel-by-pixel fold
    want_ab = scalar_fold(scalar_fold(blank(), ipts, [(0, 1)], colors[0]), ipts, [(2, 3)], colors[1])
    want_ba = scalar_fold(scalar_fold(blank(), ipts, [(2, 3)], colors[1]), ipts, [(0, 1)], colors[0])
    assert np.array_equal(ab, want_ab) and np.array_equal(ba, want_ba)


def test_skipped_primitives():
    pts = np.array([[5, 5], [np.nan, 5], [np.inf, 5], [8192.9, 5], [8193, 5], [-8192.5, 5], [-8193, 5], [20, 20]], np.float32)
    assert [R.point(pts, i) for i in range(8)] == [(5, 5), None, None, (8192, 5), None, (-8192, 5), None, (20, 20)]
    assert R.point(pts, 8) is None and R.point(pts, -1) is None
    img = R.draw_segments(blank(), pts, [[0, 1], [2, 7], [4, 0], [0, 7]], color=RED)
    assert np.array_equal(img, R.draw_segments(blank(), pts, [[0, 7]], color=RED))


# -- solid segments -----------------------------------------------------------------------------------------------------------------
def test_solid_thickness_one_covers_every_major_axis_column_and_both_ends():
    rng = np.random.default_rng(11)
    for _ in range(2000):
        p0, p1 = rng.integers(2, 62, 2), rng.integers(2, 62, 2)
        mask = R.solid_mask(64, 64, p0, p1, 1)
        assert mask[p0[1], p0[0]] and mask[p1[1], p1[0]]
        x_major = abs(p1[0] - p0[0]) >= abs(p1[1] - p0[1])
        lo, hi = sorted((p0[0], p1[0]) if x_major else (p0[1], p1[1]))
        cover = mask.any(0) if x_major else mask.any(1)
        assert cover[lo:hi + 1].all() and not cover[:lo].any() and not cover[hi + 1:].any(), (p0, p1)


@pytest.mark.parametrize("p0, p1", [((5, 9), (30, 9)), ((30, 9), (5, 9)), ((7, 3), (7, 33)), ((4, 6), (29, 31)), ((29, 6), (4, 31)), ((12, 12), (12, 12))])
def test_solid_thickness_one_equals_pil_on_axis_aligned_and_diagonal_segments(p0, p1):
    pil = Image.new("L", (41, 41), 0)
    ImageDraw.Draw(pil).line([p0, p1], fill=255, width=1)
    assert np.array_equal(R.solid_mask(41, 41, p0, p1, 1), np.asarray(pil) > 0)


def test_drawing_in_a_window_equals_the_whole_image_mask():
    rng = np.random.default_rng(12)
    for _ in range(200):
        p0, p1, t, r = rng.integers(-8, 48, 2), rng.integers(-8, 48, 2), int(rng.integers(1, 8)), int(rng.integers(1, 6))
        want = blank()
        want[R.solid_mask(41, 41, p0, p1, t)] = RED
        assert np.array_equal(R.draw_segments(blank(), np.array([p0, p1], np.float32), [[0, 1]], color=RED, thickness=t), want)
        want = blank()
        want[R.disc_mask(41, 41, p0, r)] = RED
        assert np.array_equal(R.draw_discs(blank(), np.array([p0], np.float32), r, RED), want)


def test_solid_thickness_two_horizontal_by_hand():
    # t = 2: within 1 of the segment: the row itself, the rows above and below over its span, and one pixel past each end
    mask = R.solid_mask(20, 20, (5, 10), (9, 10), 2)
    assert painted(np.repeat(mask[..., None], 3, 2).astype(np.uint8)) == (
        {(x, 10) for x in range(4, 11)} | {(x, 9) for x in range(5, 10)} | {(x, 11) for x in range(5, 10)})


# -- angles and arrows --------------------------------------------------------------------------------------------------------------
def test_limit_angle():
    for angle, want in [(0.0, 0.0), (180.0, 180.0), (-180.0, -180.0), (181.0, -179.0), (-181.0, 179.0), (359.5, -0.5), (-359.5, 0.5),
                        (540.0, -180.0), (725.0, 5.0), (-725.0, -5.0)]:
        assert overlay.limit_angle(angle) == R.limit_angle(angle) == want, angle


def seeded_rotations():
    rng = np.random.default_rng(5)
    rows = [np.array([1, 0, 0, 0, 1, 0], np.float32)]  # the identity
    for pitch in (179.9, -179.9, 180.0, 0.1, -0.1):  # a[0] - 180 on both sides of +-180
        c, s = np.cos(np.radians(pitch)), np.sin(np.radians(pitch))
        rows.append(np.array([1, 0, 0, 0, c, s], np.float32))
    rows += [r.astype(np.float32) for r in rng.normal(size=(40, 6))]
    return np.stack(rows)


def test_calculate_rpy_equals_the_line_by_line_restatement():
    rot = seeded_rotations()
    params = np.random.default_rng(6).normal(size=(len(rot), 413)).astype(np.float32)
    params[:, 403:409] = rot  # FlameParams.from_3dmm: shape 300, expression 100, jaw 3, rotation 6
    got = overlay.calculate_rpy(torch.from_numpy(params))
    assert len(got) == len(rot)
    for g, r in zip(got, rot):
        want = R.calculate_rpy(r)
        assert tuple(g) == want and all(-180.0 <= v <= 180.0 for v in g), (g, want)
    assert got[0].roll == 0.0 and abs(got[0].pitch) == 180.0 and got[0].yaw == 0.0  # the identity: a = (0, 0, 0) -> pitch -180
    assert overlay.calculate_rpy(params[3]) == [got[3]]  # one row, host array
    with pytest.raises(ValueError):
        overlay.calculate_rpy(np.zeros((2, 100), np.float32))


def test_pose_points_equal_the_restatement():
    for rpy in [overlay.RPY(0.0, -180.0, 0.0), overlay.RPY(12.5, -160.0, 30.0), overlay.RPY(-75.0, 10.0, -44.0)]:
        for h, w in [(200, 320), (954, 766)]:
            pts = overlay.pose_points(rpy, h, w)
            centre, ends = R.pose_axes(rpy, h, w)
            assert pts.dtype == np.int64 and pts.shape == (10, 2)
            assert tuple(pts[0]) == centre == (w // 2, h // 2) and [tuple(p) for p in pts[1:4]] == ends
            for k, end in enumerate(ends):
                assert [tuple(p) for p in pts[4 + 2 * k: 6 + 2 * k]] == R.arrow_tips(centre, end)
    # by hand: roll = pitch = yaw = 0, h = 400: size 40, x axis to the right; its tips are 4 long at pi +- pi / 4 from the end
    # (240, 200): 4 cos(5 pi / 4) = -2.83 -> (237, 197) first, then (237, 203)
    pts = overlay.pose_points(overlay.RPY(0.0, 0.0, 0.0), 400, 400)
    assert pts[:4].tolist() == [[200, 200], [240, 200], [200, 240], [200, 200]]
    assert pts[4:6].tolist() == [[237, 197], [237, 203]]
    assert overlay._POSE_EDGES.tolist() == [[0, 1], [1, 4], [1, 5], [0, 2], [2, 6], [2, 7], [0, 3], [3, 8], [3, 9]]
    assert overlay._POSE_SEGMENT_COLORS.tolist() == [[0, 0, 255]] * 3 + [[0, 255, 0]] * 3 + [[255, 0, 0]] * 3


# -- lists --------------------------------------------------------------------------------------------------------------------------
def test_mesh_edges_of_two_triangles():
    e = overlay.mesh_edges(np.array([[0, 1, 2], [2, 1, 3]]))
    assert e.dtype == np.int32 and e.tolist() == [[0, 1], [0, 2], [1, 2], [1, 3], [2, 3]]
    assert overlay.mesh_edges(np.array([[0, 1, 2], [2, 1, 3]]), subset=[1, 2, 3]).tolist() == [[1, 2], [1, 3], [2, 3]]
    packaged = overlay.mesh_edges()
    assert packaged.shape[1] == 2 and (packaged[:, 0] < packaged[:, 1]).all() and packaged.max() == 5022
    assert len(np.unique(packaged, axis=0)) == len(packaged)


def test_landmark_subsets(static):
    assert [len(overlay.landmark_indices(s)) for s in ("191", "445", "565")] == [191, 445, 565]
    assert np.array_equal(overlay.landmark_indices("565"), static["lmk_565"])
    for bad in ("68", "head", 445, None):
        with pytest.raises(ValueError, match="subset"):
            overlay.landmark_indices(bad)


def test_load_edges(tmp_path):
    e = np.array([[0, 1], [2, 3]], np.int16)
    np.save(tmp_path / "head_edges.npy", e)
    assert overlay.load_edges(str(tmp_path / "head_edges.npy")).tolist() == e.tolist()
    assert overlay.load_edges(tmp_path / "head_edges.npy").dtype == np.int32
    for bad in (np.zeros((3, 3), np.int32), np.zeros((3, 2), np.float32), np.zeros(4, np.int64)):
        with pytest.raises(ValueError, match="edges"):
            overlay.load_edges(bad)


# -- argument checks: all before any device work ------------------------------------------------------------------------------------
def test_python_argument_checks():
    img = torch.zeros((2, 300, 200, 3), dtype=torch.uint8)
    pred = {"points": np.zeros((2, 68, 2), int), "projected_vertices": torch.zeros((2, 5023, 2)), "3dmm_params": torch.zeros((2, 413))}
    with pytest.raises(ValueError, match="subset"):
        overlay.draw_3d_landmarks(pred, img, "68")
    for bad in (img.float(), torch.zeros((2, 300, 200, 4), dtype=torch.uint8), torch.zeros((300, 200), dtype=torch.uint8),
                [torch.zeros((300, 200, 3), dtype=torch.uint8), torch.zeros((300, 200, 1), dtype=torch.uint8)]):
        with pytest.raises(ValueError, match="images"):
            overlay.draw_landmarks(pred, bad)
    with pytest.raises(ValueError, match="thickness"):  # int(199 * 0.005) == 0
        overlay.draw_pose(pred, torch.zeros((2, 199, 300, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="thickness"):
        overlay.draw_segments(img, pred["projected_vertices"], [[0, 1]], thickness=256)
    with pytest.raises(ValueError, match="radius"):
        overlay.draw_points(img, pred["points"], radius=0)
    with pytest.raises(ValueError, match="color"):
        overlay.draw_points(img, pred["points"], color=(0, 0, 256))
    with pytest.raises(ValueError, match="edges"):
        overlay.draw_mesh(pred, img, np.array([[0, 5023]]))
    with pytest.raises(ValueError, match="edges"):
        overlay.draw_mesh(pred, img, np.zeros((4, 3), np.int32))
    with pytest.raises(ValueError, match="colors"):
        overlay.draw_segments(img, pred["projected_vertices"], [[0, 1]], colors=np.zeros((2, 3), np.uint8))
    with pytest.raises(ValueError, match="holds 2 items for 3 images"):
        overlay.draw_landmarks(pred, torch.zeros((3, 300, 200, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="CUDA"):  # valid arguments, host images: no CPU fallback
        overlay.draw_landmarks(pred, img)


def test_c_abi_argument_checks():
    lib = _lib.load()
    p = 4096  # never dereferenced: every call below is refused before any device work
    seg = lambda **k: lib.dad3d_overlay_segments(*[{**dict(src=p, dst=p, batch=1, h=8, w=8, points=p, n_points=4, edges=p, n_edges=2,
                                                             colors=None, color=0, thickness=0, device=0, stream=None), **k}[n]
                                                   for n in ("src", "dst", "batch", "h", "w", "points", "n_points", "edges", "n_edges", "colors",
                                                             "color", "thickness", "device", "stream")])
    disc = lambda **k: lib.dad3d_overlay_discs(*[{**dict(src=p, dst=p, batch=1, h=8, w=8, points=p, n_points=4, index=None, n_discs=2,
                                                         radius=1, color=0, device=0, stream=None), **k}[n]
                                                 for n in ("src", "dst", "batch", "h", "w", "points", "n_points", "index", "n_discs", "radius",
                                                           "color", "device", "stream")])
    for call, bad in [(seg, dict(thickness=-1)), (seg, dict(thickness=256)), (seg, dict(h=0)), (seg, dict(w=8193)), (seg, dict(batch=-1)),
                      (seg, dict(batch=65536)), (seg, dict(src=None)), (seg, dict(dst=None)), (seg, dict(points=None)), (seg, dict(edges=None)),
                      (seg, dict(n_edges=-1)), (seg, dict(edges=p + 2)), (disc, dict(radius=0)), (disc, dict(radius=8193)), (disc, dict(h=8193)),
                      (disc, dict(dst=None)), (disc, dict(points=None)), (disc, dict(n_discs=5)), (disc, dict(n_points=-1))]:
        lib.dad3d_clear_error()
        assert call(**bad) == _lib.E_INVALID, bad
        assert b"dad3d_overlay_" in lib.dad3d_last_error(), bad
    assert seg(batch=0, src=None, dst=None) == _lib.OK and disc(batch=0, src=None, dst=None) == _lib.OK  # nothing to do
