"""GPU: hostile meshes through the three rasters that had only ever drawn head meshes -- `frames_tile_kernel` (csrc/sim3dr_frames.hip), the
textured tile kernel (csrc/sim3dr_frames_texture.hip; both walk their lists through `walk_frame_tile`, csrc/sim3dr_frames.hpp) and
`depth_raster_kernel` (csrc/uv_texture_occlusion.hip) -- on the cases of tests/raster_cases.py: the eight profiles of
test_gpu_raster_fuzz.py as scenes of three heads in three frames, one frame-covering triangle per box width, and hand-made pairs.

Every comparison is np.array_equal against the reference (`sim3dr_oracle`; the compiled `_render_texture_core` for textures): bytes for
frames, floats for depth maps. Every flag is predicted on the CPU (`raster_cases.admitted` from the reference's box and the documented
pool; `texture_occlusion_restatement.expected_window`) and never read from the device to build an expectation.
tests/test_raster_cases_host.py certifies, in the reference alone, that the cases reach what the docstrings below claim; the counts
quoted there are its output for `raster_cases.SEEDS` (head 0 of each scene on its own canvas, summed over the four seeds)."""
import numpy as np
import pytest
import torch

import raster_cases as RC
import render_frames_restatement as RF
import render_texture_ref as RT
import texture_frames_restatement as TF
import texture_occlusion_restatement as TO
from dad_3dheads_amd import _lib
from dad_3dheads_amd.Sim3DR import Mesh
from dad_3dheads_amd.uv_texture import UVMap

pytestmark = pytest.mark.gpu
MAPPING = {0: "nearest", 1: "bilinear"}
TEX = 16
TEXTURED_PROFILES = ("pixel_centres", "tie_planes", "tile_straddle", "mixed_sizes")
SENTINEL = -7.0


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_the_constants_of_the_cases_are_the_library_s():
    assert (RC.FRAME_FLAG_INDEX, RC.FRAME_FLAG_CAPACITY) == (_lib.FRAME_FLAG_INDEX, _lib.FRAME_FLAG_CAPACITY)
    assert (TO.BAKE_FLAG_INDEX, TO.BAKE_FLAG_DEPTH_WINDOW, TO.BAKE_FLAG_NONFINITE) == (_lib.BAKE_FLAG_INDEX, _lib.BAKE_FLAG_DEPTH_WINDOW,
                                                                                      _lib.BAKE_FLAG_NONFINITE)


def device_frames(sc):
    """The scene's frames on the device: contiguous tensors, but frame `view` as a strided view at an odd address inside a wider buffer.
    -> (frames, wide, pattern): `pattern` is the wide buffer as it was, for the bytes outside the view."""
    dev = [cuda(b) for b in sc["bgs"]]
    h, w = sc["bgs"][sc["view"]].shape[:2]
    wide = cuda(np.random.default_rng(sc["seed"]).integers(0, 256, (h, w + 10, 3), dtype=np.uint8))
    wide[:, 5:5 + w] = dev[sc["view"]]
    pattern = wide.clone()
    view = wide[:, 5:5 + w]
    assert view.stride(0) == 3 * (w + 10) and view.data_ptr() % 2 == 1
    dev[sc["view"]] = view
    return dev, wide, pattern


def assert_frames(got, want, what=""):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), f"{what} frame {i} of {g.shape}: {int((g != w).any(-1).sum())} pixels differ, first at " \
                                     f"{np.argwhere((g != w).any(-1))[:4].tolist()}"


def assert_outside_the_view_untouched(sc, wide, pattern, what):
    w = sc["bgs"][sc["view"]].shape[1]
    assert torch.equal(wide[:, :5], pattern[:, :5]) and torch.equal(wide[:, 5 + w:], pattern[:, 5 + w:]), what


# ---- 1. rasterize_frames on the scenes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", RC.PROFILES)
def test_rasterize_frames_on_hostile_scenes(sim3dr_oracle, profile):
    """Three hostile heads in three frames (one not a multiple of 64 a side, one exactly 64 x 64, one a strided view at an odd address), both
    `reverse` settings, four seeds a profile. Reached, per the host test (head 0 alone, four seeds):
      * the whole-wave walk of `walk_frame_tile` and its reciprocal division: boxes of more than 32 pixels inside a tile -- pixel_centres 524,
        slivers 422, tie_planes 522, tile_straddle 486, mixed_sizes 488, split_tile 3590, wild 523, layers 4264 (of them over 64 pixels: 521,
        380, 521, 441, 447, 3565, 523, 1327);
      * the winner rule (head + 1 | depth_order_number(z) | 0xFFFE - triangle): pixels where two triangles of one head reach the winning
        depth and the lowest index must win -- tie_planes 2223, layers 889, pixel_centres 363; negative against positive depths at one
        pixel -- between 16681 (slivers) and 76474 (tile_straddle) pixels in every profile;
      * the strict interior test `u > 0, v > 0, w0 > 0` on pixel centres: pixels whose centre lies on an edge, where the strict and the
        `>=` test of the reference disagree -- pixel_centres 19244, tie_planes 17259, layers 1909;
      * inv = 0 in `tri_setup`: triangles of exactly zero area -- slivers 220, wild 37, tile_straddle 29, pixel_centres 28 (and slivers' huge inv);
      * `f2i_x86` on 1e7 and 3e38 (wild), the `z > -1e8f` test on overflowing depths (wild's 3e38 z);
      * triangles over several tiles and the frame's edge: the tile boxes of `frames_box_kernel`, both passes of `frames_bin_kernel`, the same
        triangle walked from several tiles, and the admission of `frames_plan_kernel` -- of the 32 scenes 5 have a head with
        DAD3D_FRAME_FLAG_CAPACITY (pixel_centres 4, tie_planes 4, tile_straddle 4, wild 1 and 4), tile_straddle 4 with a later head
        that is still admitted ([0, CAPACITY, 0]); in every profile at least half of the scenes draw all three heads.
    The flags equal `raster_cases.admitted`, the frames the reference's with the predicted heads skipped; no byte of the strided view's
    buffer outside [row, row + 3 w) changes, and a frame that no admitted head names keeps its bytes."""
    for seed in RC.SEEDS:
        sc = RC.scene(seed, profile)
        predicted = RC.scene_flags(sc)
        skip = {k for k, f in enumerate(predicted) if f}
        mesh = Mesh(sc["t"], sc["verts"].shape[1], device=0)
        v, col = cuda(sc["verts"]), cuda(sc["cols"])
        for reverse in (False, True):
            what = f"{profile} seed {seed} reverse {reverse}"
            dev, wide, pattern = device_frames(sc)
            flags = mesh.rasterize_frames(dev, v, col, sc["image_index"], reverse=reverse)
            torch.cuda.synchronize()
            assert flags.cpu().tolist() == predicted, what
            with np.errstate(all="ignore"):
                want = RF.expected_frames(sim3dr_oracle, sc["bgs"], sc["verts"], sc["t"], sc["cols"], sc["image_index"], reverse=reverse, skip=skip)
            got = [d.cpu().numpy() for d in dev]
            assert_frames(got, want, what)
            assert_outside_the_view_untouched(sc, wide, pattern, what)
            named = {f for k, f in enumerate(sc["image_index"]) if k not in skip}
            for f, bg in enumerate(sc["bgs"]):
                if f not in named:
                    assert np.array_equal(got[f], bg), (what, f)
            if len(skip) < 3:
                assert any(not np.array_equal(w, b) for w, b in zip(want, sc["bgs"])), what  # something was drawn


# ---- 2. every box width of the whole-wave walk ------------------------------------------------------------------------------------
def test_rasterize_frames_visits_every_pixel_of_every_box_width(sim3dr_oracle):
    """`walk_frame_tile`'s row of a pixel, `(int)((p + 0.5f) * rcp(bw))`, over every pair it can meet: 256 frames whose one triangle's clipped
    box is the whole tile part -- bw in 1..64 with bh in {1, 63, 64}, and the second tile (px0 = 64, bw wide) of frames 64 x (64 + bw) --
    so every p < bw * bh is visited (host test: of the 293 heads' boxes 256 are over 32 pixels, 217 over 64; 37 frames take a second head
    from behind). Byte-equal
    to the reference, and no background byte is left: a missed pixel shows even where the reference would be wrong in the same way."""
    wb = RC.whole_box_frames()
    bgs = [np.full((h, w, 3), RC.WHOLE_BOX_BG, np.uint8) for h, w in wb["shapes"]]
    dev = [cuda(b) for b in bgs]
    mesh = Mesh(wb["t"], 3, device=0)
    flags = mesh.rasterize_frames(dev, cuda(wb["verts"]), cuda(wb["cols"]), wb["image_index"])
    torch.cuda.synchronize()
    assert flags.cpu().tolist() == [0] * len(wb["verts"])
    got = [d.cpu().numpy() for d in dev]
    for f, g in enumerate(got):
        assert (g != RC.WHOLE_BOX_BG).all(), f"frame {f} of {wb['shapes'][f]}: pixels {np.argwhere((g == RC.WHOLE_BOX_BG).any(-1))[:4].tolist()} were missed"
    assert_frames(got, RF.expected_frames(sim3dr_oracle, bgs, wb["verts"], wb["t"], wb["cols"], wb["image_index"]), "whole boxes")


# ---- 3. textured heads ------------------------------------------------------------------------------------------------------------
def _texturing(sc):
    """Per-corner texture coordinates from a seeded draw (a little outside the texture: the clamp) and a small noise texture per head."""
    rng = np.random.default_rng([sc["seed"], 5])
    ntri = len(sc["t"])
    tc = np.zeros((3 * ntri, 3), np.float32)
    tc[:, :2] = rng.uniform(-1.5, TEX + 0.5, (3 * ntri, 2))
    tt = np.arange(3 * ntri, dtype=np.int32).reshape(ntri, 3)
    tex = rng.integers(0, 256, (3, TEX, TEX, 3), dtype=np.uint8)
    return tc, tt, tex


@pytest.mark.parametrize("profile", TEXTURED_PROFILES)
def test_render_texture_frames_on_hostile_scenes(profile):
    """The textured tile kernel on the scenes of four profiles, both mappings: the same walk and key as above, but coverage by
    `u >= 0, v >= 0, u + v < 1` (a zero-area triangle, inv = 0, covers its box) or the frame's two-pixel band, where every triangle whose
    box reaches the pixel competes with extrapolated weights -- these heads reach every frame's band, head meshes hardly do. Flags as
    predicted on the CPU; frames equal to the compiled `_render_texture_core` called per head on the running frame with the predicted heads
    skipped (where oracle/_ref holds it), and to the same loop over the batched `Mesh.render_texture`."""
    for seed in RC.SEEDS:
        sc = RC.scene(seed, profile)
        predicted = RC.scene_flags(sc)
        skip = {k for k, f in enumerate(predicted) if f}
        tc, tt, tex = _texturing(sc)
        mesh = Mesh(sc["t"], sc["verts"].shape[1], device=0).set_texcoords(tc, tt)
        v, dtex = cuda(sc["verts"]), cuda(tex)
        for mapping in (0, 1):
            what = f"{profile} seed {seed} {MAPPING[mapping]}"
            dev, wide, pattern = device_frames(sc)
            flags = mesh.render_texture_frames(dev, v, dtex, sc["image_index"], mapping=MAPPING[mapping])
            torch.cuda.synchronize()
            assert flags.cpu().tolist() == predicted, what
            got = [d.cpu().numpy() for d in dev]
            batched = [cuda(b) for b in sc["bgs"]]
            for k, f in enumerate(sc["image_index"]):
                if k not in skip:
                    mesh.render_texture(v[k][None], dtex[k], batched[f][None], mapping=MAPPING[mapping])
            torch.cuda.synchronize()
            assert_frames(got, [b.cpu().numpy() for b in batched], what + " (batched route)")
            if RT.ref_available():
                with np.errstate(all="ignore"):
                    want = TF.expected_textured_frames(sc["bgs"], sc["verts"], sc["t"], tex, tc[:, :2], tt, sc["image_index"], mapping, skip=skip)
                assert_frames(got, want, what)
                if len(skip) < 3:
                    assert any(not np.array_equal(w, b) for w, b in zip(want, sc["bgs"])), what
            assert_outside_the_view_untouched(sc, wide, pattern, what)


# ---- 4. depth maps ----------------------------------------------------------------------------------------------------------------
def depth_maps(m, shapes, verts, index, side):
    """-> (depth, window, flags) as numpy; the maps start as SENTINEL everywhere."""
    dev = [torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda") for h, w in shapes]
    out = torch.full((len(verts), side, side), SENTINEL, dtype=torch.float32, device="cuda")
    depth, window, flags = m.depth_frames(cuda(verts), dev, index, depth_side=side, out=out)
    torch.cuda.synchronize()
    return depth.cpu().numpy(), window.cpu().numpy(), flags.cpu().numpy()


def assert_depth(got, want, what=""):
    """Window, flags and every cell; outside its window (and all of a flagged head's map) the sentinel; never a stored -0."""
    (depth, window, flags), (want_maps, want_window, want_flags) = got, want
    assert flags.tolist() == want_flags.tolist(), what
    assert np.array_equal(window, want_window), (what, window.tolist(), want_window.tolist())
    for k, wm in enumerate(want_maps):
        inside = np.zeros(depth[k].shape, bool)
        if wm is not None:
            wh, ww = wm.shape
            inside[:wh, :ww] = True
            g = depth[k, :wh, :ww]
            assert np.array_equal(g, wm, equal_nan=True), f"{what} head {k}: {int((g != wm).sum())} of {wm.size} cells differ, first at " \
                                                          f"{np.argwhere(g != wm)[:4].tolist()}"
            assert not np.signbit(g[g == 0]).any(), f"{what} head {k}: a stored -0"
        assert (depth[k][~inside] == SENTINEL).all(), f"{what} head {k}: a cell outside the window was written"


@pytest.mark.parametrize("profile", RC.PROFILES)
def test_depth_frames_on_hostile_scenes(sim3dr_oracle, profile):
    """`depth_raster_kernel` on every scene: the whole-wave walk above 64 pixels with its integer division (boxes over 64 pixels per the host
    test: 521, 380, 521, 441, 447, 3565, 523, 1327 in the order of `PROFILES`), the interior test `u >= 0, v >= 0, u + v < 1` on pixel
    centres and on zero-area triangles (they cover their boxes), the `z < 1e8f` test and `f2i_x86` on wild's 1e7 and 3e38 (finite: the
    window is clipped to the frame, the head is not refused as non-finite), and the signed-minimum / unsigned-maximum winner on the
    float's bits with negative and positive depths at one pixel in either arrival order (16681 to 76474 such pixels a profile). Once
    with a `depth_side` that holds every window, once one pixel too small for the largest: DAD3D_BAKE_FLAG_DEPTH_WINDOW as
    `expected_window` predicts. Window, flags and every cell equal the reference's; cells outside a window keep the sentinel."""
    for seed in RC.SEEDS:
        sc = RC.scene(seed, profile)
        shapes = [b.shape[:2] for b in sc["bgs"]]
        m = UVMap(sc["t"], sc["verts"].shape[1], RC.tiny_atlas(sc["t"]), device=0)
        assert np.isfinite(sc["verts"]).all()
        with np.errstate(all="ignore"):
            roomy = TO.expected_depth_frames(sim3dr_oracle, shapes, sc["verts"], sc["t"], sc["image_index"], 280)
        assert roomy[2].tolist() == [0, 0, 0]
        largest = int(roomy[1][:, 2:].max())
        assert 0 < largest <= 280
        if profile == "wild":  # a huge coordinate clips the window to the frame's edge
            k = int(np.argmax(np.abs(sc["verts"][:, :, :2]).max((1, 2))))
            h, w = shapes[sc["image_index"][k]]
            assert np.abs(sc["verts"][k, :, :2]).max() >= 1e7 and (roomy[1][k, 2] == w or roomy[1][k, 3] == h)
        for side in (largest, largest - 1):
            what = f"{profile} seed {seed} depth_side {side}"
            with np.errstate(all="ignore"):
                want = TO.expected_depth_frames(sim3dr_oracle, shapes, sc["verts"], sc["t"], sc["image_index"], side)
            assert (TO.BAKE_FLAG_DEPTH_WINDOW in want[2].tolist()) == (side < largest), what
            assert_depth(depth_maps(m, shapes, sc["verts"], sc["image_index"], side), want, what)


def test_depth_frames_visit_every_pixel_of_every_box_width(sim3dr_oracle):
    """The frames of `whole_box_frames` through `depth_raster_kernel`: every box width 1..64 at heights 1, 63, 64, and boxes 65..128 wide
    (one box per triangle here, not per tile). `depth_side` 64 flags every head of the 64 frames wider than 64 (73 heads); 128 holds
    all. No cell of a drawn window is left +inf."""
    wb = RC.whole_box_frames()
    m = UVMap(wb["t"], 3, RC.tiny_atlas(wb["t"]), device=0)
    for side in (64, 128):
        want = TO.expected_depth_frames(sim3dr_oracle, wb["shapes"], wb["verts"], wb["t"], wb["image_index"], side)
        wide = [wb["shapes"][f][1] > side for f in wb["image_index"]]
        assert want[2].tolist() == [TO.BAKE_FLAG_DEPTH_WINDOW if x else 0 for x in wide] and any(wide) == (side == 64)
        got = depth_maps(m, wb["shapes"], wb["verts"], wb["image_index"], side)
        assert_depth(got, want, f"depth_side {side}")
        for k, wm in enumerate(want[0]):
            if wm is not None:
                assert np.isfinite(got[0][k, :wm.shape[0], :wm.shape[1]]).all(), (side, k)


# ---- 5. directed pairs ------------------------------------------------------------------------------------------------------------
def test_directed_pairs_in_the_depth_maps(sim3dr_oracle):
    """Two overlapping flat triangles a head, in both triangle orders, with boxes of 16 pixels (a lane's walk) and of 144 (the wave's):
    z = -1 against +1 (the signed minimum meets the unsigned maximum in either arrival order), -0.0 against +0.0 (+0 is stored), -3
    against -2, exactly 1e8f against the float below it (the `z < 1e8f` test; the products round, so the plane at 1e8f is covered in part),
    and a zero-area triangle over covered pixels, in front and behind (inv = 0: u = v = 0 counts as inside, it covers its box).
    test_raster_cases_host.py checks on the reference that each pair shows both depths and that the order of the triangles does not matter."""
    pairs = RC.directed_pairs(RC.DEPTH_PAIRS)
    verts = np.stack([v for _, v, _ in pairs])
    m = UVMap(RC.PAIR_TRIANGLES, 6, RC.tiny_atlas(RC.PAIR_TRIANGLES), device=0)
    index = [0] * len(pairs)
    want = TO.expected_depth_frames(sim3dr_oracle, [RC.PAIR_FRAME], verts, RC.PAIR_TRIANGLES, index, 32)
    assert not want[2].any()
    got = depth_maps(m, [RC.PAIR_FRAME], verts, index, 32)
    assert_depth(got, want, "directed pairs: " + ", ".join(name for name, _, _ in pairs))


def test_directed_pairs_in_the_frames(sim3dr_oracle):
    """The same pairs through `rasterize_frames`, one frame a pair, a flat colour a triangle so that the winner shows: -1 against +1 and -3
    against -2 (`depth_order_number` of negative depths), -0.0 against +0.0 (a tie: the lowest triangle wins, so swapping the triangles
    swaps the colour, as test_raster_cases_host.py checks on the reference), -1e8f against the float above it (the `z > -1e8f` test) and
    a zero-area triangle (never drawn: the strict test)."""
    pairs = RC.directed_pairs(RC.FRAME_PAIRS)
    verts, cols = np.stack([v for _, v, _ in pairs]), np.stack([c for _, _, c in pairs])
    h, w = RC.PAIR_FRAME
    bgs = [np.full((h, w, 3), 255, np.uint8) for _ in pairs]
    index = list(range(len(pairs)))
    want = RF.expected_frames(sim3dr_oracle, bgs, verts, RC.PAIR_TRIANGLES, cols, index)
    dev = [cuda(b) for b in bgs]
    mesh = Mesh(RC.PAIR_TRIANGLES, 6, device=0)
    flags = mesh.rasterize_frames(dev, cuda(verts), cuda(cols), index)
    torch.cuda.synchronize()
    assert flags.cpu().tolist() == [0] * len(pairs)
    got = [d.cpu().numpy() for d in dev]
    for (name, _, _), g, f in zip(pairs, got, want):
        assert np.array_equal(g, f), f"{name}: pixels {np.argwhere((g != f).any(-1))[:4].tolist()} differ"
