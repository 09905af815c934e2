"""GPU: several heads into their frames in one chain (csrc/sim3dr_frames.hip; `Mesh.rasterize_frames`, `Mesh.render_frames`,
`PNCCEstimator.render_frames`, `overlay.draw_heads`) against tests/render_frames_restatement.py: per frame, per head in ascending
head index, one call of the reference's `rasterize(.., bg=frame)`. Frames are compared with np.array_equal unless a test says why not.
Frames are at most 256 pixels a side and heads 40 to 120 pixels, so every triangle box is far below one tile and the list pool of
4 * ntri * N entries holds every case but the one built to overrun it."""
import ctypes as C

import numpy as np
import pytest
import torch

import render_frames_restatement as RF
from dad_3dheads_amd import _lib, synthetic
from dad_3dheads_amd.head_mesh import HeadMesh
from dad_3dheads_amd.Sim3DR import Mesh
from dad_3dheads_amd.Sim3DR.frames import DeviceFrames

pytestmark = pytest.mark.gpu
INDEX, CAPACITY = _lib.FRAME_FLAG_INDEX, _lib.FRAME_FLAG_CAPACITY


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def faces(static):
    return np.ascontiguousarray(static["faces"], dtype=np.int32)


@pytest.fixture(scope="module")
def head_mesh(flame_model, static):
    return HeadMesh(flame_model=flame_model, static=static, device=0)


@pytest.fixture(scope="module")
def heads(head_mesh):
    """Decoded vertices of the seeded synthetic model, [8,nver,3] float32 as `PNCCEstimator.render_batch` decodes them."""
    params = torch.from_numpy(synthetic.synthetic_params(8, seed=31)).cuda()
    return head_mesh.flame.decode(params, proj=True, to_2d=False, flip_z=True)["proj"].cpu().numpy()


@pytest.fixture(scope="module")
def mesh(faces, heads):
    return Mesh(faces, heads.shape[1], device=0)


@pytest.fixture(scope="module")
def colors(heads):
    return np.random.default_rng(5).random(heads.shape, dtype=np.float32)


def place(v, cx, cy, size, dz=0.0):
    """The head scaled so that the longer side of its x-y box is `size` pixels, centred at (cx, cy); z scaled alike, then moved by dz."""
    lo, hi = v[:, :2].min(0), v[:, :2].max(0)
    s = np.float32(size / (hi - lo).max())
    out = (v - np.float32([*(lo + hi) / 2, 0.0])) * s + np.float32([cx, cy, dz])
    return out.astype(np.float32)


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def draw(mesh, frames, verts, cols, index, reverse=False):
    """frames: numpy arrays or CUDA tensors (drawn in place) -> (frames as numpy, flags as numpy)."""
    dev = [f if isinstance(f, torch.Tensor) else cuda(f) for f in frames]
    flags = mesh.rasterize_frames(dev, cuda(np.stack(verts)), cuda(np.stack(cols)), index, reverse=reverse)
    torch.cuda.synchronize()
    return [f.cpu().numpy() for f in dev], flags.cpu().numpy()


def assert_frames(got, want, what=""):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), f"{what} frame {i}: {int((g != w).any(-1).sum())} of {g.shape[0] * g.shape[1]} pixels differ"


# ---- raster ---------------------------------------------------------------------------------------------------------------------
def test_mixed_sizes_a_strided_view_and_an_odd_address(mesh, faces, heads, colors, sim3dr_oracle):
    shapes = [(96, 160), (130, 70), (64, 64)]  # neither side of the second is a multiple of 64, and it is barely wider than a tile
    bgs = [noise((h, w, 3), 10 + i) for i, (h, w) in enumerate(shapes)]
    wide = cuda(noise((130, 80, 3), 20))
    pattern = wide.clone()
    wide[:, 5:75] = cuda(bgs[1])
    view = wide[:, 5:75]
    assert view.stride(0) == 240 and view.data_ptr() % 2 == 1
    dev = [cuda(bgs[0]), view, cuda(bgs[2])]
    index = [0, 1, 2, 1, 0]
    verts = [place(heads[0], 60, 50, 80), place(heads[1], 36, 60, 64), place(heads[2], 30, 34, 50), place(heads[3], 40, 100, 40),
             place(heads[4], 120, 60, 70)]
    got, flags = draw(mesh, dev, verts, colors[:5], index)
    assert flags.tolist() == [0] * 5
    want = RF.expected_frames(sim3dr_oracle, bgs, verts, faces, colors[:5], index)
    assert_frames(got, want)
    assert all(not np.array_equal(w, b) for w, b in zip(want, bgs))  # every frame was drawn into
    outside = torch.ones(80, dtype=torch.bool)
    outside[5:75] = False
    assert torch.equal(wide[:, outside.cuda()], pattern[:, outside.cuda()])  # no byte outside [row, row + 3 w)


def test_a_later_head_wins_across_a_tile_boundary_also_from_behind(mesh, faces, heads, colors, sim3dr_oracle):
    bg = noise((128, 128, 3), 30)
    first, second = place(heads[0], 56, 64, 90), place(heads[1], 76, 60, 90, dz=-200.0)  # the second lies behind the first
    assert second[:, 2].max() < first[:, 2].min()
    cover_second = RF.coverage(sim3dr_oracle, (128, 128), [second], faces, [0], 0)
    cover_first = RF.coverage(sim3dr_oracle, (128, 128), [first], faces, [0], 0)
    both = cover_first & cover_second
    assert both[:, :64].any() and both[:, 64:].any() and both[:64].any() and both[64:].any()  # the overlap spans the tile seams
    results = []
    for order in ((0, 1), (1, 0)):
        verts, cols = [[first, second][k] for k in order], [colors[k] for k in order]
        got, flags = draw(mesh, [bg], verts, cols, [0, 0])
        assert flags.tolist() == [0, 0]
        assert_frames(got, RF.expected_frames(sim3dr_oracle, [bg], verts, faces, cols, [0, 0]), str(order))
        solo = RF.expected_frames(sim3dr_oracle, [bg], verts[1:], faces, cols[1:], [0])[0]
        later = cover_second if order == (0, 1) else cover_first
        assert np.array_equal(got[0][later], solo[later])  # where the later head covers, the pixel is the later head's
        results.append(got[0])
    assert not np.array_equal(results[0][both], results[1][both])


def test_an_unsorted_index_keeps_the_order_of_the_heads_of_each_frame(mesh, faces, heads, colors, sim3dr_oracle):
    bgs = [noise((100, 120, 3), 40), noise((120, 100, 3), 41)]
    index = [1, 0, 1, 0]
    verts = [place(heads[0], 40, 50, 70), place(heads[1], 50, 50, 80), place(heads[2], 60, 70, 70), place(heads[3], 75, 45, 60)]
    got, flags = draw(mesh, bgs, verts, colors[:4], index)
    assert flags.tolist() == [0] * 4
    assert_frames(got, RF.expected_frames(sim3dr_oracle, bgs, verts, faces, colors[:4], index))
    swapped = RF.expected_frames(sim3dr_oracle, bgs, verts[::-1], faces, colors[:4][::-1], index[::-1])
    assert not np.array_equal(swapped[0], got[0])  # the order matters in this scene


def test_untouched_and_clipped_frames(mesh, faces, heads, colors, sim3dr_oracle):
    bgs = [noise((90, 110, 3), 50), noise((70, 70, 3), 51), noise((130, 66, 3), 52)]
    index = [0, 2, 0]
    verts = [place(heads[0], -400, 40, 100),  # wholly outside its frame
             place(heads[1], 0, 128, 110),    # half outside, over two edges
             place(heads[2], 108, 88, 60)]    # over the far corner
    got, flags = draw(mesh, bgs, verts, colors[:3], index)
    assert flags.tolist() == [0, 0, 0]
    want = RF.expected_frames(sim3dr_oracle, bgs, verts, faces, colors[:3], index)
    assert_frames(got, want)
    assert np.array_equal(got[1], bgs[1])  # a frame without heads keeps its bytes
    only_outside, _ = draw(mesh, [bgs[0]], verts[:1], colors[:1], [0])
    assert np.array_equal(only_outside[0], bgs[0])
    assert not np.array_equal(want[2], bgs[2]) and not np.array_equal(want[0], bgs[0])


def test_an_index_without_a_frame_is_flagged_and_draws_nothing(mesh, faces, heads, colors, sim3dr_oracle):
    bgs = [noise((96, 96, 3), 60), noise((80, 100, 3), 61)]
    index = [-1, 0, 2, 1, 2**31 - 1, -2**31]
    verts = [place(heads[k], 48, 48, 60 + 5 * k) for k in range(6)]
    d_index = cuda(np.asarray(index, np.int32))  # a CUDA tensor: used as it is, read back only below
    got, flags = draw(mesh, bgs, verts, colors[:6], d_index)
    assert flags.tolist() == [INDEX, 0, INDEX, 0, INDEX, INDEX]
    assert_frames(got, RF.expected_frames(sim3dr_oracle, bgs, verts, faces, colors[:6], index))
    assert_frames(got, RF.expected_frames(sim3dr_oracle, bgs, [verts[1], verts[3]], faces, [colors[1], colors[3]], [0, 1]))
    assert d_index.cpu().tolist() == index


# ---- the list pool --------------------------------------------------------------------------------------------------------------
def _eight_triangles(kind, seed=0):
    """24 vertices for the mesh of eight separate triangles: "cover" -- each covers a whole 256 x 256 frame (16 tiles), at its own
    depth; "small" -- eight triangles of about 20 pixels inside one tile."""
    rng = np.random.default_rng(seed)
    v = np.zeros((24, 3), np.float32)
    for t in range(8):
        if kind == "cover":
            v[3 * t: 3 * t + 3] = [[-300.5, -300.5, t], [900.5, -300.5, t], [-300.5, 900.5, t]]
        else:
            x, y = rng.uniform(70, 100, 2)
            v[3 * t: 3 * t + 3] = [[x, y, t], [x + 20.25, y + 3.5, t + 1], [x + 2.5, y + 19.75, t - 1]]
    return v


def test_a_head_that_overruns_the_pool_is_dropped_whole(sim3dr_oracle):
    tri = np.arange(24, dtype=np.int32).reshape(8, 3)
    mesh8 = Mesh(tri, 24, device=0)
    bg = noise((256, 256, 3), 70)
    cols = np.random.default_rng(71).random((4, 24, 3), dtype=np.float32)
    # 8 triangles x 16 tiles = 128 entries against a pool of 4 * 8 * 1 = 32
    got, flags = draw(mesh8, [bg], [_eight_triangles("cover")], cols[:1], [0])
    assert flags.tolist() == [CAPACITY] and np.array_equal(got[0], bg)
    # with three small heads the pool is 4 * 8 * 4 = 128: the small heads take theirs first, the large one no longer fits ...
    small = [_eight_triangles("small", s) for s in (1, 2, 3)]
    for verts, what in (([small[0], _eight_triangles("cover"), small[1], small[2]], "large second"),
                        ([_eight_triangles("cover")] + small, "large first")):  # ... or it takes all 128 and the others are dropped
        got, flags = draw(mesh8, [bg], verts, cols, [0, 0, 0, 0])
        assert set(flags.tolist()) == {0, CAPACITY}, what
        dropped = {k for k, f in enumerate(flags.tolist()) if f}
        # no head is ever drawn in part: the frame is the restatement's without the flagged heads
        assert_frames(got, RF.expected_frames(sim3dr_oracle, [bg], verts, tri, cols, [0, 0, 0, 0], skip=dropped), what)
        assert not np.array_equal(got[0], bg), what
    # the pool rule as documented: ascending order, a head that no longer fits is dropped whole
    _, flags = draw(mesh8, [bg], [small[0], _eight_triangles("cover"), small[1], small[2]], cols, [0, 0, 0, 0])
    assert flags.tolist() == [0, CAPACITY, 0, 0]
    _, flags = draw(mesh8, [bg], [_eight_triangles("cover")] + small, cols, [0, 0, 0, 0])
    assert flags.tolist() == [0, CAPACITY, CAPACITY, CAPACITY]


# ---- odd inputs -----------------------------------------------------------------------------------------------------------------
def test_one_nan_vertex_spoils_its_own_triangles_only(mesh, faces, heads, colors, sim3dr_oracle):
    bg = noise((110, 140, 3), 80)
    verts = [place(heads[0], 50, 55, 80), place(heads[1], 90, 55, 80)]
    hit = int(faces[len(faces) // 2, 0])
    verts[0][hit] = np.nan
    got, flags = draw(mesh, [bg], verts, colors[:2], [0, 0])
    assert flags.tolist() == [0, 0]
    assert_frames(got, RF.expected_frames(sim3dr_oracle, [bg], verts, faces, colors[:2], [0, 0]))
    # the other head is unaffected: alone in a frame of its own it gives the same bytes with the NaN head there or not
    two, _ = draw(mesh, [bg, bg], verts, colors[:2], [0, 1])
    alone, _ = draw(mesh, [bg], verts[1:], colors[1:2], [0])
    assert np.array_equal(two[1], alone[0])


def test_one_head_per_frame_equals_the_batched_rasterize(mesh, heads, colors):
    bg = cuda(noise((3, 128, 136, 3), 90))
    verts = cuda(np.stack([place(heads[k], 60 + 5 * k, 64, 90) for k in range(3)]))
    want = mesh.rasterize(verts, cuda(colors[:3]), bg.clone())
    got = bg.clone()
    flags = mesh.rasterize_frames(got, verts, cuda(colors[:3]), [0, 1, 2])
    assert torch.equal(got, want) and flags.tolist() == [0, 0, 0]
    assert not torch.equal(got, bg)


def test_reverse_writes_the_mirrored_rows(mesh, faces, heads, colors, sim3dr_oracle):
    bgs = [noise((90, 100, 3), 100), noise((129, 65, 3), 101)]
    index = [1, 0, 1]
    verts = [place(heads[0], 30, 40, 60), place(heads[1], 50, 30, 70), place(heads[2], 40, 100, 50)]
    got, flags = draw(mesh, bgs, verts, colors[:3], index, reverse=True)
    assert flags.tolist() == [0, 0, 0]
    want = RF.expected_frames(sim3dr_oracle, bgs, verts, faces, colors[:3], index, reverse=True)
    assert_frames(got, want)
    assert not np.array_equal(want[1], RF.expected_frames(sim3dr_oracle, bgs, verts, faces, colors[:3], index)[1])


# ---- the light ------------------------------------------------------------------------------------------------------------------
def _lit(mesh, frames, verts, index, **kw):
    dev = [cuda(f) for f in frames]
    light = torch.empty((len(verts), mesh.nver, 3), dtype=torch.float32, device="cuda")
    flags = mesh.render_frames(dev, cuda(np.stack(verts)), index, light_out=light, **kw)
    torch.cuda.synchronize()
    return [f.cpu().numpy() for f in dev], light, flags.cpu().numpy()


@pytest.mark.parametrize("specular_exp", [1, 2])
def test_render_frames_equals_the_numpy_light_where_pow_is_exact(mesh, faces, heads, sim3dr_oracle, specular_exp):
    """np.power is a product for the exponents 1 and 2 (tests/render_checks.py): light and bytes are the restatement's."""
    bgs = [noise((100, 130, 3), 110), noise((70, 90, 3), 111)]
    index = [0, 1, 0]
    verts = [place(heads[0], 45, 50, 80), place(heads[1], 45, 35, 60), place(heads[2], 85, 55, 80, dz=-300.0)]
    got, light, flags = _lit(mesh, bgs, verts, index, specular_exp=specular_exp)
    want, want_light = RF.expected_lit_frames(sim3dr_oracle, bgs, verts, faces, index, specular_exp=specular_exp)
    assert flags.tolist() == [0, 0, 0]
    assert np.array_equal(light.cpu().numpy(), want_light)
    assert_frames(got, want)


def test_render_frames_with_the_default_light(mesh, faces, heads, sim3dr_oracle):
    """The default exponent goes through the host's pow in numpy: as tests/render_checks.py states, coverage is identical and every
    byte within 1. On black frames the ambient term alone makes every drawn byte at least 75, so coverage shows in the bytes."""
    shapes = [(100, 130), (70, 90)]
    bgs = [np.zeros((h, w, 3), np.uint8) for h, w in shapes]
    index = [0, 1, 0]
    verts = [place(heads[0], 45, 50, 80), place(heads[1], 45, 35, 60), place(heads[2], 85, 55, 80, dz=-300.0)]
    got, light, flags = _lit(mesh, bgs, verts, index)
    want, _ = RF.expected_lit_frames(sim3dr_oracle, bgs, verts, faces, index)
    assert flags.tolist() == [0, 0, 0]
    for f, (g, w) in enumerate(zip(got, want)):
        cover = RF.coverage(sim3dr_oracle, shapes[f], verts, faces, index, f)
        assert cover.any() and w[cover].min() >= 75
        assert np.array_equal(g.any(2), cover) and np.array_equal(w.any(2), cover)
        assert np.abs(g.astype(int) - w.astype(int)).max() <= 1
    v = cuda(np.stack(verts))
    assert torch.equal(light, mesh.phong_light(v, None))  # bit for bit
    # and the bytes are those of the raster on that light, the route Mesh.render documents
    again = [cuda(b) for b in bgs]
    mesh.rasterize_frames(again, v, light, index)
    assert_frames([a.cpu().numpy() for a in again], got)
    rev, _, _ = _lit(mesh, bgs, verts, index, reverse=True)
    want_rev = RF.expected_frames(sim3dr_oracle, bgs, verts, faces, light.cpu().numpy(), index, reverse=True)
    assert_frames(rev, want_rev, "reverse")


# ---- graphs and scratch ---------------------------------------------------------------------------------------------------------
def test_graph_replay_and_no_allocation_once_the_scratch_is_large_enough(faces, heads, colors):
    mesh = Mesh(faces, heads.shape[1], device=0)  # a handle of its own: its scratch starts at 0
    assert mesh.frames_scratch_bytes() == 0
    bgs = [cuda(noise((100, 130, 3), 120)), cuda(noise((140, 90, 3), 121)), cuda(noise((64, 64, 3), 122))]
    work = [b.clone() for b in bgs]
    frames = DeviceFrames(work, torch.device("cuda", 0))  # the table is uploaded once, outside the capture
    verts = cuda(np.stack([place(heads[k], 40 + 10 * k, 50, 60 + 5 * k) for k in range(4)]))
    cols, index = cuda(colors[:4]), cuda(np.asarray([0, 1, 1, 2], np.int32))
    flags = mesh.rasterize_frames(frames, verts, cols, index)  # warm-up: allocates (and synchronises)
    torch.cuda.synchronize()
    eager = [w.clone() for w in work]
    assert flags.tolist() == [0] * 4 and not torch.equal(eager[1], bgs[1])
    held = mesh.frames_scratch_bytes()
    assert held > 0
    for w, b in zip(work, bgs):
        w.copy_(b)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mesh.rasterize_frames(frames, verts, cols, index)
    for w, b in zip(work, bgs):
        w.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    for w, e in zip(work, eager):
        assert torch.equal(w, e)
    assert mesh.frames_scratch_bytes() == held
    # fewer heads and frames: the scratch is large enough, nothing is allocated
    small = [bgs[1].clone()]
    mesh.rasterize_frames(small, verts[1:3], cols[1:3], [0, 0])
    torch.cuda.synchronize()
    assert mesh.frames_scratch_bytes() == held and torch.equal(small[0], eager[1])


# ---- the predictor's dicts ------------------------------------------------------------------------------------------------------
def test_pncc_and_shaded_heads_of_predict_boxes(flame_model, sim3dr_oracle, static, monkeypatch):
    from dad_3dheads_amd import overlay
    from dad_3dheads_amd.pncc import PNCCEstimator
    from dad_3dheads_amd.predictor import FaceMeshPredictor

    pred = FaceMeshPredictor.random_init(cuda_id=0, flame_model=flame_model)
    fr = [noise((150, 200, 3), 130), noise((180, 140, 3), 131)]
    boxes = [np.array([[10, 20, 90, 100], [90, 30, 100, 110]]), np.array([[20, 40, 100, 120]])]
    res = pred.predict_boxes(fr, boxes)
    assert [r["image_index"] for r in res] == [0, 0, 1]
    frames = [cuda(f) for f in fr]
    params = torch.cat([r["3dmm_params"] for r in res]).cuda()
    verts = pred.head_mesh.flame.decode(params.clone(), proj=True, to_2d=False, flip_z=True)["proj"].cpu().numpy()
    est = PNCCEstimator(head_mesh=pred.head_mesh, static=static)
    faces_pncc = np.ascontiguousarray(est.faces_wo_back_remapped, dtype=np.int32)
    pncc_cols = np.broadcast_to(est.colors.astype(np.float32), verts.shape)
    want_pncc = RF.expected_frames(sim3dr_oracle, fr, verts, faces_pncc, pncc_cols, [0, 0, 1])

    direct = [f.clone() for f in frames]
    flags = est.render_frames(params.clone(), direct, [0, 0, 1])
    assert flags.tolist() == [0, 0, 0]
    assert_frames([d.cpu().numpy() for d in direct], want_pncc, "PNCCEstimator.render_frames")

    got = overlay.draw_heads(res, frames, mode="pncc", head_mesh=pred.head_mesh)
    assert isinstance(got, list) and all(g is not f for g, f in zip(got, frames))
    assert_frames([g.cpu().numpy() for g in got], want_pncc, "draw_heads pncc")
    assert all(torch.equal(f, cuda(b)) for f, b in zip(frames, fr))  # the inputs stay as they were

    faces_all = np.ascontiguousarray(static["faces"], dtype=np.int32)
    shaded = overlay.draw_heads(res, frames, mode="shaded", head_mesh=pred.head_mesh)
    light = Mesh(faces_all, verts.shape[1], device=0).phong_light(cuda(verts), None).cpu().numpy()
    want_shaded = RF.expected_frames(sim3dr_oracle, fr, verts, faces_all, light, [0, 0, 1])
    assert_frames([s.cpu().numpy() for s in shaded], want_shaded, "draw_heads shaded")

    # device dicts: no device-to-host copy and no wait, the way test_gpu_predict_boxes.py checks predict_boxes
    dev_res = pred.predict_boxes(frames, cuda(np.concatenate(boxes).astype(np.float64)), cuda(np.asarray([0, 0, 1], np.int32)),
                                 device_outputs=True, points_on_device=True)
    assert all(r["image_index"].is_cuda and r["3dmm_params"].is_cuda for r in dev_res)
    out = [f.clone() for f in frames]
    overlay.draw_heads(dev_res, frames, mode="pncc", head_mesh=pred.head_mesh)  # renderers built, scratch allocated
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError("a host wait")

    with monkeypatch.context() as m:
        for name in ("cpu", "item", "tolist", "numpy"):
            m.setattr(torch.Tensor, name, refuse)
        m.setattr(torch.cuda, "synchronize", refuse)
        back = overlay.draw_heads(dev_res, frames, mode="pncc", out=out, head_mesh=pred.head_mesh)
        lit = overlay.draw_heads(dev_res, frames, mode="shaded", head_mesh=pred.head_mesh)
    assert back is out
    dev_params = torch.cat([r["3dmm_params"] for r in dev_res])
    dev_verts = pred.head_mesh.flame.decode(dev_params.clone(), proj=True, to_2d=False, flip_z=True)["proj"].cpu().numpy()
    assert_frames([o.cpu().numpy() for o in out],
                  RF.expected_frames(sim3dr_oracle, fr, dev_verts, faces_pncc, np.broadcast_to(est.colors.astype(np.float32), dev_verts.shape),
                                     [0, 0, 1]), "device dicts")
    assert len(lit) == 2 and all(t.is_cuda for t in lit)
    # a batch comes back as a batch
    batch = torch.stack([frames[0], frames[0]])
    both = overlay.draw_heads(res[:2], batch, mode="pncc", image_index=[1, 1], head_mesh=pred.head_mesh)
    assert both.shape == batch.shape and torch.equal(both[0], batch[0]) and torch.equal(both[1], got[0])


# ---- the C entry's argument contract --------------------------------------------------------------------------------------------
def test_refusals_before_device_work(mesh, heads, colors):
    lib = _lib.load()
    poison = cuda(noise((64, 64, 3), 140))
    before = poison.clone()
    frames = DeviceFrames([poison], torch.device("cuda", 0))
    v, col = cuda(place(heads[0], 32, 32, 50)[None]), cuda(colors[:1])
    index, flags = cuda(np.zeros(1, np.int32)), torch.full((1,), -7, dtype=torch.int32, device="cuda")
    cfg = _lib.LightC(0.3, 0.6, 0.1, 5.0, (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(0, 0, 5), (C.c_float * 3)(0, 0, 5))
    good = dict(m=mesh._handle, frames=frames.device.data_ptr(), host=frames.host.ctypes.data, n_frames=1, v=v.data_ptr(), col=col.data_ptr(),
                index=index.data_ptr(), n_heads=1, flags=flags.data_ptr())

    def raster(**kw):
        a = {**good, **kw}
        return lib.dad3d_mesh_rasterize_frames(a["m"], a["frames"], a["host"], a["n_frames"], a["v"], a["col"], a["index"], a["n_heads"], 0,
                                               a["flags"], None)

    def render(render_flags=0, cfg_ptr=C.byref(cfg), **kw):
        a = {**good, **kw}
        return lib.dad3d_mesh_render_frames(a["m"], a["frames"], a["host"], a["n_frames"], a["v"], a["col"], a["index"], a["n_heads"], cfg_ptr,
                                            render_flags, a["flags"], None)

    big_host = np.array([[poison.data_ptr(), 64 * 64 + 1, 64 * 65, 3 * 64 * 65]], np.int64)  # 65 x 65 tiles
    thin_host = np.array([[poison.data_ptr(), 64, 64, 191]], np.int64)                       # rows that overlap
    for call in (raster, render):
        for kw in (dict(m=None), dict(frames=None), dict(host=None), dict(v=None), dict(col=None), dict(index=None), dict(flags=None),
                   dict(n_frames=-1), dict(n_heads=-1), dict(n_frames=65536), dict(n_heads=65536), dict(host=big_host.ctypes.data),
                   dict(host=thin_host.ctypes.data)):
            assert call(**kw) == _lib.E_INVALID, (call.__name__, kw)
            assert lib.dad3d_last_error() != b""
        assert call(n_frames=0) == _lib.OK and call(n_heads=0) == _lib.OK  # nothing to do
        assert call(n_heads=0, v=None, col=None, index=None, flags=None) == _lib.OK
    assert render(render_flags=_lib.RENDER_CLEAR) == _lib.E_INVALID and b"DAD3D_RENDER_CLEAR" in lib.dad3d_last_error()
    assert render(render_flags=_lib.RENDER_CLEAR | _lib.RENDER_REVERSE) == _lib.E_INVALID
    assert render(cfg_ptr=None) == _lib.E_INVALID
    torch.cuda.synchronize()
    assert torch.equal(poison, before) and flags.tolist() == [-7]  # nothing was launched
    assert raster() == _lib.OK  # and the same arguments, unspoilt, draw
    torch.cuda.synchronize()
    assert flags.tolist() == [0] and not torch.equal(poison, before)
    # through Python a call without frames flags every head, and one without heads returns no flags
    assert mesh.rasterize_frames([], v, col, [0]).tolist() == [INDEX]
    assert mesh.rasterize_frames([poison], v[:0], col[:0], []).tolist() == []
