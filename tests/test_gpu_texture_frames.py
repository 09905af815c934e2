"""GPU: textured heads through the frames chain (csrc/sim3dr_frames_texture.hip; `Mesh.render_texture_frames`,
`UVTextureCreator.render_frames`, `overlay.draw_heads(mode="textured")`). Per frame, in ascending head order,
`frame = (unsigned char) _render_texture_core(image=float(frame), vertices[k], .., texture[k], a fresh depth buffer)`.

What the frames are compared with, always with np.array_equal:
  * the golden tests/golden/texture_frames_golden.npz, recorded from the compiled reference: never skipped;
  * in every other case, `tests/texture_frames_restatement.expected_textured_frames` -- the compiled reference itself, called per head on
    the running frame -- where oracle/_ref holds it, AND the same loop over the project's batched `Mesh.render_texture` on a
    `[1,H,W,3]` view of the frame (itself held to the reference's golden by test_gpu_render_texture.py), which needs nothing but
    the GPU. Each case asserts on those expected arrays that it exercises what it claims."""
import numpy as np
import pytest
import torch

import render_texture_ref as RT
import texture_frames_restatement as TF
from dad_3dheads_amd import _lib, overlay, synthetic
from dad_3dheads_amd.Sim3DR import Mesh
from dad_3dheads_amd.Sim3DR.frames import DeviceFrames
from dad_3dheads_amd.uv_texture import TextureAccumulator, UVTextureCreator, texel_coords

pytestmark = pytest.mark.gpu
INDEX, CAPACITY = _lib.FRAME_FLAG_INDEX, _lib.FRAME_FLAG_CAPACITY
MAPPING = {0: "nearest", 1: "bilinear"}
S = 64


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def yaw(v, degrees):
    c = 0.5 * (v.min(0) + v.max(0)).astype(np.float64)
    a = np.deg2rad(degrees)
    r = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    return ((v.astype(np.float64) - c) @ r.T + c).astype(np.float32)


@pytest.fixture(scope="module")
def golden():
    with np.load(RT.GOLDEN.replace("render_texture_golden", "texture_frames_golden")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def faces(static):
    return np.ascontiguousarray(static["faces"], dtype=np.int32)


@pytest.fixture(scope="module")
def tc(static):
    return RT.head_texcoords(static, S)  # [V,3]: one texel coordinate per vertex


@pytest.fixture(scope="module")
def mesh(faces, tc):
    return Mesh(faces, len(tc), device=0).set_texcoords(tc, faces)


@pytest.fixture(scope="module")
def textures():
    return np.stack([RT.smooth_texture(S, S, 3, seed=40 + k).astype(np.uint8) for k in range(6)])


def draw(mesh, frames, verts, tex, index, mapping=1, indexing="corner"):
    """frames: numpy arrays or CUDA tensors (drawn in place) -> (frames as numpy, flags as numpy)."""
    dev = [f if isinstance(f, torch.Tensor) else cuda(f) for f in frames]
    flags = mesh.render_texture_frames(dev, cuda(np.stack(verts)), tex if isinstance(tex, torch.Tensor) else cuda(tex), index,
                                       mapping=MAPPING[mapping], indexing=indexing)
    torch.cuda.synchronize()
    return [f.cpu().numpy() for f in dev], flags.cpu().numpy()


def batched_route(mesh, frames, verts, tex, index, mapping=1, indexing="corner", skip=()):
    """The route that exists without the chain: one `Mesh.render_texture` call per head, in order, on a [1,H,W,3] view of its frame."""
    out = [cuda(f) for f in frames]
    tex = tex if isinstance(tex, torch.Tensor) else cuda(tex)
    for k, f in enumerate(np.asarray(index).reshape(-1).tolist()):
        if k in skip or not 0 <= f < len(out):
            continue
        mesh.render_texture(cuda(verts[k][None]), tex[k] if tex.ndim == 4 else tex, out[f][None], mapping=MAPPING[mapping], indexing=indexing)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def assert_frames(got, want, what=""):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), f"{what} frame {i}: {int((g != w).any(-1).sum())} of {g.shape[0] * g.shape[1]} pixels differ"


def expected(mesh, frames, verts, faces, tex, tc, tt, index, mapping=1, indexing="corner", skip=()):
    """The expected frames: the batched route, and the compiled reference where it is there (the two must agree)."""
    want = batched_route(mesh, frames, verts, tex, index, mapping, indexing, skip)
    if RT.ref_available():
        tex_np = tex.cpu().numpy() if isinstance(tex, torch.Tensor) else tex
        ref = TF.expected_textured_frames(frames, verts, faces, tex_np, tc if indexing == "reference" else tc[:, :2], tt, index, mapping,
                                          indexing=indexing, skip=skip)
        assert_frames(want, ref, "batched route against the compiled reference:")
    return want


def drawn(want, bg):
    return (want != bg).any(-1)


# ---- the golden: never skipped ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("indexing", ["corner", "reference"])
def test_golden_frames_bit_equal(golden, faces, indexing):
    m = Mesh(faces, len(golden["tex_coords"]), device=0).set_texcoords(golden["tex_coords"], faces)
    for mapping in (0, 1):
        got, flags = draw(m, [golden["frame0"], golden["frame1"]], golden["vertices"], golden["textures"], golden["image_index"], mapping, indexing)
        assert flags.tolist() == [0, 0, 0]
        assert_frames(got, [golden[f"frame0_mapping{mapping}"], golden[f"frame1_mapping{mapping}"]], f"{indexing} {MAPPING[mapping]}")
    band = drawn(golden["frame1_mapping1"], golden["frame1"]) & RT.band_mask(70, 130)
    assert band.sum() > 0  # the head over the left edge pins the border-band rule


# ---- layouts ----------------------------------------------------------------------------------------------------------------------
def test_mixed_sizes_a_strided_view_and_an_odd_address(mesh, static, faces, tc, textures):
    shapes = [(96, 160), (130, 70), (64, 64)]
    bgs = [noise((h, w, 3), 10 + i) for i, (h, w) in enumerate(shapes)]
    wide = cuda(noise((130, 80, 3), 20))
    pattern = wide.clone()
    wide[:, 5:75] = cuda(bgs[1])
    view = wide[:, 5:75]
    assert view.stride(0) == 240 and view.data_ptr() % 2 == 1
    index = [0, 1, 2, 1, 0]
    verts = [RT.head_vertices(static, 96, 160, shift_x=-30.0), RT.head_vertices(static, 130, 70), RT.head_vertices(static, 64, 64),
             yaw(RT.head_vertices(static, 130, 70, shift_x=10.0), 20), RT.head_vertices(static, 96, 160, shift_x=40.0)]
    want = expected(mesh, bgs, verts, faces, textures[:5], tc, faces, index)
    assert all(0.05 < drawn(w, b).mean() < 0.95 for w, b in zip(want, bgs))  # every frame is drawn into and keeps pixels
    got, flags = draw(mesh, [cuda(bgs[0]), view, cuda(bgs[2])], verts, textures[:5], index)
    assert flags.tolist() == [0] * 5
    assert_frames(got, want)
    outside = torch.ones(80, dtype=torch.bool)
    outside[5:75] = False
    assert torch.equal(wide[:, outside.cuda()], pattern[:, outside.cuda()])  # no byte outside [row, row + 3 w)


def test_a_head_across_the_tile_boundary(mesh, static, faces, tc, textures):
    bg = noise((130, 70, 3), 30)
    v = RT.head_vertices(static, 130, 70, fill=1.9)  # taller than the frame: it reaches all six tiles
    want = expected(mesh, [bg], [v], faces, textures[:1], tc, faces, [0])
    d = drawn(want[0], bg)
    assert d[:64, :64].any() and d[:64, 64:].any() and d[64:128, :64].any() and d[64:128, 64:].any() and d[128:].any()  # six tiles
    got, flags = draw(mesh, [bg], [v], textures[:1], [0])
    assert flags.tolist() == [0]
    assert_frames(got, want)


def test_a_later_head_wins_also_from_behind_and_an_unsorted_index_keeps_the_order(mesh, static, faces, tc, textures):
    bg = noise((128, 128, 3), 31)
    first = RT.head_vertices(static, 128, 128, shift_x=-8.0)
    second = yaw(RT.head_vertices(static, 128, 128, shift_x=12.0), 20)
    second[:, 2] -= 400.0  # behind the first
    assert second[:, 2].max() < first[:, 2].min()
    results = []
    for order in ((0, 1), (1, 0)):
        verts, tex = [[first, second][k] for k in order], textures[list(order)]
        want = expected(mesh, [bg], verts, faces, tex, tc, faces, [0, 0])
        solo = expected(mesh, [bg], verts[1:], faces, tex[1:], tc, faces, [0])[0]
        later = drawn(solo, bg)
        assert later[:, :64].any() and later[:, 64:].any()
        assert np.array_equal(want[0][later], solo[later])  # where the later head covers, the pixel is the later head's
        got, flags = draw(mesh, [bg], verts, tex, [0, 0])
        assert flags.tolist() == [0, 0]
        assert_frames(got, want, str(order))
        results.append(want[0])
    assert not np.array_equal(results[0], results[1])
    # an unsorted index: the heads of each frame in ascending head order
    bgs = [noise((100, 120, 3), 32), noise((120, 100, 3), 33)]
    index = [1, 0, 1, 0]
    verts = [RT.head_vertices(static, 120, 100, shift_x=-10.0), RT.head_vertices(static, 100, 120, shift_x=-10.0),
             RT.head_vertices(static, 120, 100, shift_x=15.0), RT.head_vertices(static, 100, 120, shift_x=15.0)]
    want = expected(mesh, bgs, verts, faces, textures[:4], tc, faces, index)
    swapped = expected(mesh, bgs, verts[::-1], faces, textures[:4][::-1].copy(), tc, faces, index[::-1])
    assert not np.array_equal(swapped[0], want[0])  # the order matters in this scene
    got, flags = draw(mesh, bgs, verts, textures[:4], index)
    assert flags.tolist() == [0] * 4
    assert_frames(got, want)


def test_the_border_band_of_each_frame(mesh, static, faces, tc, textures):
    shapes = [(96, 80), (70, 130)]
    bgs = [noise((h, w, 3), 34 + i) for i, (h, w) in enumerate(shapes)]
    verts = [RT.head_vertices(static, 96, 80, shift_x=35.0),   # over the right edge of a narrow frame
             RT.head_vertices(static, 70, 130, shift_x=-50.0)]  # over the left edge of a wide one
    verts[1][:, 1] += 30.0  # and over its lower edge
    for mapping in (0, 1):
        want = expected(mesh, bgs, verts, faces, textures[:2], tc, faces, [0, 1], mapping)
        for w, b, (h, wd) in zip(want, bgs, shapes):
            assert (drawn(w, b) & RT.band_mask(h, wd)).sum() > 20  # the expected image draws band pixels, on the frame's own size
        got, flags = draw(mesh, bgs, verts, textures[:2], [0, 1], mapping)
        assert flags.tolist() == [0, 0]
        assert_frames(got, want, MAPPING[mapping])


# ---- texture forms and sampling ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mapping", [0, 1])
@pytest.mark.parametrize("indexing", ["corner", "reference"])
def test_texture_forms_sampling_and_indexing(static, faces, tc, indexing, mapping):
    tt = np.ascontiguousarray(np.roll(faces, 17, axis=0))  # other texture triangles than mesh triangles: the two modes differ
    m = Mesh(faces, len(tc), device=0).set_texcoords(tc, tt)
    bgs = [noise((96, 80, 3), 36), noise((80, 96, 3), 37)]
    index = [0, 1, 0]
    verts = [RT.head_vertices(static, 96, 80, shift_x=-10.0), RT.head_vertices(static, 80, 96), yaw(RT.head_vertices(static, 96, 80, shift_x=14.0), -20)]
    rect = np.stack([RT.smooth_texture(33, 47, 4, seed=50 + k) for k in range(3)])  # float32 in [0, 255], 33 x 47 texels, four channels
    assert rect.dtype == np.float32 and 0 <= rect.min() and rect.max() <= 255
    results = {}
    for name, tex in (("float32 per head", rect), ("uint8 per head", rect.astype(np.uint8)), ("float32 shared", rect[1]), ("uint8 shared", rect[1].astype(np.uint8))):
        want = expected(m, bgs, verts, faces, tex, tc, tt, index, mapping, indexing)
        got, flags = draw(m, bgs, verts, tex, index, mapping, indexing)
        assert flags.tolist() == [0, 0, 0]
        assert_frames(got, want, name)
        results[name] = want
    assert not np.array_equal(results["float32 per head"][0], results["float32 shared"][0])  # head k samples texture k
    if mapping == 1:
        assert not np.array_equal(results["float32 per head"][0], results["uint8 per head"][0])  # the texel type matters to the blend
    other = expected(m, bgs, verts, faces, rect, tc, tt, index, mapping, "reference" if indexing == "corner" else "corner")
    assert not np.array_equal(other[0], results["float32 per head"][0])  # and so does the indexing mode


def test_one_head_per_frame_equals_the_batched_render_texture(mesh, static, textures):
    bg = cuda(noise((3, 96, 136, 3), 38))
    verts = cuda(np.stack([RT.head_vertices(static, 96, 136, shift_x=-60.0 + 40.0 * k) for k in range(3)]))
    for mapping in ("nearest", "bilinear"):
        want = mesh.render_texture(verts, cuda(textures[:3]), bg.clone(), mapping=mapping)
        got = bg.clone()
        flags = mesh.render_texture_frames(got, verts, cuda(textures[:3]), [0, 1, 2], mapping=mapping)
        assert torch.equal(got, want) and flags.tolist() == [0, 0, 0] and not torch.equal(got, bg)


# ---- flags ------------------------------------------------------------------------------------------------------------------------
def test_an_index_without_a_frame_is_flagged_and_draws_nothing(mesh, static, faces, tc, textures):
    bgs = [noise((96, 96, 3), 39), noise((80, 100, 3), 40)]
    index = [-1, 0, 2, 1, 2**31 - 1, -2**31]
    verts = [RT.head_vertices(static, 80, 96, shift_x=4.0 * k) for k in range(6)]
    wide = cuda(noise((80, 110, 3), 41))
    pattern = wide.clone()
    wide[:, 3:103] = cuda(bgs[1])
    d_index = cuda(np.asarray(index, np.int32))
    want = expected(mesh, bgs, [verts[1], verts[3]], faces, textures[[1, 3]], tc, faces, [0, 1])
    got, flags = draw(mesh, [cuda(bgs[0]), wide[:, 3:103]], verts, textures, d_index)
    assert flags.tolist() == [INDEX, 0, INDEX, 0, INDEX, INDEX]
    assert_frames(got, want)
    assert not np.array_equal(want[0], bgs[0]) and d_index.cpu().tolist() == index
    outside = torch.ones(110, dtype=torch.bool)
    outside[3:103] = False
    assert torch.equal(wide[:, outside.cuda()], pattern[:, outside.cuda()])
    # all heads flagged: no byte changes
    got, flags = draw(mesh, bgs, verts[:2], textures[:2], [5, -3])
    assert flags.tolist() == [INDEX, INDEX] and np.array_equal(got[0], bgs[0]) and np.array_equal(got[1], bgs[1])


def _eight_triangles(kind, seed=0):
    """The construction of test_gpu_render_frames.py: 24 vertices for the mesh of eight separate triangles: "cover" -- each covers a
    whole 256 x 256 frame (16 tiles), at its own depth; "small" -- eight triangles of about 20 pixels inside one tile."""
    rng = np.random.default_rng(seed)
    v = np.zeros((24, 3), np.float32)
    for t in range(8):
        if kind == "cover":
            v[3 * t: 3 * t + 3] = [[-300.5, -300.5, t], [900.5, -300.5, t], [-300.5, 900.5, t]]
        else:
            x, y = rng.uniform(70, 100, 2)
            v[3 * t: 3 * t + 3] = [[x, y, t], [x + 20.25, y + 3.5, t + 1], [x + 2.5, y + 19.75, t - 1]]
    return v


def test_a_head_that_overruns_the_pool_is_dropped_whole(textures):
    tri = np.arange(24, dtype=np.int32).reshape(8, 3)
    tc8 = np.zeros((24, 3), np.float32)
    tc8[:, :2] = np.random.default_rng(42).uniform(0, S - 1, (24, 2))
    mesh8 = Mesh(tri, 24, device=0).set_texcoords(tc8, tri)
    bg = noise((256, 256, 3), 43)
    # 8 triangles x 16 tiles = 128 entries against a pool of 4 * 8 * 1 = 32
    got, flags = draw(mesh8, [bg], [_eight_triangles("cover")], textures[:1], [0])
    assert flags.tolist() == [CAPACITY] and np.array_equal(got[0], bg)
    small = [_eight_triangles("small", s) for s in (1, 2, 3)]
    for verts, want_flags in (([small[0], _eight_triangles("cover"), small[1], small[2]], [0, CAPACITY, 0, 0]),
                              ([_eight_triangles("cover")] + small, [0, CAPACITY, CAPACITY, CAPACITY])):
        got, flags = draw(mesh8, [bg], verts, textures[:4], [0, 0, 0, 0])
        assert flags.tolist() == want_flags
        dropped = {k for k, f in enumerate(want_flags) if f}
        # no head is ever drawn in part: the frame is the expected one without the flagged heads
        want = expected(mesh8, [bg], verts, tri, textures[:4], tc8, tri, [0, 0, 0, 0], skip=dropped)
        assert not np.array_equal(want[0], bg)
        assert_frames(got, want, str(want_flags))


def test_refusals_before_device_work(mesh, static, textures):
    lib = _lib.load()
    poison = cuda(noise((64, 64, 3), 44))
    before = poison.clone()
    frames = DeviceFrames([poison], torch.device("cuda", 0))
    v, tex = cuda(RT.head_vertices(static, 64, 64)[None]), cuda(textures[:1])
    index, flags = cuda(np.zeros(1, np.int32)), torch.full((1,), -7, dtype=torch.int32, device="cuda")
    bare = Mesh(np.ascontiguousarray(mesh._triangles), mesh.nver, device=0)  # no texture coordinates attached
    xy_only = Mesh(np.ascontiguousarray(mesh._triangles), mesh.nver, device=0).set_texcoords(np.zeros((mesh.nver, 2), np.float32))
    good = dict(m=mesh._handle, frames=frames.device.data_ptr(), host=frames.host.ctypes.data, n_frames=1, v=v.data_ptr(), tex=tex.data_ptr(),
                dtype=_lib.DTYPE_U8, tex_c=3, indexing=0, index=index.data_ptr(), n_heads=1, flags=flags.data_ptr())

    def call(**kw):
        a = {**good, **kw}
        return lib.dad3d_mesh_render_texture_frames(a["m"], a["frames"], a["host"], a["n_frames"], a["v"], a["tex"], a["dtype"], 1, S, S, a["tex_c"],
                                                    1, a["indexing"], a["index"], a["n_heads"], a["flags"], None)

    thin_host = np.array([[poison.data_ptr(), 64, 64, 191]], np.int64)  # rows that overlap
    for kw in (dict(m=None), dict(frames=None), dict(host=None), dict(v=None), dict(tex=None), dict(index=None), dict(flags=None), dict(n_frames=-1),
               dict(n_heads=-1), dict(n_frames=65536), dict(n_heads=65536), dict(host=thin_host.ctypes.data), dict(tex_c=2), dict(dtype=7),
               dict(indexing=2), dict(m=bare._handle), dict(m=xy_only._handle, indexing=_lib.TEX_INDEX_REFERENCE)):
        lib.dad3d_clear_error()
        assert call(**kw) == _lib.E_INVALID, kw
        assert lib.dad3d_last_error() != b""
    assert call(m=bare._handle) == _lib.E_INVALID and b"no texture coordinates" in lib.dad3d_last_error()
    assert call(n_frames=0) == _lib.OK and call(n_heads=0) == _lib.OK  # nothing to do
    torch.cuda.synchronize()
    assert torch.equal(poison, before) and flags.tolist() == [-7]  # nothing was launched
    assert call() == _lib.OK
    torch.cuda.synchronize()
    assert flags.tolist() == [0] and not torch.equal(poison, before)
    with pytest.raises(ValueError, match="mode"):
        overlay.draw_heads([], [poison], mode="flat")
    with pytest.raises(ValueError, match="only with mode='textured'"):
        overlay.draw_heads([], [poison], mode="shaded", textures=tex)
    with pytest.raises(ValueError, match="needs textures"):
        overlay.draw_heads([], [poison], mode="textured")


# ---- graphs and scratch -----------------------------------------------------------------------------------------------------------
def test_graph_replay_allocates_nothing_once_the_scratch_is_large_enough(static, faces, tc, textures):
    m = Mesh(faces, len(tc), device=0).set_texcoords(tc, faces)  # a handle of its own: its scratch starts at 0
    assert m.frames_scratch_bytes() == 0
    bgs = [cuda(noise((100, 130, 3), 45)), cuda(noise((140, 90, 3), 46)), cuda(noise((64, 64, 3), 47))]
    work = [b.clone() for b in bgs]
    frames = DeviceFrames(work, torch.device("cuda", 0))  # the table is uploaded once, outside the capture
    verts = cuda(np.stack([RT.head_vertices(static, 100, 130), RT.head_vertices(static, 140, 90), RT.head_vertices(static, 140, 90, shift_x=20.0),
                           RT.head_vertices(static, 64, 64)]))
    tex, index = cuda(textures[:4]), cuda(np.asarray([0, 1, 1, 2], np.int32))
    flags = m.render_texture_frames(frames, verts, tex, index)  # warm-up: allocates (and synchronises)
    torch.cuda.synchronize()
    eager = [w.clone() for w in work]
    assert flags.tolist() == [0] * 4 and all(not torch.equal(e, b) for e, b in zip(eager, bgs))
    held = m.frames_scratch_bytes()
    assert held > 0
    for w, b in zip(work, bgs):
        w.copy_(b)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.render_texture_frames(frames, verts, tex, index)
    for w, b in zip(work, bgs):
        w.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    for w, e in zip(work, eager):
        assert torch.equal(w, e)
    assert m.frames_scratch_bytes() == held
    small = [bgs[1].clone()]
    m.render_texture_frames(small, verts[1:3], tex[1:3], [0, 0])  # fewer heads and frames: nothing is allocated
    torch.cuda.synchronize()
    assert m.frames_scratch_bytes() == held and torch.equal(small[0], eager[1])


# ---- bake, then draw --------------------------------------------------------------------------------------------------------------
def test_round_trip_add_over_three_poses_then_draw_heads_textured(static, flame_model, faces, monkeypatch):
    atlas = dict(synthetic.synthetic_texture_data(S, seed=0, static=static, duplicates=50))
    atlas.update(synthetic.synthetic_texcoords(S, static))
    creator = UVTextureCreator(texture_data=atlas, flame_model=flame_model, static=static, device=0)
    flame = creator.head_mesh.flame
    fr = [noise((256, 256, 3), 48), noise((300, 280, 3), 49)]
    frames = [cuda(f) for f in fr]
    params = torch.from_numpy(synthetic.synthetic_params(6, seed=23)).cuda()
    index = [1, 0]  # slot 0 lives in frame 1, slot 1 in frame 0
    acc = TextureAccumulator(creator, 2)
    want_tex, want_sc = np.zeros((2, S, S, 3), np.uint8), np.full((2, S, S), -1.0, np.float32)
    seen = []
    for step in range(3):
        p = params[[step, step + 3]].contiguous()
        dicts = [{"3dmm_params": p[k], "image_index": torch.tensor(index[k], dtype=torch.int32, device="cuda")} for k in range(2)]
        verts = flame.decode(p.clone(), proj=True, to_2d=False, mutate=True)["proj"].cpu().numpy()
        want_tex, want_sc, _, stats = TF.expected_bake_frames(atlas, fr, verts, faces, index, want_tex, want_sc)
        seen.append(stats)
        assert acc.add(dicts, frames).tolist() == [0, 0]
        assert torch.equal(p, params[[step, step + 3]])  # the dicts' params are not mutated
    assert all(st["candidates"] > 500 for stats in seen for st in stats)
    assert all(st["replaced"] > 0 and st["kept"] > 0 for stats in seen[1:] for st in stats)
    assert np.array_equal(acc.score.cpu().numpy(), want_sc) and np.array_equal(acc.textures.cpu().numpy(), want_tex)
    # the last pose of each slot, drawn with the texture it has gathered
    p = params[[2, 5]].contiguous()
    dicts = [{"3dmm_params": p[k], "image_index": torch.tensor(index[k], dtype=torch.int32, device="cuda")} for k in range(2)]
    overlay.draw_heads(dicts, frames, mode="textured", textures=acc)  # warm-up: the renderer is built, the scratch allocated
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError("a host wait")

    with monkeypatch.context() as mp:
        for name in ("cpu", "item", "tolist", "numpy"):
            mp.setattr(torch.Tensor, name, refuse)
        mp.setattr(torch.cuda, "synchronize", refuse)
        got = overlay.draw_heads(dicts, frames, mode="textured", textures=acc)
        nearest = overlay.draw_heads(dicts, frames, mode="textured", textures=acc.textures, creator=creator, mapping="nearest")
    assert isinstance(got, list) and all(g is not f for g, f in zip(got, frames)) and all(torch.equal(f, cuda(b)) for f, b in zip(frames, fr))
    rm = creator.renderer
    lay = synthetic.synthetic_texcoords(S, static)
    keep = (np.asarray(lay["ft"]) >= 0).all(1)
    tc2 = np.ascontiguousarray(texel_coords(lay["vt"], S), dtype=np.float32)
    tri, tt = np.ascontiguousarray(faces[keep]), np.ascontiguousarray(np.asarray(lay["ft"])[keep], dtype=np.int32)
    verts = flame.decode(p.clone(), proj=True, to_2d=False, flip_z=True)["proj"].cpu().numpy()
    tc3 = np.concatenate([tc2, np.zeros((len(tc2), 1), np.float32)], 1)
    for mapping, result in ((1, got), (0, nearest)):
        want = expected(rm, fr, verts, tri, want_tex, tc3, tt, index, mapping)
        assert all(0.02 < drawn(w, b).mean() < 0.98 for w, b in zip(want, fr))
        assert_frames([g.cpu().numpy() for g in result], want, MAPPING[mapping])
