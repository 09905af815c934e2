"""GPU: the occlusion-aware texture bake (csrc/uv_texture_occlusion.hip; `UVMap.depth_frames`, `UVMap.bake_frames(occlusion="self")`,
`TextureAccumulator(occlusion="self")`) against tests/texture_occlusion_restatement.py: the depth maps are the oracle's
`rasterize_triangles` on the head with z negated (the reference's own compiled C++ where oracle/_ref holds it), the bake is the float64
restatement of the reference's candidate rule plus the depth test. Every comparison is np.array_equal. Each case asserts on the EXPECTED
arrays that it exercises what it claims. Heads are `RT.head_vertices` with column 2 negated -- the face looks at -z, as the decode's
output does -- turned with the `yaw` helper of test_gpu_bake_frames.py."""
import numpy as np
import pytest
import torch

import render_texture_ref as RT
import texture_frames_restatement as TF
import texture_occlusion_restatement as TO
from dad_3dheads_amd import _lib, synthetic
from dad_3dheads_amd.Sim3DR.frames import DeviceFrames
from dad_3dheads_amd.uv_texture import TextureAccumulator, UVMap, UVTextureCreator
from test_gpu_bake_frames import yaw

pytestmark = pytest.mark.gpu
INDEX, WINDOW, NONFINITE = _lib.BAKE_FLAG_INDEX, _lib.BAKE_FLAG_DEPTH_WINDOW, _lib.BAKE_FLAG_NONFINITE
ATLASES = [(37, 50), (64, 0), (64, 50)]  # (S, duplicates): 37 * 37 texels are no multiple of a lane's four
D = 128
# (frame h, w, yaw in degrees): unclipped heads; the last one's box is larger than 128
POSES = [(96, 80, 0), (96, 80, 50), (96, 80, 30), (70, 130, -50), (64, 64, 70), (160, 160, 50)]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def head(static, h, w, degrees=0, **kw):
    v = RT.head_vertices(static, h, w, **kw).copy()
    v[:, 2] = -v[:, 2]
    return yaw(v, degrees) if degrees else v


@pytest.fixture(scope="module")
def faces(static):
    return np.ascontiguousarray(static["faces"], dtype=np.int32)


@pytest.fixture(scope="module")
def maps(static, faces):
    """(S, duplicates) -> (atlas, UVMap), built once."""
    out = {}
    for s, dups in ATLASES:
        td = synthetic.synthetic_texture_data(s, seed=s + dups, static=static, duplicates=dups)
        out[(s, dups)] = (td, UVMap(faces, 5023, td, device=0))
    return out


def depth_maps(m, frames, verts, index, side=D, out=None):
    dev = [f if isinstance(f, torch.Tensor) else cuda(f) for f in frames]
    depth, window, flags = m.depth_frames(cuda(np.stack(verts)), dev, index, depth_side=side, out=out)
    torch.cuda.synchronize()
    return depth.cpu().numpy(), window.cpu().numpy(), flags.cpu().numpy()


def assert_depth(got, want, what=""):
    (depth, window, flags), (want_maps, want_window, want_flags) = got, want
    assert flags.tolist() == want_flags.tolist(), what
    assert np.array_equal(window, want_window), (what, window.tolist(), want_window.tolist())
    for k, wm in enumerate(want_maps):
        if wm is not None:
            wh, ww = wm.shape
            assert np.array_equal(depth[k, :wh, :ww], wm), f"{what} head {k}: {int((depth[k, :wh, :ww] != wm).sum())} of {wm.size} entries differ"


def bake(m, frames, verts, index, side=D, out=None, score=None, **kw):
    """-> (textures, score, flags) as numpy, with occlusion="self"."""
    dev = [f if isinstance(f, torch.Tensor) else cuda(f) for f in frames]
    v = cuda(np.stack(verts))
    tex, flags = m.bake_frames(v, m.vertex_normals(v), dev, index, out=out, score=score, occlusion="self", depth_side=side, **kw)
    torch.cuda.synchronize()
    return tex.cpu().numpy(), None if score is None else score.cpu().numpy(), flags.cpu().numpy()


def fresh(n, s):
    return torch.zeros((n, s, s, 3), dtype=torch.uint8, device="cuda"), torch.full((n, s, s), -1.0, dtype=torch.float32, device="cuda")


# ---- 1. depth maps ----------------------------------------------------------------------------------------------------------------
def test_depth_maps_of_mixed_frames_an_unsorted_index_and_a_clipped_head(static, faces, maps, sim3dr_oracle):
    _, m = maps[(64, 0)]
    shapes = [(96, 80), (70, 130), (64, 64)]
    index = [2, 0, 1, 0, 1]  # unsorted, two heads in frame 0 and two in frame 1
    verts = [head(static, 64, 64), head(static, 96, 80, 20), head(static, 70, 130, -35),
             head(static, 96, 80, shift_x=-40.0),  # half outside its frame
             head(static, 70, 130, 60, shift_x=20.0)]
    want = TO.expected_depth_frames(sim3dr_oracle, shapes, verts, faces, index, D)
    assert want[2].tolist() == [0] * 5 and want[1][3, 0] == 0 and RT.head_vertices(static, 96, 80, shift_x=-40.0)[:, 0].min() < -5
    for wm in want[0]:  # every window is partly covered, and the depths are of both signs somewhere
        assert 0.3 < np.isfinite(wm).mean() < 0.95
    assert any((wm[np.isfinite(wm)] < 0).any() and (wm[np.isfinite(wm)] > 0).any() for wm in want[0])
    sentinel = torch.full((5, D, D), -7.0, dtype=torch.float32, device="cuda")
    got = depth_maps(m, [cuda(noise((h, w, 3), i)) for i, (h, w) in enumerate(shapes)], verts, index, out=sentinel)
    assert_depth(got, want)
    for k in range(5):  # entries outside ww x wh are not written
        _, _, ww, wh = want[1][k]
        outside = np.ones((D, D), bool)
        outside[:wh, :ww] = False
        assert (got[0][k][outside] == -7.0).all() and outside.any()
    # the device index is used as it is, and the frames' pixels are never read: the table alone gives the same maps
    again = depth_maps(m, [cuda(np.zeros((h, w, 3), np.uint8)) for h, w in shapes], verts, cuda(np.asarray(index, np.int32)))
    assert_depth(again, want, "device index")


def test_depth_map_of_the_two_planes_and_of_heads_off_their_frames(static, faces, maps, sim3dr_oracle):
    v, tri, td, _ = TO.two_planes()
    m = UVMap(tri, 8, td, device=0)
    off = v + np.float32(100)  # outside its 32 x 40 frame: an empty window, no flag
    clipped = v - np.array([15.5, 12.25, 0], np.float32)  # over the corner: large triangles, walked by the wave, clipped at 0
    tilted = v.copy()
    tilted[[1, 3, 5, 7], 2] -= 7.5  # depths of both signs, and the planes cross the front one
    verts = [v, off, clipped, tilted]
    want = TO.expected_depth_frames(sim3dr_oracle, [(32, 40)], verts, tri, [0, 0, 0, 0], 32)
    assert want[1].tolist() == [[10, 10, 21, 11], [0, 0, 0, 0], [0, 0, 16, 9], [10, 10, 21, 11]] and want[2].tolist() == [0] * 4
    assert (want[0][3] < 0).any() and (want[0][3] > 0).any() and np.isinf(want[0][0]).any()
    got = depth_maps(m, [noise((32, 40, 3), 3)], verts, [0, 0, 0, 0], side=32)
    assert_depth(got, want)
    # D = 21 holds the 21 x 11 window exactly, D = 20 does not; D = 1 holds nothing of these
    for side, flag in ((21, 0), (20, WINDOW), (1, WINDOW)):
        want = TO.expected_depth_frames(sim3dr_oracle, [(32, 40)], [v], tri, [0], side)
        assert want[2].tolist() == [flag]
        assert_depth(depth_maps(m, [noise((32, 40, 3), 3)], [v], [0], side=side), want, f"D = {side}")
    # the head template in a frame it has left on the right, and one it only touches
    _, hm = maps[(64, 0)]
    verts = [head(static, 64, 64, shift_x=80.0), head(static, 64, 64, shift_x=50.0)]
    want = TO.expected_depth_frames(sim3dr_oracle, [(64, 64)], verts, faces, [0, 0], D)
    assert want[1][0].tolist() == [0, 0, 0, 0] and 0 < want[1][1][2] < 16 and want[2].tolist() == [0, 0]
    assert_depth(depth_maps(hm, [noise((64, 64, 3), 4)], verts, [0, 0]), want)


# ---- 2. the occluded bake ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,dups", ATLASES)
def test_occluded_bake_plain_and_accumulate_from_reset(static, faces, maps, sim3dr_oracle, size, dups):
    td, m = maps[(size, dups)]
    shapes = [(96, 80), (70, 130), (64, 64), (160, 160)]
    frame_of = {(96, 80): 0, (70, 130): 1, (64, 64): 2, (160, 160): 3}
    frames = [noise((h, w, 3), 10 + i) for i, (h, w) in enumerate(shapes)]
    dev = [cuda(f) for f in frames]
    verts = [head(static, h, w, deg) for h, w, deg in POSES]
    index = [frame_of[(h, w)] for h, w, _ in POSES]
    # the first five heads with D = 128, the last (a 114 x 129 window) with D = 160
    for sel, side in ((slice(0, 5), D), (slice(5, 6), 160)):
        v, idx = verts[sel], index[sel]
        n = len(v)
        dm = TO.expected_depth_frames(sim3dr_oracle, shapes, v, faces, idx, side)
        assert dm[2].tolist() == [0] * n
        without, _, _, _ = TF.expected_bake_frames(td, frames, v, faces, idx)
        for biases in ((1.0, 1.0), (0.0, 0.0)):
            kw = dict(depth_bias=biases[0], slope_bias=biases[1])
            want, _, want_flags, stats = TO.expected_bake_frames_occluded(td, frames, v, faces, idx, *dm, *biases)
            for k, st in enumerate(stats):
                pose = POSES[sel][k]
                if biases == (1.0, 1.0):  # the defaults hide the samples behind the nose and little else
                    assert 5 <= st["hidden"] <= 0.05 * st["accepted"], (pose, st)
                else:  # without a bias a head hides itself: shadow acne
                    assert st["hidden"] >= 0.2 * st["accepted"], (pose, st)
                    if ((size, dups), pose) in (((64, 50), (96, 80, 30)), ((37, 50), (70, 130, -50))):
                        assert st["moved"] >= 2, (pose, st)  # a hidden candidate hands its texel to the texel's next one
            assert not np.array_equal(want, without)
            got, _, flags = bake(m, dev, v, idx, side=side, **kw)
            assert flags.tolist() == want_flags.tolist() == [0] * n
            assert np.array_equal(got, want), (biases, [int((got[k] != want[k]).any(-1).sum()) for k in range(n)])
            # accumulation from reset gives the same bytes where a texel was filled, and zeros elsewhere
            tex, score = fresh(n, size)
            acc, sc, flags = bake(m, dev, v, idx, side=side, out=tex, score=score, **kw)
            want_acc, want_sc, _, _ = TO.expected_bake_frames_occluded(td, frames, v, faces, idx, *dm, *biases, textures=np.zeros_like(want),
                                                                       score=np.full((n, size, size), -1.0, np.float32))
            assert flags.tolist() == [0] * n
            assert np.array_equal(acc, want_acc) and np.array_equal(sc, want_sc) and np.array_equal(acc, want)
    # the defaults of the keywords are the biases 1.0 and 1.0
    got, _, _ = bake(m, dev, verts[:1], index[:1])
    dm = TO.expected_depth_frames(sim3dr_oracle, shapes, verts[:1], faces, index[:1], D)
    assert np.array_equal(got, TO.expected_bake_frames_occluded(td, frames, verts[:1], faces, index[:1], *dm)[0])


def test_occluded_bake_of_the_two_planes(sim3dr_oracle):
    v, tri, td, groups = TO.two_planes()
    m = UVMap(tri, 8, td, device=0)
    frame = np.random.default_rng(5).integers(1, 256, (32, 40, 3), dtype=np.uint8)
    dm = TO.expected_depth_frames(sim3dr_oracle, [(32, 40)], [v], tri, [0], 32)
    for bias, hidden in ((0.0, 4), (4.9, 4), (5.1, 0), (6.0, 0)):
        want, _, _, stats = TO.expected_bake_frames_occluded(td, [frame], [v], tri, [0], *dm, bias, 0.0)
        assert stats[0]["hidden"] == hidden and want.reshape(-1, 3)[groups["under"]].any() == (hidden == 0)
        got, _, flags = bake(m, [frame], [v], [0], side=32, depth_bias=bias, slope_bias=0.0)
        assert flags.tolist() == [0] and np.array_equal(got, want), bias


# ---- 3. flags ---------------------------------------------------------------------------------------------------------------------
def test_flags_of_four_heads_in_one_call(static, faces, maps, sim3dr_oracle):
    td, m = maps[(37, 50)]
    side = 48
    frames = [noise((96, 80, 3), 20), noise((64, 64, 3), 21)]
    spoilt = head(static, 64, 64, 15, fill=0.55)
    spoilt[1234, 1] = np.nan
    verts = [head(static, 64, 64, fill=0.55), head(static, 96, 80), spoilt, head(static, 64, 64, -20, fill=0.55)]
    index = [-1, 0, 1, 1]  # no frame | a 51 x 65 window against D = 48 | one NaN vertex | clean
    dm = TO.expected_depth_frames(sim3dr_oracle, [(96, 80), (64, 64)], verts, faces, index, side)
    assert dm[2].tolist() == [INDEX, WINDOW, NONFINITE, 0] and max(dm[1][3, 2:]) <= side
    assert TO.expected_window((96, 80), verts[1], 128) == (0, [15, 16, 51, 65])
    sentinel = torch.full((4, side, side), -7.0, dtype=torch.float32, device="cuda")
    got_dm = depth_maps(m, frames, verts, cuda(np.asarray(index, np.int32)), side=side, out=sentinel)
    assert_depth(got_dm, dm)
    assert (got_dm[0][:3] == -7.0).all() and got_dm[1][:3].tolist() == [[0, 0, 0, 0]] * 3  # no byte of a flagged head's map is written
    # accumulate: the three flagged heads keep a noise-filled texture and score byte for byte
    tex = cuda(noise((4, 37, 37, 3), 22))
    score = cuda(np.random.default_rng(23).uniform(-1, 1, (4, 37, 37)).astype(np.float32))
    tex0, score0 = tex.cpu().numpy(), score.cpu().numpy()
    with np.errstate(invalid="ignore"):
        want_acc, want_sc, want_flags, stats = TO.expected_bake_frames_occluded(td, frames, verts, faces, index, *dm, textures=tex0, score=score0)
    assert want_flags.tolist() == [INDEX, WINDOW, NONFINITE, 0] and stats[:3] == [None] * 3
    assert stats[3]["replaced"] > 100 and stats[3]["kept"] > 100 and stats[3]["hidden"] > 0
    acc, sc, flags = bake(m, frames, verts, index, side=side, out=tex, score=score)
    assert flags.tolist() == [INDEX, WINDOW, NONFINITE, 0]
    assert np.array_equal(acc, want_acc) and np.array_equal(sc, want_sc)
    for k in range(3):
        assert np.array_equal(acc[k], tex0[k]) and np.array_equal(sc[k], score0[k])
    # plain: the flagged heads give zeros
    poison = torch.full((4, 37, 37, 3), 9, dtype=torch.uint8, device="cuda")
    want, _, _, _ = TO.expected_bake_frames_occluded(td, frames, verts, faces, index, *dm)
    got, _, flags = bake(m, frames, verts, index, side=side, out=poison)
    assert flags.tolist() == [INDEX, WINDOW, NONFINITE, 0] and np.array_equal(got, want) and not got[:3].any() and got[3].any()
    # a head that is both off the table and not finite carries both flags
    _, _, flags = bake(m, frames, [spoilt], [7], side=side)
    assert flags.tolist() == [INDEX | NONFINITE]


# ---- 4. heads do not see each other -----------------------------------------------------------------------------------------------
def test_two_overlapping_heads_in_one_frame_give_the_bytes_each_gives_alone(static, maps):
    _, m = maps[(64, 50)]
    frame = cuda(noise((96, 80, 3), 30))
    a, b = head(static, 96, 80, 30, shift_x=-6.0), head(static, 96, 80, -20, shift_x=8.0)
    b[:, 2] += 100.0  # wholly behind the first: its depths still compare only with its own
    assert b[:, 2].min() > a[:, 2].max() and abs(a[:, 0].mean() - b[:, 0].mean()) < 20
    both, _, flags = bake(m, [frame], [a, b], [0, 0])
    alone_a, _, _ = bake(m, [frame], [a], [0])
    alone_b, _, _ = bake(m, [frame], [b], [0])
    assert flags.tolist() == [0, 0] and np.array_equal(both[0], alone_a[0]) and np.array_equal(both[1], alone_b[0])
    assert both[0].any() and both[1].any() and not np.array_equal(both[0], both[1])
    d_both = depth_maps(m, [frame], [a, b], [0, 0])
    d_a, d_b = depth_maps(m, [frame], [a], [0]), depth_maps(m, [frame], [b], [0])
    for k, alone in enumerate((d_a, d_b)):
        _, _, ww, wh = alone[1][0]
        assert np.array_equal(d_both[1][k], alone[1][0]) and np.array_equal(d_both[0][k, :wh, :ww], alone[0][0, :wh, :ww]) and ww > 0


# ---- 5. the default is today's call -----------------------------------------------------------------------------------------------
def test_occlusion_none_is_the_bake_without_the_test(static, faces, maps):
    td, m = maps[(37, 50)]
    frames = [noise((96, 80, 3), 40), noise((70, 130, 3), 41)]
    verts = [head(static, 96, 80, 50), head(static, 70, 130, -50), head(static, 96, 80)]
    index = [0, 1, 3]
    want, _, want_flags, _ = TF.expected_bake_frames(td, frames, verts, faces, index)
    dev, v = [cuda(f) for f in frames], cuda(np.stack(verts))
    normals = m.vertex_normals(v)
    today, today_flags = m.bake_frames(v, normals, dev, index)
    # the occlusion keywords are ignored without occlusion="self", whatever they hold
    got, flags = m.bake_frames(v, normals, dev, index, occlusion=None, depth_side=1, depth_bias=0.0, slope_bias=0.0)
    assert torch.equal(got, today) and torch.equal(flags, today_flags) and flags.tolist() == want_flags.tolist() == [0, 0, INDEX]
    assert np.array_equal(got.cpu().numpy(), want)
    tex, score = fresh(3, 37)
    tex2, score2 = fresh(3, 37)
    m.bake_frames(v, normals, dev, index, out=tex, score=score)
    m.bake_frames(v, normals, dev, index, out=tex2, score=score2, occlusion=None)
    assert torch.equal(tex, tex2) and torch.equal(score, score2) and bool(tex.any())
    hidden, _ = m.bake_frames(v, normals, dev, index, occlusion="self", depth_side=D)
    assert not torch.equal(hidden, today)
    for bad in (dict(occlusion="other"), dict(occlusion="self", depth_bias=-1.0), dict(occlusion="self", slope_bias=float("nan")),
                dict(occlusion="self", depth_side=0), dict(occlusion="self", depth_side=4097)):
        with pytest.raises(ValueError):
            m.bake_frames(v, normals, dev, index, **bad)


# ---- 6. the accumulator -----------------------------------------------------------------------------------------------------------
def test_texture_accumulator_with_self_occlusion_over_three_yaws(static, flame_model, faces, sim3dr_oracle, monkeypatch):
    td = synthetic.synthetic_texture_data(64, seed=114, static=static, duplicates=50)
    creator = UVTextureCreator(texture_data=td, flame_model=flame_model, static=static, device=0)
    flame = creator.head_mesh.flame
    side = 256
    params = synthetic.synthetic_params(6, seed=23)
    params[:, :403] *= 0.2
    params[:, 409:411], params[:, 412] = 0.0, 6.0
    for k, degrees in enumerate((50, 0, -50, -50, 50, 0)):  # slot 0 sees yaw 50, 0, -50; slot 1 yaw -50, 50, 0
        a = np.deg2rad(degrees)
        params[k, 403:409] = [np.cos(a), 0.0, -np.sin(a), 0.0, 1.0, 0.0]
    params = torch.from_numpy(params).cuda()
    fr = [noise((256, 256, 3), 50), noise((300, 280, 3), 51)]
    table = DeviceFrames([cuda(f) for f in fr], torch.device("cuda", 0))  # uploaded once, outside the capture
    index = cuda(np.asarray([1, 0], np.int32))
    acc = TextureAccumulator(creator, 2, occlusion="self", depth_side=side)
    plain = TextureAccumulator(creator, 2)
    assert plain.occlusion is None and plain._depth is None and acc._depth[0].shape == (2, side, side)
    want_tex, want_sc = np.zeros((2, 64, 64, 3), np.uint8), np.full((2, 64, 64), -1.0, np.float32)
    none_tex, none_sc = want_tex.copy(), want_sc.copy()
    acc.add(params[[0, 3]].contiguous(), table, index)  # warm-up: the handles are built
    acc.reset()
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError("a host wait")

    seen = []
    for step in range(3):
        p = params[[step, step + 3]].contiguous()
        verts = flame.decode(p.clone(), proj=True, to_2d=False, mutate=True)["proj"].cpu().numpy()
        dm = TO.expected_depth_frames(sim3dr_oracle, [f.shape[:2] for f in fr], verts, faces, [1, 0], side)
        want_tex, want_sc, want_flags, stats = TO.expected_bake_frames_occluded(td, fr, verts, faces, [1, 0], *dm, textures=want_tex, score=want_sc)
        none_tex, none_sc, _, _ = TF.expected_bake_frames(td, fr, verts, faces, [1, 0], none_tex, none_sc)
        seen.append(stats)
        assert want_flags.tolist() == [0, 0]
        with monkeypatch.context() as mp:  # nothing waits for the device
            for name in ("cpu", "item", "tolist", "numpy"):
                mp.setattr(torch.Tensor, name, refuse)
            mp.setattr(torch.cuda, "synchronize", refuse)
            flags = acc.add(p, table, index)
            plain.add(p, table, index)
        assert flags.tolist() == [0, 0] and torch.equal(p, params[[step, step + 3]])
    assert all(st["candidates"] > 500 and st["hidden"] > 0 for stats in seen for st in stats)
    assert all(st["replaced"] > 0 and st["kept"] > 0 for stats in seen[1:] for st in stats)
    assert np.array_equal(acc.score.cpu().numpy(), want_sc) and np.array_equal(acc.textures.cpu().numpy(), want_tex)
    assert np.array_equal(plain.score.cpu().numpy(), none_sc) and np.array_equal(plain.textures.cpu().numpy(), none_tex)
    assert (want_tex != none_tex).any(-1).sum() >= 1  # at least one texel holds a different sample than without the depth test
    # one graph of `add`, replayed from reset on the last frame set, against the eager result
    p = params[[2, 5]].contiguous()
    acc.reset()
    acc.add(p, table, index)
    torch.cuda.synchronize()
    eager_tex, eager_sc = acc.textures.clone(), acc.score.clone()
    acc.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        acc.add(p, table, index)
    acc.reset()
    acc._depth[0].fill_(-3.0)  # the replay draws its own depth maps
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(acc.textures, eager_tex) and torch.equal(acc.score, eager_sc) and bool(eager_tex.any())
    with pytest.raises(ValueError, match="occlusion"):
        TextureAccumulator(creator, 2, occlusion="others")
    with pytest.raises(ValueError, match="depth_side"):
        TextureAccumulator(creator, 2, occlusion="self", depth_side=5000)
