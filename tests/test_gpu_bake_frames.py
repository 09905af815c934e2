"""GPU: the UV-texture bake from frames (csrc/uv_texture_frames.hip; `UVMap.bake_frames`, `UVTextureCreator.bake_frames`,
`uv_texture.TextureAccumulator`) against tests/texture_frames_restatement.py `expected_bake_frames`: the float64 restatement of the
reference's candidate rule on the frame each head names, the plain bake or "best view wins". Every comparison is np.array_equal: the
kernel is an unfused restatement. Each case asserts on the EXPECTED arrays that it exercises what it claims."""
import numpy as np
import pytest
import torch

import render_texture_ref as RT
import texture_frames_restatement as TF
from dad_3dheads_amd import _lib, synthetic
from dad_3dheads_amd.Sim3DR.frames import DeviceFrames
from dad_3dheads_amd.uv_texture import TextureAccumulator, UVMap, UVTextureCreator

pytestmark = pytest.mark.gpu
FLAG = _lib.BAKE_FLAG_INDEX
ATLASES = [(37, 0), (64, 50), (37, 50), (64, 0)]  # (S, duplicates): 37 * 37 texels are no multiple of a lane's four


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


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


def yaw(v, degrees):
    """The head turned about the vertical axis through the centre of its box."""
    c = 0.5 * (v.min(0) + v.max(0)).astype(np.float64)
    a = np.deg2rad(degrees)
    r = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    return ((v.astype(np.float64) - c) @ r.T + c).astype(np.float32)


def bake(m, frames, verts, index, out=None, score=None):
    """frames: numpy arrays or CUDA tensors -> (textures, score, flags) as numpy."""
    dev = [f if isinstance(f, torch.Tensor) else cuda(f) for f in frames]
    v = cuda(np.stack(verts))
    tex, flags = m.bake_frames(v, m.vertex_normals(v), dev, index, out=out, score=score)
    torch.cuda.synchronize()
    return tex.cpu().numpy(), None if score is None else score.cpu().numpy(), flags.cpu().numpy()


def fresh(n, s):
    return torch.zeros((n, s, s, 3), dtype=torch.uint8, device="cuda"), torch.full((n, s, s), -1.0, dtype=torch.float32, device="cuda")


@pytest.mark.parametrize("size,dups", ATLASES)
def test_mixed_sizes_and_layouts_in_one_call(static, faces, maps, size, dups):
    td, m = maps[(size, dups)]
    bgs = [noise((96, 80, 3), 1), noise((70, 130, 3), 2), noise((64, 64, 3), 3)]
    wide = cuda(noise((70, 140, 3), 4))
    wide[:, 4:134] = cuda(bgs[1])
    view = wide[:, 4:134]  # a strided view of a wider buffer
    flat = torch.zeros(64 * 64 * 3 + 1, dtype=torch.uint8, device="cuda")
    odd = flat[1:].view(64, 64, 3)  # starts at an odd address
    odd.copy_(cuda(bgs[2]))
    assert view.stride(0) == 420 and odd.data_ptr() % 2 == 1
    index = [2, 0, 1, 0, 1]  # unsorted
    verts = [RT.head_vertices(static, 64, 64), RT.head_vertices(static, 96, 80), RT.head_vertices(static, 70, 130),
             RT.head_vertices(static, 96, 80, shift_x=-40.0),  # half outside its frame
             yaw(RT.head_vertices(static, 70, 130, shift_x=20.0), 25)]
    want, _, want_flags, stats = TF.expected_bake_frames(td, bgs, verts, faces, index)
    assert stats[3]["outside"] > 100 and stats[3]["inside"] > 100  # some candidates fail 0 < x < w and some pass
    assert all(st["candidates"] > 100 for st in stats) and all(st["outside"] == 0 for st in (stats[0], stats[1], stats[2]))
    got, _, flags = bake(m, [cuda(bgs[0]), view, odd], verts, index)
    assert flags.tolist() == want_flags.tolist() == [0] * 5
    assert np.array_equal(got, want)
    assert len({want[k].tobytes() for k in range(5)}) == 5
    # accumulation from reset gives the same bytes where a texel was filled, and zeros elsewhere
    tex, score = fresh(5, size)
    acc, sc, flags = bake(m, [cuda(bgs[0]), view, odd], verts, index, out=tex, score=score)
    want_acc, want_sc, _, _ = TF.expected_bake_frames(td, bgs, verts, faces, index, np.zeros_like(want), np.full((5, size, size), -1.0, np.float32))
    assert np.array_equal(acc, want_acc) and np.array_equal(sc, want_sc) and np.array_equal(acc, want)
    assert ((sc > -1) | (acc == 0).all(-1)).all() and (sc > -1).any() and not (sc > -1).all()


@pytest.mark.parametrize("size,dups", [(37, 50), (64, 0)])
def test_plain_bake_of_one_head_per_equal_size_frame_equals_the_batched_bake(static, maps, size, dups):
    _, m = maps[(size, dups)]
    images = cuda(noise((3, 96, 80, 3), 10))
    verts = cuda(np.stack([RT.head_vertices(static, 96, 80), yaw(RT.head_vertices(static, 96, 80), 30), RT.head_vertices(static, 96, 80, shift_x=30.0)]))
    normals = m.vertex_normals(verts)
    want = m.bake(verts, normals, images)
    got, flags = m.bake_frames(verts, normals, images, [0, 1, 2])
    assert torch.equal(got, want) and flags.tolist() == [0, 0, 0] and bool(want.any())
    got, _ = m.bake_frames(verts, normals, images.flip(0).contiguous(), cuda(np.asarray([2, 1, 0], np.int32)))
    assert torch.equal(got, want)


def test_accumulation_over_poses(static, faces, maps):
    td, m = maps[(64, 50)]
    base = RT.head_vertices(static, 96, 80)
    tex, score = fresh(1, 64)
    want_tex, want_sc = np.zeros((1, 64, 64, 3), np.uint8), np.full((1, 64, 64), -1.0, np.float32)
    for step, degrees in enumerate((0, 35, -35, 10), 1):
        frame = noise((96, 80, 3), 20 + step)
        v = yaw(base, degrees)
        want_tex, want_sc, _, stats = TF.expected_bake_frames(td, [frame], [v], faces, [0], want_tex, want_sc)
        st = stats[0]
        if step == 1:
            assert st["first"] == st["candidates"] > 1000 and st["replaced"] == st["kept"] == 0
        else:  # later views replace some texels, lose to the older sample on others and (while the head still turns away) fill new ones
            assert st["replaced"] > 100 and st["kept"] > 100, (step, st)
            assert (st["first"] > 100) if step < 4 else (st["first"] == 0), (step, st)
        got, sc, flags = bake(m, [frame], [v], [0], out=tex, score=score)
        assert flags.tolist() == [0]
        assert np.array_equal(sc, want_sc), step
        assert np.array_equal(got, want_tex), step
    assert ((want_sc > -1).sum() > 2000)


def test_a_tie_keeps_the_older_sample(static, faces, maps):
    td, m = maps[(64, 0)]
    v = yaw(RT.head_vertices(static, 96, 80), 15)
    first, second = noise((96, 80, 3), 30), noise((96, 80, 3), 31)
    tex, score = fresh(1, 64)
    one, sc_one, _ = bake(m, [first], [v], [0], out=tex, score=score)
    want, want_sc, _, stats = TF.expected_bake_frames(td, [second], [v], faces, [0], one, sc_one)
    assert stats[0]["kept"] == stats[0]["candidates"] > 1000 and stats[0]["replaced"] == 0  # every score ties
    two, sc_two, _ = bake(m, [second], [v], [0], out=tex, score=score)
    assert np.array_equal(two, one) and np.array_equal(sc_two, sc_one) and np.array_equal(two, want)
    plain, _, _ = bake(m, [second], [v], [0])
    assert not np.array_equal(plain, one)  # the second frame's bytes differ: only the rule kept them out


def test_flagged_heads(static, faces, maps):
    td, m = maps[(37, 50)]
    bgs = [noise((96, 80, 3), 40), noise((80, 96, 3), 41)]
    index = [0, -1, 1, 2, 0]  # the tracker's lost slot, and n_frames itself
    verts = [yaw(RT.head_vertices(static, 96, 80), 10 * k) for k in range(5)]
    want, _, want_flags, _ = TF.expected_bake_frames(td, bgs, verts, faces, index)
    assert want_flags.tolist() == [0, FLAG, 0, FLAG, 0]
    poison = torch.full((5, 37, 37, 3), 9, dtype=torch.uint8, device="cuda")
    got, _, flags = bake(m, bgs, verts, cuda(np.asarray(index, np.int32)), out=poison)
    assert flags.tolist() == want_flags.tolist()
    assert np.array_equal(got, want) and not got[1].any() and not got[3].any() and got[0].any() and got[2].any()
    # the neighbours are those of a call without the flagged heads
    alone, _, _ = bake(m, bgs, [verts[0], verts[2], verts[4]], [0, 1, 0])
    assert np.array_equal(got[[0, 2, 4]], alone)
    # accumulate: a flagged head changes no byte of its texture or score
    tex = cuda(noise((5, 37, 37, 3), 42))
    score = cuda(np.random.default_rng(43).uniform(-1, 1, (5, 37, 37)).astype(np.float32))
    tex0, score0 = tex.cpu().numpy(), score.cpu().numpy()
    want_acc, want_sc, _, stats = TF.expected_bake_frames(td, bgs, verts, faces, index, tex0, score0)
    assert stats[0]["replaced"] > 0 and stats[0]["kept"] > 0
    acc, sc, flags = bake(m, bgs, verts, index, out=tex, score=score)
    assert flags.tolist() == [0, FLAG, 0, FLAG, 0]
    assert np.array_equal(acc, want_acc) and np.array_equal(sc, want_sc)
    for k in (1, 3):
        assert np.array_equal(acc[k], tex0[k]) and np.array_equal(sc[k], score0[k])
    # without frames every head is flagged
    got, _, flags = bake(m, [], verts[:2], [0, 1])
    assert flags.tolist() == [FLAG, FLAG] and not got.any()


def test_one_nan_vertex_spoils_only_the_texels_whose_candidates_use_it(static, faces, maps):
    td, m = maps[(64, 50)]
    frame = noise((96, 80, 3), 50)
    clean = RT.head_vertices(static, 96, 80)
    vf = np.asarray(td["valid_pixel_3d_faces"])
    hit = int(vf[len(vf) // 3, 0])
    spoilt = clean.copy()
    spoilt[hit] = np.nan
    uses = (vf == hit).any(1)
    ids = np.asarray(td["valid_pixel_ids"])
    texel = (np.asarray(td["y_coords"])[ids].astype(int) % 64) * 64 + np.asarray(td["x_coords"])[ids].astype(int) % 64
    touched = np.zeros(64 * 64, bool)
    touched[texel[uses]] = True
    assert 0 < touched.sum() < 200
    with np.errstate(invalid="ignore"):
        want, _, _, _ = TF.expected_bake_frames(td, [frame], [spoilt, clean], faces, [0, 0])
    got, _, flags = bake(m, [frame], [spoilt, clean], [0, 0])
    assert flags.tolist() == [0, 0] and np.array_equal(got, want)
    differs = (want[0] != want[1]).any(-1).reshape(-1)
    assert differs.any() and not differs[~touched].any()
    # accumulate: the NaN score never replaces
    tex, score = fresh(2, 64)
    with np.errstate(invalid="ignore"):
        want_acc, want_sc, _, _ = TF.expected_bake_frames(td, [frame], [spoilt, clean], faces, [0, 0], np.zeros_like(want), np.full((2, 64, 64), -1.0, np.float32))
    acc, sc, _ = bake(m, [frame], [spoilt, clean], [0, 0], out=tex, score=score)
    assert np.array_equal(acc, want_acc) and np.array_equal(sc, want_sc) and not np.isnan(sc).any()


def test_texture_accumulator_on_predict_boxes_results(flame_model, static, faces, monkeypatch):
    from dad_3dheads_amd.predictor import FaceMeshPredictor

    pred = FaceMeshPredictor.random_init(cuda_id=0, flame_model=flame_model)
    td = synthetic.synthetic_texture_data(64, seed=0, static=static, duplicates=50)
    creator = UVTextureCreator(texture_data=td, head_mesh=pred.head_mesh, static=static)
    fr = [noise((150, 200, 3), 60), noise((180, 140, 3), 61)]
    frames = [cuda(f) for f in fr]
    boxes = cuda(np.array([[10, 20, 90, 100], [90, 30, 100, 110], [20, 40, 100, 120]], np.float64))
    res = pred.predict_boxes(frames, boxes, cuda(np.asarray([0, 0, 1], np.int32)), device_outputs=True, points_on_device=True)
    lost = [dict(r) for r in res]
    lost[1]["image_index"] = torch.full_like(res[1]["image_index"], -1)  # what the tracker reports for a lost slot
    table = DeviceFrames(frames, torch.device("cuda", 0))  # uploaded once, outside the capture
    acc = TextureAccumulator(creator, 3)
    assert acc.textures.shape == (3, 64, 64, 3) and not bool(acc.filled().any())
    acc.add(res, table)  # warm-up: the handles are built
    acc.reset()
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError("a host wait")

    with monkeypatch.context() as mp:
        for name in ("cpu", "item", "tolist", "numpy"):
            mp.setattr(torch.Tensor, name, refuse)
        mp.setattr(torch.cuda, "synchronize", refuse)
        flags = acc.add(res, table)
        filled = acc.filled()
        acc.reset(torch.tensor([1], device="cuda"))
    eager_tex, eager_sc = acc.textures.clone(), acc.score.clone()
    assert flags.tolist() == [0, 0, 0] and bool(filled.any(-1).any(-1).all())
    # reset([slot]) cleared only that slot
    assert not bool(eager_tex[1].any()) and bool((eager_sc[1] == -1).all()) and bool(eager_tex[0].any()) and bool(eager_tex[2].any())
    # against the restatement on the decoded vertices
    params = torch.cat([r["3dmm_params"].reshape(1, -1) for r in res]).float()
    verts = pred.head_mesh.flame.decode(params.clone(), proj=True, to_2d=False, mutate=False)["proj"].cpu().numpy()
    want, want_sc, _, stats = TF.expected_bake_frames(td, fr, verts, faces, [0, 0, 1], np.zeros((3, 64, 64, 3), np.uint8), np.full((3, 64, 64), -1.0, np.float32))
    assert all(st["candidates"] > 100 for st in stats)
    want[1], want_sc[1] = 0, -1.0
    assert np.array_equal(eager_tex.cpu().numpy(), want) and np.array_equal(eager_sc.cpu().numpy(), want_sc)
    # a lost slot keeps its state
    before = acc.textures.clone()
    assert acc.add(lost, table).tolist() == [0, FLAG, 0] and torch.equal(acc.textures, before)
    # one graph of `add`, replayed from reset, against the eager result
    acc.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        acc.add(res, table)
    acc.reset()
    graph.replay()
    acc.reset([1])
    torch.cuda.synchronize()
    assert torch.equal(acc.textures, eager_tex) and torch.equal(acc.score, eager_sc)
    with pytest.raises(ValueError, match="slots"):
        TextureAccumulator(creator, 2).add(res, table)
