"""GPU: the UV-texture bake (csrc/uv_texture.hip, dad-3dheads_amd/uv_texture.py) against the reference's own
`_compute_texture_map` (tests/golden/uv_texture_golden.npz) and the float64 restatement (tests/uv_texture_restatement.py):
normals bit-equal, textures byte-equal on identical vertices; end to end against the CPU oracle's decode."""
import os

import numpy as np
import pytest
import torch

import uv_texture_restatement as R
from dad_3dheads_amd import synthetic, writers
from dad_3dheads_amd.uv_texture import UVMap, UVTextureCreator
from oracle import flame_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


@pytest.fixture(scope="module")
def photo():
    with np.load(os.path.join(R.ROOT, "tests", "golden", "demo_image.npz")) as z:
        return z["resized"]


@pytest.fixture(scope="module")
def atlas(static):
    return synthetic.synthetic_texture_data(256, seed=0, static=static)


@pytest.fixture(scope="module")
def creator(atlas, flame_model, static):
    return UVTextureCreator(texture_data=atlas, flame_model=flame_model, static=static, device=0)


def adversarial_atlas(g):
    return {"x_coords": g["adv_x_coords"], "y_coords": g["adv_y_coords"], "valid_pixel_ids": g["adv_valid_pixel_ids"],
            "valid_pixel_3d_faces": g["adv_valid_pixel_3d_faces"], "valid_pixel_b_coords": g["adv_valid_pixel_b_coords"],
            "img_size": int(g["adv_img_size"])}


def restated(td, images, verts, faces, hw=None):
    out = []
    with np.errstate(invalid="ignore"):
        for i in range(len(verts)):
            img = images[i] if hw is None else images[i][:hw[i][0], :hw[i][1]]
            out.append(R.compute_texture_map(td, img, verts[i], faces))
    return np.stack(out)


def test_vertex_normals_bit_equal(golden, static, atlas):
    faces = static["faces"]
    m = UVMap(faces, 5023, atlas, device=0)
    rng = np.random.default_rng(5)
    for b in (1, 4, 19):
        v = golden["verts"][rng.integers(0, 4, b)].copy()
        v += rng.normal(0, 3.0, v.shape).astype(np.float32)  # every mesh of the batch different
        got = m.vertex_normals(torch.from_numpy(v).cuda()).cpu().numpy()
        assert got.dtype == np.float64
        for i in range(b):
            assert np.array_equal(got[i], R.vertex_normals(v[i], faces)), (b, i)
    adv = UVMap(golden["adv_faces"], len(golden["adv_verts"]), adversarial_atlas(golden), device=0)
    v = golden["adv_verts"]
    got = adv.vertex_normals(torch.from_numpy(np.stack([v, v])).cuda()).cpu().numpy()
    with np.errstate(invalid="ignore"):
        want = R.vertex_normals(v, golden["adv_faces"])
    assert np.array_equal(got[0], want, equal_nan=True) and np.array_equal(got[1], want, equal_nan=True)
    real = ~np.isnan(want)  # a NaN's sign bit carries no meaning (x86 and gfx950 produce different ones); signed zeros do
    assert np.array_equal(np.signbit(got[0])[real], np.signbit(want)[real])


def test_bake_equals_reference_on_golden_vertices(golden, static, photo):
    maps = {}
    for i in range(len(golden["verts"])):
        key = (int(golden["atlas_size"][i]), int(golden["atlas_seed"][i]), int(golden["atlas_duplicates"][i]))
        if key not in maps:
            td = synthetic.synthetic_texture_data(key[0], seed=key[1], static=static, duplicates=key[2])
            assert synthetic.texture_data_digest(td) == str(golden["atlas_sha256"][i])
            maps[key] = UVMap(static["faces"], 5023, td, device=0)
        m = maps[key]
        v = torch.from_numpy(golden["verts"][i][None]).cuda()
        tex = m.bake(v, m.vertex_normals(v), torch.from_numpy(photo[None]).cuda())
        assert np.array_equal(tex[0].cpu().numpy(), golden["textures"][i]), i
    h, w = (int(x) for x in golden["adv_crop_hw"])
    adv = UVMap(golden["adv_faces"], len(golden["adv_verts"]), adversarial_atlas(golden), device=0)
    v = torch.from_numpy(golden["adv_verts"][None]).cuda()
    crop = torch.from_numpy(np.ascontiguousarray(photo[None, :h, :w])).cuda()
    tex = adv.bake(v, adv.vertex_normals(v), crop)
    assert np.array_equal(tex[0].cpu().numpy(), golden["adv_texture"])
    # the same crop as a (h, w) bound inside the whole photo
    tex = adv.bake(v, adv.vertex_normals(v), torch.from_numpy(photo[None]).cuda(),
                   hw=torch.tensor([[h, w]], dtype=torch.int32, device="cuda"))
    assert np.array_equal(tex[0].cpu().numpy(), golden["adv_texture"])


@pytest.mark.parametrize("size,batch,dups", [(512, 3, 0), (37, 5, 300), (256, 1, 0), (256, 64, 2000)])
def test_bake_shapes_against_restatement(creator, static, size, batch, dups):
    td = synthetic.synthetic_texture_data(size, seed=size, static=static, duplicates=dups)
    m = UVMap(static["faces"], 5023, td, device=0)
    rng = np.random.default_rng(size + batch)
    params = torch.from_numpy(synthetic.synthetic_params(batch, seed=size + batch)).cuda()
    v = creator.head_mesh.flame.decode(params, proj=True, to_2d=False, mutate=True)["proj"]
    images = rng.integers(0, 256, (batch, 240, 230, 3), dtype=np.uint8)
    tex = m.bake(v, m.vertex_normals(v), torch.from_numpy(images).cuda()).cpu().numpy()
    want = restated(td, images, v.cpu().numpy(), static["faces"])
    assert tex.shape == (batch, size, size, 3)
    assert np.array_equal(tex, want)
    assert tex.reshape(batch, -1).any(1).all()


def test_ragged_batch_bounds(creator, static, atlas):
    hw = np.array([[256, 206], [300, 260], [200, 180], [1, 1], [290, 100], [0, 0]], np.int32)
    b = len(hw)
    rng = np.random.default_rng(9)
    images = rng.integers(0, 256, (b, 300, 260, 3), dtype=np.uint8)
    params = torch.from_numpy(synthetic.synthetic_params(b, seed=41)).cuda()
    tex = creator.bake_batch(params, torch.from_numpy(images).cuda(), hw=torch.from_numpy(hw).cuda()).cpu().numpy()
    v = creator.head_mesh.flame.decode(params, proj=True, to_2d=False)["proj"].cpu().numpy()
    assert np.array_equal(tex, restated(atlas, images, v, static["faces"], hw=hw))
    assert not tex[3].any() and not tex[5].any()


def test_single_image_call_equals_batch_row(creator):
    params = torch.from_numpy(synthetic.synthetic_params(4, seed=23))
    rng = np.random.default_rng(3)
    images = rng.integers(0, 256, (4, 256, 256, 3), dtype=np.uint8)
    batch = creator.bake_batch(params.clone().cuda(), torch.from_numpy(images).cuda()).cpu().numpy()
    for i in range(4):
        row = params[i:i + 1].clone()
        assert row[0, 411] != 0
        single = creator(images[i], {"3dmm_params": row})
        assert single.dtype == np.uint8 and single.shape == (256, 256, 3)
        assert np.array_equal(single, batch[i]), i
        assert row[0, 411] == 0  # head_mesh.py:41, replayed on the caller's CPU tensor
        assert np.array_equal(writers.get_uv_texture({"3dmm_params": params[i:i + 1].clone()}, images[i], creator), batch[i])
    mesh = creator.get_mesh({"3dmm_params": params[:1].clone()})
    assert mesh.v.dtype == np.float64 and mesh.v.shape == (5023, 3) and mesh.f.shape == (9976, 3)
    with pytest.raises(ValueError):
        creator(images[0].astype(np.float32), {"3dmm_params": params[:1].clone()})


def test_end_to_end_against_oracle(creator, flame_consts, static, atlas, photo):
    """GPU decode + bake against the CPU oracle's decode + the restatement. The decodes differ by ~1e-4 px, so a few texels
    may legitimately differ: every one must be explained by a float64 arbiter on its winning candidate (either side)."""
    b = 8
    params = synthetic.synthetic_params(b, seed=61)
    images = np.broadcast_to(photo, (b,) + photo.shape).copy()
    tex = creator.bake_batch(torch.from_numpy(params).cuda(), torch.from_numpy(images).cuda()).cpu().numpy()
    v_gpu = creator.head_mesh.flame.decode(torch.from_numpy(params).cuda(), proj=True, to_2d=False)["proj"].cpu().numpy()
    v_ref = flame_ref.reprojected_vertices(flame_consts, torch.from_numpy(params), to_2d=False).numpy()
    faces = static["faces"]
    h, w = photo.shape[:2]
    n_diff = n_written = 0
    unexplained = []
    for i in range(b):
        want = R.compute_texture_map(atlas, photo, v_ref[i], faces)
        diff = np.flatnonzero((tex[i] != want).any(-1).reshape(-1))
        n_written += int(want.any(-1).sum())
        if not len(diff):
            continue
        n_diff += len(diff)
        wins = [R.winning_candidates(atlas, photo, v, faces) for v in (v_gpu[i], v_ref[i])]
        for t in diff:
            explained, closest = False, []
            for win, _, _, _ in wins:
                c = win[t]
                if c < 0:
                    continue
                for _, p, ndv, _ in wins:
                    xy = p[c, :2]
                    d_half = float(np.abs(xy - np.floor(xy) - 0.5).min())
                    d_bound = float(min(np.abs(xy - 0.5).min(), np.abs(xy - np.array([w - 0.5, h - 0.5])).min()))
                    explained |= d_half < 2e-3 or d_bound < 2e-3 or abs(ndv[c]) < 1e-5
                    closest.append((int(c), d_half, float(ndv[c])))
            if not explained:
                unexplained.append((i, int(t), closest))
    print(f"end to end: {n_diff} of {n_written} written texels differ from the oracle chain, "
          f"{n_diff - len(unexplained)} explained by the arbiter")
    assert not unexplained, unexplained[:10]


def test_graph_capture_on_side_stream(creator):
    b = 16
    rng = np.random.default_rng(4)
    images = torch.from_numpy(rng.integers(0, 256, (b, 256, 240, 3), dtype=np.uint8)).cuda()
    p = torch.from_numpy(synthetic.synthetic_params(b, seed=70)).cuda()
    out = torch.empty((b, 256, 256, 3), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    creator.reserve(b)
    with torch.cuda.stream(side):
        creator.bake_batch(p.clone(), images, out=out)  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        creator.bake_batch(p, images, out=out)
    for seed in (71, 72):
        new = torch.from_numpy(synthetic.synthetic_params(b, seed=seed)).cuda()
        p.copy_(new)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got = out.clone()
        assert p[:, 411].abs().max() == 0
        with torch.cuda.stream(side):
            eager = creator.bake_batch(new.clone(), images)
        torch.cuda.synchronize()
        assert torch.equal(got, eager) and got.any()
