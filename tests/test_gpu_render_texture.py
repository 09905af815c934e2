"""GPU: the textured render (`render_texture_kernel` in csrc/sim3dr_kernels.hip, `Mesh.render_texture`, `Sim3DR.render_texture`,
`UVTextureCreator.render_batch`) against the reference's own `_render_texture_core` (rasterize_kernel.cpp:358-463): the goldens
recorded from the compiled reference, and the compiled reference itself where oracle/_ref holds it. Float images and depth
buffers are compared with np.array_equal throughout: the kernel is built without contraction and keeps the reference's order."""
import numpy as np
import pytest
import torch

import render_texture_ref as RT
from dad_3dheads_amd import Sim3DR, synthetic
from dad_3dheads_amd.Sim3DR import Mesh
from dad_3dheads_amd.uv_texture import UVTextureCreator, texel_coords

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not RT.ref_available(), reason="oracle/_ref/libsim3dr_ref.so (the compiled reference) is absent")
MAPPING = {0: "nearest", 1: "bilinear"}


@pytest.fixture(scope="module")
def golden():
    with np.load(RT.GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def faces(static):
    return np.ascontiguousarray(static["faces"], dtype=np.int32)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gpu_render(mesh, vertices, texture, h, w, c, mapping_type, indexing, image=None, depth=None):
    """One image or a batch ([nver,3] or [B,nver,3]) through Mesh.render_texture -> (image, depth) as numpy, float path."""
    v = np.asarray(vertices, np.float32)
    single = v.ndim == 2
    v = v[None] if single else v
    b = len(v)
    img = np.zeros((b, h, w, c), np.float32) if image is None else np.array(image, np.float32).reshape(b, h, w, c)
    dep = np.full((b, h, w), -1e8, np.float32) if depth is None else np.array(depth, np.float32).reshape(b, h, w)
    img_d, dep_d = cuda(img), cuda(dep)
    mesh.render_texture(cuda(v), cuda(texture), img_d, depth=dep_d, mapping=MAPPING[mapping_type], indexing=indexing)
    torch.cuda.synchronize()
    gi, gd = img_d.cpu().numpy(), dep_d.cpu().numpy()
    return (gi[0], gd[0]) if single else (gi, gd)


def mismatch(a, b):
    return f"{int((a != b).sum())} of {a.size} values differ, first at {np.argwhere(a != b)[:3].tolist()}"


# ---------------------------------------------------------------------------------------------------------------------
# goldens: never skipped
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("indexing", ["reference", "corner"])
def test_goldens_bit_equal(golden, faces, indexing):
    tc = golden["tex_coords"]
    mesh = Mesh(faces, len(tc), device=0)
    mesh.set_texcoords(tc if indexing == "reference" else np.ascontiguousarray(tc[:, :2]), faces)
    band = RT.band_mask(96, 96)
    band_drawn = 0
    for name in ("centre", "left"):
        for mapping in (0, 1):
            img, dep = gpu_render(mesh, golden[f"{name}_vertices"], golden["texture"], 96, 96, 3, mapping, indexing)
            want_img, want_dep = golden[f"{name}_image{mapping}"], golden[f"{name}_depth{mapping}"]
            assert np.array_equal(dep, want_dep), (name, mapping, mismatch(dep, want_dep))
            assert np.array_equal(img, want_img), (name, mapping, mismatch(img, want_img))
            band_drawn += int(((want_dep > -1e8) & band).sum())
    assert band_drawn > 0  # the shifted head pins the border-band rule


def test_depth_none_and_shared_texture_equal_the_goldens(golden, faces):
    mesh = Mesh(faces, len(golden["tex_coords"]), device=0).set_texcoords(golden["tex_coords"], faces)
    v = cuda(np.stack([golden["centre_vertices"], golden["left_vertices"]]))
    out = mesh.render_texture(v, cuda(golden["texture"]), torch.zeros((2, 96, 96, 3), device="cuda"), indexing="reference")
    assert np.array_equal(out[0].cpu().numpy(), golden["centre_image1"]) and np.array_equal(out[1].cpu().numpy(), golden["left_image1"])
    per_image = cuda(np.stack([golden["texture"], golden["texture"][::-1].copy()]))
    out2 = mesh.render_texture(v, per_image, torch.zeros((2, 96, 96, 3), device="cuda"), indexing="reference")
    assert np.array_equal(out2[0].cpu().numpy(), golden["centre_image1"])
    assert not np.array_equal(out2[1].cpu().numpy(), golden["left_image1"])  # image 1 sampled its own (flipped) texture
    alone = mesh.render_texture(v[1:], cuda(golden["texture"][::-1].copy()), torch.zeros((1, 96, 96, 3), device="cuda"), indexing="reference")
    assert torch.equal(out2[1], alone[0])


def test_sim3dr_numpy_wrapper_equals_the_goldens(golden, faces):
    for mapping in (0, 1):
        img = Sim3DR.render_texture(golden["left_vertices"], faces, golden["texture"], golden["tex_coords"], faces, 96, 96, 3, mapping)
        assert img.dtype == np.float32 and np.array_equal(img, golden[f"left_image{mapping}"])
    bg = np.full((96, 96, 3), 7.5, np.float32)
    img = Sim3DR.render_texture(golden["centre_vertices"], faces, golden["texture"], golden["tex_coords"], faces, 96, 96, bg=bg)
    drawn = golden["centre_depth1"] > -1e8
    assert np.array_equal(img[drawn], golden["centre_image1"][drawn]) and (img[~drawn] == 7.5).all() and (bg == 7.5).all()


# ---------------------------------------------------------------------------------------------------------------------
# live fuzz against the compiled reference
# ---------------------------------------------------------------------------------------------------------------------
def soup_case(seed, h, w, tex_h, tex_w, tex_c, c):
    """Random small mesh: off-screen parts, exact depth ties, duplicated, degenerate and zero-area triangles, texel coordinates
    outside the texture, tex_triangles unrelated to triangles, a background and a partly pre-filled depth buffer."""
    rng = np.random.default_rng(seed)
    nver, ntri, ntex = 120, 300, 150
    v = np.empty((nver, 3), np.float32)
    v[:, 0] = rng.uniform(-15, w + 15, nver)
    v[:, 1] = rng.uniform(-15, h + 15, nver)
    v[:, 2] = rng.integers(-2, 4, nver).astype(np.float32)  # few distinct depths: many exact ties
    v[:20, :2] = np.round(v[:20, :2])  # corners exactly on pixel centres: the >= 0 / < 1 edges of the test
    v[20:24, 0] = rng.choice([-1e4, 1e4], 4)  # far off screen
    t = rng.integers(0, nver, (ntri, 3)).astype(np.int32)
    t[:10, 1] = t[:10, 0]  # degenerate: a repeated index
    t[10:20] = t[30:40]  # duplicated triangles: equal depth everywhere, the lower index wins
    v[30] = v[31] * 0.5 + v[32] * 0.5  # a collinear triple ...
    t[20] = (31, 30, 32)  # ... as a zero-area triangle
    tc = np.zeros((ntex, 3), np.float32)
    tc[:, 0] = rng.uniform(-10, tex_w + 10, ntex)
    tc[:, 1] = rng.uniform(-10, tex_h + 10, ntex)
    tc[:, 2] = rng.uniform(-1, 1, ntex)  # never read
    tc[:15, :2] = np.round(tc[:15, :2]) + 0.5  # exact halves: round half away from zero
    tt = rng.integers(0, ntex, (ntri, 3)).astype(np.int32)
    tex = RT.smooth_texture(tex_h, tex_w, tex_c, seed)
    bg = rng.uniform(0, 255, (h, w, c)).astype(np.float32)
    depth = np.full((h, w), -1e8, np.float32)
    depth[:, : w // 4] = 2.5  # something already in front of most fragments
    depth[0, -1] = np.inf
    return dict(v=v, t=t, tc=tc, tt=tt, tex=tex, bg=bg, depth=depth, h=h, w=w, c=c)


def head_case(static, faces, seed, h, w, tex_h, tex_w, tex_c, c, shift_x, shift_y):
    rng = np.random.default_rng(seed)
    v = RT.head_vertices(static, h, w, shift_x=shift_x, fill=rng.uniform(0.6, 1.3))
    v[:, 1] += shift_y
    tc = np.zeros((len(v), 3), np.float32)
    tc[:, :2] = texel_coords(synthetic.synthetic_texcoords(256, static)["vt"], 256) * [tex_w / 256.0, tex_h / 256.0]
    tt = np.roll(faces, 17 * (seed % 5), axis=0) if seed % 2 else faces  # other texture triangles than mesh triangles
    return dict(v=v, t=faces, tc=tc, tt=np.ascontiguousarray(tt), tex=RT.smooth_texture(tex_h, tex_w, tex_c, seed), bg=None, depth=None, h=h, w=w, c=c)


def fuzz_cases(static, faces):
    cases = []
    for seed, (h, w, th, tw, tcn, c) in enumerate([(48, 64, 16, 24, 3, 3), (64, 48, 33, 9, 4, 1), (70, 130, 8, 8, 1, 1), (5, 200, 40, 7, 5, 3),
                                                   (96, 96, 64, 64, 3, 3), (129, 65, 20, 31, 4, 3)]):
        cases.append((f"soup{seed}", soup_case(100 + seed, h, w, th, tw, tcn, c)))
    for seed, (h, w, th, tw, tcn, c, sx, sy) in enumerate([(96, 96, 64, 64, 3, 3, 0, 0), (96, 128, 32, 48, 3, 3, -70, 10), (150, 100, 64, 40, 4, 3, 40, -60),
                                                           (200, 256, 256, 256, 3, 1, 130, 90), (64, 64, 17, 17, 3, 3, 0, 30)]):
        cases.append((f"head{seed}", head_case(static, faces, seed, h, w, th, tw, tcn, c, sx, sy)))
    return cases


@needs_ref
def test_live_fuzz_against_the_compiled_reference(static, faces):
    head_mesh = Mesh(faces, 5023, device=0)
    drawn_total = band_total = 0
    for name, k in fuzz_cases(static, faces):
        mesh = head_mesh if name.startswith("head") else Mesh(k["t"], len(k["v"]), device=0)
        mesh.set_texcoords(k["tc"], k["tt"])
        for mapping in (0, 1):
            want_img, want_dep = RT.ref_render(k["v"], k["t"], k["tex"], k["tc"], k["tt"], k["h"], k["w"], k["c"], mapping, image=k["bg"], depth=k["depth"])
            img, dep = gpu_render(mesh, k["v"], k["tex"], k["h"], k["w"], k["c"], mapping, "reference", image=k["bg"], depth=k["depth"])
            assert np.array_equal(dep, want_dep), (name, mapping, mismatch(dep, want_dep))
            assert np.array_equal(img, want_img), (name, mapping, mismatch(img, want_img))
            start = np.full_like(want_dep, -1e8) if k["depth"] is None else k["depth"]
            drawn_total += int((want_dep != start).sum())
            band_total += int(((want_dep != start) & RT.band_mask(k["h"], k["w"])).sum())
    assert drawn_total > 20000 and band_total > 500, (drawn_total, band_total)  # the cases do draw, band pixels included


@needs_ref
def test_corner_indexing_equals_the_reference_on_the_unrolled_mesh(static, faces):
    lay = synthetic.synthetic_texcoords(64, static)
    tc2 = texel_coords(lay["vt"], 64).astype(np.float32)
    # a layout with seams: every face gets corners of its own, some faces shifted as a seam duplicate would be
    rng = np.random.default_rng(8)
    corners = tc2[faces.reshape(-1)].copy()
    moved = rng.random(len(faces)) < 0.2
    corners.reshape(-1, 3, 2)[moved] += rng.uniform(-20, 20, (int(moved.sum()), 1, 2)).astype(np.float32)
    tt = np.arange(3 * len(faces), dtype=np.int32).reshape(-1, 3)
    mesh = Mesh(faces, 5023, device=0).set_texcoords(corners, tt)
    tex = RT.smooth_texture(64, 64, 3, 4)
    for shift in (0.0, -45.0):
        v = RT.head_vertices(static, 96, 96, shift_x=shift)
        uv, ut, utc, utt = RT.unrolled(v, faces, corners, tt)
        for mapping in (0, 1):
            want_img, want_dep = RT.ref_render(uv, ut, tex, utc, utt, 96, 96, 3, mapping)
            img, dep = gpu_render(mesh, v, tex, 96, 96, 3, mapping, "corner")
            assert np.array_equal(dep, want_dep) and np.array_equal(img, want_img), (shift, mapping, mismatch(img, want_img))
    with pytest.raises(Exception, match="reference indexing"):  # 2-column coordinates carry no reference layout
        mesh.render_texture(cuda(v[None]), cuda(tex), torch.zeros((1, 96, 96, 3), device="cuda"), indexing="reference")


# ---------------------------------------------------------------------------------------------------------------------
# dtypes, batches, non-finite input
# ---------------------------------------------------------------------------------------------------------------------
def test_uint8_paths_equal_the_float_image_cast(golden, faces):
    mesh = Mesh(faces, len(golden["tex_coords"]), device=0).set_texcoords(golden["tex_coords"], faces)
    rng = np.random.default_rng(2)
    tex_u8 = rng.integers(0, 256, (64, 64, 3)).astype(np.uint8)
    bg = rng.integers(0, 256, (1, 96, 96, 3)).astype(np.uint8)
    v = cuda(golden["left_vertices"][None])
    for tex in (golden["texture"], tex_u8):
        for mapping in (0, 1):
            flt, dep = gpu_render(mesh, golden["left_vertices"], tex.astype(np.float32), 96, 96, 3, mapping, "reference")
            drawn = dep > -1e8
            got = mesh.render_texture(v, cuda(tex), cuda(bg), mapping=MAPPING[mapping], indexing="reference")[0].cpu().numpy()
            assert got.dtype == np.uint8
            assert np.array_equal(got[drawn], flt.astype(np.uint8)[drawn]) and np.array_equal(got[~drawn], bg[0][~drawn])
            # uint8 texture into a float image: the widened texels, same arithmetic
            flt2 = mesh.render_texture(v, cuda(tex), torch.zeros((1, 96, 96, 3), device="cuda"), mapping=MAPPING[mapping], indexing="reference")
            assert np.array_equal(flt2[0].cpu().numpy(), flt)


def test_batch_equals_images_one_by_one(static, faces, golden):
    mesh = Mesh(faces, 5023, device=0).set_texcoords(golden["tex_coords"], faces)
    rng = np.random.default_rng(6)
    b, h, w = 7, 80, 112
    v = np.stack([RT.head_vertices(static, h, w, shift_x=rng.uniform(-60, 60), fill=rng.uniform(0.5, 1.4)) for _ in range(b)])
    tex = rng.integers(0, 256, (b, 64, 64, 3)).astype(np.uint8)
    bg = rng.integers(0, 256, (b, h, w, 3)).astype(np.uint8)
    dep0 = np.full((b, h, w), -1e8, np.float32)
    dep0[:, :, w // 2:] = 0.0
    img_d, dep_d = cuda(bg), cuda(dep0)
    mesh.render_texture(cuda(v), cuda(tex), img_d, depth=dep_d)
    for i in range(b):
        img_i, dep_i = cuda(bg[i:i + 1]), cuda(dep0[i:i + 1])
        mesh.render_texture(cuda(v[i:i + 1]), cuda(tex[i:i + 1]), img_i, depth=dep_i)
        assert torch.equal(img_d[i], img_i[0]) and torch.equal(dep_d[i], dep_i[0]), i
    assert not torch.equal(img_d, cuda(bg))


def test_non_finite_image_leaves_the_others_alone(static, faces, golden):
    tc = golden["tex_coords"].copy()
    rng = np.random.default_rng(7)
    b, h, w = 4, 96, 96
    v = np.stack([RT.head_vertices(static, h, w, shift_x=s) for s in (0.0, -40.0, 25.0, 50.0)])
    tex = cuda(rng.integers(0, 256, (b, 64, 64, 3)).astype(np.uint8))
    clean_mesh = Mesh(faces, 5023, device=0).set_texcoords(tc, faces)
    clean = clean_mesh.render_texture(cuda(v), tex, torch.zeros((b, h, w, 3), dtype=torch.uint8, device="cuda"))
    # image 2: NaN and infinite vertices; NaN / infinite texel coordinates for every image (they are static per mesh)
    bad_v = v.copy()
    bad_v[2, ::7] = np.nan
    bad_v[2, 3::11, 0] = np.inf
    got = clean_mesh.render_texture(cuda(bad_v), tex, torch.zeros((b, h, w, 3), dtype=torch.uint8, device="cuda"))
    for i in (0, 1, 3):
        assert torch.equal(got[i], clean[i]), i
    bad_tc = tc.copy()
    bad_tc[::5, :2] = np.nan
    bad_tc[1::9, 0] = np.inf
    bad_tc[2::9, 1] = -np.inf
    bad_mesh = Mesh(faces, 5023, device=0).set_texcoords(bad_tc, faces)
    dep_bad, dep_clean = (torch.full((b, h, w), -1e8, device="cuda") for _ in range(2))
    bad_mesh.render_texture(cuda(v), tex, torch.zeros((b, h, w, 3), device="cuda"), depth=dep_bad)  # must not fault: indices are clamped
    clean_mesh.render_texture(cuda(v), tex, torch.zeros((b, h, w, 3), device="cuda"), depth=dep_clean)
    torch.cuda.synchronize()
    assert torch.equal(dep_bad, dep_clean)  # coverage and depth do not depend on the texture coordinates


# ---------------------------------------------------------------------------------------------------------------------
# UVTextureCreator.render_batch
# ---------------------------------------------------------------------------------------------------------------------
def test_render_batch_end_to_end_and_graph_replay(static, flame_model):
    atlas = dict(synthetic.synthetic_texture_data(256, seed=0, static=static))
    atlas.update(synthetic.synthetic_texcoords(256, static))
    creator = UVTextureCreator(texture_data=atlas, flame_model=flame_model, static=static, device=0)
    b, size = 5, (256, 256)
    params = torch.from_numpy(synthetic.synthetic_params(b, seed=21)).cuda()
    rng = np.random.default_rng(3)
    textures = cuda(rng.integers(0, 256, (b, 256, 256, 3)).astype(np.uint8))
    got = creator.render_batch(params, textures, size=size)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (b, 256, 256, 3)
    assert (got.reshape(b, -1).amax(1) > 0).all()

    # the same vertices through the mesh entry, and through the compiled reference when it is there
    verts = creator.head_mesh.flame.decode(params, proj=True, to_2d=False, flip_z=True)["proj"]
    mesh = creator.renderer
    kept = (atlas["ft"] >= 0).all(1)
    assert mesh.ntri == int(kept.sum()) and 0 < int((~kept).sum()) <= 0.01 * len(kept)
    direct = mesh.render_texture(verts, textures, torch.zeros((b, 256, 256, 3), dtype=torch.uint8, device="cuda"))
    assert torch.equal(got, direct)
    if RT.ref_available():
        faces_kept = np.ascontiguousarray(static["faces"][kept], dtype=np.int32)
        tc2 = texel_coords(atlas["vt"], 256).astype(np.float32)
        ft = np.ascontiguousarray(atlas["ft"][kept], dtype=np.int32)
        for i in range(b):
            uv, ut, utc, utt = RT.unrolled(verts[i].cpu().numpy(), faces_kept, tc2, ft)
            want, dep = RT.ref_render(uv, ut, textures[i].cpu().numpy().astype(np.float32), utc, utt, 256, 256, 3, 1)
            drawn = dep > -1e8
            g = got[i].cpu().numpy()
            assert np.array_equal(g[drawn], want.astype(np.uint8)[drawn]) and (g[~drawn] == 0).all(), i

    # replay from a captured graph: same bytes, and new inputs in the same buffers are picked up
    creator.reserve_render(b, size)
    out = torch.zeros((b, 256, 256, 3), dtype=torch.uint8, device="cuda")
    static_params = params.clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        creator.render_batch(static_params, textures, out=out, mutate=False)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    out.zero_()
    with torch.cuda.graph(graph):
        creator.render_batch(static_params, textures, out=out, mutate=False)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, got)
    params2 = torch.from_numpy(synthetic.synthetic_params(b, seed=22)).cuda()
    want2 = creator.render_batch(params2.clone(), textures, size=size)
    static_params.copy_(params2)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want2) and not torch.equal(out, got)
