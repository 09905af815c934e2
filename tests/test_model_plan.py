"""CPU: the host planners behind dad3d_flame_create, dad3d_flame_set_landmarks, dad3d_mesh_create, dad3d_mesh_set_texcoords and
dad3d_uvmap_create (csrc/flame_plan.hpp, csrc/mesh_plan.hpp) under AddressSanitizer and UndefinedBehaviorSanitizer. The stand-alone
program tests/model_plan_main.cpp (its own `main`, plain C++, nothing preloaded, no GPU) runs them on small inputs and writes their
outputs to files; the numpy restatement of tests/model_plan_restatement.py says what those files must hold. FLAME, texture
coordinates and UV map: exact equality. Chunk plans: their invariants."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import model_plan_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPILER = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
STATIC = ["-static-libasan", "-static-libubsan"] if COMPILER.endswith("g++") and "clang" not in COMPILER else []  # clang links them statically
pytestmark = pytest.mark.skipif(not os.path.exists(COMPILER), reason="no host C++ compiler")

LAYOUT_D = dict(shape=300, expression=100, jaw=3, rotation=6, eyeballs=0, neck=0, translation=3, scale=1)
LAYOUT_FULL = dict(LAYOUT_D, eyeballs=6, neck=3)
FLAME_TREE, JAW_CHILD_TREE = [-1, 0, 1, 1, 1], [-1, 0, 1, 2, 1]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("model_plan") / "model_plan")
    built = subprocess.run([COMPILER, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                            *STATIC, os.path.join(ROOT, "tests", "model_plan_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    return exe


def run(program, mode, directory, meta, **arrays):
    np.asarray(meta, np.int32).tofile(directory / "meta.i32")
    for name, a in arrays.items():
        np.ascontiguousarray(a).tofile(directory / name.replace("__", "."))
    ran = subprocess.run([program, mode, str(directory)], capture_output=True, text=True)
    assert ran.returncode == 0, (ran.stdout[-1000:], ran.stderr[-3000:])
    return lambda name, dtype: np.fromfile(directory / name, dtype)


@pytest.fixture(scope="module")
def model():
    """V = 45: the last tile is partial in both tilings (2 x 21 + 3, 2 x 20 + 5). A few regressor entries are exactly 0."""
    rng = np.random.default_rng(5)
    V, NB = 45, 400
    reg = rng.random((R.JOINTS, V), dtype=np.float32)
    reg[:, ::7] = 0.0
    reg[2, 3] = 0.0
    w = rng.random((V, R.JOINTS), dtype=np.float32)
    return dict(v_template=rng.standard_normal((V, 3), dtype=np.float32), shapedirs=rng.standard_normal((V, 3, NB), dtype=np.float32),
                posedirs=rng.standard_normal((36, V * 3), dtype=np.float32), j_regressor=reg, lbs_weights=w / w.sum(1, keepdims=True))


# 12 slots over 9 distinct vertices (9 <= 45 / 3), with repeats, in the first and the third tile of 20; 16 distinct vertices: too many
LISTS = [np.array([41, 3, 19, 3, 20, 44, 7, 41, 0, 12, 3, 39], np.int64), np.arange(0, 45, 3, dtype=np.int64)[:15].tolist() + [1], []]


@pytest.mark.parametrize("consts, parents", [(LAYOUT_D, FLAME_TREE), (LAYOUT_FULL, FLAME_TREE), (LAYOUT_D, JAW_CHILD_TREE)],
                         ids=["layout_D", "neck_and_eyeballs", "child_of_the_jaw"])
def test_flame_plan_is_the_restatement(program, model, tmp_path, consts, parents):
    m = dict(model, parents=parents)
    V = 45
    lists = {f"idx_{k}__i64": np.asarray(l, np.int64) for k, l in enumerate(LISTS)}
    out = run(program, "flame", tmp_path, [V, 400, *[consts[k] for k in R.SLICES], *parents, len(LISTS)],
              v_template__f32=m["v_template"], shapedirs__f32=m["shapedirs"], posedirs__f32=m["posedirs"], j_regressor__f32=m["j_regressor"],
              lbs_weights__f32=m["lbs_weights"], **lists)
    d = R.dims(m, consts)
    assert list(out("dims.i32", np.int32)) == d
    jaw_only, pipe_ok, feats, kgroups = d[14], d[15], d[16], d[19]
    assert (jaw_only, pipe_ok, feats, kgroups) == ((1, 1, 9, 26) if consts is LAYOUT_D and parents is FLAME_TREE else (0, 0, 36, 28))
    assert np.array_equal(out("bpack.f32", np.uint32), R.basis_pack(m, d).view(np.uint32))  # every fragment, to the bit
    j0, jdirs = R.joint_regressors(m)
    assert np.array_equal(out("j0.f32", np.uint32), j0.view(np.uint32))
    assert np.array_equal(out("jdirs.f32", np.uint32), jdirs.ravel().view(np.uint32))
    w8 = R.weights8(m)
    assert np.array_equal(out("w8.f32", np.uint32), w8.ravel().view(np.uint32))
    assert os.path.exists(tmp_path / "bpack_pipe.f32") == bool(pipe_ok)  # the pipelined pack is built for layout D only
    if pipe_ok:
        full = R.pipe_pack(m, d, np.arange(V))
        assert np.array_equal(out("bpack_pipe.f32", np.uint32), full.view(np.uint32))
        assert out("max_abs.f32", np.float32)[0] == np.abs(full).max()
    for k, idx in enumerate(LISTS):
        head2, nxt = R.chains(idx, V)
        assert np.array_equal(out(f"head2_{k}.i32", np.int32), head2.ravel())
        assert np.array_equal(out(f"next_{k}.i32", np.int32), nxt)
        if not pipe_ok:
            assert not os.path.exists(tmp_path / f"vtab_{k}.f32")
            continue
        vtab = R.vtab(w8, head2)
        assert np.array_equal(out(f"vtab_{k}.f32", np.uint32), vtab.ravel().view(np.uint32))
        uniq = R.sub_vertices(idx, V)
        assert list(out(f"uniq_{k}.i32", np.int32)) == uniq and (len(uniq) == 9) == (k == 0)  # lists 1 and 2: no sub-model
        assert os.path.exists(tmp_path / f"sub_pack_{k}.f32") == (k == 0)
        if uniq:
            assert out(f"sub_tiles_{k}.i32", np.int32)[0] == 1 and max(uniq) >= 40 and min(uniq) < 20  # named in two tiles, packed into one
            assert np.array_equal(out(f"sub_pack_{k}.f32", np.uint32), R.pipe_pack(m, d, uniq).view(np.uint32))
            assert np.array_equal(out(f"sub_vtab_{k}.f32", np.uint32), vtab[uniq].ravel().view(np.uint32))


def grid(n):
    """n x n vertices, two triangles per cell."""
    v = np.arange(n * n).reshape(n, n)
    a, b, c, d = v[:-1, :-1].ravel(), v[:-1, 1:].ravel(), v[1:, :-1].ravel(), v[1:, 1:].ravel()
    return np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)]).astype(np.int32), n * n


def fan(spokes):
    """A hub (the last vertex) with `spokes` triangles around it: degree above 8."""
    rim = np.arange(spokes)
    return np.stack([np.full(spokes, spokes), rim, (rim + 1) % spokes], 1).astype(np.int32), spokes + 1


# the 9 x 9 grid: 128 faces, more than 32 per chunk, so the group fill and the spill run. The 90 x 90 grid: 8100 vertices, whose staged
# copy leaves the face table room for 4099 faces: the chunkings of 1, 2 and 4 are refused, 8 (2182 faces at most) is built.
MESHES = {"grid_4x4": grid(4), "grid_9x9": grid(9), "fan_12": fan(12), "empty": (np.zeros((0, 3), np.int32), 0), "grid_90x90": grid(90)}


@pytest.mark.parametrize("name", list(MESHES))
def test_mesh_plan_keeps_its_invariants(program, tmp_path, name):
    tri, nver = MESHES[name]
    out = run(program, "mesh", tmp_path, [len(tri), nver], tri__i32=tri)
    ptr, face, adj_tri = out("ptr.i32", np.int32), out("face.i32", np.int32), out("adj_tri.i32", np.int32).reshape(-1, 4)
    # the CSR: per vertex its (face, corner) incidences in ascending face order; adj_tri: that face's corners and its index
    order = np.argsort(tri.ravel(), kind="stable")  # the (face, corner) pairs by vertex, faces ascending inside a vertex
    assert list(ptr) == list(np.concatenate([[0], np.cumsum(np.bincount(tri.ravel(), minlength=nver))]))
    assert np.array_equal(face, order // 3)
    assert np.array_equal(adj_tri[:, :3], tri[face]) and np.array_equal(adj_tri[:, 3], face)
    built = []
    for k in range(4):
        tag = f"nc{k}_"
        arrays = {"meta": out(tag + "meta.i32", np.int32)}
        if arrays["meta"][0]:
            arrays.update(face_ptr=out(tag + "face_ptr.i32", np.int32), full_groups=out(tag + "full_groups.i32", np.int32),
                          faces=out(tag + "faces.u32", np.uint32), slot=out(tag + "slot.u16", np.uint16), row8=out(tag + "row8.u32", np.uint32))
        built.append(R.check_chunk_plan(tri, nver, 1 << k, arrays, ptr, face))
    assert built == {"empty": [False] * 4, "grid_90x90": [False, False, False, True]}.get(name, [True] * 4)
    if name == "grid_9x9":
        assert out("nc0_full_groups.i32", np.int32)[0] >= 1  # the group fill ran
    if name == "fan_12":
        assert out("nc0_row8.u32", np.uint32).view(np.uint16).reshape(-1, 8)[12, 7] == 0xFFFE  # the hub: degree 12


def test_texcoord_tables_are_the_restatement(program, tmp_path):
    tri, nver = grid(4)
    rng = np.random.default_rng(9)
    tex_triangles = rng.integers(0, nver + 5, tri.shape, dtype=np.int32)
    for stride, n_tex, ok in ((3, nver + 5, True), (2, nver + 5, False)):
        directory = tmp_path / f"{stride}_{n_tex}"
        directory.mkdir()
        tex_coords = rng.random((n_tex, stride), dtype=np.float32)
        out = run(program, "tex", directory, [len(tri), n_tex, stride], tri__i32=tri, tex_coords__f32=tex_coords, tex_triangles__i32=tex_triangles)
        ref_ok, corner, ref = R.texcoords(tri, tex_coords, tex_triangles)
        assert ref_ok == ok and out("ref_ok.i32", np.int32)[0] == ok  # stride 2 has no reference indexing
        assert np.array_equal(out("corner.f32", np.uint32), corner.ravel().view(np.uint32))
        assert np.array_equal(out("ref.f32", np.uint32), ref.ravel().view(np.uint32))
    # three-float rows, but fewer rows than the mesh has vertices: no reference indexing either
    directory = tmp_path / "short"
    directory.mkdir()
    tex_coords = rng.random((nver - 1, 3), dtype=np.float32)
    out = run(program, "tex", directory, [len(tri), nver - 1, 3], tri__i32=tri, tex_coords__f32=tex_coords, tex_triangles__i32=tex_triangles % (nver - 1))
    assert out("ref_ok.i32", np.int32)[0] == 0 and R.texcoords(tri, tex_coords, tex_triangles % (nver - 1))[0] is False
    assert out("ref.f32", np.uint32).size == 0


def test_uvmap_tables_are_the_restatement(program, tmp_path):
    faces = np.array([[0, 1, 2], [2, 1, 3], [3, 4, 3], [4, 4, 0], [1, 3, 0]], np.int32)  # faces 2 and 3 name a vertex twice: one row, multiplicity 2
    nver, n_tex = 5, 16
    cand_texel = np.array([5, 2, 5, 15, 5, 0], np.int32)  # three candidates on texel 5: they must come out as 4, 2, 0
    rng = np.random.default_rng(3)
    cand_verts = rng.integers(0, nver, (len(cand_texel), 3), dtype=np.int32)
    cand_bary = rng.random((len(cand_texel), 3))
    out = run(program, "uv", tmp_path, [len(faces), nver, len(cand_texel), n_tex], faces__i32=faces, cand_texel__i32=cand_texel,
              cand_verts__i32=cand_verts, cand_bary__f64=cand_bary)
    ptr, adj = R.uv_adjacency(faces, nver)
    assert np.array_equal(out("ptr.i32", np.int32), ptr) and np.array_equal(out("adj.i32", np.int32).reshape(-1, 4), adj)
    assert [3, 4, 3, 2] in adj[ptr[3]:ptr[4]].tolist() and [4, 4, 0, 2] in adj[ptr[4]:ptr[5]].tolist()
    tptr, verts, bary = R.uv_texel_tables(cand_texel, cand_verts, cand_bary, n_tex)
    assert np.array_equal(out("tptr.i32", np.int32), tptr)
    assert np.array_equal(out("verts.i32", np.int32).reshape(-1, 3), verts) and np.array_equal(out("bary.f64", np.float64).reshape(-1, 3), bary)
    assert np.array_equal(verts[tptr[5]:tptr[6]], cand_verts[[4, 2, 0]])
