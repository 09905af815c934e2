"""What the host planners (csrc/flame_plan.hpp, csrc/mesh_plan.hpp) must produce, restated in numpy from the layouts the kernels read
(csrc/common.hpp: DecodeArgs, PipeArgs, MeshDev, NormalChunksDev; csrc/uv_texture.hpp), not from the planners' loops. Shared by
tests/test_model_plan.py; every FLAME quantity is exact, the chunk plans are checked through their invariants (`check_chunk_plan`).

FLAME
  * A basis pack is [tile][group of 16 k][wave][lane][4 MFMA steps] float32: lane (q = lane >> 4, n = lane & 15) of wave w holds, for step
    s, basis row k = 16 g + 4 q + s of column 16 w + n. Rows: the betas' directions, the pose features in use (all 36, or the jaw's 9
    starting at feature 9), then the template; zero above. Columns of the two-role pack: 21 vertices x 3 components, one zero. Columns of
    the pipelined pack: 20 vertices x 3, then the jaw joint's three (its beta directions, and its rest position in the template row),
    one zero.
  * j0 / jdirs: for joint j and component c the float64 sum over the vertices, in ascending order and without the regressor entries that
    are 0, of regressor x template and regressor x direction, each sum rounded to float32 once.
  * w8: w0..w4, ((w0 + w1) + w3) + w4 in float32, 0, 0. vtab: {w8[5] + w2, w2, bits of the first slot, bits of the slot after it}.
  * chains: head2[v] = the first two slots that name v, next[s] = the next slot that names idx[s]; -1 where there is none.
  * the sub-model: the pipelined pack of the distinct named vertices, ascending, as if they were the whole mesh; none when they are more
    than a third of it.
"""
import numpy as np

JOINTS, TILE, PIPE_TILE, PIPE_KGROUPS = 5, 21, 20, 26
SLICES = ("shape", "expression", "jaw", "rotation", "eyeballs", "neck", "translation", "scale")


def layout(consts):
    """dims.i32's first 14 words: n_params, then offset (and size, where the kernels need it) in `FlameParams.from_3dmm` order."""
    off, cur = {}, 0
    for k in SLICES:
        off[k] = cur
        cur += consts[k]
    return [cur, off["shape"], consts["shape"], off["expression"], consts["expression"], off["jaw"], consts["jaw"], off["rotation"],
            off["eyeballs"], consts["eyeballs"], off["neck"], consts["neck"], off["translation"], off["scale"]]


def dims(model, consts):
    V, NB = model["v_template"].shape[0], model["shapedirs"].shape[2]
    jaw_only = consts["neck"] == 0 and consts["eyeballs"] == 0 and 2 not in list(model["parents"][1:])
    feats, first = (9, 9) if jaw_only else (36, 0)
    k_used = NB + feats + 1
    kgroups = -(-k_used // 16)
    lay = layout(consts)
    pipe_ok = jaw_only and [consts[k] for k in SLICES] == [300, 100, 3, 6, 0, 0, 3, 1] and kgroups == PIPE_KGROUPS
    return lay + [int(jaw_only), int(pipe_ok), feats, first, k_used, kgroups, -(-V // TILE), -(-V // PIPE_TILE)]


def _rows(model, feats, first, verts):
    """[k_used][len(verts)][3]: the basis rows of the listed vertices."""
    V = model["v_template"].shape[0]
    pose = model["posedirs"].reshape(36, V, 3)[first:first + feats]
    return np.concatenate([model["shapedirs"][verts].transpose(2, 0, 1), pose[:, verts], model["v_template"][verts][None]], axis=0)


def _fragment_order(cols, kgroups):
    """cols [k][tile][64] -> the pack, flat."""
    k, tiles, _ = cols.shape
    full = np.zeros((kgroups * 16, tiles, 64), np.float32)
    full[:k] = cols
    # k = 16 g + 4 q + s, column = 16 w + n  ->  [tile][g][w][q][n][s]
    return full.reshape(kgroups, 4, 4, tiles, 4, 16).transpose(3, 0, 4, 1, 5, 2).ravel()


def basis_pack(model, d):
    feats, first, k_used, kgroups, tiles = d[16], d[17], d[18], d[19], d[20]
    V = model["v_template"].shape[0]
    cols = np.zeros((k_used, tiles * TILE, 3), np.float32)
    cols[:, :V] = _rows(model, feats, first, np.arange(V))
    cols = np.concatenate([cols.reshape(k_used, tiles, TILE * 3), np.zeros((k_used, tiles, 1), np.float32)], axis=2)
    return _fragment_order(cols, kgroups)


def joint_regressors(model):
    V, NB = model["v_template"].shape[0], model["shapedirs"].shape[2]
    acc = np.zeros((JOINTS, 3, NB + 1), np.float64)
    x = np.concatenate([model["shapedirs"], model["v_template"][:, :, None]], axis=2).astype(np.float64)  # [V][3][NB + 1]
    for j in range(JOINTS):
        for v in range(V):
            r = np.float64(model["j_regressor"][j, v])
            if r != 0.0:
                acc[j] += r * x[v]
    acc = acc.astype(np.float32)
    return acc[:, :, NB].ravel(), acc[:, :, :NB].reshape(JOINTS * 3, NB)


def pipe_pack(model, d, verts):
    """The pipelined pack of the vertices `verts` (all of them: the model's; the named ones: the sub-model's)."""
    feats, first, k_used = d[16], d[17], d[18]
    NB = model["shapedirs"].shape[2]
    j0, jdirs = joint_regressors(model)
    n, tiles = len(verts), -(-len(verts) // PIPE_TILE)
    cols = np.zeros((k_used, tiles * PIPE_TILE, 3), np.float32)
    cols[:, :n] = _rows(model, feats, first, np.asarray(verts, np.int64))
    jaw = np.zeros((k_used, 3), np.float32)
    jaw[:NB] = jdirs[6:9].T
    jaw[NB + feats] = j0[6:9]
    cols = np.concatenate([cols.reshape(k_used, tiles, PIPE_TILE * 3), np.broadcast_to(jaw[:, None, :], (k_used, tiles, 3)),
                           np.zeros((k_used, tiles, 1), np.float32)], axis=2)
    return _fragment_order(cols, PIPE_KGROUPS)


def weights8(model):
    w = model["lbs_weights"]
    w8 = np.zeros((w.shape[0], 8), np.float32)
    w8[:, :5] = w
    w8[:, 5] = ((w[:, 0] + w[:, 1]) + w[:, 3]) + w[:, 4]
    return w8


def chains(idx, V):
    idx = [int(i) for i in idx]
    head2, nxt = np.full((V, 2), -1, np.int32), np.full(len(idx), -1, np.int32)
    for v in range(V):
        slots = [s for s, i in enumerate(idx) if i == v]
        head2[v, :len(slots[:2])] = slots[:2]
        for a, b in zip(slots, slots[1:]):
            nxt[a] = b
    return head2, nxt


def vtab(w8, head2):
    t = np.zeros((w8.shape[0], 4), np.float32)
    t[:, 0], t[:, 1] = w8[:, 5] + w8[:, 2], w8[:, 2]
    t[:, 2:] = head2.view(np.float32)
    return t


def sub_vertices(idx, V):
    uniq = sorted({int(i) for i in idx})
    return uniq if 3 * len(uniq) <= V else []


def table_lds_bytes(nver, max_faces):
    """The normals' face table in LDS: the staged vertices (3 floats each and 8 more, in whole float4s), then a float4 per face."""
    return (((nver * 3 + 8 + 3) & ~3) + 4 * max_faces) * 4


def check_chunk_plan(tri, nver, chunks, out, ptr, face):
    """The invariants of one chunking's plan. `out`: the planner's arrays by name (meta = built, chunks, vpb, max_faces); ptr / face: the
    mesh's vertex -> face CSR. The order inside a chunk list is a heuristic's and free; what the normals' bits rest on is not."""
    ntri = len(tri)
    vpb = -(-nver // chunks) if nver else 0
    lists = [sorted({f for f in range(ntri) if any(v // vpb == ch for v in tri[f])}) for ch in range(chunks)] if ntri and nver else []
    max_faces = max((len(l) for l in lists), default=0)
    refused = not (0 < nver <= 65535 and ntri > 0) or max_faces >= 0xFFFE or table_lds_bytes(nver, max_faces) > 160 * 1024 - 1024
    assert bool(out["meta"][0]) == (not refused), (chunks, max_faces)
    if refused:
        return False
    assert list(out["meta"][1:]) == [chunks, vpb, max_faces]
    face_ptr, faces, slot = out["face_ptr"], out["faces"].reshape(-1, 2), out["slot"]
    assert list(face_ptr) == list(np.concatenate([[0], np.cumsum([len(l) for l in lists])]))  # the running sum
    corners = np.stack([faces[:, 0] & 0xFFFF, faces[:, 0] >> 16, faces[:, 1]], axis=1).astype(np.int64)
    key = {tuple(t): f for f, t in enumerate(tri.tolist())}  # the meshes of the test repeat no face
    for ch in range(chunks):
        part = corners[face_ptr[ch]:face_ptr[ch + 1]]
        assert sorted(key[tuple(c)] for c in part.tolist()) == lists[ch]  # exactly the faces touching the chunk, once
        for g in range(out["full_groups"][ch]):  # a group counted as full: 32 faces on 32 banks for each corner
            assert all(len(set(part[32 * g:32 * g + 32, c] % 32)) == 32 for c in range(3)), (ch, g)
        assert 32 * out["full_groups"][ch] <= len(part)
    row8 = out["row8"].view(np.uint16).reshape(nver, 8)
    for v in range(nver):
        ch, row = v // vpb, slot[ptr[v]:ptr[v + 1]]
        named = [key[tuple(corners[face_ptr[ch] + s].tolist())] for s in row]
        assert named == list(face[ptr[v]:ptr[v + 1]]) and named == sorted(named)  # the summation order: ascending faces
        want = [int(s) for s in row[:8]] + [0xFFFF] * (8 - min(len(row), 8))
        if len(row) > 8:
            want[7] = 0xFFFE
        assert list(row8[v]) == want, v
    return True


def uv_adjacency(faces, nver):
    """ptr [nver + 1], adj [][4]: per vertex its faces ascending, each once, as (v0, v1, v2, times the face names the vertex)."""
    rows = [[] for _ in range(nver)]
    for t in faces.tolist():
        for v in sorted(set(t)):
            rows[v].append(t + [t.count(v)])
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return ptr, np.array([e for r in rows for e in r], np.int32).reshape(-1, 4)


def uv_texel_tables(cand_texel, cand_verts, cand_bary, n_tex):
    """tptr [n_tex + 1], then the candidates of texel after texel, the highest candidate index first."""
    order = sorted(range(len(cand_texel)), key=lambda i: (cand_texel[i], -i))
    tptr = np.concatenate([[0], np.cumsum(np.bincount(cand_texel, minlength=n_tex))]).astype(np.int32)
    return tptr, cand_verts[order], cand_bary[order]


def texcoords(tri, tex_coords, tex_triangles):
    """ref_ok, corner [ntri][8], ref [ntri][8]: x0 y0 x1 y1 | x2 y2 0 0, y of `ref` from the row of the MESH index (three-float rows only)."""
    n_tex, stride = tex_coords.shape
    ref_ok = stride == 3 and (tri.size == 0 or int(tri.max()) < n_tex)
    def table(y_rows):
        t = np.zeros((len(tri), 8), np.float32)
        t[:, 0:6:2], t[:, 1:6:2] = tex_coords[tex_triangles, 0], tex_coords[y_rows, 1]
        return t
    return ref_ok, table(tex_triangles), table(tri) if ref_ok else np.zeros((0, 8), np.float32)
