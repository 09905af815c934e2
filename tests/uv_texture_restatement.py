"""Float64 NumPy restatement of the reference demo's UV-texture bake (inference/uv_texture.py `UVTextureCreator`, steps 2-3:
`Mesh(v, f)` and `_compute_texture_map`) that the UV-texture tests check the golden and the GPU path against. Independent of
dad-3dheads_amd/uv_texture.py: only the packaged face list and the synthetic atlas are shared (data).

`RestatedMesh.estimate_vertex_normals` is psbody-mesh's `Mesh.estimate_vertex_normals` restated from its published source
(psbody is not installed anywhere this project runs: unpinned here):

    face_normals = TriNormalsScaled(v, f)               # cross(v[f1] - v[f0], v[f2] - v[f0]) per face
    ftov = faces_by_vertex(as_sparse_matrix=True)       # scipy CSR [V,F], a 1 per (corner vertex, face), duplicates summed
    non_scaled_normals = ftov * face_normals
    norms = (sum(non_scaled_normals ** 2.0, axis=1) ** 0.5).T;  norms[norms == 0] = 1.0
    return (non_scaled_normals.T / norms).T
"""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "uv_texture_golden.npz")


def load_golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def face_normals(v, f):
    """TriNormalsScaled: np.cross(v[f1] - v[f0], v[f2] - v[f0]), each product and difference rounded on its own."""
    a = v[f[:, 1]] - v[f[:, 0]]
    b = v[f[:, 2]] - v[f[:, 0]]
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def vertex_normals(v, f):
    """The scipy CSR product written out: per vertex, y = 0 and y += m * n_face over its faces in ascending face order (m =
    how often the face names the vertex); then divided by ((x*x + y*y) + z*z) ** 0.5, a zero norm read as 1."""
    v = np.asarray(v, np.float64)
    f = np.asarray(f, np.int64)
    fn = face_normals(v, f)
    rows = [[] for _ in range(len(v))]
    for fi, tri in enumerate(f):
        for c in range(3):
            if c > 0 and tri[c] in tri[:c]:
                rows[tri[c]][-1][1] += 1.0
            else:
                rows[tri[c]].append([fi, 1.0])
    # vectorised over vertices: the k-th face of every vertex is added in step k
    deg = np.array([len(r) for r in rows], np.int64)
    out = np.zeros((len(v), 3))
    for k in range(int(deg.max()) if len(deg) else 0):
        sel = np.flatnonzero(deg > k)
        fi = np.array([rows[i][k][0] for i in sel], np.int64)
        m = np.array([rows[i][k][1] for i in sel])
        out[sel] = out[sel] + m[:, None] * fn[fi]
    norm = ((out[:, 0] * out[:, 0] + out[:, 1] * out[:, 1]) + out[:, 2] * out[:, 2]) ** 0.5
    norm[norm == 0] = 1.0
    return out / norm[:, None]


def vertex_normals_scipy(v, f):
    """The literal psbody form on scipy (the cross-check of `vertex_normals`; needs scipy)."""
    import scipy.sparse as sp

    v = np.asarray(v, np.float64)
    f = np.asarray(f, np.int64)
    row = f.flatten()
    col = np.array([range(f.shape[0])] * 3).T.flatten()
    ftov = sp.csr_matrix((np.ones(len(col)), (row, col)), shape=(v.shape[0], f.shape[0]))
    non_scaled = ftov * face_normals(v, f)
    norms = (np.sum(non_scaled ** 2.0, axis=1) ** 0.5).T
    norms[norms == 0] = 1.0
    return (non_scaled.T / norms).T


class RestatedMesh:
    """psbody.mesh.Mesh as far as the bake uses it: `v` float64, `f` uint32, `estimate_vertex_normals`."""

    def __init__(self, v, f):
        self.v = np.array(v, dtype=np.float64)
        self.f = np.array(f, dtype=np.uint32)

    def estimate_vertex_normals(self):
        return vertex_normals(self.v, self.f)


def compute_texture_map(texture_data, source_img, v, f):
    """`_compute_texture_map(source_img, Mesh(v, f))`, the per-candidate loop vectorised: candidates that pass both tests
    write in candidate order, so each texel keeps the last of them. IndexError where such a candidate's texel is outside the
    texture (the reference raises there too)."""
    td = texture_data
    v = np.asarray(v, np.float64)
    ids = td["valid_pixel_ids"]
    vf = td["valid_pixel_3d_faces"]
    bc = td["valid_pixel_b_coords"]
    s = td["img_size"]
    p = v[vf[:, 0], :] * bc[:, 0][:, None] + v[vf[:, 1], :] * bc[:, 1][:, None] + v[vf[:, 2], :] * bc[:, 2][:, None]
    n = vertex_normals(v, f)
    pn = n[vf[:, 0], :] * bc[:, 0][:, None] + n[vf[:, 1], :] * bc[:, 1][:, None] + n[vf[:, 2], :] * bc[:, 2][:, None]
    ndv = -pn[:, 2]
    with np.errstate(invalid="ignore"):
        xy = np.round(p[:, :2], 0).astype(int)
    h, w = source_img.shape[:2]
    x, y = xy[:, 0], xy[:, 1]
    ok = ~(ndv < 0.0) & (x > 0) & (x < w) & (y > 0) & (y < h)
    idx = np.flatnonzero(ok)
    ty = td["y_coords"][ids[idx]].astype(int)
    tx = td["x_coords"][ids[idx]].astype(int)
    if len(idx) and (ty.min() < -s or ty.max() >= s or tx.min() < -s or tx.max() >= s):
        raise IndexError("a passing candidate's texel is outside the texture")
    texel = (ty % s) * s + (tx % s)
    last = len(texel) - 1 - np.unique(texel[::-1], return_index=True)[1]  # the last writer of every texel
    texture = np.zeros((s * s, 3), np.uint8)
    texture[texel[last]] = source_img[y[idx[last]], x[idx[last]]]
    return texture.reshape(s, s, 3)


def winning_candidates(texture_data, source_img, v, f):
    """Per texel the index of the candidate the bake takes (-1: none), with the per-candidate point and n_dot_view: what the
    end-to-end test's float64 arbiter looks at."""
    td = texture_data
    v = np.asarray(v, np.float64)
    vf, bc, ids, s = td["valid_pixel_3d_faces"], td["valid_pixel_b_coords"], td["valid_pixel_ids"], td["img_size"]
    p = v[vf[:, 0], :] * bc[:, 0][:, None] + v[vf[:, 1], :] * bc[:, 1][:, None] + v[vf[:, 2], :] * bc[:, 2][:, None]
    n = vertex_normals(v, f)
    pn = n[vf[:, 0], :] * bc[:, 0][:, None] + n[vf[:, 1], :] * bc[:, 1][:, None] + n[vf[:, 2], :] * bc[:, 2][:, None]
    ndv = -pn[:, 2]
    with np.errstate(invalid="ignore"):
        xy = np.round(p[:, :2], 0).astype(int)
    h, w = source_img.shape[:2]
    ok = ~(ndv < 0.0) & (xy[:, 0] > 0) & (xy[:, 0] < w) & (xy[:, 1] > 0) & (xy[:, 1] < h)
    texel = (td["y_coords"][ids].astype(int) % s) * s + (td["x_coords"][ids].astype(int) % s)
    win = np.full(s * s, -1, np.int64)
    idx = np.flatnonzero(ok)
    t = texel[idx]
    last = len(t) - 1 - np.unique(t[::-1], return_index=True)[1]
    win[t[last]] = idx[last]
    return win, p, ndv, texel
