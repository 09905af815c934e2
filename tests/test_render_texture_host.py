"""CPU: the host side of the textured render -- argument validation of the C entry before any device work, the typed-buffer
errors of `Sim3DR.render_texture`, and the synthetic corner layout against the synthetic atlas it belongs to."""
import numpy as np
import pytest

from dad_3dheads_amd import Sim3DR, _lib, synthetic
from dad_3dheads_amd.uv_texture import texel_coords


def render(lib, m=None, image_dtype=0, texture_dtype=0, batch=1, h=8, w=8, c=3, tex=(4, 4, 3), mapping=1, indexing=0):
    return lib.dad3d_mesh_render_texture(m, None, image_dtype, None, None, texture_dtype, 0, None, batch, h, w, c, tex[0], tex[1], tex[2],
                                         mapping, indexing, None)


def test_render_texture_refuses_bad_arguments_before_device_work():
    lib = _lib.load()
    for kwargs, word in [(dict(c=0), b"c = 0"), (dict(c=5, tex=(4, 4, 8)), b"c = 5"), (dict(c=3, tex=(4, 4, 2)), b"tex_c = 2"),
                         (dict(image_dtype=2), b"float32"), (dict(texture_dtype=-1), b"uint8"), (dict(indexing=2), b"indexing mode 2"),
                         (dict(tex=(0, 4, 3)), b"texture of 0"), (dict(batch=-1), b"negative"), (dict(h=-2), b"negative"),
                         (dict(), b"null handle")]:
        lib.dad3d_clear_error()
        assert render(lib, **kwargs) == _lib.E_INVALID, kwargs
        assert word in lib.dad3d_last_error(), (kwargs, lib.dad3d_last_error())
    lib.dad3d_clear_error()
    assert lib.dad3d_mesh_set_texcoords(None, None, 0, 2, None) == _lib.E_INVALID and b"null handle" in lib.dad3d_last_error()


def test_sim3dr_render_texture_typed_buffer_errors():
    v = np.zeros((3, 3), np.float32)
    t = np.array([[0, 1, 2]], np.int32)
    tex = np.zeros((4, 4, 3), np.float32)
    tc = np.zeros((3, 3), np.float32)
    ok = dict(vertices=v, triangles=t, texture=tex, tex_coords=tc, tex_triangles=t, h=8, w=8)
    with pytest.raises(ValueError, match="Buffer dtype mismatch, expected 'float' but got 'double'"):
        Sim3DR.render_texture(**{**ok, "vertices": v.astype(np.float64)})
    with pytest.raises(ValueError, match="Buffer dtype mismatch, expected 'int' but got 'long'"):
        Sim3DR.render_texture(**{**ok, "tex_triangles": t.astype(np.int64)})
    with pytest.raises(ValueError, match="Buffer dtype mismatch, expected 'float' but got 'unsigned char'"):
        Sim3DR.render_texture(**{**ok, "texture": tex.astype(np.uint8)})
    with pytest.raises(ValueError, match="wrong number of dimensions"):
        Sim3DR.render_texture(**{**ok, "texture": tex[0]})
    with pytest.raises(ValueError, match="not C-contiguous"):
        Sim3DR.render_texture(**{**ok, "tex_coords": np.zeros((3, 6), np.float32)[:, ::2]})
    with pytest.raises(TypeError, match="must not be None"):
        Sim3DR.render_texture(**{**ok, "triangles": None})
    with pytest.raises(TypeError, match="incorrect type"):
        Sim3DR.render_texture(**{**ok, "tex_coords": tc.tolist()})
    with pytest.raises(ValueError, match="image: expected shape"):
        Sim3DR.render_texture(**ok, bg=np.zeros((4, 4, 3), np.float32))
    with pytest.raises(ValueError, match=r"tex_coords \[T,3\]"):
        Sim3DR.render_texture(**{**ok, "tex_coords": np.zeros((3, 2), np.float32)})


def test_synthetic_corner_layout_reproduces_the_atlas(static):
    s = 256
    atlas = synthetic.synthetic_texture_data(s, seed=0, static=static)
    lay = synthetic.synthetic_texcoords(s, static)
    faces = static["faces"].astype(np.int64)
    vt, ft = lay["vt"], lay["ft"]
    assert vt.shape == (5023, 2) and ft.shape == faces.shape and ft.dtype == np.int32
    assert vt.min() >= 0.0 and vt.max() <= 1.0
    left_out = (ft < 0).any(1)
    assert (ft[left_out] == -1).all() and 0 < left_out.sum() <= 0.01 * len(faces), int(left_out.sum())
    assert np.array_equal(ft[~left_out], faces[~left_out])
    tex_coords = texel_coords(vt, s)  # float64, texel units
    # every candidate of the atlas: its face (looked up by its vertex triple), its barycentrics, its texel
    face_of = {tuple(f): i for i, f in reversed(list(enumerate(map(tuple, faces))))}
    cand_faces = np.array([face_of[tuple(t)] for t in atlas["valid_pixel_3d_faces"]])
    assert not left_out[cand_faces].any()  # the atlas leaves the seam faces out, and so does the layout
    corners = tex_coords[ft[cand_faces]]  # [n,3,2]
    pos = (atlas["valid_pixel_b_coords"][:, :, None] * corners).sum(1)
    ids = atlas["valid_pixel_ids"]
    texel = np.stack([atlas["x_coords"][ids], atlas["y_coords"][ids]], 1)
    assert np.abs(pos - texel).max() < 1e-9, float(np.abs(pos - texel).max())
    # a smaller atlas keeps the same faces out
    assert np.array_equal((synthetic.synthetic_texcoords(64, static)["ft"] < 0).any(1), left_out)
    assert synthetic.texture_data_digest(atlas) == synthetic.texture_data_digest(synthetic.synthetic_texture_data(s, seed=0, static=static))
