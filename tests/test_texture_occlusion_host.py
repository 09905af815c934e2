"""CPU: the host side of the occlusion-aware texture bake -- the argument refusals of `dad3d_uvmap_depth_frames` and
`dad3d_uvmap_bake_frames_occluded` before any device work, and the restatement the GPU tests compare with
(tests/texture_occlusion_restatement.py) on a hand-made mesh of two parallel squares, where what is hidden can be said by hand."""
import numpy as np
import pytest

import render_texture_ref as RT
import texture_frames_restatement as TF
import texture_occlusion_restatement as TO
from dad_3dheads_amd import _lib, synthetic


def test_flags_mirror_the_library():
    assert (TO.BAKE_FLAG_INDEX, TO.BAKE_FLAG_DEPTH_WINDOW, TO.BAKE_FLAG_NONFINITE) == (
        _lib.BAKE_FLAG_INDEX, _lib.BAKE_FLAG_DEPTH_WINDOW, _lib.BAKE_FLAG_NONFINITE) == (1, 2, 4)
    assert _lib.BAKE_MAX_DEPTH_SIDE == 4096


P = 64  # any non-null address: nothing is dereferenced before the refusal
OK_HOST = np.array([[P, 8, 8, 24]], np.int64)
BAD_TABLES = [(dict(host=None), b"null host frame table"),
              (dict(host=np.array([[P, 8, 8, 23]], np.int64)), b"row stride of 23"),
              (dict(host=np.array([[0, 8, 8, 24]], np.int64)), b"no address"),
              (dict(host=np.array([[P, 0, 8, 24]], np.int64)), b"0 x 8"),
              (dict(host=np.array([[P, 8, 8, 24], [P, 8, -1, 24]], np.int64), n_frames=2), b"frame 1 is 8 x -1"),
              (dict(n_heads=-1), b"negative"), (dict(n_frames=-1), b"negative"), (dict(n_heads=65536), b"65535")]


def _refused(call, cases):
    lib = _lib.load()
    for kwargs, word in cases:
        lib.dad3d_clear_error()
        assert call(**kwargs) == _lib.E_INVALID, kwargs
        assert word in lib.dad3d_last_error(), (kwargs, lib.dad3d_last_error())


def test_depth_frames_refuses_bad_arguments_before_device_work():
    lib = _lib.load()

    def call(m=None, depth=P, window=P, vertices=P, frames=P, host=OK_HOST, n_frames=1, index=P, n_heads=1, side=128, flags=P):
        return lib.dad3d_uvmap_depth_frames(m, depth, window, vertices, frames, None if host is None else host.ctypes.data, n_frames, index,
                                            n_heads, side, flags, None)

    _refused(call, BAD_TABLES + [(dict(side=0), b"depth_side 0 outside 1..4096"), (dict(side=4097), b"depth_side 4097"), (dict(side=-5), b"depth_side -5"),
                                 (dict(depth=None), b"null buffer"), (dict(window=None), b"null buffer"), (dict(index=None), b"null buffer"),
                                 (dict(flags=None), b"null buffer"), (dict(frames=None), b"null device frame table"),
                                 (dict(), b"null handle"), (dict(side=1), b"null handle"), (dict(side=4096), b"null handle"),
                                 (dict(n_heads=0), b"null handle")])


def test_bake_frames_occluded_refuses_bad_arguments_before_device_work():
    lib = _lib.load()

    def call(m=None, texture=P, score=None, frames=P, host=OK_HOST, n_frames=1, index=P, n_heads=1, depth=P, window=P, depth_flags=P, side=128,
             depth_bias=1.0, slope_bias=1.0, flags=P):
        return lib.dad3d_uvmap_bake_frames_occluded(m, texture, score, P, P, frames, None if host is None else host.ctypes.data, n_frames, index,
                                                    n_heads, depth, window, depth_flags, side, depth_bias, slope_bias, flags, None)

    word = b"must be finite and not negative"
    _refused(call, BAD_TABLES + [(dict(side=0), b"depth_side 0 outside 1..4096"), (dict(side=4097), b"depth_side 4097"),
                                 (dict(depth_bias=-1e-300), word), (dict(slope_bias=-0.5), word), (dict(depth_bias=float("nan")), word),
                                 (dict(slope_bias=float("nan")), word), (dict(depth_bias=float("inf")), word), (dict(slope_bias=float("inf")), word),
                                 (dict(depth_bias=float("-inf")), word),
                                 (dict(texture=None), b"null buffer"), (dict(depth=None), b"null buffer"), (dict(window=None), b"null buffer"),
                                 (dict(depth_flags=None), b"null buffer"), (dict(index=None), b"null buffer"), (dict(flags=None), b"null buffer"),
                                 (dict(frames=None), b"null device frame table"),
                                 (dict(), b"null handle"), (dict(depth_bias=0.0, slope_bias=0.0), b"null handle"), (dict(score=P), b"null handle")])


def test_window_in_float_clipped_flagged_and_empty():
    v = np.array([[3.25, 4.75, 0.0], [20.5, 9.0, 1.0], [7.0, 30.0, 2.0]], np.float32)
    assert TO.expected_window((40, 50), v, 128) == (0, [3, 4, 19, 27])            # floor(3.25) .. ceil(20.5), floor(4.75) .. 30
    assert TO.expected_window((20, 10), v, 128) == (0, [3, 4, 7, 16])             # clipped to w - 1 = 9 and h - 1 = 19
    assert TO.expected_window((40, 50), v - np.float32(5), 128) == (0, [0, 0, 17, 26])  # clipped at 0
    assert TO.expected_window((40, 50), v, 26) == (TO.BAKE_FLAG_DEPTH_WINDOW, [0, 0, 0, 0]) and TO.expected_window((40, 50), v, 27)[0] == 0
    assert TO.expected_window((40, 50), v + np.float32(60), 128) == (0, [0, 0, 0, 0])  # outside its frame: empty, no flag
    assert TO.expected_window((40, 50), v - np.float32(60), 128) == (0, [0, 0, 0, 0])
    for bad in (np.nan, np.inf, -np.inf):
        spoilt = v.copy()
        spoilt[1, 2] = bad
        assert TO.expected_window((40, 50), spoilt, 128) == (TO.BAKE_FLAG_NONFINITE, [0, 0, 0, 0])


def test_two_parallel_squares(sim3dr_oracle):
    v, faces, td, groups = TO.two_planes()
    h, w = 32, 40
    frame = np.random.default_rng(5).integers(1, 256, (h, w, 3), dtype=np.uint8)
    maps, window, flags = TO.expected_depth_frames(sim3dr_oracle, [(h, w)], [v], faces, [0], 32)
    assert flags.tolist() == [0] and window.tolist() == [[10, 10, 21, 11]] and maps[0].shape == (11, 21)
    # the front square (x 10..20) is at depth 0, the back square beside it at 5 up to the float32 weights' rounding; is_point_in_tri keeps
    # the edges u = 0 and v = 0 and drops u + v = 1, so of the row y = 20 only rounding decides
    assert (maps[0][:-1, :11] == 0).all() and np.allclose(maps[0][:-1, 11:], 5.0, rtol=1e-6, atol=0) and np.isinf(maps[0][-1]).any()
    p, _, _ = TO.candidates(td, v, faces)
    assert np.round(p[:, :2]).astype(int).tolist() == [[13, 13], [12, 15], [18, 16], [17, 18], [14, 12], [12, 14], [16, 18], [18, 17],
                                                       [24, 11], [22, 13], [26, 18], [28, 16]]
    plain, _, _, _ = TF.expected_bake_frames(td, [frame], [v], faces, [0])
    all_texels = groups["front"] + groups["under"] + groups["beside"]
    assert plain.reshape(-1, 3)[all_texels].all(1).all()  # without the test every candidate is baked

    def run(depth_bias, slope_bias=0.0, **kw):
        return TO.expected_bake_frames_occluded(td, [frame], [v], faces, [0], maps, window, flags, depth_bias, slope_bias, **kw)

    tex, _, out_flags, stats = run(0.0)
    tex = tex.reshape(-1, 3)
    assert out_flags.tolist() == [0] and stats[0]["accepted"] == 12 and stats[0]["hidden"] == 4 and stats[0]["moved"] == 0
    assert not tex[groups["under"]].any()  # back texels under the front square are hidden
    assert np.array_equal(tex[groups["front"] + groups["beside"]], plain.reshape(-1, 3)[groups["front"] + groups["beside"]])
    for bias in (4.9, 5.1, 6.0):  # the squares are 5 apart
        tex, _, _, stats = run(bias)
        assert stats[0]["hidden"] == (4 if bias < 5 else 0)
    assert np.array_equal(run(6.0)[0], plain)  # depth_bias = 6: nothing is hidden
    # the normals are (0, 0, -1): the slope term is 0 whatever slope_bias is
    assert np.array_equal(run(0.0, 1000.0)[0].reshape(-1, 3), run(0.0)[0].reshape(-1, 3))
    # accumulate: a hidden texel keeps its state, a visible one takes the sample with score 1
    old_tex, old_sc = np.full((1, 8, 8, 3), 9, np.uint8), np.full((1, 8, 8), 0.5, np.float32)
    acc, sc, _, stats = run(0.0, textures=old_tex, score=old_sc)
    acc, sc = acc.reshape(-1, 3), sc.reshape(-1)
    assert (acc[groups["under"]] == 9).all() and (sc[groups["under"]] == 0.5).all() and (sc[groups["front"] + groups["beside"]] == 1.0).all()
    assert stats[0]["replaced"] == 8 and np.array_equal(acc[groups["beside"]], plain.reshape(-1, 3)[groups["beside"]])
    # a flagged depth map flags the bake, and a flagged head changes nothing
    _, _, out_flags, stats = TO.expected_bake_frames_occluded(td, [frame], [v], faces, [0], [None], np.zeros((1, 4), np.int32), [TO.BAKE_FLAG_DEPTH_WINDOW])
    assert out_flags.tolist() == [TO.BAKE_FLAG_DEPTH_WINDOW] and stats == [None]
    _, _, out_flags, _ = TO.expected_bake_frames_occluded(td, [frame], [v], faces, [3], [None], np.zeros((1, 4), np.int32), [TO.BAKE_FLAG_NONFINITE])
    assert out_flags.tolist() == [TO.BAKE_FLAG_NONFINITE | TO.BAKE_FLAG_INDEX]


def test_a_bias_beyond_the_head_gives_the_bake_without_the_test_and_the_walk_goes_on(static, sim3dr_oracle):
    faces = np.ascontiguousarray(static["faces"], dtype=np.int32)
    td = synthetic.synthetic_texture_data(64, seed=114, static=static, duplicates=50)
    v = RT.head_vertices(static, 96, 80).copy()
    v[:, 2] = -v[:, 2]  # the face looks at -z, as the decode's output does
    frame = np.random.default_rng(6).integers(0, 256, (96, 80, 3), dtype=np.uint8)
    maps, window, flags = TO.expected_depth_frames(sim3dr_oracle, [(96, 80)], [v], faces, [0], 128)
    assert flags.tolist() == [0] and window[0, 2] <= 128 and window[0, 3] <= 128 and np.isfinite(maps[0]).mean() > 0.5
    plain, _, _, plain_stats = TF.expected_bake_frames(td, [frame], [v], faces, [0])
    far, _, _, stats = TO.expected_bake_frames_occluded(td, [frame], [v], faces, [0], maps, window, flags, 1e6, 0.0)
    assert np.array_equal(far, plain) and stats[0]["hidden"] == 0 and stats[0]["candidates"] == plain_stats[0]["candidates"] > 1000
    default, _, _, stats = TO.expected_bake_frames_occluded(td, [frame], [v], faces, [0], maps, window, flags)
    assert 5 <= stats[0]["hidden"] <= 0.05 * stats[0]["accepted"] and not np.array_equal(default, plain)
    _, _, _, acne = TO.expected_bake_frames_occluded(td, [frame], [v], faces, [0], maps, window, flags, 0.0, 0.0)
    assert acne[0]["hidden"] >= 0.2 * acne[0]["accepted"] and acne[0]["moved"] >= 1  # a hidden duplicate hands its texel to the next candidate
