"""CPU: the host side of the GPU `.obj` vertex formatter (csrc/obj_text.hip, writers.ObjFormatter). The integer rule restated in
tests/obj_text_restatement.py reproduces the bytes of the reference's own MeshSaver (tests/golden/obj_text_golden.npz) and
Python's '%.8f' on a seeded sweep; the C ABI validates its arguments without a GPU; the host paths of `save_obj_batch` write
what they wrote before."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import obj_text_restatement as R
from dad_3dheads_amd import _lib, writers

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "obj_text_golden.npz")


@pytest.fixture(scope="module")
def golden():
    return R.load_golden(GOLDEN)


def test_fixture_is_small_and_inside_the_domain(golden):
    assert os.path.getsize(GOLDEN) < 512 * 1024
    assert list(golden) == ["metre", "pixel", "edge"]
    for name, (v, text) in golden.items():
        assert v.dtype == np.float32 and v.ndim == 2 and v.shape[1] == 3
        assert np.isfinite(v).all() and (np.abs(v.astype(np.float64)) < R.DOMAIN_LIMIT).all(), name
        assert text.count(b"\n") == len(v) and len(text) <= len(v) * R.MAX_LINE_BYTES
    assert len(golden["metre"][0]) == len(golden["pixel"][0]) == 5023
    assert np.abs(golden["metre"][0]).max() < 1.0 < np.abs(golden["pixel"][0]).max()


def test_restatement_reproduces_the_reference_bytes(golden):
    for name, (v, text) in golden.items():
        got, flags = R.vertex_block(v)
        assert flags == 0, name
        assert got == text, name


def test_host_writer_reproduces_the_fixture_too(golden):
    """The parent's host path on the stored floats: the yardstick of the GPU tests agrees with the reference's bytes."""
    for name, (v, text) in golden.items():
        assert writers._vertex_block(v).encode("ascii") == text, name


def _sweep():
    rng = np.random.default_rng(20240611)
    bits = rng.integers(0, 2 ** 32, 360000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    metre = (rng.standard_normal(60000) * 0.08).astype(np.float32)
    pixel = (rng.random(60000) * 300.0 - 20.0).astype(np.float32)
    sub = rng.integers(0, 2 ** 23, 20000, dtype=np.uint64).astype(np.uint32)
    sub = np.concatenate([sub, sub | np.uint32(0x80000000)]).view(np.float32)
    k = np.arange(1, 40001, 2, dtype=np.float64)
    ties = np.concatenate([k / 2 ** 9, -k / 2 ** 9, k / 2 ** 12, 1000.0 + k / 2 ** 9, k / 2 ** 17]).astype(np.float32)
    small = (rng.standard_normal(40000) * 10.0 ** rng.integers(-12, -6, 40000)).astype(np.float32)
    big = (rng.standard_normal(40000) * 10.0 ** rng.integers(3, 13, 40000)).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 5e-9, -5e-9, 4.9999999e-9, 0.99999999, 0.999999995, 9.9999999, 99999.999, 2.0 ** 37,
                        -2.0 ** 37, np.nextafter(np.float32(2.0 ** 37), np.float32(0)), 3e38, -3e38, np.inf, -np.inf, np.nan], dtype=np.float32)
    return np.concatenate([bits, metre, pixel, sub, ties, small, big, special])


def test_restatement_agrees_with_python_percent_on_a_seeded_sweep():
    x = _sweep()
    assert x.size > 600000
    got = R.numbers(x)
    want = R.python_numbers(x)
    with np.errstate(invalid="ignore"):
        outside = ~np.isfinite(x) | ~(np.abs(x.astype(np.float64)) < R.DOMAIN_LIMIT)
    assert 1000 < outside.sum() < x.size // 2  # both sides of the domain are in the sweep
    flagged = np.array([g is None for g in got])
    assert np.array_equal(flagged, outside)  # out of the domain: reported as flagged, never as text
    bad = [(float(v), g, w) for v, g, w in zip(x, got, want) if g is not None and g != w]
    assert not bad, bad[:10]
    _, _, flags = R.fixed8(np.array([np.nan, np.inf, -np.inf, 2.0 ** 37, 3e38, 1.0], dtype=np.float32))
    assert flags.tolist() == [R.FLAG_NONFINITE] * 3 + [R.FLAG_LARGE] * 2 + [0]
    assert R.vertex_block(np.array([[1.0, np.nan, 2.0]], dtype=np.float32)) == (None, R.FLAG_NONFINITE)


def test_line_length_bounds():
    """A line is 5 fixed bytes + three numbers of 10 to 22 bytes: at most 71 bytes inside the domain."""
    top = np.nextafter(np.float32(2.0 ** 37), np.float32(0))
    longest, _ = R.vertex_block(np.array([[-top, -top, -top]], dtype=np.float32))
    shortest, _ = R.vertex_block(np.zeros((1, 3), dtype=np.float32))
    assert len(longest) == R.MAX_LINE_BYTES == _lib.OBJ_MAX_LINE_BYTES and len(shortest) == 5 + 3 * 10
    assert (R.FLAG_NONFINITE, R.FLAG_LARGE) == (_lib.OBJ_FLAG_NONFINITE, _lib.OBJ_FLAG_LARGE)


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(os.path.dirname(HERE), "include", "dad3d.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("dad3d_obj_format_vertices", "dad3d_obj_format_scratch_bytes"):
        assert re.search(r"DAD3D_EXPORT [a-z_0-9]+ " + name + r"\(", header), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert "demo_utils.py:130-144" in header


def test_argument_validation_runs_before_any_device_work():
    lib = _lib.load()
    n, b = 100, 4
    stride = (n * _lib.OBJ_MAX_LINE_BYTES + 15) // 16 * 16
    assert lib.dad3d_obj_format_scratch_bytes(b, n) == b * 8
    assert lib.dad3d_obj_format_scratch_bytes(256, 5023) == 256 * 20 * 8
    assert lib.dad3d_obj_format_scratch_bytes(-1, n) == 0 and lib.dad3d_obj_format_scratch_bytes(b, -1) == 0
    ptr = 0x10000  # never dereferenced: every call below is refused on the host
    good = dict(vertices=ptr, batch=b, nver=n, text=ptr, text_stride=stride, lengths=ptr, flags=ptr, scratch=ptr, scratch_bytes=b * 8,
                device=0, stream=None)

    def call(**change):
        a = {**good, **change}
        lib.dad3d_clear_error()
        return lib.dad3d_obj_format_vertices(a["vertices"], a["batch"], a["nver"], a["text"], a["text_stride"], a["lengths"], a["flags"],
                                             a["scratch"], a["scratch_bytes"], a["device"], a["stream"])

    for name in ("vertices", "text", "lengths", "flags", "scratch"):
        assert call(**{name: None}) == _lib.E_INVALID, name
        assert b"null" in lib.dad3d_last_error()
    assert call(nver=-1) == _lib.E_INVALID and call(batch=-1) == _lib.E_INVALID
    assert call(text_stride=n * _lib.OBJ_MAX_LINE_BYTES - 4) == _lib.E_INVALID  # below the worst case
    assert b"worst case" in lib.dad3d_last_error()
    assert call(text_stride=stride + 4) == _lib.E_INVALID and call(text=ptr + 4) == _lib.E_INVALID  # 16-byte units
    assert call(scratch_bytes=b * 8 - 1) == _lib.E_INVALID
    assert b"scratch" in lib.dad3d_last_error()
    assert call(batch=0, vertices=None, text=None) == _lib.OK  # nothing to do


def test_save_obj_batch_host_paths_write_the_same_bytes_as_before(tmp_path, golden, static):
    faces = static["faces"]
    face_text = writers._face_block(faces + 1.0)
    verts = torch.from_numpy(np.stack([golden["metre"][0], golden["pixel"][0]]))
    for tag, kwargs in (("default", {}), ("host", {"formatter": "host"})):
        paths = [str(tmp_path / f"{tag}_{i}.obj") for i in range(2)]
        writers.save_obj_batch(verts, faces, paths, **kwargs)
        for path, name in zip(paths, ("metre", "pixel")):
            data = open(path, "rb").read()
            assert data == golden[name][1] + face_text.encode("ascii"), (tag, name)
            assert data.decode("ascii") == writers.obj_text(golden[name][0], faces + 1.0)
    p64 = [str(tmp_path / "f64.obj")]
    writers.save_obj_batch(verts[:1].double(), faces, p64)  # another dtype: the host path, as before
    assert open(p64[0], "rb").read().decode("ascii") == writers.obj_text(golden["metre"][0].astype(np.float64), faces + 1.0)
    with pytest.raises(ValueError, match="formatter"):
        writers.save_obj_batch(verts, faces, paths, formatter="gpu?")
    assert writers.obj_text_batch(verts, faces + 1.0) == [golden[n][1] + face_text.encode("ascii") for n in ("metre", "pixel")]


@pytest.mark.skipif(not os.path.isdir("/root/reference/dad_3dheads_benchmark"), reason="reference tree not present on this machine")
def test_committed_fixture_is_what_the_reference_produces_here(tmp_path):
    """Authoring container only: re-run the generator (the reference's own MeshSaver) and compare with the committed fixture."""
    out = tmp_path / "obj_text_golden.npz"
    subprocess.run([sys.executable, os.path.join(HERE, "golden", "make_obj_text_golden.py"), str(out)], check=True, capture_output=True, timeout=300)
    with np.load(out) as fresh, np.load(GOLDEN) as committed:
        assert sorted(fresh.files) == sorted(committed.files)
        for k in fresh.files:
            assert np.array_equal(fresh[k], committed[k]), k
