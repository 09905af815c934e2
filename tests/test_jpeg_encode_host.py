"""CPU: the JPEG encode rules held to PIL's bytes, twice: tests/jpeg_encode_restatement.py, and
dad3d_jpeg_encode_host, which runs the `__host__ __device__` routines of csrc/jpeg_fdct.hpp and csrc/jpeg_huff_encode.hpp that the
kernels of csrc/jpeg_encode.hip run. The corpus is built here from seeds (tests/jpeg_encode_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import jpeg_encode_restatement as R
from jpeg_cases import markers
from jpeg_encode_cases import QUALITIES, SIDES, corpus, corpus_pil, corpus_restated, host_encode, image, pil_bytes
from dad_3dheads_amd import _lib, writers


def test_corpus_is_what_the_issue_asks():
    cases = corpus()
    assert 100 <= len(cases) <= 150
    assert all(img.shape[0] <= 140 and img.shape[1] <= 140 and img.dtype == np.uint8 for _, img, _ in cases)
    ranged = [(img, o) for name, img, o in cases if name.startswith(("grey", "rgb"))]
    assert {img.shape[0] for img, _ in ranged} == set(SIDES) and {img.shape[1] for img, _ in ranged} == set(SIDES)
    assert len(ranged) < 4 * len(SIDES) ** 2  # not the full square
    assert {img.shape[2] for img, _ in ranged} == {1, 3}
    assert {o["subsampling"] for img, o in ranged if img.shape[2] == 3} == {0, 1, 2}
    assert {o["quality"] for _, o in ranged} == set(QUALITIES) and {o["restart_marker_rows"] for _, o in ranged} == {0, 1, 2}
    shapes = {(img.shape, o.get("subsampling")) for _, img, o in cases}
    assert {((8, 8, 3), 2), ((8, 17, 3), 2), ((1, 1, 1), 2), ((1, 1, 3), 2), ((17, 9, 3), 1)} <= shapes
    files = dict(zip((name for name, _, _ in cases), corpus_pil()))
    dense = next(f for name, f in files.items() if name.startswith("noise at 100 33x31x3"))
    assert dense.count(b"\xff\x00") >= 10  # stuffed bytes
    flat = next(f for name, f in files.items() if name.startswith("constant 33x33x1"))
    assert len(flat) - R.header(33, 33, 1, 75, 0, 0).__len__() - 2 <= 5 * 5  # EOB only: a few bytes per MCU row
    wrapped = next(f for name, f in files.items() if name.startswith("13 intervals"))
    assert wrapped.count(b"\xff\xd0") == 2 and wrapped.count(b"\xff\xd7") == 1  # RST0 .. RST7, RST0 .. RST3


def test_restatement_equals_pil_on_the_corpus():
    for (name, _, _), want, got in zip(corpus(), corpus_pil(), corpus_restated()):
        assert got == want, name


def test_host_entry_equals_pil_on_the_corpus_and_flags_nothing():
    for (name, img, options), want in zip(corpus(), corpus_pil()):
        flag, got = host_encode(img, **options)
        assert flag == 0, name
        assert got == want, name


def test_an_interval_that_is_no_multiple_of_a_row():
    img = image(33, 33, 3, 3, "noise")  # 3 x 3 MCUs at 4:2:0
    for blocks in (1, 2, 3, 4, 8, 9, 10):  # 9: one interval, ending at the last MCU; 10: longer than the scan
        want = pil_bytes(img, quality=75, subsampling=2, restart_marker_blocks=blocks)
        assert R.encode(img, 75, 2, restart_marker_blocks=blocks) == want, blocks
        assert host_encode(img, 75, 2, restart_marker_blocks=blocks) == (0, want), blocks


@pytest.mark.parametrize("c, interval", [(1, 0), (1, 3), (3, 0), (3, 3)])
def test_header_layout_is_pils(c, interval):
    img = image(17, 33, c, 1, "ramp")
    data = pil_bytes(img, quality=50, subsampling=1, restart_marker_blocks=interval)
    segments = markers(data)
    tables = 1 if c == 1 else 2
    want = [0xE0] + [0xDB] * tables + [0xC0] + [0xC4] * (2 * tables) + ([0xDD] if interval else []) + [0xDA]
    assert [m for m, _, _ in segments] == want
    head = R.header(17, 33, c, 50, 1, interval)
    assert data[:segments[-1][2]] == head
    assert data[2:20] == b"\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"  # units 0, density 1 x 1
    dht = [data[s + 4] for m, s, _ in segments if m == 0xC4]
    assert dht == [0x00, 0x10, 0x01, 0x11][:2 * tables]  # DC then AC, per table
    assert host_encode(img, 50, 1, restart_marker_blocks=interval)[1][:len(head)] == head


def test_quality_tables_are_libjpegs():
    for quality in range(1, 101):
        data = pil_bytes(image(8, 8, 3, 0, "flat"), quality=quality)
        tables = [data[s + 5:e] for m, s, e in markers(data) if m == 0xDB]
        for which in (0, 1):
            assert bytes(R.quant_table(which, quality)[R.ZIGZAG].tolist()) == tables[which], quality


def test_restart_rows_that_pass_the_interval_raise():
    # 65535 x 8 pixels wide: 8192 MCUs per row at 4:4:4
    with pytest.raises(ValueError, match="65535"):
        writers._jpeg_options(3, 8, 65535, restart_marker_rows=8, subsampling=0)
    assert writers._jpeg_options(3, 8, 65535, restart_marker_rows=7, subsampling=0)[3] == 7 * 8192
    assert writers._jpeg_options(3, 8, 65535, restart_marker_rows=15)[3] == 15 * 4096  # PIL's default for RGB: 4:2:0
    with pytest.raises(ValueError, match="65535"):
        writers._jpeg_options(3, 8, 65535, restart_marker_rows=16)
    with pytest.raises(ValueError, match="65535"):
        R.restart_interval(8, 65535, 1, 0, 8)
    with pytest.raises(ValueError, match="65535"):
        writers._jpeg_host(np.zeros((8, 8, 1), np.uint8), restart_marker_rows=65536)
    for bad in ({"quality": 0}, {"quality": 101}, {"subsampling": 3}, {"restart_marker_rows": -1}):
        with pytest.raises(ValueError, match="JPEG"):
            writers._jpeg_options(3, 8, 8, **bad)


def test_host_paths_of_the_writers_give_pils_bytes(tmp_path):
    batch = np.stack([image(17, 33, 3, k, kind) for k, kind in enumerate(("noise", "ramp", "flat"))])
    for options in ({}, {"quality": 95, "subsampling": 0}, {"quality": 24, "subsampling": 1, "restart_marker_rows": 1}):
        want = [pil_bytes(img, **options) for img in batch]
        assert writers.jpeg_batch(batch, **options) == want
        paths = [str(tmp_path / f"{i}.jpg") for i in range(3)]
        writers.save_jpeg_batch(batch, paths, encoder="host", **options)
        assert [open(p, "rb").read() for p in paths] == want
    grey = batch[:, :, :, :1].copy()
    assert writers.jpeg_batch(grey, quality=60, subsampling=2) == [pil_bytes(img, quality=60) for img in grey]  # no subsampling for L
    assert writers._jpeg_host(grey[0, :, :, 0]) == pil_bytes(grey[0])
    with pytest.raises(ValueError, match="encoder"):
        writers.save_jpeg_batch(batch, paths, encoder="gpu")
    with pytest.raises(ValueError, match="image"):
        writers._jpeg_host(np.zeros((4, 4, 4), np.uint8))


def test_size_calls_and_the_argument_contract_of_the_host_entry():
    lib = _lib.load()
    assert lib.dad3d_jpeg_max_bytes(8, 8, 1, 0) == (2 + 18 + 69 + 13 + 216 + 6 + 10) + 2 * 208 + 4 + 16
    assert lib.dad3d_jpeg_max_bytes(16, 16, 3, 2) == 629 + 2 * 208 * 6 + 4 + 16
    assert lib.dad3d_jpeg_max_bytes(17, 17, 3, 2) == 629 + 2 * 208 * 24 + 4 * 4 + 16  # dummy blocks count
    for bad in ((0, 8, 3, 0), (8, 0, 3, 0), (65536, 8, 3, 0), (8, 65536, 1, 0), (8, 8, 2, 0), (8, 8, 4, 0), (8, 8, 3, 3), (8, 8, 3, -1),
                (65535, 65535, 1, 0)):
        assert lib.dad3d_jpeg_max_bytes(*bad) == 0, bad
        assert lib.dad3d_jpeg_encode_scratch_bytes(1, *bad) == 0, bad
    assert lib.dad3d_jpeg_encode_scratch_bytes(0, 8, 8, 3, 0) == 0 and lib.dad3d_jpeg_encode_scratch_bytes(65536, 8, 8, 3, 0) == 0
    assert lib.dad3d_jpeg_encode_scratch_bytes(2, 17, 17, 3, 2) == 2 * 24 * (128 + 4)
    img = np.zeros((8, 8, 3), np.uint8)
    out = np.zeros(4096, np.uint8)
    n, flag = C.c_int64(), C.c_int32()
    good = dict(image=img.ctypes.data, h=8, w=8, c=3, quality=75, subsampling=2, interval=0, out=out.ctypes.data, capacity=4096)
    for change in ({"image": None}, {"out": None}, {"c": 2}, {"h": 0}, {"w": 65536}, {"quality": 0}, {"quality": 101}, {"subsampling": 3},
                   {"interval": -1}, {"interval": 65536}, {"capacity": 100}):
        a = {**good, **change}
        status = lib.dad3d_jpeg_encode_host(a["image"], a["h"], a["w"], a["c"], a["quality"], a["subsampling"], a["interval"], a["out"],
                                            a["capacity"], C.byref(n), C.byref(flag))
        assert status == _lib.E_INVALID, change
    assert lib.dad3d_jpeg_encode_host(*good.values(), C.byref(n), C.byref(flag)) == _lib.OK and flag.value == 0
    assert out[:n.value].tobytes() == pil_bytes(img, quality=75, subsampling=2)
