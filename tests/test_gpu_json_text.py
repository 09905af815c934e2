"""GPU: the JSON formatter (csrc/json_text.hip, writers.JsonFormatter, benchmark_export.SubmissionFormatter / SubmissionWriter)
against `json.dumps` itself -- the rule runs on integers, so every expectation here is Python's own output for the same float32
values -- and against the reference `JsonSaver`'s bytes of tests/golden/writers_golden.npz."""
import json
import os

import numpy as np
import pytest
import torch

import json_text_restatement as R
from dad_3dheads_amd import _lib, benchmark_export, synthetic, writers

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "writers_golden.npz")


@pytest.fixture()
def host_calls(monkeypatch):
    """Counts the calls of the host formatter: the GPU path must take none for an item without NaN / inf."""
    calls = []
    real = writers._json_item_host

    def counted(template, row):
        calls.append(tuple(row.shape))
        return real(template, row)

    monkeypatch.setattr(writers, "_json_item_host", counted)
    return calls


def capi_format(template, values):
    """dad3d_json_format_values on `values [B,n_slots]` (CUDA float32) -> (list of bytes per item, lengths, flags), straight through
    ctypes, the text buffer pre-filled with a sentinel."""
    lib = _lib.load()
    b, n = values.shape
    assert n == template.n_slots
    image = template.device_image(values.device)
    offsets = np.ascontiguousarray(template.offsets)
    text = torch.full((b, template.stride), 0x23, dtype=torch.uint8, device="cuda")
    lengths = torch.full((b,), -1, dtype=torch.int64, device="cuda")
    flags = torch.full((b,), -1, dtype=torch.int32, device="cuda")
    nbytes = lib.dad3d_json_format_scratch_bytes(b, n)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _lib.check(lib.dad3d_json_format_values(values.data_ptr(), b, n, image.data_ptr(), offsets.ctypes.data, text.data_ptr(), template.stride,
                                            lengths.data_ptr(), flags.data_ptr(), scratch.data_ptr(), nbytes, 0,
                                            torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    host, ln, fl = text.cpu().numpy(), lengths.cpu().numpy(), flags.cpu().numpy()
    for i in range(b):  # nothing behind an item's text is touched
        assert 0 <= ln[i] <= template.stride and (host[i, ln[i]:] == 0x23).all(), i
    return [host[i, :ln[i]].tobytes() for i in range(b)], ln, fl


def expected(template, rows):
    """Python's own text for float32 `rows [B,n_slots]`."""
    return [template.render(R.python_numbers(row)) for row in rows]


def wide_values(rng, shape):
    """Seeded float32 values of every size: plain, tiny, huge, exact integers, powers of two, zeros of both signs."""
    n = int(np.prod(shape))
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-12, 13, n)
    pick = rng.integers(0, 8, n)
    x = np.where(pick == 0, np.round(x), x)
    x = np.where(pick == 1, 2.0 ** rng.integers(-140, 120, n), x)
    x = np.where(pick == 2, rng.choice([0.0, -0.0, 0.1, 1e-4, 1e-5, 123.0, 16777216.0], size=n), x)
    with np.errstate(over="ignore"):
        x = x.astype(np.float32)
    x[~np.isfinite(x)] = np.float32(3.4028234663852886e+38)
    return x.reshape(shape)


def test_reference_bytes_of_json_saver(host_calls):
    with np.load(GOLDEN) as z:
        want = [bytes(z["json_0"]), bytes(z["json_1"])]
    params = torch.from_numpy(synthetic.synthetic_params(2, seed=205)).cuda()
    assert writers.flame_params_json_batch(params) == want
    assert host_calls == []


def test_edge_cases_and_a_slice_of_the_sample_set_through_the_c_abi():
    bits = R.sample_bits()
    x = np.concatenate([R.NAMED, bits[::31][: 65536 - R.NAMED.size].view(np.float32)])
    assert x.size == 65536 and len(np.unique((x.view(np.uint32) >> 23) & 0xff)) == 255  # every exponent is in the slice
    t = writers.JsonTemplate.from_structure(x.size)
    got, lengths, flags = capi_format(t, torch.from_numpy(x[None]).cuda())
    assert flags.tolist() == [0]
    want = R.one_list_json(x)
    assert lengths.tolist() == [len(want)]
    assert got[0] == want
    assert max(len(s) for s in want[1:-1].split(b", ")) == 23


@pytest.mark.parametrize("batch", [1, 3, 65])
@pytest.mark.parametrize("n_slots", [1, 255, 256, 257, 413, 513])
def test_tile_and_batch_edges(n_slots, batch):
    rng = np.random.default_rng(1000 * n_slots + batch)
    x = wide_values(rng, (batch, n_slots))
    t = writers.JsonTemplate.from_structure({"values": n_slots})
    got, lengths, flags = capi_format(t, torch.from_numpy(x).cuda())
    assert not flags.any()
    want = expected(t, x)
    assert want[0] == json.dumps({"values": x[0].astype(np.float64).tolist()}).encode()
    assert lengths.tolist() == [len(w) for w in want]
    for i in range(batch):
        assert got[i] == want[i], i


def test_literals_at_the_cap_and_empty_lists():
    rng = np.random.default_rng(64)
    cap = _lib.JSON_MAX_LITERAL_BYTES
    n = 300  # more than one tile of worst-case literals
    capped = writers.JsonTemplate([bytes((0x41 + (i + j) % 26) for j in range(cap)) for i in range(n + 1)])
    assert capped.stride >= n * (cap + 23) + cap
    empties = writers.JsonTemplate.from_structure({"first": [], "a": 3, "mid": [], "also": 0, "b": (2, 2), "last": [], "end": []})
    assert empties.literals[0] == b'{"first": [], "a": [' and empties.literals[-1] == b']], "last": [], "end": []}'
    for t in (capped, empties):
        x = wide_values(rng, (3, t.n_slots))
        x[1] = np.float32(-1.1754942106924411e-38)  # every number at its longest
        got, lengths, flags = capi_format(t, torch.from_numpy(x).cuda())
        assert not flags.any()
        assert got == expected(t, x)
    x = wide_values(rng, (2, empties.n_slots))
    assert expected(empties, x)[0] == json.dumps({"first": [], "a": x[0, :3].astype(np.float64).tolist(), "mid": [], "also": [],
                                                   "b": x[0, 3:].astype(np.float64).reshape(2, 2).tolist(), "last": [], "end": []}).encode()


@pytest.mark.parametrize("value, token", [(np.nan, b"NaN"), (np.inf, b" Infinity"), (-np.inf, b"-Infinity")], ids=["nan", "inf", "-inf"])
def test_a_non_finite_value_flags_its_item_only(value, token, host_calls):
    rng = np.random.default_rng(11)
    t = writers.JsonTemplate.from_structure({"a": (100, 3), "b": 213})
    x = wide_values(rng, (3, t.n_slots))
    fmt = writers.JsonFormatter(t, device=0)
    clean = fmt.format(torch.from_numpy(x).cuda())
    assert [bytes(b) for b in clean.to_host()] == expected(t, x)
    assert host_calls == []  # all finite: the device's text for every item
    x[1, 400] = value
    dev = torch.from_numpy(x).cuda()
    got, lengths, flags = capi_format(t, dev)
    assert flags.tolist() == [0, _lib.JSON_FLAG_NONFINITE, 0] and lengths[1] == 0
    want = expected(t, x)
    assert got[0] == want[0] and got[2] == want[2]
    text = fmt.format(dev)
    blocks = [bytes(b) for b in text.to_host()]
    assert host_calls == [(t.n_slots,)]  # the flagged item alone went through the host formatter
    item1 = json.dumps({"a": x[1, :300].astype(np.float64).reshape(100, 3).tolist(), "b": x[1, 300:].astype(np.float64).tolist()}).encode()
    assert blocks == [want[0], item1, want[2]]
    assert token in item1


@pytest.fixture(scope="module")
def predictions():
    """Five images' worth of submission fields, int32 2-D points, the full 5023-vertex layout; the host path's entries, once."""
    rng = np.random.default_rng(2024)
    b = 5
    points = torch.from_numpy(rng.integers(-20, 300, (b, 68, 2)).astype(np.int32)).cuda()
    vertices = torch.from_numpy((rng.standard_normal((b, 5023, 3)) * 0.1).astype(np.float32)).cuda()
    lmk68 = torch.from_numpy((rng.standard_normal((b, 68, 3)) * 0.1).astype(np.float32)).cuda()
    rotation = torch.from_numpy(np.linalg.qr(rng.standard_normal((b, 3, 3)))[0].astype(np.float32)).cuda()
    entries = [benchmark_export.submission_entry(points[i], vertices[i], lmk68[i], rotation[i]) for i in range(b)]
    return (points, vertices, lmk68, rotation), entries


def test_submission_entries_match_json_dumps(predictions):
    (points, vertices, lmk68, rotation), entries = predictions
    fmt = benchmark_export.SubmissionFormatter(device=0)
    assert fmt.template.n_slots == 68 * 2 + 5023 * 3 + 7 * 3 + 9
    text = fmt.format(points[:3], vertices[:3], lmk68[:3], rotation[:3])
    torch.cuda.synchronize()
    assert text.flags.cpu().tolist() == [0, 0, 0]  # before the bytes: the host fallback must not be able to hide a kernel fault
    got = fmt.entries(points[:3], vertices[:3], lmk68[:3], rotation[:3])
    for i in range(3):
        assert got[i] == json.dumps(entries[i]).encode(), i
    staging = fmt.formatter._staging.data_ptr()
    fmt.entries(points[:2], vertices[:2], lmk68[:2], rotation[:2])
    assert fmt.formatter._staging.data_ptr() == staging  # reserved once


def test_submission_writer_file_equals_write_submission(tmp_path, predictions):
    (points, vertices, lmk68, rotation), entries = predictions
    ids = ["img_%d.png" % i for i in range(4)] + [17]
    want_path, got_path = str(tmp_path / "host.json"), str(tmp_path / "device.json")
    benchmark_export.write_submission(want_path, dict(zip(ids, entries)))
    with benchmark_export.SubmissionWriter(got_path, device=0) as w:
        for lo in range(0, 5, 2):
            w.add(ids[lo:lo + 2], points[lo:lo + 2], vertices[lo:lo + 2], lmk68[lo:lo + 2], rotation[lo:lo + 2])
    data = open(got_path, "rb").read()
    assert data == open(want_path, "rb").read()
    loaded = json.load(open(got_path))
    assert list(loaded) == [str(k) for k in ids] and loaded["17"] == entries[4]
    empty = str(tmp_path / "empty.json")
    with benchmark_export.SubmissionWriter(empty, device=0):
        pass
    benchmark_export.write_submission(want_path, {})
    assert open(empty, "rb").read() == open(want_path, "rb").read() == b"{}"


def test_an_integer_beyond_2_to_24_falls_back_to_the_host(predictions):
    (points, vertices, lmk68, rotation), entries = predictions
    big = points[:3].clone()
    big[1, 40, 1] = 2 ** 24 + 1  # no float32
    big[2, 0, 0] = -(2 ** 24)    # a float32: stays on the device
    fmt = benchmark_export.SubmissionFormatter(device=0)
    text = fmt.format(big, vertices[:3], lmk68[:3], rotation[:3])
    torch.cuda.synchronize()
    assert text.flags.cpu().tolist() == [0, benchmark_export.SUBMISSION_FLAG_INEXACT, 0]
    got = [bytes(x) for x in text.to_host()]
    for i in range(3):
        assert got[i] == json.dumps(benchmark_export.submission_entry(big[i], vertices[i], lmk68[i], rotation[i])).encode(), i
    assert b"[-16777216.0, " in got[2] and b"16777217.0]" in got[1]


def test_two_runs_and_a_graph_replay_give_identical_bytes():
    rng = np.random.default_rng(3)
    t = writers.JsonTemplate.from_structure({"a": (90, 3), "b": [], "c": 143})
    x = wide_values(rng, (5, t.n_slots))
    values = torch.from_numpy(x).cuda()
    want = expected(t, x)
    fmt = writers.JsonFormatter(t, device=0)
    fmt.reserve(5)
    fmt._text.fill_(0)
    fmt.format(values)
    torch.cuda.synchronize()
    first = fmt._text.clone()
    fmt._text.fill_(0)
    fmt.format(values)
    torch.cuda.synchronize()
    assert torch.equal(first, fmt._text)  # deterministic
    src = torch.zeros_like(values)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fmt.format(src)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        text = fmt.format(src)  # no allocation, no sync: capturable, one stream
    src.copy_(values)
    fmt._text.fill_(0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(first, fmt._text)
    assert [bytes(b) for b in text.to_host()] == want


def test_other_layouts_and_dtypes(tmp_path, host_calls):
    """`JsonFormatter.format` refuses what the kernel cannot read with a ValueError that names the argument;
    `save_flame_params_batch` sends such a tensor down the host path. Same bytes."""
    params = torch.from_numpy(synthetic.synthetic_params(3, seed=9)).cuda()
    fmt = writers.JsonFormatter(writers.JsonTemplate.from_structure(413), device=0)
    strided = params.t().contiguous().t()
    assert not strided.is_contiguous()
    for bad in (strided, params.double(), params.cpu(), params[:, :100].contiguous()):
        with pytest.raises(ValueError, match="values"):
            fmt.format(bad)
    paths = [[str(tmp_path / f"{k}{i}.json") for i in range(3)] for k in "abcd"]
    writers.save_flame_params_batch(params, paths[0])
    writers.save_flame_params_batch(strided, paths[1])
    writers.save_flame_params_batch(params.cpu(), paths[2])
    writers.save_flame_params_batch(params, paths[3], formatter="host")
    assert host_calls == []  # json.dump, not the per-item fallback
    for i in range(3):
        data = open(paths[0][i], "rb").read()
        assert data == open(paths[1][i], "rb").read() == open(paths[2][i], "rb").read() == open(paths[3][i], "rb").read()
        assert data == json.dumps(writers.get_flame_params({"3dmm_params": params[i:i + 1]})).encode()
    assert writers.flame_params_json_batch(params[:0]) == []
