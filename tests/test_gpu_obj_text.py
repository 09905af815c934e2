"""GPU: the `.obj` vertex formatter (csrc/obj_text.hip, writers.ObjFormatter) against the bytes the reference's own MeshSaver wrote
for the stored float32 meshes of tests/golden/obj_text_golden.npz, and against the host path of `writers` (itself pinned to the
reference by tests/test_host_logic.py). Lines are independent of each other, so the expected text of the first N rows of a mesh,
or of its rows repeated, is the matching lines of the fixture."""
import os

import numpy as np
import pytest
import torch

import obj_text_restatement as R
from dad_3dheads_amd import _lib, synthetic, writers
from dad_3dheads_amd.head_mesh import HeadMesh

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "obj_text_golden.npz")
NAMES = ("metre", "pixel", "edge")


@pytest.fixture(scope="module")
def golden():
    return R.load_golden(GOLDEN)


@pytest.fixture(scope="module")
def meshes(golden):
    """{name: (vertices [5023,3], list of its 5023 lines)}: the edge mesh's rows repeated to the full size."""
    out = {}
    for name, (v, text) in golden.items():
        lines = text.splitlines(keepends=True)
        assert len(lines) == len(v)
        idx = np.arange(5023) % len(v)
        out[name] = (np.ascontiguousarray(v[idx]), [lines[i] for i in idx])
    return out


@pytest.fixture()
def host_calls(monkeypatch):
    """Counts the calls of the host formatter: the GPU path must take none for a mesh inside the domain."""
    calls = []
    real = writers._vertex_block

    def counted(vertices):
        calls.append(np.asarray(vertices).shape)
        return real(vertices)

    monkeypatch.setattr(writers, "_vertex_block", counted)
    return calls


def capi_format(verts):
    """dad3d_obj_format_vertices on `verts [B,N,3]` -> (list of bytes per mesh, lengths, flags), straight through ctypes."""
    lib = _lib.load()
    b, n, _ = verts.shape
    stride = max((n * _lib.OBJ_MAX_LINE_BYTES + 15) // 16 * 16, 16)
    text = torch.full((b, stride), 0x23, dtype=torch.uint8, device="cuda")
    lengths = torch.full((b,), -1, dtype=torch.int64, device="cuda")
    flags = torch.full((b,), -1, dtype=torch.int32, device="cuda")
    nbytes = lib.dad3d_obj_format_scratch_bytes(b, n)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _lib.check(lib.dad3d_obj_format_vertices(verts.data_ptr(), b, n, text.data_ptr(), stride, lengths.data_ptr(), flags.data_ptr(),
                                             scratch.data_ptr(), nbytes, 0, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    host, ln, fl = text.cpu().numpy(), lengths.cpu().numpy(), flags.cpu().numpy()
    for i in range(b):  # nothing behind a mesh's text is touched
        assert (host[i, ln[i]:] == 0x23).all(), i
    return [host[i, :ln[i]].tobytes() for i in range(b)], ln, fl


def test_fixture_bytes_through_the_c_abi(golden):
    for name, (v, want) in golden.items():
        got, lengths, flags = capi_format(torch.from_numpy(v[None]).cuda())
        assert flags.tolist() == [0], name  # before the bytes: a host fallback must not be able to hide a kernel fault
        assert lengths.tolist() == [len(want)], name
        assert got[0] == want, name


def test_fixture_bytes_through_obj_text_batch(golden, static, host_calls):
    faces1 = static["faces"] + 1.0
    face_text = writers._face_block(faces1).encode("ascii")
    for name, (v, want) in golden.items():
        dev = torch.from_numpy(v[None]).cuda()
        text = writers.ObjFormatter(len(v), device=0).format(dev)
        torch.cuda.synchronize()
        assert text.flags.cpu().tolist() == [0] and text.lengths.cpu().tolist() == [len(want)], name
        assert writers.obj_text_batch(dev, faces1) == [want + face_text], name
    assert host_calls == []


@pytest.mark.parametrize("batch", [1, 3, 64, 256])
def test_mixed_batches_give_each_mesh_its_own_bytes(meshes, batch, host_calls):
    rng = np.random.default_rng(batch)
    order = [NAMES[i] for i in rng.permutation(np.arange(batch) % 3)]
    verts = torch.from_numpy(np.stack([meshes[n][0] for n in order])).cuda()
    want = [b"".join(meshes[n][1]) for n in order]
    got, lengths, flags = capi_format(verts)
    assert not flags.any()
    assert lengths.tolist() == [len(w) for w in want]
    for i in range(batch):
        assert got[i] == want[i], (i, order[i])
    fmt = writers.ObjFormatter(5023, device=0)
    text = fmt.format(verts)
    assert text.batch == batch and text.offsets == [i * fmt.stride for i in range(batch)] and fmt.stride % 16 == 0
    flat = text.text.reshape(-1)
    torch.cuda.synchronize()
    assert not text.flags.cpu().any()
    ln = text.lengths.cpu().tolist()
    assert ln == [len(w) for w in want] and all(length <= fmt.stride for length in ln)
    for i in (0, batch // 2, batch - 1):  # offsets and lengths address the device buffer
        assert flat[text.offsets[i]: text.offsets[i] + ln[i]].cpu().numpy().tobytes() == want[i]
    blocks = text.to_host()
    assert [bytes(x) for x in blocks] == want
    assert host_calls == []  # to_host() took the device's text for every mesh


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 5023])
def test_vertex_counts(meshes, n):
    verts = torch.from_numpy(np.stack([meshes[name][0][:n] for name in NAMES])).cuda()
    got, lengths, flags = capi_format(verts)
    assert not flags.any()
    for i, name in enumerate(NAMES):
        assert got[i] == b"".join(meshes[name][1][:n]), (n, name)
    # rows from the middle of a mesh: the tiles start at other byte offsets
    verts = torch.from_numpy(np.stack([meshes[name][0][7:7 + n] for name in NAMES])).cuda()
    got, _, flags = capi_format(verts)
    assert not flags.any()
    for i, name in enumerate(NAMES):
        assert got[i] == b"".join(meshes[name][1][7:7 + n]), (n, name)


def test_zero_vertices_and_empty_batch():
    got, lengths, flags = capi_format(torch.zeros((2, 0, 3), dtype=torch.float32, device="cuda"))
    assert got == [b"", b""] and lengths.tolist() == [0, 0] and flags.tolist() == [0, 0]
    assert writers.obj_text_batch(torch.zeros((0, 5, 3), dtype=torch.float32, device="cuda"), np.ones((1, 3))) == []


def test_out_of_domain_mesh_is_flagged_and_formatted_by_the_host(tmp_path, meshes, static, host_calls):
    faces = static["faces"]
    v = np.stack([meshes["metre"][0], meshes["pixel"][0].copy(), meshes["edge"][0], meshes["pixel"][0]])
    v[1, [0, 300, 2500, 5000, 5022], [0, 1, 2, 0, 2]] = [np.nan, np.inf, -np.inf, 2.0 ** 37, 3e38]
    verts = torch.from_numpy(v).cuda()
    got, lengths, flags = capi_format(verts)
    assert flags.tolist() == [0, _lib.OBJ_FLAG_NONFINITE | _lib.OBJ_FLAG_LARGE, 0, 0]  # exactly that mesh
    assert lengths[1] == 0
    for i, name in ((0, "metre"), (2, "edge"), (3, "pixel")):
        assert got[i] == b"".join(meshes[name][1]), name  # the neighbours' bytes are untouched
    for value, bit in ((np.nan, _lib.OBJ_FLAG_NONFINITE), (-np.inf, _lib.OBJ_FLAG_NONFINITE), (2.0 ** 37, _lib.OBJ_FLAG_LARGE), (-3e38, _lib.OBJ_FLAG_LARGE)):
        one = meshes["metre"][0].copy()
        one[4000, 1] = value
        assert capi_format(torch.from_numpy(one[None]).cuda())[2].tolist() == [bit], value
    paths = [str(tmp_path / f"m{i}.obj") for i in range(4)]
    host_calls.clear()
    writers.save_obj_batch(verts, faces, paths)
    assert host_calls == [(5023, 3)]  # the flagged mesh alone went through the host formatter
    host_calls.clear()
    for i, path in enumerate(paths):
        assert open(path, "rb").read().decode("ascii") == writers.obj_text(v[i], faces + 1.0), i
    text = open(paths[1]).read()
    assert "nan" in text and "inf" in text and "-inf" in text and "137438953472.00000000" in text


def test_save_obj_batch_cuda_and_cpu_write_identical_files(tmp_path, meshes, static, host_calls):
    faces = static["faces"]
    rng = np.random.default_rng(3)
    v = np.stack([meshes[n][0] for n in ("metre", "pixel", "edge", "pixel", "metre")])
    v[3] += rng.normal(0, 2.0, v[3].shape).astype(np.float32)
    v[4] *= rng.normal(1, 0.1, v[4].shape).astype(np.float32)
    verts = torch.from_numpy(v).cuda()
    gpu = [str(tmp_path / f"gpu{i}.obj") for i in range(5)]
    cpu = [str(tmp_path / f"cpu{i}.obj") for i in range(5)]
    forced = [str(tmp_path / f"host{i}.obj") for i in range(5)]
    writers.save_obj_batch(verts, faces, gpu)
    assert host_calls == []
    writers.save_obj_batch(verts.cpu(), faces, cpu)
    writers.save_obj_batch(verts, faces, forced, formatter="host")
    assert len(host_calls) == 10
    for a, b, c in zip(gpu, cpu, forced):
        data = open(a, "rb").read()
        assert data == open(b, "rb").read() == open(c, "rb").read()
        assert data.count(b"\nf ") == len(faces)


def test_save_obj_from_params_matches_save_obj_batch(tmp_path, flame_model, static):
    hm = HeadMesh(flame_model=flame_model, static=static, device=0)
    params = torch.from_numpy(synthetic.synthetic_params(3 * 64, seed=77)).cuda()
    faces = static["faces"]
    piped = [str(tmp_path / f"p{i}.obj") for i in range(len(params))]
    whole = [str(tmp_path / f"w{i}.obj") for i in range(len(params))]
    writers.save_obj_from_params(hm, params, piped, faces=faces, batch_size=64)
    writers.save_obj_batch(hm.vertices_3d(params), faces, whole)
    host = [str(tmp_path / f"h{i}.obj") for i in (0, 100, 191)]
    writers.save_obj_batch(hm.vertices_3d(params)[[0, 100, 191]].cpu(), faces, host)
    for i, (a, b) in enumerate(zip(piped, whole)):
        assert open(a, "rb").read() == open(b, "rb").read(), i
    for i, h in zip((0, 100, 191), host):
        assert open(piped[i], "rb").read() == open(h, "rb").read(), i
    short = [str(tmp_path / f"s{i}.obj") for i in range(70)]  # a last batch that is not full, default faces
    writers.save_obj_from_params(hm, params[:70], short, batch_size=32)
    for i in (0, 31, 32, 63, 64, 69):
        assert open(short[i], "rb").read() == open(whole[i], "rb").read(), i


def test_two_runs_and_a_graph_replay_give_identical_buffers(meshes):
    order = [NAMES[i % 3] for i in range(64)]
    verts = torch.from_numpy(np.stack([meshes[n][0] for n in order])).cuda()
    want = [b"".join(meshes[n][1]) for n in order]
    fmt = writers.ObjFormatter(5023, device=0)
    fmt.reserve(64)
    fmt._text.fill_(0)
    fmt.format(verts)
    torch.cuda.synchronize()
    first = fmt._text.clone()
    fmt._text.fill_(0)
    fmt.format(verts)
    torch.cuda.synchronize()
    assert torch.equal(first, fmt._text)  # deterministic
    src = torch.zeros_like(verts)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fmt.format(src)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        text = fmt.format(src)  # no allocation, no sync: capturable
    src.copy_(verts)
    fmt._text.fill_(0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(first, fmt._text)
    assert [bytes(x) for x in text.to_host()] == want


def test_other_layouts_and_dtypes(tmp_path, meshes, static, host_calls):
    """Decision: `ObjFormatter.format` refuses what the kernel cannot read with a ValueError that names the argument;
    `save_obj_batch` / `obj_text_batch` send such a tensor down the host path."""
    faces = static["faces"]
    v = torch.from_numpy(np.stack([meshes["metre"][0], meshes["pixel"][0]])).cuda()
    fmt = writers.ObjFormatter(5023, device=0)
    strided = v.transpose(1, 2).contiguous().transpose(1, 2)  # same values, not contiguous
    assert not strided.is_contiguous()
    for bad in (strided, v.double(), v.cpu(), v[:, :100]):
        with pytest.raises(ValueError, match="vertices"):
            fmt.format(bad)
    paths = [str(tmp_path / f"{k}{i}.obj") for k in "abc" for i in range(2)]
    writers.save_obj_batch(v, faces, paths[0:2])
    assert host_calls == []
    writers.save_obj_batch(strided, faces, paths[2:4])
    assert len(host_calls) == 2
    writers.save_obj_batch(v.double(), faces, paths[4:6])
    assert len(host_calls) == 4
    for i in range(2):
        assert open(paths[i], "rb").read() == open(paths[2 + i], "rb").read() == open(paths[4 + i], "rb").read()
