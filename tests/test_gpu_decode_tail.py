"""GPU: the two ends of a pipelined decode launch (csrc/flame_decode_pipe.hip, profiles/r07_kernel_log.md).

* The LAST half-block of a launch (or chunk) is finished behind the last barrier by all eight waves, in a lane layout of its own. The
  sizes below are the smallest at which a tail can go wrong, whichever way it is cut (they also held the row-block tail of
  profiles/r07_tail_rowblocks_experiment.patch): the first 16-image row block of the last half-block with one live row (33), one short
  / full / one over (47, 48, 49), the ragged and the full end (63, 64), a steady-state half-block in front of the last (65, 96), and the
  single half-block (32). Every row must come out with the BITS it has in a half-block that is not the last (another code path,
  another lane layout, another constants slot, the same accumulation order).
* The landmark slots and `translation z := 0` leave as write-through stores: nothing else is written, every slot is written (also
  along the chain of duplicate indices), and the values are there for a reader ordered behind the launch by an event only.
"""
import numpy as np
import pytest
import torch

from dad_3dheads_amd import landmarks, synthetic
from dad_3dheads_amd.head_mesh import HeadMesh
from oracle import flame_ref

pytestmark = pytest.mark.gpu
TOL_V, TOL_PX = 5e-6, 1e-3  # the bars of tests/test_gpu_decode.py (north star: 1e-4 abs)
SIZES = [32, 33, 47, 48, 49, 63, 64, 65, 96]
HOST = 128       # rows of the host batch: four half-blocks, the rows under test end with its third
TZ = 409 + 2     # translation z in the dad_3dnet.yaml params layout
KEYS = ("verts3d", "proj", "lmk_xy", "lmk_px")


def _offset(batch):
    return 96 - batch  # the batch's rows inside the host batch: rows [96 - B, 96), half-blocks 0..2 of 4, other positions inside them


def _poisoned(batch, n_lmk, to_2d=True, vertex_outputs=True):
    """Output buffers in which a slot the kernel skipped shows (NaN / a pixel no projection has)."""
    out = {"lmk_xy": torch.full((batch, n_lmk, 2), float("nan"), device="cuda"),
           "lmk_px": torch.full((batch, n_lmk, 2), -(1 << 30), dtype=torch.int32, device="cuda")}
    if vertex_outputs:
        out["verts3d"] = torch.full((batch, 5023, 3), float("nan"), device="cuda")
        out["proj"] = torch.full((batch, 5023, 2 if to_2d else 3), float("nan"), device="cuda")
    return out


@pytest.fixture(scope="module")
def lmk445(static):
    return torch.from_numpy(landmarks.canonical("445", static)).cuda()


@pytest.fixture(scope="module")
def pipe(flame_model, static):
    hm = HeadMesh(flame_model=flame_model, landmarks=landmarks.canonical("445", static), static=static, device=0)
    hm.flame.select_kernel("pipelined")  # raises instead of falling back
    return hm


@pytest.fixture(scope="module")
def auto(flame_model, static):
    """An unpinned handle: a landmark-only launch takes the landmark sub-model, the CHUNKED instantiation of the same kernel."""
    return HeadMesh(flame_model=flame_model, landmarks=landmarks.canonical("445", static), static=static, device=0)


@pytest.fixture(scope="module")
def host(pipe, flame_consts):
    """The host batch, decoded once per projection form, and the oracle on its rows (read-only for every test)."""
    params = synthetic.synthetic_params(HOST, seed=9100)
    got = {}
    for to_2d in (True, False):
        got[to_2d] = pipe.decode(torch.from_numpy(params).cuda(), to_2d=to_2d, landmarks=True, landmarks_px=True, mutate=False)
    torch.cuda.synchronize()
    p = torch.from_numpy(params.copy())
    ref = {"verts3d": flame_ref.vertices_3d(flame_consts, p).numpy(),
           "proj": flame_ref.reprojected_vertices(flame_consts, p, to_2d=False).numpy()}
    return params, got, ref


@pytest.mark.parametrize("to_2d", [True, False], ids=["to2d", "proj3"])
@pytest.mark.parametrize("batch", SIZES)
def test_rows_of_the_last_half_block_have_the_bits_of_any_other(pipe, host, lmk445, batch, to_2d):
    params, got, ref = host
    o = _offset(batch)
    out = pipe.decode(torch.from_numpy(params[o:o + batch]).cuda(), to_2d=to_2d, landmarks=True, landmarks_px=True, mutate=False,
                      out=_poisoned(batch, 445, to_2d))
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(out[k], got[to_2d][k][o:o + batch]), k  # row for row, bit for bit (and no slot left poisoned)
    err_v = np.abs(out["verts3d"].cpu().numpy() - ref["verts3d"][o:o + batch]).max()
    err_p = np.abs(out["proj"].cpu().numpy() - ref["proj"][o:o + batch, :, :2 if to_2d else 3]).max()
    print(f"B={batch} to_2d={to_2d}: |dv|={err_v:.2e} |dproj|={err_p:.2e}")
    assert err_v < TOL_V and err_p < TOL_PX
    assert torch.equal(out["lmk_xy"], out["proj"][:, lmk445, :2])
    assert torch.equal(out["lmk_px"], out["proj"][:, lmk445, :2].int())  # numpy .astype(int): toward zero


@pytest.mark.parametrize("batch", SIZES)
def test_landmark_only_launches_of_the_same_rows(auto, host, batch):
    """The sub-model's launch (chunks of one half-block at these sizes) writes the landmark rows of the full launch, bit for bit."""
    params, got, _ = host
    o = _offset(batch)
    out = auto.decode(torch.from_numpy(params[o:o + batch]).cuda(), verts3d=False, proj=False, landmarks=True, landmarks_px=True,
                      mutate=False, out=_poisoned(batch, 445, vertex_outputs=False))
    torch.cuda.synchronize()
    assert torch.equal(out["lmk_xy"], got[True]["lmk_xy"][o:o + batch])
    assert torch.equal(out["lmk_px"], got[True]["lmk_px"][o:o + batch])


# landmark-only launches whose CHUNKS hold two or more half-blocks (23 tiles -> up to 11 chunks: from 12 half-blocks on), so that a
# chunk of the chunked instantiation has a pipeline in front of its tail: 353 = chunks of 2, the last one 32 + 1 rows; 720 = chunks of 3,
# the last one 32 + 16
@pytest.mark.parametrize("batch", [353, 720])
def test_landmark_only_chunks_of_several_half_blocks(auto, pipe, batch):
    params = synthetic.synthetic_params(batch, seed=9200 + batch)
    full = pipe.decode(torch.from_numpy(params).cuda(), landmarks=True, landmarks_px=True, mutate=False)
    out = auto.decode(torch.from_numpy(params).cuda(), verts3d=False, proj=False, landmarks=True, landmarks_px=True, mutate=False,
                      out=_poisoned(batch, 445, vertex_outputs=False))
    torch.cuda.synchronize()
    assert torch.equal(out["lmk_xy"], full["lmk_xy"])
    assert torch.equal(out["lmk_px"], full["lmk_px"])


@pytest.mark.parametrize("batch", [33, 64])
def test_duplicate_landmark_indices_walk_the_chain_in_both_tail_layouts(flame_model, static, batch):
    """The 565 list, and behind it vertices listed again: twice (the second slot a lane keeps), three and four times (the chain in
    memory behind it) -- among them the list's first vertex, vertex 0 and the last vertex of the partial last tile."""
    base = landmarks.canonical("565", static)
    idx = np.concatenate([base, base[:3], base[:1], base[:1], [5022, 0, 5022, 0, 5022]]).astype(np.int64)
    assert np.bincount(idx).max() >= 4
    hm = HeadMesh(flame_model=flame_model, landmarks=idx, static=static, device=0)
    hm.flame.select_kernel("pipelined")
    p = torch.from_numpy(synthetic.synthetic_params(batch, seed=9300 + batch)).cuda()
    out = hm.decode(p, landmarks=True, landmarks_px=True, out=_poisoned(batch, len(idx)))
    torch.cuda.synchronize()
    gather = out["proj"][:, torch.from_numpy(idx).cuda()]
    assert torch.equal(out["lmk_xy"], gather)  # every slot written (none left NaN) and equal to the gather
    assert torch.equal(out["lmk_px"], gather.int())


@pytest.mark.parametrize("kernel", ["pipelined", "split_bf16", "split_f16"])
@pytest.mark.parametrize("batch", [33, 64])
def test_mutate_params_writes_translation_z_and_nothing_else(flame_model, static, kernel, batch):
    hm = HeadMesh(flame_model=flame_model, landmarks=landmarks.canonical("445", static), static=static, device=0)
    hm.flame.select_kernel(kernel)
    before = synthetic.synthetic_params(batch, seed=9400 + batch)
    before[:, TZ] = np.linspace(0.25, 0.75, batch, dtype=np.float32)  # nothing here is zero to begin with
    kept, mutated = torch.from_numpy(before).cuda(), torch.from_numpy(before).cuda()
    hm.decode(kept, landmarks_px=True, mutate=False)
    hm.decode(mutated, landmarks_px=True, mutate=True)
    torch.cuda.synchronize()
    bits = torch.from_numpy(before).view(torch.int32)
    assert torch.equal(kept.cpu().view(torch.int32), bits)  # bytewise untouched
    want = bits.clone()
    want[:, TZ] = 0  # +0.0f
    assert torch.equal(mutated.cpu().view(torch.int32), want)


def test_written_through_values_reach_a_reader_ordered_by_an_event_only(pipe, host):
    """The launch on one stream, the copy to the host on another, an event between them and nothing else; then a second launch with
    other params into other buffers, which must leave the first one's values alone."""
    params, got, _ = host
    batch = 64
    o = _offset(batch)
    first = torch.from_numpy(params[o:o + batch].copy())
    first[:, TZ] = 0.5
    first = first.cuda()
    bufs = _poisoned(batch, 445)
    pinned_px = torch.empty((batch, 445, 2), dtype=torch.int32).pin_memory()
    pinned_xy = torch.empty((batch, 445, 2), dtype=torch.float32).pin_memory()
    pinned_tz = torch.empty((batch,), dtype=torch.float32).pin_memory()
    torch.cuda.synchronize()
    launch, reader = torch.cuda.Stream(), torch.cuda.Stream()
    done = torch.cuda.Event()
    with torch.cuda.stream(launch):
        pipe.decode(first, landmarks=True, landmarks_px=True, mutate=True, out=bufs)
        done.record(launch)
    with torch.cuda.stream(reader):
        reader.wait_event(done)
        pinned_px.copy_(bufs["lmk_px"], non_blocking=True)
        pinned_xy.copy_(bufs["lmk_xy"], non_blocking=True)
        pinned_tz.copy_(first[:, TZ], non_blocking=True)
    reader.synchronize()
    assert torch.equal(pinned_px, got[True]["lmk_px"][o:o + batch].cpu())
    assert torch.equal(pinned_xy, got[True]["lmk_xy"][o:o + batch].cpu())
    assert torch.equal(pinned_tz, torch.zeros(batch))
    other = torch.from_numpy(synthetic.synthetic_params(batch, seed=9500)).cuda()
    with torch.cuda.stream(launch):
        pipe.decode(other, landmarks=True, landmarks_px=True, mutate=True, out=_poisoned(batch, 445))
    torch.cuda.synchronize()
    assert torch.equal(bufs["lmk_px"], got[True]["lmk_px"][o:o + batch])
    assert torch.equal(bufs["lmk_xy"], got[True]["lmk_xy"][o:o + batch])
    assert torch.equal(first[:, TZ].cpu(), torch.zeros(batch))
