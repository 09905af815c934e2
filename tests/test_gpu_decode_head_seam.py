"""GPU: the seams of whole-mesh launches of 49..64 rows (csrc/flame_decode_head.hip): between pass 1 (rows 0..47) and the chain of rows
48..63, whose hooks and whose neighbours, the stagers, read pass 1's parked accumulators, and between the chain and the tail. The stagers
finish vertices 16..19 of rows 0..47 in one call of 48 lanes, and the tail reads its constants, its vertex-table row, masks and offsets in
front of the last barrier. Whatever stands at the seams -- a workgroup barrier, or the arrival words of profiles/r12_seam_experiment.patch --
no bit may change: the rows of a launch are `torch.equal` to the same rows inside a batch of 128, which takes the unchanged pipelined kernel
(the construction of tests/test_gpu_decode_head.py), and a launch never shows a row of the launch before it on the same CUs."""
import numpy as np
import pytest
import torch

from dad_3dheads_amd import landmarks, synthetic
from dad_3dheads_amd.head_mesh import HeadMesh
from guarded import Guarded

pytestmark = pytest.mark.gpu
SIZES = [49, 56, 64]  # one live row in the chain's row block, half of it, all of it
KEYS = ("verts3d", "proj", "lmk_xy", "lmk_px")
V, N_LMK, TILE = 5023, 445, 20
LAST_TILE = slice((V // TILE) * TILE, V)  # 3 live vertices of 20
TILE_0 = slice(0, TILE)
assert LAST_TILE.stop - LAST_TILE.start == 3


@pytest.fixture(scope="module")
def mesh(flame_model, static):
    return HeadMesh(flame_model=flame_model, landmarks=landmarks.canonical("445", static), static=static, device=0)


def decode(mesh, p, to_2d=True, **kw):
    return mesh.decode(p, to_2d=to_2d, landmarks=True, landmarks_px=True, **kw)


_pipelined = {}


def pipelined(mesh, batch, to_2d):
    """(the seeded rows, every output of the same rows at 0.. of a batch of 128, its params after the launch), once per (batch, projection)."""
    key = (batch, to_2d)
    if key not in _pipelined:
        rows = synthetic.synthetic_params(batch, seed=9900 + batch)
        big = synthetic.synthetic_params(128, seed=9950 + batch)
        big[:batch] = rows
        p_big = torch.from_numpy(big).cuda()
        ref = decode(mesh, p_big, to_2d=to_2d, mutate=True)
        torch.cuda.synchronize()
        _pipelined[key] = (rows, ref, p_big)
    return _pipelined[key]


@pytest.mark.parametrize("outputs", ["verts3d", "proj", "both"])  # which of the hooks' and the stagers' stores run
@pytest.mark.parametrize("to_2d", [True, False])
@pytest.mark.parametrize("batch", SIZES)
def test_sizes_and_outputs(mesh, batch, to_2d, outputs):
    rows, ref, p_big = pipelined(mesh, batch, to_2d)
    p = torch.from_numpy(rows).cuda()
    got = decode(mesh, p, to_2d=to_2d, mutate=True, verts3d=outputs != "proj", proj=outputs != "verts3d")
    torch.cuda.synchronize()
    wanted = [k for k in KEYS if k in ("lmk_xy", "lmk_px") or outputs in (k, "both")]
    for k in wanted:
        assert torch.equal(got[k], ref[k][:batch]), (batch, to_2d, outputs, k)
    assert torch.equal(p, p_big[:batch])  # params after the launch


def test_alternating_sizes_without_a_synchronise(mesh):
    """64, 48, 49, 64, ... on one stream and one handle, two inputs per size, sixteen launches: a hook or a stager that read the accumulator
    tile before this launch's park, an mma wave that read rows 48..63 or the vertex table before this launch's arrival, or an arrival word
    that was not zeroed shows as another launch's row (or as a hang)."""
    sizes = [64, 48, 49]
    ins = {(b, j): torch.from_numpy(synthetic.synthetic_params(b, seed=9800 + 2 * b + j)).cuda() for b in sizes for j in range(2)}
    alone = {}
    for key, p in ins.items():  # each alone, synchronised
        alone[key] = decode(mesh, p, mutate=False)
        torch.cuda.synchronize()
    order = [(sizes[i % 3], (i // 3) & 1) for i in range(16)]
    runs = [decode(mesh, ins[key], mutate=False) for key in order]  # back to back
    torch.cuda.synchronize()
    for b in sizes:
        assert not torch.equal(alone[(b, 0)]["verts3d"], alone[(b, 1)]["verts3d"])
    for i, (key, r) in enumerate(zip(order, runs)):
        for k in KEYS:
            assert torch.equal(r[k], alone[key][k]), (i, key, k)


@pytest.mark.parametrize("differ", ["rows 0..47", "rows 48..63"])
def test_late_reader(mesh, differ):
    """Two 64-row inputs that differ only in the rows of one pass, alternated back to back. A reader that runs ahead of the park (rows 0..47)
    or a chain fed a stale fragment (rows 48..63) shows as a row of the other input."""
    x = synthetic.synthetic_params(64, seed=9700)
    y = synthetic.synthetic_params(64, seed=9701)
    same = slice(48, 64) if differ == "rows 0..47" else slice(0, 48)
    y[same] = x[same]
    named = 5 if differ == "rows 0..47" else 50  # a row of the hooks (wave 0) / of the chain's row block
    dev = [torch.from_numpy(v).cuda() for v in (x, y)]
    alone = []
    for p in dev:
        alone.append(decode(mesh, p, mutate=False))
        torch.cuda.synchronize()
    assert torch.equal(alone[0]["verts3d"][same], alone[1]["verts3d"][same])
    assert not torch.equal(alone[0]["verts3d"][named], alone[1]["verts3d"][named])
    runs = [decode(mesh, dev[i & 1], mutate=False) for i in range(12)]
    torch.cuda.synchronize()
    for i, r in enumerate(runs):
        mine, other = alone[i & 1], alone[1 - (i & 1)]
        for k in ("verts3d", "proj"):
            for tile, name in ((LAST_TILE, "the last tile (3 live vertices)"), (TILE_0, "tile 0")):
                if not torch.equal(r[k][named, tile], mine[k][named, tile]):
                    whose = "the OTHER input's" if torch.equal(r[k][named, tile], other[k][named, tile]) else "neither input's"
                    pytest.fail(f"launch {i} ({differ} differ): {k} row {named} of {name} is {whose}")
        for k in KEYS:
            assert torch.equal(r[k], mine[k]), (i, k)


@pytest.mark.parametrize("to_2d", [True, False])
def test_49_rows_between_guard_words(mesh, to_2d):
    """B = 49: rows 49..63 of the A image re-read row 48 and write nothing -- in the chain's tail, and in the stagers' call of 48 lanes, whose
    lanes 32..47 take rows 32..47 and whose lanes 48..63 take nothing. Every output sits between guard words."""
    batch = 49
    rows, ref, p_big = pipelined(mesh, batch, to_2d)
    c = 2 if to_2d else 3
    g = {"verts3d": Guarded(batch * V * 3, torch.float32), "proj": Guarded(batch * V * c, torch.float32),
         "lmk_xy": Guarded(batch * N_LMK * 2, torch.float32), "lmk_px": Guarded(batch * N_LMK * 2, torch.int32)}
    shapes = {"verts3d": (batch, V, 3), "proj": (batch, V, c), "lmk_xy": (batch, N_LMK, 2), "lmk_px": (batch, N_LMK, 2)}
    p = torch.from_numpy(rows).cuda()
    decode(mesh, p, to_2d=to_2d, mutate=True, out={k: g[k].body.view(shapes[k]) for k in KEYS})
    torch.cuda.synchronize()
    for k in KEYS:
        got = g[k].host().reshape(shapes[k])  # (asserts the guard words)
        assert np.array_equal(got, ref[k][:batch].cpu().numpy()), k
    assert torch.equal(p, p_big[:batch])
