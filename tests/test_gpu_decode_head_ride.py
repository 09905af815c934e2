"""GPU: rows 48..63 of whole-mesh launches of 49..64 rows (csrc/flame_decode_head.hip), whose k-slices may be multiplied at another time than
those of rows 0..47 -- behind pass 1 as a chain today, inside pass 1 in the ride experiment of profiles/r11_kernel_log.md -- and whose
vertices are finished by three different roles. Whatever the schedule, every accumulator sums each k-slice once and in order: the rows of
a launch are `torch.equal` to the same rows inside a batch of 128, which takes the unchanged pipelined kernel (the construction of
tests/test_gpu_decode_head.py).

An MFMA (G, s) of the basis pack multiplies k = 16 G + 4 j + s, j = 0..3. The seam indices below lie either side of every hand-over a
schedule of block 3's accumulator can have: s = 1 | 2 inside a group (k 1 | 2), two groups (15 | 16), the A slabs the stagers publish one
by one (127 | 128, 255 | 256, 383 | 384), the end of a 13-group ride and the start of its chain (207 | 208 = 16 n - 1 | 16 n), and the
last beta against the pose feature (399). A dropped or doubled slice changes a one-hot row by whole terms, not by rounding."""
import numpy as np
import pytest
import torch

from dad_3dheads_amd import landmarks, synthetic
from dad_3dheads_amd.head_mesh import HeadMesh
from guarded import Guarded

pytestmark = pytest.mark.gpu
SIZES = [50, 57, 64]
KEYS = ("verts3d", "proj", "lmk_xy", "lmk_px")
SEAM_K = [1, 2, 15, 16, 127, 128, 207, 208, 255, 256, 383, 384, 399]  # in the pack's k order
N_BETA = 400
V, N_LMK = 5023, 445


@pytest.fixture(scope="module")
def mesh(flame_model, static):
    return HeadMesh(flame_model=flame_model, landmarks=landmarks.canonical("445", static), static=static, device=0)


def decode(mesh, rows, to_2d=True, **kw):
    return mesh.decode(torch.from_numpy(rows).cuda(), to_2d=to_2d, landmarks=True, landmarks_px=True, **kw)


@pytest.mark.parametrize("to_2d", [True, False])
@pytest.mark.parametrize("batch", SIZES)
def test_rows_equal_the_pipelined_kernels(mesh, batch, to_2d):
    rows = synthetic.synthetic_params(batch, seed=9500 + batch)
    big = synthetic.synthetic_params(128, seed=9600 + batch)
    big[:batch] = rows
    big[64:64 + batch] = rows
    p_small, p_big = torch.from_numpy(rows).cuda(), torch.from_numpy(big).cuda()
    small = mesh.decode(p_small, to_2d=to_2d, landmarks=True, landmarks_px=True, mutate=True)
    ref = mesh.decode(p_big, to_2d=to_2d, landmarks=True, landmarks_px=True, mutate=True)
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(small[k], ref[k][:batch]), (k, "rows 0..")
        assert torch.equal(small[k], ref[k][64:64 + batch]), (k, "rows 64..")
    assert torch.equal(p_small, p_big[:batch]) and torch.equal(p_small, p_big[64:64 + batch])  # params after the launch


def one_hot_rows(batch, seed):
    """For each seam index k a pair of rows whose betas are zero but for beta k (pose, rotation, translation and scale stay seeded): the
    pair goes to rows 48 and batch - 1 of the launch made for k."""
    rows = synthetic.synthetic_params(2 * len(SEAM_K), seed=seed)
    value = rows[:, :N_BETA].copy()
    rows[:, :N_BETA] = 0.0
    for i, k in enumerate(SEAM_K):
        for r in (2 * i, 2 * i + 1):
            rows[r, k] = value[r, k] if value[r, k] != 0.0 else 1.5
    return rows


@pytest.mark.parametrize("batch", SIZES)
def test_one_hot_rows_at_the_seams_of_k(mesh, batch):
    base = synthetic.synthetic_params(batch, seed=9700 + batch)
    hot = one_hot_rows(batch, seed=9800 + batch)
    big = synthetic.synthetic_params(128, seed=9900 + batch)
    big[:batch] = base
    big[64:64 + len(hot)] = hot
    ref = decode(mesh, big)  # every row here is the pipelined kernel's
    torch.cuda.synchronize()
    for i, k in enumerate(SEAM_K):
        rows = base.copy()
        rows[48], rows[batch - 1] = hot[2 * i], hot[2 * i + 1]
        got = decode(mesh, rows)
        torch.cuda.synchronize()
        others = torch.tensor([r for r in range(batch) if r not in (48, batch - 1)], device="cuda")
        for key in KEYS:
            assert torch.equal(got[key][48], ref[key][64 + 2 * i]), (k, key, "row 48")
            assert torch.equal(got[key][batch - 1], ref[key][64 + 2 * i + 1]), (k, key, "last row")
            assert torch.equal(got[key][others], ref[key][others]), (k, key, "the other rows")
        assert not torch.equal(got["verts3d"][48], got["verts3d"][batch - 1])  # (two different inputs)


@pytest.mark.parametrize("k", [37, 300])  # a k of the first 13 groups (the ride experiment's) and one of the chain in either schedule
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_poison_in_row_48_of_49_stays_there(mesh, k, bad):
    """B = 49: row 48 is the last row of the batch and the only live row of its row block -- rows 49..63 of the A image re-read it and must
    write nothing. Every output sits between guard words."""
    batch = 49
    clean = synthetic.synthetic_params(batch, seed=9310)
    a = decode(mesh, clean)
    dirty = clean.copy()
    dirty[48, k] = bad
    g = {"verts3d": Guarded(batch * V * 3, torch.float32), "proj": Guarded(batch * V * 2, torch.float32),
         "lmk_xy": Guarded(batch * N_LMK * 2, torch.float32), "lmk_px": Guarded(batch * N_LMK * 2, torch.int32)}
    shapes = {"verts3d": (batch, V, 3), "proj": (batch, V, 2), "lmk_xy": (batch, N_LMK, 2), "lmk_px": (batch, N_LMK, 2)}
    decode(mesh, dirty, out={key: g[key].body.view(shapes[key]) for key in KEYS})
    torch.cuda.synchronize()
    for key in KEYS:
        got = g[key].host().reshape(shapes[key])  # (asserts the guard words)
        assert np.array_equal(got[:48], a[key][:48].cpu().numpy()), key
    assert not np.isfinite(g["proj"].host().reshape(shapes["proj"])[48]).all()  # the poisoned row is not silently "repaired"


def test_two_inputs_alternating_back_to_back(mesh):
    """Twelve launches of two different 64-row inputs, alternating, on one stream without a synchronisation between them: a launch that
    read A rows or constants before this launch's own arrival would see the other input's."""
    ins = [synthetic.synthetic_params(64, seed=9410 + i) for i in range(2)]
    dev = [torch.from_numpy(x).cuda() for x in ins]
    first = []
    for p in dev:
        first.append(mesh.decode(p, to_2d=True, landmarks=True, landmarks_px=True))
        torch.cuda.synchronize()
    runs = [mesh.decode(dev[i & 1], to_2d=True, landmarks=True, landmarks_px=True) for i in range(12)]
    torch.cuda.synchronize()
    assert not torch.equal(first[0]["verts3d"], first[1]["verts3d"])
    for i, r in enumerate(runs):
        for key in KEYS:
            assert torch.equal(r[key], first[i & 1][key]), (i, key)
