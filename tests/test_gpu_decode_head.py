"""GPU: the decode kernel of whole-mesh launches of 33..64 rows (csrc/flame_decode_head.hip: rows 0..47 multiply while the basis streams in,
rows 48..63 behind it) against the unchanged pipelined kernel -- the same rows inside a batch of 128 take it -- bit for bit, and against the
CPU oracle at the project's bars. Sizes: one row into the second 16-row block of pass 1's third row block (33), either side of the end of
pass 1 (47, 48, 49: 48 is the last launch without a pass 2) and of the full launch (63, 64)."""
import numpy as np
import pytest
import torch

from dad_3dheads_amd import landmarks, synthetic
from dad_3dheads_amd.head_mesh import HeadMesh
from guarded import Guarded
from oracle import flame_ref

pytestmark = pytest.mark.gpu
TOL_V, TOL_PX = 5e-6, 1e-3  # the bars of tests/test_gpu_decode.py
SIZES = [33, 47, 48, 49, 63, 64]
KEYS = ("verts3d", "proj", "lmk_xy", "lmk_px")
V, N_LMK = 5023, 445


@pytest.fixture(scope="module")
def mesh(flame_model, static):
    # the default choice of kernel: what a caller gets (33..64 rows with a vertex output: the 48 + 16 kernel; anything else: as before)
    return HeadMesh(flame_model=flame_model, landmarks=landmarks.canonical("445", static), static=static, device=0)


def duplicate_positions(batch):
    return [r for r in sorted({0, 31, 32, 47, 48, batch - 1}) if r < batch]


def seeded_rows(batch):
    """`batch` seeded rows with ONE row repeated at every seam of the kernel: first and last row of the first two row blocks' hook layout, the
    last row of pass 1, the first of pass 2, the last of the launch."""
    rows = synthetic.synthetic_params(batch, seed=9100 + batch)
    rows[duplicate_positions(batch)] = rows[5]
    return rows


_decoded = {}


def decoded(mesh, batch, to_2d):
    """(outputs of the launch of `batch` rows, its params after the launch, outputs of the same rows at 0.. and 64.. of a batch of 128, its
    params after the launch), computed once per (batch, projection)."""
    key = (batch, to_2d)
    if key not in _decoded:
        rows = seeded_rows(batch)
        big = synthetic.synthetic_params(128, seed=9200 + batch)
        big[:batch] = rows
        big[64:64 + batch] = rows
        p_small, p_big = torch.from_numpy(rows).cuda(), torch.from_numpy(big).cuda()
        small = mesh.decode(p_small, to_2d=to_2d, landmarks=True, landmarks_px=True, mutate=True)
        ref = mesh.decode(p_big, to_2d=to_2d, landmarks=True, landmarks_px=True, mutate=True)
        torch.cuda.synchronize()
        _decoded[key] = (small, p_small, ref, p_big)
    return _decoded[key]


@pytest.mark.parametrize("to_2d", [True, False])
@pytest.mark.parametrize("batch", SIZES)
def test_bits_of_the_unchanged_pipeline(mesh, batch, to_2d):
    small, p_small, ref, p_big = decoded(mesh, batch, to_2d)
    for k in KEYS:
        assert torch.equal(small[k], ref[k][:batch]), (k, "rows 0..")
        assert torch.equal(small[k], ref[k][64:64 + batch]), (k, "rows 64..")
    # MUTATE_PARAMS: translation z := 0 in every row of the batch, nothing else touched
    assert torch.equal(p_small, p_big[:batch]) and torch.equal(p_small, p_big[64:64 + batch])
    expect = torch.from_numpy(seeded_rows(batch)).cuda()
    expect[:, 411] = 0.0
    assert torch.equal(p_small, expect)
    dup = torch.tensor(duplicate_positions(batch), device="cuda")
    for k in KEYS:
        rows = small[k][dup]
        assert torch.equal(rows, rows[:1].expand_as(rows)), k


_oracle = {}


def oracle(flame_consts, batch):
    if batch not in _oracle:
        p = torch.from_numpy(seeded_rows(batch))
        _oracle[batch] = (flame_ref.vertices_3d(flame_consts, p.clone()).numpy(), flame_ref.reprojected_vertices(flame_consts, p.clone(), to_2d=False).numpy())
    return _oracle[batch]


@pytest.mark.parametrize("to_2d", [True, False])
@pytest.mark.parametrize("batch", SIZES)
def test_matches_the_oracle(mesh, flame_consts, static, batch, to_2d):
    small = decoded(mesh, batch, to_2d)[0]
    v_ref, p3_ref = oracle(flame_consts, batch)
    p_ref = p3_ref[..., :2] if to_2d else p3_ref
    err_v = np.abs(small["verts3d"].cpu().numpy() - v_ref).max()
    err_p = np.abs(small["proj"].cpu().numpy() - p_ref).max()
    print(f"B = {batch} to_2d = {to_2d}: 3-D {err_v:.3g}, projection {err_p:.3g} px")
    assert err_v < TOL_V and err_p < TOL_PX
    lm = landmarks.canonical("445", static)
    ref_xy = p3_ref[:, lm, :2]
    assert np.abs(small["lmk_xy"].cpu().numpy() - ref_xy).max() < TOL_PX
    d = np.abs(small["lmk_px"].cpu().numpy() - ref_xy.astype(np.int32))  # demo_utils.py:42-46: truncation
    near_integer = np.abs(ref_xy - np.round(ref_xy)) < 1e-3
    assert ((d == 0) | ((d == 1) & near_integer)).all()


@pytest.mark.parametrize("with_landmarks", [False, True])
@pytest.mark.parametrize("only", ["verts3d", "proj"])
@pytest.mark.parametrize("batch", [33, 49])
def test_output_subsets_between_guard_words(mesh, batch, only, with_landmarks):
    """One vertex output with a null pointer for the other, with and without landmarks. 33 and 49 rows: pass 1's (pass 2's) rows past the
    batch re-read its last row and must write nothing -- every output sits between guard words."""
    full = decoded(mesh, batch, True)[0]
    g = {"verts3d": Guarded(batch * V * 3, torch.float32), "proj": Guarded(batch * V * 2, torch.float32),
         "lmk_xy": Guarded(batch * N_LMK * 2, torch.float32), "lmk_px": Guarded(batch * N_LMK * 2, torch.int32)}
    shapes = {"verts3d": (batch, V, 3), "proj": (batch, V, 2), "lmk_xy": (batch, N_LMK, 2), "lmk_px": (batch, N_LMK, 2)}
    wanted = [only] + (["lmk_xy", "lmk_px"] if with_landmarks else [])
    out = {k: g[k].body.view(shapes[k]) for k in wanted}
    p = torch.from_numpy(seeded_rows(batch)).cuda()
    mesh.decode(p, verts3d=only == "verts3d", proj=only == "proj", to_2d=True, landmarks=with_landmarks, landmarks_px=with_landmarks, mutate=True, out=out)
    torch.cuda.synchronize()
    for k, buf in g.items():
        got = buf.host()  # (asserts the guard words)
        if k in wanted:
            assert np.array_equal(got.reshape(shapes[k]), full[k].cpu().numpy()), k
        else:
            assert (got == buf.sentinel).all(), k
    assert torch.equal(p, decoded(mesh, batch, True)[1])


def test_poisoned_rows_poison_only_themselves(mesh):
    """The construction of tests/test_gpu_decode_pipe.py at the seam between the passes: NaN and Inf rows at 47 and 48, in a beta (the GEMM),
    in the jaw (the pose feature columns of the A image) and in the scale (the constants)."""
    clean = synthetic.synthetic_params(64, seed=9300)
    a = mesh.decode(torch.from_numpy(clean).cuda(), to_2d=True, landmarks_px=True)
    for bad in ({47: (5, np.nan), 48: (401, np.inf)}, {47: (412, np.nan), 48: (299, -np.inf)}):
        dirty = clean.copy()
        for row, (col, val) in bad.items():
            dirty[row, col] = val
        b = mesh.decode(torch.from_numpy(dirty).cuda(), to_2d=True, landmarks_px=True)
        torch.cuda.synchronize()
        good = torch.tensor([r for r in range(64) if r not in bad], device="cuda")
        for k in KEYS:
            assert torch.equal(a[k][good], b[k][good]), k
        for row in bad:
            assert not bool(torch.isfinite(b["proj"][row]).all())  # the poisoned row itself is not silently "repaired"


def test_launch_sequences_and_a_graph_replay(mesh):
    """Back-to-back launches of changing sizes on one handle -- the 48 + 16 kernel between launches of the pipelined one --, then a captured
    64-row launch replayed twice: every result equals the first eager result of its input."""
    sizes = [64, 32, 64, 128, 48, 16]
    ins = [synthetic.synthetic_params(b, seed=9400 + i) for i, b in enumerate(sizes)]
    first = []
    for x in ins:  # each alone, synchronised
        first.append(mesh.decode(torch.from_numpy(x).cuda(), to_2d=True, landmarks_px=True))
        torch.cuda.synchronize()
    again = [mesh.decode(torch.from_numpy(x).cuda(), to_2d=True, landmarks_px=True) for x in ins]  # back to back
    torch.cuda.synchronize()
    for b, f, o in zip(sizes, first, again):
        for k in KEYS:
            assert torch.equal(f[k], o[k]), (b, k)
    p = torch.from_numpy(ins[0]).cuda()
    bufs = {"verts3d": torch.empty((64, V, 3), device="cuda"), "proj": torch.empty((64, V, 2), device="cuda"),
            "lmk_xy": torch.empty((64, N_LMK, 2), device="cuda"), "lmk_px": torch.empty((64, N_LMK, 2), dtype=torch.int32, device="cuda")}
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        mesh.decode(p, to_2d=True, landmarks_px=True, out=bufs)  # warm-up on the capture stream
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            mesh.decode(p, to_2d=True, landmarks_px=True, out=bufs)
        for _ in range(2):
            for k in bufs:
                bufs[k].zero_()
            g.replay()
            s.synchronize()
            for k in KEYS:
                assert torch.equal(bufs[k], first[0][k]), k
