"""GPU: the prologue of a pipelined decode launch (csrc/flame_decode_pipe.hip, profiles/r08_kernel_log.md).

Constants round 0 -- Rodrigues of the jaw, the 6-DoF matrix, scale and translation of the launch's first 128 rows, the tail rows
k = 400..415 of the first A image and `translation z := 0` -- is written in front of the first MFMA, among the mma waves' basis requests
(launches and chunks of one half-block: behind group 6 of the first GEMM, as before), and an arrival word in LDS says "round 0 is there"
where a workgroup barrier used to. Rounds r >= 1 stay in the steady state. So:

* every output against the oracle at sizes with partial half-blocks and clamped rows (9, 31, 33), whole ones (32, 64) and both sides of
  the seam between round 0 and round 1 (127, 128, 129, 160);
* one params row placed in round 0 (both half-blocks of a 64-row block), on the seam and in round 1: the same bits everywhere -- the
  moved code rounds like the steady-state code;
* landmark-only launches whose chunks start at a row offset;
* the `translation z := 0` store, which moved with the round; a NaN that must stay in its row; and repeated launches, which differ if a
  reader gets ahead of the arrival word.
"""
import numpy as np
import pytest
import torch

from dad_3dheads_amd import landmarks, synthetic
from dad_3dheads_amd.head_mesh import HeadMesh
from oracle import flame_ref

pytestmark = pytest.mark.gpu
TOL_V, TOL_PX = 5e-6, 1e-3  # the bars of tests/test_gpu_decode.py
SIZES = [9, 31, 32, 33, 64, 127, 128, 129, 160]
ROWS = max(SIZES)  # every batch is a prefix of one 160-row array: one oracle run for all of them
TZ, SCALE, JAW = 411, 412, 400  # columns of the dad_3dnet.yaml params layout
KEYS = ("verts3d", "proj", "lmk_xy", "lmk_px")


def _poisoned(batch, n_lmk=445, to_2d=True, vertex_outputs=True):
    """Output buffers in which a slot the kernel skipped shows (NaN / a pixel no projection has)."""
    out = {"lmk_xy": torch.full((batch, n_lmk, 2), float("nan"), device="cuda"),
           "lmk_px": torch.full((batch, n_lmk, 2), -(1 << 30), dtype=torch.int32, device="cuda")}
    if vertex_outputs:
        out["verts3d"] = torch.full((batch, 5023, 3), float("nan"), device="cuda")
        out["proj"] = torch.full((batch, 5023, 2 if to_2d else 3), float("nan"), device="cuda")
    return out


@pytest.fixture(scope="module")
def lmk445(static):
    return landmarks.canonical("445", static)


@pytest.fixture(scope="module")
def pipe(flame_model, static, lmk445):
    hm = HeadMesh(flame_model=flame_model, landmarks=lmk445, static=static, device=0)
    hm.flame.select_kernel("pipelined")  # raises instead of falling back
    return hm


@pytest.fixture(scope="module")
def auto(flame_model, static, lmk445):
    """An unpinned handle: its landmark-only launches take the landmark sub-model, the CHUNKED instantiation of the same kernel (a
    pinned handle decodes the whole mesh in one chunk)."""
    return HeadMesh(flame_model=flame_model, landmarks=lmk445, static=static, device=0)


@pytest.fixture(scope="module")
def reference(flame_consts):
    """160 params rows and the oracle on them, computed once (read-only for every test)."""
    params = synthetic.synthetic_params(ROWS, seed=8100)
    p = torch.from_numpy(params.copy())
    return params, {"verts3d": flame_ref.vertices_3d(flame_consts, p).numpy(),
                    "proj": flame_ref.reprojected_vertices(flame_consts, p, to_2d=False).numpy()}


@pytest.mark.parametrize("to_2d", [True, False], ids=["to2d", "proj3"])
@pytest.mark.parametrize("batch", SIZES)
def test_every_output_against_the_oracle(pipe, reference, lmk445, batch, to_2d):
    params, ref = reference
    out = pipe.decode(torch.from_numpy(params[:batch]).cuda(), to_2d=to_2d, landmarks=True, landmarks_px=True, mutate=False,
                      out=_poisoned(batch, to_2d=to_2d))
    torch.cuda.synchronize()
    want_v, want_p = ref["verts3d"][:batch], ref["proj"][:batch, :, :2 if to_2d else 3]
    err_v = np.abs(out["verts3d"].cpu().numpy() - want_v).max()
    err_p = np.abs(out["proj"].cpu().numpy() - want_p).max()
    want_l = ref["proj"][:batch][:, lmk445, :2]
    err_l = np.abs(out["lmk_xy"].cpu().numpy() - want_l).max()
    print(f"B={batch} to_2d={to_2d}: |dv|={err_v:.2e} |dproj|={err_p:.2e} |dlmk|={err_l:.2e}")
    assert err_v < TOL_V and err_p < TOL_PX and err_l < TOL_PX  # (NaN left in a poisoned buffer fails these too)
    # integer pixels: equal to the oracle's truncation wherever its float coordinate is not within the bar of an integer
    clear = np.abs(want_l - np.rint(want_l)) > TOL_PX
    px = out["lmk_px"].cpu().numpy()
    assert clear.mean() > 0.99
    assert np.array_equal(px[clear], want_l.astype(np.int64)[clear])
    assert np.abs(px - want_l).max() < 1.0 + TOL_PX  # and no slot left unwritten next to an integer


@pytest.mark.parametrize("to_2d", [True, False], ids=["to2d", "proj3"])
def test_one_row_has_the_same_bits_in_round_0_on_the_seam_and_in_round_1(pipe, reference, to_2d):
    params = reference[0].copy()
    places = [0, 31, 32, 63, 127, 128, 159]
    params[places] = params[77]
    out = pipe.decode(torch.from_numpy(params).cuda(), to_2d=to_2d, landmarks=True, landmarks_px=True, mutate=False,
                      out=_poisoned(ROWS, to_2d=to_2d))
    torch.cuda.synchronize()
    for k in KEYS:
        assert not torch.isnan(out[k][places[0]].float()).any(), k
        for r in places[1:]:
            assert torch.equal(out[k][r], out[k][places[0]]), (k, r)
        assert torch.equal(out[k][77], out[k][places[0]]), k


@pytest.mark.parametrize("batch", [64, 96, 160])
def test_landmark_only_chunks_at_a_row_offset(auto, pipe, reference, batch):
    """23 tiles of the sub-model x chunks of one half-block: every chunk runs the prologue on rows [32 c, 32 c + 32)."""
    p = reference[0][:batch]
    whole = auto.decode(torch.from_numpy(p).cuda(), landmarks=True, landmarks_px=True, mutate=False)
    pinned = pipe.decode(torch.from_numpy(p).cuda(), landmarks=True, landmarks_px=True, mutate=False)
    out = auto.decode(torch.from_numpy(p).cuda(), verts3d=False, proj=False, landmarks=True, landmarks_px=True, mutate=False,
                      out=_poisoned(batch, vertex_outputs=False))
    torch.cuda.synchronize()
    for k in ("lmk_xy", "lmk_px"):
        assert torch.equal(out[k], whole[k]), k
        assert torch.equal(out[k], pinned[k]), k


@pytest.mark.parametrize("batch", [33, 129])
def test_mutate_params_zeroes_column_411_of_every_row_and_nothing_else(pipe, reference, batch):
    before = reference[0][:batch].copy()
    before[:, TZ] = np.linspace(0.25, 0.75, batch, dtype=np.float32)  # nothing here is zero to begin with
    kept, mutated = torch.from_numpy(before).cuda(), torch.from_numpy(before).cuda()
    a = pipe.decode(kept, landmarks=True, landmarks_px=True, mutate=False)
    b = pipe.decode(mutated, landmarks=True, landmarks_px=True, mutate=True)
    torch.cuda.synchronize()
    bits = torch.from_numpy(before).view(torch.int32)
    assert torch.equal(kept.cpu().view(torch.int32), bits)  # bytewise untouched without the flag
    want = bits.clone()
    want[:, TZ] = 0  # +0.0f
    assert torch.equal(mutated.cpu().view(torch.int32), want)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k  # the projection never reads translation z


@pytest.mark.parametrize("row", [5, 37], ids=["first_half_block", "second_half_block"])
@pytest.mark.parametrize("column", [SCALE, JAW], ids=["scale", "jaw"])
def test_a_nan_in_round_0_stays_in_its_row(pipe, reference, column, row):
    batch = 64
    clean_p = reference[0][:batch]
    clean = pipe.decode(torch.from_numpy(clean_p).cuda(), landmarks=True, landmarks_px=True, mutate=False)
    bad_p = clean_p.copy()
    bad_p[row, column] = np.nan
    bad = pipe.decode(torch.from_numpy(bad_p).cuda(), landmarks=True, landmarks_px=True, mutate=False, out=_poisoned(batch))
    torch.cuda.synchronize()
    others = torch.tensor([r for r in range(batch) if r != row], device="cuda")
    for k in KEYS:
        assert torch.equal(bad[k][others], clean[k][others]), k
    assert torch.isnan(bad["proj"][row]).all() and torch.isnan(bad["lmk_xy"][row]).all()


def test_repeated_launches_are_bit_identical(pipe, reference):
    """A reader ahead of the arrival word would see an LDS ring that is not written yet -- now and then, not always."""
    p = torch.from_numpy(reference[0][:64]).cuda()
    first = pipe.decode(p, landmarks=True, landmarks_px=True, mutate=False)
    first = {k: first[k].clone() for k in KEYS}
    for i in range(19):
        again = pipe.decode(p, landmarks=True, landmarks_px=True, mutate=False, out=_poisoned(64))
        for k in KEYS:
            assert torch.equal(again[k], first[k]), (k, i)
