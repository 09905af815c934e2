"""GPU: every argument of the pipelined decode kernels arrives in its own place. The kernels take flat positional arguments (the first
fourteen dwords preloaded into SGPRs, the rest one struct read through the kernarg pointer: csrc/flame_decode_pipe.hip), and positional
arguments can be swapped silently -- so each one is pinned by a launch that goes wrong if it lands in another's slot:

  * every non-empty subset of the four outputs {verts3d, proj, lmk_xy, lmk_px} is launched on its own and must be `torch.equal` to the
    same tensors of the all-outputs launch: a null pointer moves through all four output slots, and the landmark-only subsets run the
    CHUNKED instantiation on the landmark sub-model (other `vtab`, `bpack`, `n_verts`, chunk geometry in the packed word);
  * the all-outputs launch is held to `oracle.flame_ref` within the bars of tests/test_gpu_decode.py (`batch`, `n_params`, `n_verts`,
    `n_lmk`, `image_size`, `lmk_next` -- the landmark list carries duplicates -- and the flag bits);
  * `params[:, 411]` is zeroed exactly when DAD3D_MUTATE_PARAMS is set, and nothing else in `params` is ever touched.

Every launch writes into buffers filled with NaN (int landmarks: a sentinel no pixel can be), so a row that no workgroup wrote fails the
comparison instead of showing what an earlier launch left in a reused block. The landmark-only subsets are asserted to run on the landmark
sub-model (`dad3d_flame_num_landmark_vertices`, DAD3D_LANDMARK_SUBSET unset), which with two or more half-blocks is the CHUNKED
instantiation. Its widest geometry has a test of its own: a list inside ONE tile at n_half = 256 is 256 chunks of one half-block.

B = 9 and 32: one half-block, ragged and full; 64: two half-blocks; 65: three, with a one-row tail (and, landmark-only, three chunks of one
half-block). Both projection widths; DAD3D_FLIP_Z on the 3-component one only (the C ABI refuses it with DAD3D_TO_2D). The mesh has 5023
vertices -- not a multiple of the tile's 20 -- and a launch without landmark outputs is the n_lmk = 0 one."""
import itertools
import os

import numpy as np
import pytest
import torch

from dad_3dheads_amd import _lib, synthetic
from dad_3dheads_amd.head_mesh import HeadMesh
from decode_layouts import landmark_list
from oracle import flame_ref

pytestmark = pytest.mark.gpu
TOL_V, TOL_PX = 5e-6, 1e-3  # tests/test_gpu_decode.py
OUTPUTS = ("verts3d", "proj", "lmk_xy", "lmk_px")
SUBSETS = [s for n in range(1, 5) for s in itertools.combinations(OUTPUTS, n)]
BATCHES = (9, 32, 64, 65)
FORMS = {"2d": (True, False), "3d": (False, False), "3d_flip_z": (False, True)}  # (to_2d, flip_z)
INT_POISON = -(2 ** 31)  # no landmark pixel: the synthetic heads project into a 256 px image


@pytest.fixture(scope="module")
def heads(flame_model, static):
    lmk = landmark_list(static)
    auto = HeadMesh(flame_model=flame_model, landmarks=lmk, static=static, device=0)
    pinned = HeadMesh(flame_model=flame_model, landmarks=lmk, static=static, device=0)
    pinned.flame.select_kernel("pipelined")  # raises rather than falling back
    return auto, pinned, torch.from_numpy(lmk).cuda()


_REF = {}


def _reference(flame_consts, batch):
    """(params, vertices, 3-component projection, params after) of the oracle for a launch of `batch` rows, computed once."""
    if batch not in _REF:
        params = synthetic.synthetic_params(batch, seed=4100 + batch)
        p = torch.from_numpy(params.copy())
        v = flame_ref.vertices_3d(flame_consts, p)
        pr = flame_ref.reprojected_vertices(flame_consts, p, to_2d=False)  # zeroes tz in `p`, like the reference
        _REF[batch] = (params, v.cuda(), pr.cuda(), p.numpy())
    return _REF[batch]


def _poisoned(hm, batch, wanted, to_2d):
    """The output buffers of a launch, every element something no launch writes."""
    n_lmk = hm.flame.n_landmarks
    shapes = {"verts3d": (batch, 5023, 3), "proj": (batch, 5023, 2 if to_2d else 3), "lmk_xy": (batch, n_lmk, 2), "lmk_px": (batch, n_lmk, 2)}
    return {k: torch.full(shapes[k], INT_POISON, dtype=torch.int32, device="cuda") if k == "lmk_px"
            else torch.full(shapes[k], float("nan"), device="cuda") for k in wanted}


def _launch(hm, params, wanted, to_2d, flip_z, mutate):
    dev = torch.from_numpy(params.copy()).cuda()
    bufs = _poisoned(hm, len(params), wanted, to_2d)
    out = hm.decode(dev, verts3d="verts3d" in wanted, proj="proj" in wanted, to_2d=to_2d, landmarks="lmk_xy" in wanted,
                    landmarks_px="lmk_px" in wanted, flip_z=flip_z, mutate=mutate, out=dict(bufs))
    torch.cuda.synchronize()
    assert set(out) == set(wanted) and all(out[k] is bufs[k] for k in wanted)  # written in place, no fresh allocation
    for k in wanted:  # every element written
        assert not bool((out[k] == INT_POISON).any() if k == "lmk_px" else torch.isnan(out[k]).any()), k
    return out, dev.cpu().numpy()


def _runs_on_sub_model(hm):
    """Landmark-only launches of this handle take the landmark sub-model (capi.cpp: `on_sub`)."""
    assert os.environ.get("DAD3D_LANDMARK_SUBSET") is None and os.environ.get("DAD3D_DECODE_KERNEL") is None
    n_sub = int(_lib.load().dad3d_flame_num_landmark_vertices(hm.flame._handle))
    assert 0 < n_sub < 5023, n_sub
    return n_sub


@pytest.mark.parametrize("mutate", [False, True], ids=["keep_tz", "mutate"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("batch", BATCHES)
def test_every_argument_in_its_place(heads, flame_consts, batch, form, mutate):
    auto, pinned, lmk = heads
    _runs_on_sub_model(auto)
    to_2d, flip_z = FORMS[form]
    params, v_ref, pr_ref, after_ref = _reference(flame_consts, batch)
    want_after = after_ref if mutate else params

    full, after = _launch(auto, params, OUTPUTS, to_2d, flip_z, mutate)
    assert np.array_equal(after, want_after)
    assert np.array_equal(after[:, 411] == 0.0, np.full(batch, mutate))  # (the rows carry a non-zero tz: the test below)
    # the all-outputs launch against the oracle
    pr = pr_ref.clone()
    if flip_z:
        pr[..., 2] *= -1.0
    width = 2 if to_2d else 3
    assert full["proj"].shape == (batch, 5023, width) and full["lmk_xy"].shape == (batch, lmk.numel(), 2)
    err_v = (full["verts3d"] - v_ref).abs().max().item()
    err_p = (full["proj"] - pr[..., :width]).abs().max().item()
    print(f"B={batch} {form} mutate={mutate}: |dv| {err_v:.2e} |dproj| {err_p:.2e}")
    assert err_v < TOL_V and err_p < TOL_PX
    assert torch.equal(full["lmk_xy"], full["proj"][:, lmk, :2])  # an exact gather, duplicates in the list included
    assert torch.equal(full["lmk_px"], full["proj"][:, lmk, :2].to(torch.int32))  # truncation toward zero
    # it IS the pipelined kernel that ran: the pinned handle raises where that kernel does not cover the launch
    same, after = _launch(pinned, params, OUTPUTS, to_2d, flip_z, mutate)
    assert np.array_equal(after, want_after)
    for key in OUTPUTS:
        assert torch.equal(same[key], full[key]), key

    for wanted in SUBSETS[:-1]:
        got, after = _launch(auto, params, wanted, to_2d, flip_z, mutate)
        assert np.array_equal(after, want_after), wanted
        for key in wanted:
            assert got[key].shape == full[key].shape and torch.equal(got[key], full[key]), (wanted, key)


def test_one_tile_sub_model_in_256_chunks(flame_model, static):
    """The widest chunk geometry: a landmark list inside one tile of 20 vertices, n_half = 256 with a ragged last half-block -> 256 chunks of
    one half-block in runs of 32 per XCD. Landmark-only on the sub-model against the same outputs of the whole-mesh kernel (the pinned handle
    never chunks and never takes the sub-model)."""
    lmk = np.array([4001, 4003, 4003, 4017], dtype=np.int64)
    sub = HeadMesh(flame_model=flame_model, landmarks=lmk, static=static, device=0)
    whole = HeadMesh(flame_model=flame_model, landmarks=lmk, static=static, device=0)
    whole.flame.select_kernel("pipelined")
    assert _runs_on_sub_model(sub) <= 20
    batch = 256 * 32 - 5
    params = np.tile(synthetic.synthetic_params(64, seed=4164), (128, 1))[:batch]
    params[:, 409:412] += np.linspace(-0.05, 0.05, batch, dtype=np.float32)[:, None]  # no two chunks alike
    got, after = _launch(sub, params, ("lmk_xy", "lmk_px"), True, False, True)
    want, after_w = _launch(whole, params, ("lmk_xy", "lmk_px"), True, False, True)
    assert np.array_equal(after, after_w) and not after[:, 411].any() and np.array_equal(after[:, :411], params[:, :411])
    assert torch.equal(got["lmk_xy"], want["lmk_xy"]) and torch.equal(got["lmk_px"], want["lmk_px"])
    assert torch.unique(got["lmk_xy"][:, 0, 0]).numel() > batch // 2  # the rows do differ: a chunk written from another chunk's rows shows


def test_the_rows_move_translation_z():
    """The mutate check above means something: the synthetic rows carry a non-zero translation z."""
    for batch in BATCHES:
        assert synthetic.synthetic_params(batch, seed=4100 + batch)[:, 411].all()
