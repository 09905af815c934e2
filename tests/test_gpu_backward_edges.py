"""GPU: the backward of the decode (csrc/flame_backward.hip, autograd.py) where tests/test_gpu_autograd.py does not go -- the
edge rows of tests/backward_edges.py (every quadrant of the jaw angle and past sinf's fast range, the scale clamp, degenerate
6-DoF vectors, zeros), each row held to ITS OWN bar against the float64 statement of the oracle; the chain kernels alone on the
same rows and on the full layout; DAD3D_FLIP_Z through the C ABI; the batch seams of the split backward and of the hand-over to
the library GEMM on one handle; and row isolation under poisoned rows.

Bars (tests/backward_edges.py `row_bars`): max(2e-4, 4 e32) of the row's largest float64 gradient entry, e32 = the float32
oracle's own error on that row; tests/test_backward_edges_host.py caps which rows may exceed 2e-4. The measured errors, kernel
and float32 oracle side by side, are written as a table to the file DAD3D_BACKWARD_EDGE_RECORD names, if it is set (the run on an
MI355X is committed as profiles/backward_edge_error.md)."""
import os
import types

import numpy as np
import pytest
import torch

import backward_edges as be
from dad_3dheads_amd import _lib, landmarks, synthetic
from dad_3dheads_amd import autograd as ag
from dad_3dheads_amd.flame import FLAME_CONSTS
from dad_3dheads_amd.head_mesh import HeadMesh

pytestmark = pytest.mark.gpu
CONFIGS = [(True, True), (False, False)]  # (zero_rotation, to_2d)
SEAM_BATCHES = (2, 33, 32, 128, 1, 65, 64, 86, 85, 97, 96, 129, 257)  # grows and shrinks; nsplit 8..1; HIP / library GEMM at 96 | 97
RECORD = []  # (section, row, kernel error, float32 oracle error, bar)


@pytest.fixture(scope="module", autouse=True)
def record():
    yield
    path = os.environ.get("DAD3D_BACKWARD_EDGE_RECORD")
    if not path or not RECORD:
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("# Backward of the decode at edges and batch seams: measured relative error per row\n\n"
                "Written by tests/test_gpu_backward_edges.py on an MI355X. Error = max |g - g64| over the row's largest |g64| entry, g64 the\n"
                "float64 statement; `float32 oracle` is the same figure for the CPU oracle in float32; bar = max(2e-4, 4 x float32 oracle).\n"
                "Seam batches tile 8 rows: the figure is the largest over the batch's rows.\n\n"
                "| section | row | kernel | float32 oracle | bar |\n|---|---|---|---|---|\n")
        for section, row, err, e32, bar in RECORD:
            f.write(f"| {section} | {row} | {err:.2e} | {e32:.2e} | {bar:.2e} |\n")


@pytest.fixture(scope="module")
def hm(flame_model, static):
    return HeadMesh(flame_model=flame_model, landmarks=landmarks.canonical("445", static), static=static, device=0)


@pytest.fixture(scope="module")
def edge(flame_consts):
    """The edge rows and, per configuration, upstream gradients, float64 gradients, float32-oracle errors and bars: once."""
    names, params = be.edge_params()
    c64 = be.oracle64(flame_consts)
    per = {}
    for zr, t2 in CONFIGS:
        wv, wp = be.weights(len(names), t2)
        g32, _ = be.oracle_grad(flame_consts, params, wv, wp, zr, t2, torch.float32)
        g64, _ = be.oracle_grad(c64, params, wv, wp, zr, t2, torch.float64)
        per[zr, t2] = types.SimpleNamespace(wv=wv, wp=wp, g64=g64, e32=be.row_errors(g32, g64), bars=be.row_bars(g32, g64))
    return names, params, per


def hold_rows(section, names, g, ref, rows=None):
    """Every row of g within its bar of the float64 row (rows: which reference row a row of g is). Records, then asserts."""
    g = g.detach().cpu()
    rows = np.arange(g.shape[0]) if rows is None else rows
    err = be.row_errors(g, ref.g64[rows])
    bad = []
    for i, r in enumerate(rows):
        print(f"{section} {i:3d} {names[r]:20s} kernel {float(err[i]):.2e}  float32 oracle {float(ref.e32[r]):.2e}  bar {float(ref.bars[r]):.2e}")
        if not float(err[i]) <= float(ref.bars[r]):
            bad.append((i, names[r], float(err[i]), float(ref.bars[r])))
    return err, bad


def train_grad(mesh, params, wv, wp, zero_rot, to_2d):
    """d/d(params) of (v . wv).sum() + 1e-2 (proj . wp).sum() through the HIP decode, on one prediction tensor."""
    p = params.detach().clone().cuda().requires_grad_(True)
    q = p * 1.0
    v = mesh.vertices_3d(q, zero_rotation=zero_rot)
    pr = mesh.reprojected_vertices(q, to_2d=to_2d)
    ((v * wv).sum() + 1e-2 * (pr * wp).sum()).backward()
    return p.grad


@pytest.mark.parametrize("zero_rot,to_2d", CONFIGS)
def test_edge_rows_end_to_end(hm, edge, zero_rot, to_2d):
    names, params, per = edge
    ref = per[zero_rot, to_2d]
    g = train_grad(hm, torch.from_numpy(params), ref.wv.cuda(), ref.wp.cuda(), zero_rot, to_2d).cpu()
    section = f"edges zero_rot={int(zero_rot)} to_2d={int(to_2d)}"
    err, bad = hold_rows(section, names, g, ref)
    RECORD.extend((section, n, float(e), float(e32), float(b)) for n, e, e32, b in zip(names, err, ref.e32, ref.bars))
    assert bool(torch.isfinite(g).all()), [n for n, row in zip(names, g) if not bool(torch.isfinite(row).all())]
    assert not bad, bad
    assert float(g[:, be.TZ].abs().max()) == 0.0
    scale = dict(zip(names, g[:, be.SCALE].tolist()))
    # clamp(scale + 1, 1e-8) passes nothing below the floor; scale = -1 gives 0 < 1e-8, below it as well (the float32 and
    # float64 oracle both say exactly 0 there: tests/test_backward_edges_host.py); one float above -1 it passes
    assert scale["scale_clamped"] == 0.0 and scale["scale_at_clamp"] == 0.0
    assert scale["scale_above_clamp"] != 0.0


def chain_reference(layer, consts, params, g_in, g_c, dtype):
    """`autograd.pose_chain` on the CPU in `dtype` -> (inputs, consts, d/d(params) of <inputs, g_in> + <consts, g_c>)."""
    t = layer.decode_tables()
    tables = types.SimpleNamespace(joints0=t.joints0.cpu().to(dtype), joint_dirs=t.joint_dirs.cpu().to(dtype), parents=t.parents)
    p = torch.from_numpy(params).to(dtype).requires_grad_(True)
    chain = ag.pose_chain(tables, consts, p)
    (g,) = torch.autograd.grad([chain["inputs"], chain["consts"]], [p], [g_in.to(dtype), g_c.to(dtype)])
    return chain["inputs"].detach().double(), chain["consts"].detach().double(), g.double()


def hold_chain(section, layer, consts, names, params):
    lib = _lib.load()
    b, k = params.shape[0], lib.dad3d_flame_num_chain_inputs(layer._handle)
    gen = torch.Generator().manual_seed(8)
    g_in, g_c = torch.randn((b, k), generator=gen), torch.randn((b, 72), generator=gen)
    in32, c32, g32 = chain_reference(layer, consts, params, g_in, g_c, torch.float32)
    in64, c64, g64 = chain_reference(layer, consts, params, g_in, g_c, torch.float64)
    assert bool(torch.isfinite(g32).all()) and bool(torch.isfinite(g64).all())
    p = torch.from_numpy(params).cuda()
    inputs, c72 = torch.full((b, k), float("nan"), device="cuda"), torch.full((b, 72), float("nan"), device="cuda")
    _lib.check(lib.dad3d_flame_pose_chain(layer._handle, p.data_ptr(), b, inputs.data_ptr(), c72.data_ptr(), None))
    g = torch.full_like(p, float("nan"))  # every entry must be written
    d_in, d_c = g_in.cuda(), g_c.cuda()
    _lib.check(lib.dad3d_flame_pose_chain_backward(layer._handle, p.data_ptr(), b, d_in.data_ptr(), d_c.data_ptr(), g.data_ptr(), None))
    torch.cuda.synchronize()
    # the forward values are the value half of the dual numbers: written everywhere and finite (their accuracy at ordinary rows
    # is test_chain_kernels_match_the_torch_statement_of_the_chain's); the figure against float64 is printed next to torch's own
    assert bool(torch.isfinite(inputs).all()) and bool(torch.isfinite(c72).all())
    fwd = torch.cat([inputs, c72], dim=1).cpu().double()
    for n, e, e32 in zip(names, (fwd - torch.cat([in64, c64], dim=1)).abs().amax(dim=1),
                         (torch.cat([in32, c32], dim=1) - torch.cat([in64, c64], dim=1)).abs().amax(dim=1)):
        print(f"{section} forward {n:20s} kernel {float(e):.2e}  float32 torch {float(e32):.2e}")
    ref = types.SimpleNamespace(g64=g64, e32=be.row_errors(g32, g64), bars=be.row_bars(g32, g64))
    # the cap, as for the end-to-end bars: torch's own float32 chain may lift a bar only where an angle's float32 norm is already
    # 2e-4 rad or more off (8191 and up) or the Gram-Schmidt is 1e-4 from degenerate
    lifted = [n for n, bb in zip(names, ref.bars) if float(bb) > be.RTOL]
    assert all(n.endswith(("_8191", "_8193", "_1e6", "near_parallel")) for n in lifted), lifted
    assert float(ref.bars.max()) < 5e-2
    err, bad = hold_rows(section, names, g, ref)
    RECORD.extend((section, n, float(e), float(e32), float(bb)) for n, e, e32, bb in zip(names, err, ref.e32, ref.bars))
    assert bool(torch.isfinite(g).all()), [n for n, row in zip(names, g.cpu()) if not bool(torch.isfinite(row).all())]
    assert not bad, bad


def test_chain_kernels_alone_on_the_edge_rows(hm, edge):
    names, params, _ = edge
    hold_chain("chain", hm.flame, FLAME_CONSTS, names, params)


def test_chain_kernels_sweep_neck_and_eyeballs(flame_model, static):
    """The full layout (neck + eyeballs are inputs): each of the three extra joints through zero, a denormal and the jaw's
    angles, the other joints at ordinary values."""
    mesh = HeadMesh(flame_config=be.FULL, flame_model=flame_model, static=static, device=0)
    names, rows = be.joint_sweep()  # eye0, eye1, neck: the joints the shipped layout lacks
    hold_chain("chain, full layout", mesh.flame, be.FULL, names, rows)


def backward_through_the_c_abi(layer, params, flags, g_v3, g_pj):
    """forward (v_posed), chain, `dad3d_flame_decode_backward` with `flags`, contraction, chain VJP -> (g_posed, g_consts, g_params)."""
    lib, h = _lib.load(), layer._handle
    b, k = params.shape[0], lib.dad3d_flame_num_chain_inputs(layer._handle)
    v3, posed = torch.empty((b, 5023, 3), device="cuda"), torch.empty((b, 15069), device="cuda")
    _lib.check(lib.dad3d_flame_decode_posed(h, params.data_ptr(), b, 0, v3.data_ptr(), None, posed.data_ptr(), None))
    inputs, c72 = torch.empty((b, k), device="cuda"), torch.empty((b, 72), device="cuda")
    _lib.check(lib.dad3d_flame_pose_chain(h, params.data_ptr(), b, inputs.data_ptr(), c72.data_ptr(), None))
    g_posed, g_consts = torch.full_like(posed, float("nan")), torch.full_like(c72, float("nan"))
    _lib.check(lib.dad3d_flame_decode_backward(h, b, flags, c72.data_ptr(), posed.data_ptr(), g_v3.data_ptr(), g_pj.data_ptr(),
                                               g_posed.data_ptr(), g_consts.data_ptr(), None))
    g_inputs = torch.full((b, k), float("nan"), device="cuda")
    _lib.check(lib.dad3d_flame_grad_inputs(h, g_posed.data_ptr(), b, g_inputs.data_ptr(), None))
    g_params = torch.full_like(params, float("nan"))
    _lib.check(lib.dad3d_flame_pose_chain_backward(h, params.data_ptr(), b, g_inputs.data_ptr(), g_consts.data_ptr(), g_params.data_ptr(), None))
    torch.cuda.synchronize()
    return g_posed, g_consts, g_params


def test_flip_z_in_the_backward(hm, edge):
    """DAD3D_FLIP_Z multiplies the projection's z by -1: its backward equals the plain call fed the gradient with z negated, bit
    for bit (the same arithmetic), and both equal the float64 statement of (v . wv).sum() + 1e-2 (proj . wp).sum()."""
    names, params, per = edge
    ref = per[False, False]
    p = torch.from_numpy(params).cuda()
    g_v3 = ref.wv.cuda().contiguous()
    g_pj = (1e-2 * ref.wp).cuda().contiguous()
    negated = (g_pj * g_pj.new_tensor([1.0, 1.0, -1.0])).contiguous()
    plain = backward_through_the_c_abi(hm.flame, p, 0, g_v3, g_pj)
    flipped = backward_through_the_c_abi(hm.flame, p, _lib.FLIP_Z, g_v3, negated)
    wrong = backward_through_the_c_abi(hm.flame, p, 0, g_v3, negated)
    for a, b in zip(plain, flipped):
        assert torch.equal(a, b)  # NaN nowhere: equal() would be False
    assert not torch.equal(plain[2], wrong[2])  # the z column matters to this gradient
    for section, g in (("C ABI, plain", plain[2]), ("C ABI, FLIP_Z", flipped[2])):
        err, bad = hold_rows(section, names, g, ref)
        RECORD.extend((section, n, float(e), float(e32), float(bb)) for n, e, e32, bb in zip(names, err, ref.e32, ref.bars))
        assert not bad, bad
    lib = _lib.load()
    st = lib.dad3d_flame_decode_backward(hm.flame._handle, 1, _lib.FLIP_Z | _lib.TO_2D, plain[1].data_ptr(), plain[0].data_ptr(),
                                         g_v3.data_ptr(), g_pj.data_ptr(), plain[0].data_ptr(), plain[1].data_ptr(), None)
    assert st != 0 and b"DAD3D_FLIP_Z needs a 3-component projection" in lib.dad3d_last_error()


@pytest.fixture(scope="module")
def seam(flame_consts):
    """8 distinct rows (six ordinary ones, a jaw in the second quadrant, a clamped scale) and 8 upstream-gradient rows that
    every seam batch tiles: the float64 oracle runs once, on 8 rows."""
    params = synthetic.synthetic_params(8, seed=104)
    params[6, be.JAW] = be.axis_angle(2.5)
    params[7, be.SCALE] = -1.5
    names = [f"row {i}" for i in range(8)]
    wv, wp = be.weights(8, True, seed=11)
    g32, _ = be.oracle_grad(flame_consts, params, wv, wp, True, True, torch.float32)
    g64, _ = be.oracle_grad(be.oracle64(flame_consts), params, wv, wp, True, True, torch.float64)
    ref = types.SimpleNamespace(wv=wv.cuda(), wp=wp.cuda(), g64=g64, e32=be.row_errors(g32, g64), bars=be.row_bars(g32, g64))
    assert float(ref.bars.max()) == be.RTOL  # ordinary rows: no reference-derived lift
    return names, torch.from_numpy(params).cuda(), ref


def test_batch_seams_on_one_handle(flame_model, static, seam):
    """One handle through batches that grow and shrink the partial-sum buffer and cross every `nsplit` of the vertex kernel
    (8 ... 2 at 86-128, 1 from 129: g_consts written directly) and the hand-over from the split-K HIP contraction to the library
    GEMM (96 | 97). Up to 96 the whole backward is this project's kernels, no atomics: equal rows are bit-equal wherever they
    sit in the launch (0, 31, 32, 63, 64 included: 8 divides 32 and 64)."""
    names, params8, ref = seam
    mesh = HeadMesh(flame_model=flame_model, landmarks=landmarks.canonical("445", static), static=static, device=0)
    failures = []
    for batch in SEAM_BATCHES:
        rows = np.arange(batch) % 8
        at = torch.from_numpy(rows).cuda()
        g = train_grad(mesh, params8[at], ref.wv[at], ref.wp[at], True, True)
        err, bad = hold_rows(f"batch {batch}", names, g, ref, rows)
        worst = int(torch.argmax(err))
        RECORD.append((f"seam, batch {batch}", f"worst of {batch}", float(err[worst]), float(ref.e32[rows[worst]]), float(ref.bars[rows[worst]])))
        failures += [(batch,) + x for x in bad]
        if batch <= ag.GRAD_INPUTS_HIP_MAX_BATCH:
            for i in range(8, batch):
                if not torch.equal(g[i], g[i % 8]):
                    failures.append((batch, i, "differs in bits from row", i % 8))
    assert not failures, failures


def test_poisoned_rows_stay_in_their_rows(hm, seam):
    """Batch 70 (two 32-row half-blocks and a ragged third; nsplit 3): NaN parameters in rows 0 and 31, +inf in row 32, one inf
    in the upstream gradient of row 64 at one vertex. Every other row's gradient is bit-equal to the clean launch's."""
    _, params8, ref = seam
    at = torch.from_numpy(np.arange(70) % 8).cuda()
    params, wv, wp = params8[at].clone(), ref.wv[at].clone(), ref.wp[at].clone()
    clean = train_grad(hm, params, wv, wp, True, True)
    assert bool(torch.isfinite(clean).all())
    params[0, 17] = float("nan")  # a shape coefficient: through the blend-shape GEMM
    params[31, 401] = float("nan")  # the jaw: through the chain
    params[32, 405] = float("inf")  # the 6-DoF rotation
    wv[64, 2500, 1] = float("inf")
    dirty = train_grad(hm, params, wv, wp, True, True)
    poisoned = [0, 31, 32, 64]
    keep = torch.ones(70, dtype=torch.bool)
    keep[poisoned] = False
    assert torch.equal(dirty[keep.cuda()], clean[keep.cuda()])
    for r in poisoned:
        assert not bool(torch.isfinite(dirty[r]).all()), r
