"""GPU: the two-role decode kernel (csrc/flame_decode.hip) on every constants layout and batch seam -- the instantiations
`launch_flame_decode` picks for a full pose (KG = 28, the general kinematic chain, 21 float4s handed over per image), narrow
shape / expression widths (the `beta_at` gather), both, and a layout without a jaw input, next to the default one as a control
(pinned with `select_kernel("two_role")`); at 1, 16 | 17 images (RB = 1 | 4), one full row block, one row past it and three
blocks with a ragged tail; with every output and flag of a launch. Rows, float64 statement and per-row bars:
tests/decode_layouts.py (held on their own in tests/test_decode_layouts_host.py). The measured errors are written as a table
to the file DAD3D_DECODE_LAYOUTS_RECORD names, if it is set (the run on an MI355X is committed as
profiles/decode_layouts_error.md)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import backward_edges as be
import decode_layouts as dl
from dad_3dheads_amd import _lib
from dad_3dheads_amd import autograd as ag
from dad_3dheads_amd.head_mesh import HeadMesh

pytestmark = pytest.mark.gpu
RECORD = []  # (layout, launch, row, kernel v, kernel px, e32 v, e32 px, cond v, cond px, bar v, bar px)
OUTPUTS = ("verts3d", "proj", "lmk_xy", "lmk_px")


@pytest.fixture(scope="module", autouse=True)
def record():
    yield
    path = os.environ.get("DAD3D_DECODE_LAYOUTS_RECORD")
    if not path or not RECORD:
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("# The two-role decode on every constants layout and batch seam: measured error against float64\n\n"
                "Written by tests/test_gpu_decode_layouts.py on an MI355X. `kernel` = largest |output - float64 statement| of the row over\n"
                "vertices (rotated and unrotated, model units) | over pixels (3 and 2 components); `e32` = the same for the CPU oracle in\n"
                "float32; `cond` = change of the float64 outputs under 4 fp32 ulps of the swept angle; bar = max(floor, 4 e32, cond from\n"
                "8191 rad up), floor = 4 x the largest e32 over the layout's 64 ordinary rows. A batch line carries its worst row (largest\n"
                "kernel / bar). Layouts: D default, F full pose, N narrow, FN both, J0 no jaw input (tests/decode_layouts.py).\n\n"
                "| layout | launch | row | kernel | e32 | cond | bar | kernel / bar |\n|---|---|---|---|---|---|---|---|\n")
        for lay, launch, row, kv, kp, ev, ep, cv, cp, bv, bp in RECORD:
            f.write(f"| {lay} | {launch} | {row} | {kv:.2e} / {kp:.2e} | {ev:.2e} / {ep:.2e} | {cv:.2e} / {cp:.2e} | {bv:.2e} / {bp:.2e} | "
                    f"{kv / bv:.2f} / {kp / bp:.2f} |\n")
        for lay, (v, px, reason) in dl.RAISED_FLOORS.items():
            f.write(f"\nFloor of {lay} raised to {v:.2e} / {px:.2e}: {reason}\n")


@pytest.fixture(scope="module")
def meshes(flame_model, static):
    """One HeadMesh per layout, made on first use."""
    made = {}

    def get(layout):
        if layout not in made:
            hm = HeadMesh(flame_config=dl.LAYOUTS[layout], flame_model=flame_model, landmarks=dl.landmark_list(static), static=static, device=0)
            if layout == "D":
                hm.flame.select_kernel("two_role")  # every other layout gets it anyway: the pipelined and split kernels do not cover them
            made[layout] = hm
        return made[layout]

    return get


@pytest.fixture(scope="module")
def device_refs(flame_consts):
    """The float64 statement of a layout on the device, once."""
    made = {}

    def get(layout):
        if layout not in made:
            ref = dl.reference(flame_consts, layout)
            made[layout] = (ref, {k: getattr(ref, k).cuda() for k in ("v64", "v064", "p64", "bar_v", "bar_px")})
        return made[layout]

    return get


def bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def hold_launch(mesh, ref, dev, rows, launch, per_row=False):
    """One set of rows through every output and flag of a launch; records, then returns (outputs of the full launch, failures)."""
    lay = ref.layout
    at = torch.from_numpy(rows).cuda()
    params = ref.params[rows]
    fresh = lambda: torch.from_numpy(params.copy()).cuda()  # noqa: E731
    lm = torch.from_numpy(mesh.flame.landmark_indices).cuda()
    tz = dl.offsets(ref.consts)["translation"].start + 2
    bad = []

    a_in = fresh()
    full = mesh.decode(a_in, to_2d=False, landmarks=True, landmarks_px=True)
    two = mesh.decode(fresh(), verts3d=False, to_2d=True, landmarks=False)
    unrot = mesh.decode(fresh(), proj=False, landmarks=False, zero_rotation=True)
    keep = fresh()
    only = mesh.decode(keep, verts3d=False, proj=False, landmarks=True, landmarks_px=True, mutate=False)
    flip = mesh.decode(fresh(), to_2d=False, landmarks=False, flip_z=True)
    torch.cuda.synchronize()

    # against float64, row by row
    err = {"verts3d": dl.row_max(full["verts3d"].double() - dev["v64"][at]), "unrotated": dl.row_max(unrot["verts3d"].double() - dev["v064"][at]),
           "proj3": dl.row_max(full["proj"].double() - dev["p64"][at]), "proj2": dl.row_max(two["proj"].double() - dev["p64"][at][..., :2])}
    for k, e in err.items():
        bar = dev["bar_px" if k.startswith("proj") else "bar_v"][at]
        for i in torch.nonzero(~(e <= bar)).flatten().tolist():  # NaN fails
            bad.append((lay, launch, i, ref.names[rows[i]], k, float(e[i]), float(bar[i])))
    kv = torch.maximum(err["verts3d"], err["unrotated"]).cpu()
    kp = torch.maximum(err["proj3"], err["proj2"]).cpu()
    ratio = torch.maximum(kv / ref.bar_v[rows], kp / ref.bar_px[rows])
    for i in (range(len(rows)) if per_row else [int(torch.argmax(torch.nan_to_num(ratio, nan=float("inf"))))]):
        r = rows[i]
        print(f"{lay:2s} {launch:12s} {i:3d} {ref.names[r]:20s} kernel {float(kv[i]):.2e} {float(kp[i]):.2e}  e32 {float(ref.e32_v[r]):.2e} "
              f"{float(ref.e32_px[r]):.2e}  bar {float(ref.bar_v[r]):.2e} {float(ref.bar_px[r]):.2e}")
        if per_row and r < ref.first_edge:
            continue  # the ordinary rows that fill the edge launch: printed, and recorded with their batches
        RECORD.append((lay, launch, ref.names[r] if per_row else f"worst of {len(rows)}: {ref.names[r]}", float(kv[i]), float(kp[i]),
                       float(ref.e32_v[r]), float(ref.e32_px[r]), float(ref.cond_v[r]), float(ref.cond_px[r]), float(ref.bar_v[r]), float(ref.bar_px[r])))

    def check(ok, what):
        if not ok:
            bad.append((lay, launch, what))

    # landmarks: the exact gather of this launch's projection, truncated toward zero; against the oracle a pixel may differ only
    # where the float64 coordinate is within the row's pixel bar of an integer
    gathered = full["proj"][:, lm, :2]
    check(torch.equal(full["lmk_xy"], gathered), "lmk_xy is not the gather of proj")
    check(torch.equal(full["lmk_px"], gathered.to(torch.int32)), "lmk_px is not the truncation of proj")
    want = dev["p64"][at][:, lm, :2]
    bar = dev["bar_px"][at][:, None, None]  # under half a pixel this says: off by one only within the bar of an integer
    px = full["lmk_px"].double()
    check(bool(((torch.trunc(want - bar) <= px) & (px <= torch.trunc(want + bar))).all()), "lmk_px differs from the float64 pixel away from an integer")
    check(torch.equal(only["lmk_xy"], full["lmk_xy"]) and torch.equal(only["lmk_px"], full["lmk_px"]), "landmark-only launch differs in bits")
    # DAD3D_FLIP_Z negates z and nothing else
    check(torch.equal(flip["verts3d"], full["verts3d"]) and torch.equal(flip["proj"][..., :2], full["proj"][..., :2])
          and torch.equal(flip["proj"][..., 2], -full["proj"][..., 2]), "flip_z")
    # tz := 0 written back, nothing else touched; mutate=False: nothing touched
    after = params.copy()
    after[:, tz] = 0.0
    check(np.array_equal(bits(a_in), after.view(np.int32)), "write-back of tz")
    check(np.array_equal(bits(keep), params.view(np.int32)), "mutate=False touched the params")
    # a repeated row gives the same bits wherever it sits in the launch
    first = {}
    for i, r in enumerate(rows.tolist()):
        j = first.setdefault(r, i)
        if j != i:
            for k in OUTPUTS:
                check(torch.equal(full[k][i], full[k][j]), f"row {i} differs in bits from row {j} in {k}")
            check(torch.equal(two["proj"][i], two["proj"][j]) and torch.equal(unrot["verts3d"][i], unrot["verts3d"][j]), f"row {i} / {j}, to_2d or zero_rotation")
    return full, bad


CASES = [(layout, batch) for layout in dl.LAYOUTS for batch in dl.BATCHES[layout]]


@pytest.mark.parametrize("layout,batch", CASES, ids=[f"{la}-{b}" for la, b in CASES])
def test_every_output_of_a_launch_against_float64(meshes, device_refs, layout, batch):
    ref, dev = device_refs(layout)
    _, bad = hold_launch(meshes(layout), ref, dev, dl.launch_rows(batch), f"batch {batch}")
    assert not bad, bad


@pytest.mark.parametrize("layout", ["F", "N"])
def test_edge_rows_in_two_row_blocks_and_in_a_launch_of_sixteen(meshes, device_refs, layout):
    """The edge rows in one launch of 70 (two row blocks, RB = 4), each held to its own bar; the first 16 again on their own
    (RB = 1): the same rows through the other instantiation, to the same bars."""
    ref, dev = device_refs(layout)
    rows = dl.edge_launch_rows(ref)
    _, bad = hold_launch(meshes(layout), ref, dev, rows, "edges, 70", per_row=True)
    _, bad16 = hold_launch(meshes(layout), ref, dev, rows[:16], "edges, 16", per_row=True)
    assert not bad + bad16, bad + bad16


@pytest.mark.parametrize("layout", [la for la in dl.LAYOUTS if 130 in dl.BATCHES[la]])
def test_rows_shared_by_the_launches_of_65_and_130_are_bit_equal(meshes, device_refs, layout):
    """Rows 0 .. 64 of the 130-row launch (three row blocks) are the 65-row launch (two): the same bits, whatever the grid."""
    ref, _ = device_refs(layout)
    mesh = meshes(layout)
    outs = {}
    for batch in (65, 130):
        p = torch.from_numpy(ref.params[dl.launch_rows(batch)]).cuda()
        outs[batch] = mesh.decode(p, to_2d=False, landmarks=True, landmarks_px=True)
    torch.cuda.synchronize()
    for k in OUTPUTS:
        assert torch.equal(outs[130][k][:65], outs[65][k]), k


POISON = [(0, "neck", 1, float("nan")), (3, "eyeballs", 4, float("inf")), (4, "shape", 17, float("-inf")), (63, "scale", 0, float("nan")),
          (64, "neck", 0, float("-inf")), (69, "scale", 0, float("inf")), (69, "expression", 99, float("nan")), (64, "eyeballs", 0, float("nan"))]


def test_poisoned_rows_stay_in_their_rows(meshes, device_refs):
    """F at batch 70 (two row blocks, the second ragged): NaN and +-Inf in a neck, an eyeball, a beta and the scale entry of rows
    0, 3, 4 (one pose workgroup: rows 0 .. 3, and its neighbour), 63 | 64 (the block seam) and 69 (the last). Those rows are not
    finite; every other row is the clean launch bit for bit."""
    ref, _ = device_refs("F")
    mesh = meshes("F")
    off = dl.offsets(ref.consts)
    clean_p = ref.params[dl.launch_rows(70)]
    dirty_p = clean_p.copy()
    for row, key, i, value in POISON:
        dirty_p[row, off[key].start + i] = value
    clean = mesh.decode(torch.from_numpy(clean_p.copy()).cuda(), to_2d=False, landmarks=True, landmarks_px=True)
    dirty = mesh.decode(torch.from_numpy(dirty_p).cuda(), to_2d=False, landmarks=True, landmarks_px=True)
    torch.cuda.synchronize()
    poisoned = sorted({row for row, *_ in POISON})
    keep = torch.ones(70, dtype=torch.bool)
    keep[poisoned] = False
    keep = keep.cuda()
    assert bool(torch.isfinite(clean["verts3d"]).all()) and bool(torch.isfinite(clean["proj"]).all())
    for k in OUTPUTS:
        assert torch.equal(dirty[k][keep], clean[k][keep]), k
    for row, key, _, _ in POISON:
        out = dirty["proj"] if key == "scale" else dirty["verts3d"]  # the scale enters the projection only
        assert not bool(torch.isfinite(out[row]).all()), (row, key)


@pytest.mark.parametrize("layout,batch,zero_rot,to_2d", [(la, b, zr, t2) for la in ("F", "N", "FN") for b, zr, t2 in ((17, True, True), (65, False, False))])
def test_posed_forward_and_gradient_against_float64(meshes, device_refs, flame_consts, layout, batch, zero_rot, to_2d):
    """The training forward (POSED instantiation, always RB = 4) through `HeadMesh.vertices_3d` / `reprojected_vertices` on one
    prediction tensor: values to the bars of the inference launch, the gradient to `backward_edges.row_bars` against the float64
    oracle of the layout."""
    ref, dev = device_refs(layout)
    mesh = meshes(layout)
    rows = dl.launch_rows(batch)
    g = dl.grad_reference(flame_consts, layout, min(batch, dl.N_ORDINARY), zero_rot, to_2d)
    at = torch.from_numpy(rows).cuda()
    wv, wp = g.wv[rows].cuda(), g.wp[rows].cuda()
    p = torch.from_numpy(ref.params[rows]).cuda().requires_grad_(True)
    q = p * 1.0
    v = mesh.vertices_3d(q, zero_rotation=zero_rot)
    pr = mesh.reprojected_vertices(q, to_2d=to_2d)
    assert v.requires_grad and pr.requires_grad and pr.shape[-1] == (2 if to_2d else 3)
    ((v * wv).sum() + 1e-2 * (pr * wp).sum()).backward()
    tz = dl.offsets(ref.consts)["translation"].start + 2
    assert float(q.detach()[:, tz].abs().max()) == 0.0 and float(p.grad[:, tz].abs().max()) == 0.0
    e_v = dl.row_max(v.detach().double() - dev["v064" if zero_rot else "v64"][at])
    e_p = dl.row_max(pr.detach().double() - dev["p64"][at][..., :pr.shape[-1]])
    err = be.row_errors(p.grad, g.g64[rows])
    worst = int(torch.argmax(err))
    print(f"{layout} posed batch {batch}: values {float(e_v.max()):.2e} {float(e_p.max()):.2e} (bars {ref.floor_v:.2e} {ref.floor_px:.2e}); "
          f"gradient {float(err[worst]):.2e}, float32 oracle {float(g.e32[rows[worst]]):.2e}, bar {float(g.bars[rows[worst]]):.2e}")
    assert bool((e_v <= dev["bar_v"][at]).all()) and bool((e_p <= dev["bar_px"][at]).all()), (float(e_v.max()), float(e_p.max()))
    assert bool(torch.isfinite(p.grad).all())
    assert bool((err <= g.bars[rows]).all()), [(i, float(err[i]), float(g.bars[rows[i]])) for i in range(batch) if not err[i] <= g.bars[rows[i]]]
    assert batch <= ag.GRAD_INPUTS_HIP_MAX_BATCH  # the whole backward is this project's kernels, no atomics: repeats are bit-equal
    for i in range(dl.N_ORDINARY, batch):
        assert torch.equal(p.grad[i], p.grad[rows[i]]), i


def test_a_captured_launch_replays_on_new_params(meshes, device_refs):
    """F at batch 17, captured once on a side stream: the capture takes the device-epoch instantiation (no per-launch arrival
    target). Two replays on new rows give the bits of the eager launch on those rows, and no hand-off timed out."""
    ref, _ = device_refs("F")
    mesh = meshes("F")
    kw = dict(to_2d=False, landmarks=True, landmarks_px=True)
    static_in = torch.from_numpy(ref.params[:17].copy()).cuda()
    mesh.decode(static_in.clone(), **kw)  # the handle's buffers for this batch exist before the capture
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = mesh.decode(static_in, **kw)
    tz = dl.offsets(ref.consts)["translation"].start + 2
    for first in (20, 40):
        new = ref.params[first:first + 17]
        static_in.copy_(torch.from_numpy(new.copy()).cuda())
        graph.replay()
        torch.cuda.synchronize()
        want = mesh.decode(torch.from_numpy(new.copy()).cuda(), **kw)
        torch.cuda.synchronize()
        for k in OUTPUTS:
            assert torch.equal(out[k], want[k]), (first, k)
        after = new.copy()
        after[:, tz] = 0.0
        assert np.array_equal(bits(static_in), after.view(np.int32))
    n = C.c_uint()
    _lib.check(_lib.load().dad3d_flame_handoff_timeouts(mesh.flame._handle, C.byref(n)))
    assert n.value == 0
