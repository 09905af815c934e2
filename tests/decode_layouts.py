"""The FLAME constants layouts, the rows, the float64 statement and the per-row bars that tests/test_decode_layouts_host.py and
tests/test_gpu_decode_layouts.py share. Test infrastructure in the manner of tests/backward_edges.py, not a conftest.

Five layouts of the params row (order: `oracle.flame_ref.split_3dmm`), one instantiation of the two-role kernel each
(csrc/flame_decode.hip `launch_flame_decode`: <KG, JAW_ONLY, CONTIG>):
  D   the shipped 300 / 100 / jaw 3, the control                <26, jaw-only, contiguous>
  F   full pose: neck 3 and eyeballs 6 are inputs               <28, general chain, contiguous>
  N   narrow: shape 100, expression 50, zero-padded             <26, jaw-only, gathered betas>
  FN  both                                                      <28, general chain, gathered betas>
  J0  the shipped widths without a jaw input (`jaw: 0`)         <26, jaw-only, contiguous>, the `lay.jaw_n == 0` branches

Rows. Ordinary: `synthetic.synthetic_params(64, seed)` re-cut to the layout as tests/test_gpu_autograd.py `_configs` does, neck
and eyeball extras 0.2 N(0,1); a launch of B rows takes the first min(B, 64) and, from row 64 on, the same rows again rotated
by ROTATE, so that a repeated row sits in another row block, another 16-row MFMA block and another lane than its first copy.
Edge: for F each of neck, jaw and the two eyeballs through zero, a denormal and `backward_edges.ANGLES`
(`backward_edges.joint_sweep`) plus the scale, 6-DoF, all-zero and x4 rows of `backward_edges.edge_params()`; for N all of
`edge_params()`. The two points backward_edges.py leaves out (jaw exactly -1e-8, exactly parallel 6-DoF halves) stay out.

Bars, from the reference alone. The float64 statement is `oracle.flame_ref` over `backward_edges.oracle64`; e32(row) is the
float32 oracle's own largest error on that row, for vertices (rotated and unrotated, model units) and for pixels (three
components). floor(layout) = 4 x the largest e32 over the layout's 64 ordinary rows (the 4: room for another fp32 evaluation
order, as in `backward_edges.row_bars`); bar(row) = max(floor, 4 e32(row), cond(row)). cond(row) is nonzero on angle-sweep
rows only: the largest change of the float64 outputs when the swept axis-angle vector is scaled by 1 +- 2^-21 (4 fp32 ulps of
the angle: the kernel's pose feature takes the angle as n2 * rsq(n2), good to about 2.5 ulp, the reference's sqrt to 0.5).
tests/test_decode_layouts_host.py holds every floor under the suite's TOL_V / TOL_PX and caps which rows a bar may exceed
the floor on: LIFTED. cond enters the bar on those rows only. At 100 rad it already exceeds the floor (neck 2.5e-6 model units
against 4.7e-7: 4 ulps of 100 rad are 4.8e-5 rad, times the lever of a vertex about the joint), and is NOT granted there: the
100 rad rows are held to the floor like every smaller angle (the kernel's chain takes the angle with a correctly rounded sqrt,
as the reference does; only the pose feature, scaled by the small pose correctives, sees the rsq)."""
import types

import numpy as np
import torch

import backward_edges as be
from dad_3dheads_amd import landmarks, synthetic
from oracle import flame_ref

TOL_V, TOL_PX = 5e-6, 1e-3  # the bars of tests/test_gpu_decode.py: no floor may exceed them
N_ORDINARY, ROTATE = 64, 21
EDGE_LAUNCH = 70  # two 64-image row blocks, the second ragged; its first 16 rows run again on their own (RB = 1)
COND_SCALE = 2.0 ** -21
LIFTED = ("_8191", "_8193", "_1e6", "rot6_near_parallel", "shape_expr_x4")  # the only rows whose bar may exceed the floor


def _layout(shape=300, expression=100, jaw=3, eyeballs=0, neck=0):
    return {"shape": shape, "expression": expression, "jaw": jaw, "rotation": 6, "eyeballs": eyeballs, "neck": neck,
            "translation": 3, "scale": 1}


LAYOUTS = {"D": _layout(), "F": _layout(eyeballs=6, neck=3), "N": _layout(100, 50), "FN": _layout(100, 50, eyeballs=6, neck=3),
           "J0": _layout(jaw=0)}
assert LAYOUTS["F"] == be.FULL
# the RB switch (16 | 17), one full row block, one row past it, three blocks with a ragged tail
BATCHES = {"D": (5, 17, 65), "F": (1, 16, 17, 64, 65, 130), "N": (1, 16, 17, 64, 65, 130), "FN": (5, 17, 65), "J0": (5, 17, 65)}
SEEDS = {"D": 7100, "F": 7101, "N": 7102, "FN": 7103, "J0": 7104}
# a layout's floor, raised (never past TOL_V / TOL_PX) where an ordinary row came in over 4 e32 on the GPU for a reason read in
# the kernel: {layout: (vertices, pixels, reason)}; profiles/decode_layouts_error.md carries the ratio
RAISED_FLOORS = {}


def offsets(consts):
    """{key: slice} of a params row cut by `consts`, in `split_3dmm` order."""
    out, cur = {}, 0
    for key in ("shape", "expression", "jaw", "rotation", "eyeballs", "neck", "translation", "scale"):
        out[key] = slice(cur, cur + consts[key])
        cur += consts[key]
    return out


def n_params(consts):
    return offsets(consts)["scale"].stop


def extras(n, seed=3):
    """[n,9] eyeball (6) and neck (3) poses, 0.2 N(0,1) rad."""
    return (0.2 * np.random.default_rng(seed).standard_normal((n, 9))).astype(np.float32)


def recut(p413, consts, extra):
    """[n,413] rows of the shipped layout -> [n,P] rows of `consts`: the leading shape / expression entries, the jaw if it is an
    input, `extra` [n,9] for eyeballs and neck where they are inputs."""
    p413 = np.atleast_2d(p413)
    parts = [p413[:, :consts["shape"]], p413[:, 300:300 + consts["expression"]], p413[:, 400:400 + consts["jaw"]], p413[:, 403:409],
             extra[:, :consts["eyeballs"]], extra[:, 6:6 + consts["neck"]], p413[:, 409:413]]
    return np.ascontiguousarray(np.concatenate(parts, axis=1), dtype=np.float32)


def launch_rows(batch):
    """Which ordinary row each row of a launch of `batch` is: 0 .. 63, then the same rows again from ROTATE on."""
    first = np.arange(min(batch, N_ORDINARY))
    return np.concatenate([first, (np.arange(max(batch - N_ORDINARY, 0)) + ROTATE) % N_ORDINARY])


def landmark_list(static):
    """The canonical 445 list with a few duplicates appended (a vertex listed twice gets both slots written)."""
    lm = landmarks.canonical("445", static)
    return np.concatenate([lm, lm[[0, 0, 17, 444]]]).astype(np.int64)


def edge_rows(layout):
    """(names, [n,P] float32, {name: slice swept}) of a layout's edge rows; () for the layouts that have none."""
    consts = LAYOUTS[layout]
    if layout == "F":
        off = offsets(consts)
        joints = (("neck", off["neck"].start), ("jaw", off["jaw"].start), ("eye0", off["eyeballs"].start), ("eye1", off["eyeballs"].start + 3))
        names, rows = be.joint_sweep(joints)
        swept = {f"{j}_{a}": slice(at, at + 3) for j, at in joints for a in ["0", "1e-40"] + [n for n, _ in be.ANGLES]}
        e_names, e413 = be.edge_params()
        keep = [i for i, n in enumerate(e_names) if n.startswith(("scale_", "rot6_", "all_zero", "shape_expr_x4"))]
        more = recut(e413[keep], consts, np.repeat(rows[0][None, 409:418], len(keep), axis=0))
        more[[e_names[i] for i in keep].index("all_zero")] = 0.0  # all of it: neck and eyeballs too
        return names + [e_names[i] for i in keep], np.concatenate([rows, more]), swept
    if layout == "N":
        e_names, e413 = be.edge_params()
        jaw = offsets(consts)["jaw"]
        return e_names, recut(e413, consts, np.zeros((len(e_names), 9), np.float32)), {n: jaw for n in e_names if n.startswith("jaw_")}
    return [], np.zeros((0, n_params(consts)), np.float32), {}


def statement(fc, consts, params, dtype):
    """(vertices, unrotated vertices, 3-component pixels) of the oracle in `dtype`, as float64 tensors."""
    p = torch.as_tensor(params).to(dtype)
    v = flame_ref.vertices_3d(fc, p.clone(), consts=consts)
    v0 = flame_ref.vertices_3d(fc, p.clone(), zero_rotation=True, consts=consts)
    proj = flame_ref.reprojected_vertices(fc, p.clone(), to_2d=False, consts=consts)
    return v.double(), v0.double(), proj.double()


def row_max(d):
    """[n,V,C] -> the largest |entry| of each row (NaN where a row holds one)."""
    return d.abs().flatten(1).amax(dim=1)


_REFERENCES = {}


def reference(flame_consts, layout):
    """Everything a launch of `layout` is held to, computed once: rows 0 .. 63 are the ordinary ones, the edge rows follow.
    names, params [n,P]; v64, v064, p64 float64 [n,5023,3]; e32_*, cond_*, bar_* float64 [n]; floor_*; first_edge."""
    if layout in _REFERENCES:
        return _REFERENCES[layout]
    consts = LAYOUTS[layout]
    ordinary = recut(synthetic.synthetic_params(N_ORDINARY, seed=SEEDS[layout]), consts, extras(N_ORDINARY))
    e_names, e_params, swept = edge_rows(layout)
    names = [f"row {i}" for i in range(N_ORDINARY)] + list(e_names)
    params = np.concatenate([ordinary, e_params])
    c64 = be.oracle64(flame_consts)
    v64, v064, p64 = statement(c64, consts, params, torch.float64)
    v32, v032, p32 = statement(flame_consts, consts, params, torch.float32)
    e32_v = torch.maximum(row_max(v32 - v64), row_max(v032 - v064))
    e32_px = row_max(p32 - p64)
    cond_v, cond_px = torch.zeros_like(e32_v), torch.zeros_like(e32_px)
    at = [i for i, n in enumerate(names) if n in swept]
    for factor in (1.0 + COND_SCALE, 1.0 - COND_SCALE):
        moved = params[at].astype(np.float64)
        for k, i in enumerate(at):
            moved[k, swept[names[i]]] *= factor
        if at:
            mv, mv0, mp = statement(c64, consts, moved, torch.float64)
            cond_v[at] = torch.maximum(cond_v[at], torch.maximum(row_max(mv - v64[at]), row_max(mv0 - v064[at])))
            cond_px[at] = torch.maximum(cond_px[at], row_max(mp - p64[at]))
    floor_v, floor_px = 4.0 * float(e32_v[:N_ORDINARY].max()), 4.0 * float(e32_px[:N_ORDINARY].max())
    if layout in RAISED_FLOORS:
        floor_v, floor_px = max(floor_v, RAISED_FLOORS[layout][0]), max(floor_px, RAISED_FLOORS[layout][1])
    ref = types.SimpleNamespace(
        layout=layout, consts=consts, names=names, params=params, first_edge=N_ORDINARY, v64=v64, v064=v064, p64=p64,
        e32_v=e32_v, e32_px=e32_px, cond_v=cond_v, cond_px=cond_px, floor_v=floor_v, floor_px=floor_px,
        bar_v=torch.clamp(4.0 * e32_v, min=floor_v), bar_px=torch.clamp(4.0 * e32_px, min=floor_px))
    may = torch.tensor([n.endswith(LIFTED) for n in names])  # cond counts from 8191 rad up only: see the module docstring
    ref.bar_v = torch.where(may, torch.maximum(ref.bar_v, cond_v), ref.bar_v)
    ref.bar_px = torch.where(may, torch.maximum(ref.bar_px, cond_px), ref.bar_px)
    _REFERENCES[layout] = ref
    return ref


def edge_launch_rows(ref):
    """The edge launch: every edge row, then ordinary rows up to EDGE_LAUNCH rows (indices into the reference's rows)."""
    edge = np.arange(ref.first_edge, len(ref.names))
    return np.concatenate([edge, np.arange(max(EDGE_LAUNCH - len(edge), 0))])


_GRADS = {}


def grad_reference(flame_consts, layout, n, zero_rot, to_2d):
    """Upstream gradients, the float64 gradient and `backward_edges.row_bars` of the layout's first n ordinary rows, once."""
    key = (layout, n, zero_rot, to_2d)
    if key not in _GRADS:
        ref = reference(flame_consts, layout)
        wv, wp = be.weights(n, to_2d)
        g32, _ = be.oracle_grad(flame_consts, ref.params[:n], wv, wp, zero_rot, to_2d, torch.float32, ref.consts)
        g64, _ = be.oracle_grad(be.oracle64(flame_consts), ref.params[:n], wv, wp, zero_rot, to_2d, torch.float64, ref.consts)
        _GRADS[key] = types.SimpleNamespace(wv=wv, wp=wp, g64=g64, e32=be.row_errors(g32, g64), bars=be.row_bars(g32, g64))
    return _GRADS[key]
