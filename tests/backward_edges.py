"""Edge rows, the float64 statement and the per-row bars that the backward tests share (tests/test_backward_edges_host.py,
tests/test_gpu_backward_edges.py, the tie cases of tests/test_gpu_autograd.py; tests/decode_layouts.py takes the rows, the joint
sweep and the float64 statement for the forward on every constants layout). Test infrastructure, not a conftest.

The float64 statement is `oracle.flame_ref` itself, unmodified, over a `FlameConstants` whose five float buffers are cast
to double: torch promotes the oracle's own float32 zeros, so every product of the chain is a double product.

A row's gradient is judged against THAT row's largest float64 entry, never the batch's: the rows with a degenerate 6-DoF
vector have gradients near 1e13 and would hide every other row behind a batch maximum.

Two parameter points are left out, with the reference:
  * jaw exactly -1e-8 in every component: smplx's `angle = ||r + 1e-8||` is 0 there and `r / angle` is -inf; the
    reference's own float32 gradient is non-finite, so there is nothing to hold a kernel to;
  * a 6-DoF vector whose halves are exactly parallel: `cross(b1, vy)` is 0 up to rounding, F.normalize's eps floor takes
    over and the float32 and float64 reference gradients differ by 100 %. The near-parallel row (1e-4 off) is kept.
"""
import dataclasses

import numpy as np
import torch

from dad_3dheads_amd import synthetic
from oracle import flame_ref

RTOL = 2e-4  # tests/test_gpu_autograd.py: fp32 sums over 15069 terms in two different orders
JAW, ROT, TZ, SCALE = slice(400, 403), slice(403, 409), 411, 412
AXIS = np.array([2.0, -3.0, 6.0]) / 7.0  # 4 + 9 + 36 = 49; no component of angle * AXIS is a round float32
# first quadrant, every other quadrant, the quadrant borders, more than a turn, and past the fast range reduction of sinf
ANGLES = [("1e-6", 1e-6), ("1e-3", 1e-3), ("1.2", 1.2), ("pi/2", float(np.float32(np.pi / 2))), ("2.5", 2.5),
          ("pi", float(np.float32(np.pi))), ("4.0", 4.0), ("5.5", 5.5), ("7.0", 7.0), ("100", 100.0), ("8191", 8191.0),
          ("8193", 8193.0), ("1e6", 1e6)]
# the rows whose float32 reference gradient is itself more than RTOL / 4 off the float64 one (measured on the CPU, asserted
# in tests/test_backward_edges_host.py): only these may get a bar above RTOL
ILL_CONDITIONED = ("jaw_1e6", "rot6_near_parallel")


def axis_angle(angle):
    return (AXIS * angle).astype(np.float32)


def edge_params():
    """(names, [N,413] float32): `synthetic_params(1, seed=103)[0]` with one change per row."""
    base = synthetic.synthetic_params(1, seed=103)[0]
    rows = [("unchanged", base.copy())]

    def add(name, edit):
        p = base.copy()
        edit(p)
        rows.append((name, p))

    def put(where, value):
        def edit(p):
            p[where] = value
        return edit

    add("jaw_0", put(JAW, 0.0))
    add("jaw_1e-40", put(JAW, np.float32(1e-40)))  # denormal
    for name, angle in ANGLES:
        add("jaw_" + name, put(JAW, axis_angle(angle)))
    add("scale_clamped", put(SCALE, -1.5))  # clamp(scale + 1, 1e-8): below the floor
    # scale + 1 == 0 < 1e-8: clamped like the row above. torch passes the gradient at x == min, but x == 1e-8 cannot be reached:
    # float32 has no scale with scale + 1 == 1e-8 (the sum rounds to 0 or to 6e-8), so 0 is the nearest point to the floor
    add("scale_at_clamp", put(SCALE, -1.0))
    add("scale_above_clamp", put(SCALE, np.nextafter(np.float32(-1.0), np.float32(0.0))))  # scale + 1 == 2^-24 > 1e-8: passes
    add("rot6_0", put(ROT, 0.0))
    add("rot6_x1e-20", put(ROT, base[ROT] * np.float32(1e-20)))
    add("rot6_x1e15", put(ROT, base[ROT] * np.float32(1e15)))

    def near_parallel(p):
        p[406:409] = 2.0 * p[403:406]
        p[406] += 1e-4

    add("rot6_near_parallel", near_parallel)
    add("all_zero", put(slice(0, 413), 0.0))
    add("shape_expr_x4", put(slice(0, 400), base[:400] * 4.0))
    return [n for n, _ in rows], np.stack([p for _, p in rows]).astype(np.float32)


FULL = {"shape": 300, "expression": 100, "jaw": 3, "rotation": 6, "eyeballs": 6, "neck": 3, "translation": 3, "scale": 1}
EXTRA_JOINTS = (("eye0", 409), ("eye1", 412), ("neck", 415))  # where the full layout keeps the joints the shipped one lacks


def joint_sweep(joints=EXTRA_JOINTS):
    """(names, [N,422] float32) on the full layout (neck + eyeballs are inputs): `edge_params()`'s plain row with ordinary
    neck / eyeball values, then each of `joints` (name, offset) in turn through zero, a denormal and ANGLES on AXIS, the other
    joints at their ordinary values."""
    base413 = edge_params()[1][0]
    extra = (0.2 * np.random.default_rng(3).standard_normal(9)).astype(np.float32)
    base = np.concatenate([base413[:409], extra, base413[409:]])
    names, rows = ["unchanged"], [base]
    for joint, at in joints:
        for name, value in [("0", np.zeros(3, np.float32)), ("1e-40", np.full(3, 1e-40, np.float32))] + \
                           [(n, axis_angle(a)) for n, a in ANGLES]:
            row = base.copy()
            row[at:at + 3] = value
            names.append(f"{joint}_{name}")
            rows.append(row)
    return names, np.stack(rows)


def oracle64(flame_consts):
    """The oracle's constants with the five float buffers in double: `flame_ref` then runs in float64 throughout."""
    f = ("v_template", "shapedirs", "posedirs", "j_regressor", "lbs_weights")
    return dataclasses.replace(flame_consts, **{k: getattr(flame_consts, k).double() for k in f})


def weights(n, to_2d, seed=5):
    """Upstream gradients of the summed loss: wv [n,5023,3], wp [n,5023,2|3] (float32, seeded). The float32 oracle's own
    error on the jaw_8191 / jaw_8193 rows moves between 3e-6 and 7e-5 with the draw (seeds 1-8 on the CPU); this draw keeps
    it under RTOL / 4, so those rows are held to RTOL itself and not to a wider reference-derived bar."""
    gen = torch.Generator().manual_seed(seed)
    return torch.randn((n, 5023, 3), generator=gen), torch.randn((n, 5023, 2 if to_2d else 3), generator=gen)


def oracle_grad(consts, params, wv, wp, zero_rot, to_2d, dtype, layout=flame_ref.DEFAULT_CONSTS):
    """d/d(params) of (v . wv).sum() + 1e-2 (proj . wp).sum() through the oracle in `dtype` -> ([N,P] float64, value).
    `layout`: the FLAME constants dict the params rows are cut by (P = 413 for the shipped one)."""
    p = torch.as_tensor(params).to(dtype).clone().requires_grad_(True)
    q = p * 1.0  # the network output: a non-leaf that reprojected_vertices writes tz := 0 into
    v = flame_ref.vertices_3d(consts, q, zero_rotation=zero_rot, consts=layout)
    proj = flame_ref.reprojected_vertices(consts, q, to_2d=to_2d, consts=layout)
    value = (v * wv.to(dtype)).sum() + 1e-2 * (proj * wp.to(dtype)).sum()
    value.backward()
    return p.grad.double(), value.detach().double()


def row_errors(g, g64):
    """Per row: max |g - g64| over the row's largest |g64| entry (inf where g is not finite)."""
    g, g64 = torch.as_tensor(g).detach().cpu().double(), torch.as_tensor(g64).double()
    err = (g - g64).abs().amax(dim=1) / g64.abs().amax(dim=1)
    return torch.where(torch.isfinite(g).all(dim=1), err, torch.full_like(err, float("inf")))


def row_bars(g32, g64):
    """Per row: max(RTOL, 4 e32), as a fraction of the row's largest float64 entry; e32 = the float32 oracle's own error
    there. The 4 leaves a kernel room for another summation order where the reference itself is ill-conditioned."""
    return torch.clamp(4.0 * row_errors(g32, g64), min=RTOL)


# ---- normalize_to_cube: exact ties (small integers, so float32 and float64 tie alike) ----------------------------------
def tie_cases():
    """(name, n_verts, [region index lists], pred [n_verts,3] float32 integers). torch routes the gradient of the scale
    `v.max(-1)[0].max(-2)[0]` to the first vertex POSITION whose row maximum is the global one, then to that vertex's first
    axis; the gradients of `min(1)` / `max(1)` go to the first position that holds the extremum."""
    f = lambda rows: np.asarray(rows, dtype=np.float32)  # noqa: E731
    pad = [[1, 1, 1], [2, 1, 2], [1, 2, 2]]  # interior vertices: no extremum, no tie
    cases = [
        # extents (4, 4, 2): y's maximum sits at position 1, x's at position 2 -> torch picks (position 1, y)
        ("two_axes_equal", f([[0, 0, 0], [1, 4, 1], [4, 1, 1]] + pad), [[0, 1, 2, 3, 4, 5]]),
        # extents (4, 4, 4), maxima at positions 3 (z), 4 (y), 5 (x) -> (position 3, z)
        ("three_axes_equal", f([[0, 0, 0]] + pad[:2] + [[1, 1, 4], [1, 4, 1], [4, 1, 1]]), [[0, 1, 2, 3, 4, 5]]),
        ("minimum_twice", f([[3, 2, 1], [0, 0, 0], [5, 3, 2], [0, 0, 0], [2, 1, 1]]), [[0, 1, 2, 3, 4]]),
        ("maximum_twice", f([[0, 0, 0], [5, 3, 2], [1, 1, 1], [5, 3, 2], [2, 1, 1]]), [[0, 1, 2, 3, 4]]),
        # vertex 1 holds every maximum and is listed twice; vertex 0 holds every minimum and is listed twice
        ("extremum_listed_twice", f([[0, 0, 0], [6, 3, 2], [1, 1, 1], [2, 2, 1]]), [[2, 1, 0, 3, 1, 0]]),
        # region 1 sees the vertices of region 0 in another order plus one more: other ties, other winners
        ("overlapping_regions", f([[0, 0, 0], [1, 4, 1], [4, 1, 1], [2, 2, 2], [1, 1, 4], [4, 4, 0]]),
         [[0, 1, 2, 3], [4, 2, 1, 0, 3], [5, 0, 3, 1]]),
    ]
    return [(name, v.shape[0], [np.asarray(r) for r in regions], v) for name, v, regions in cases]


def tie_target(pred):
    """A target for a tie case: seeded noise, so that a difference of the normalised values is exactly 0 or far from it (asserted in
    tests/test_backward_edges_host.py: L1's own kink stays out of the tie test)."""
    return (2.0 * np.random.default_rng(3).standard_normal(pred.shape)).astype(np.float32)
