"""CPU: the yardstick of tests/test_gpu_backward_edges.py, held on its own before any kernel is held to it -- the float64
statement of the decode (tests/backward_edges.py `oracle64`) against the float32 oracle, the edge rows' reference gradients,
the cap on the reference-derived bars, and torch's routing on the tie cases of the `normalize_to_cube` kernel tests."""
import numpy as np
import pytest
import torch

import backward_edges as be
from dad_3dheads_amd.losses import normalize_to_cube

CONFIGS = [(True, True), (False, False)]  # (zero_rotation, to_2d) of the GPU test


@pytest.fixture(scope="module")
def edge_grads(flame_consts):
    """{(zero_rot, to_2d): (g32, g64, v32, v64)} over the edge rows, computed once."""
    names, params = be.edge_params()
    c64 = be.oracle64(flame_consts)
    out = {}
    for zr, t2 in CONFIGS:
        wv, wp = be.weights(len(names), t2)
        g32, v32 = be.oracle_grad(flame_consts, params, wv, wp, zr, t2, torch.float32)
        g64, v64 = be.oracle_grad(c64, params, wv, wp, zr, t2, torch.float64)
        out[zr, t2] = (g32, g64, v32, v64)
    return names, out


def test_edge_rows_are_what_the_module_says():
    names, p = be.edge_params()
    assert p.dtype == np.float32 and p.shape == (len(names), 413) and len(set(names)) == len(names)
    row = dict(zip(names, p))
    base = row["unchanged"]
    for n in names[1:]:
        assert (row[n] != base).any(), n
    assert 0.0 < float(row["jaw_1e-40"][400]) < np.finfo(np.float32).tiny  # a denormal, not a flushed zero
    for name, angle in be.ANGLES:
        got = float(np.linalg.norm(row["jaw_" + name][be.JAW].astype(np.float64)))
        assert abs(got - angle) <= 1e-7 * angle, name
    assert float(row["scale_at_clamp"][412]) + 1.0 == 0.0 and float(row["scale_clamped"][412]) == -1.5
    assert float(np.float32(row["scale_above_clamp"][412]) + np.float32(1.0)) > 1e-8
    assert not row["all_zero"].any() and not row["rot6_0"][be.ROT].any()
    vx, vy = row["rot6_near_parallel"][403:406].astype(np.float64), row["rot6_near_parallel"][406:409].astype(np.float64)
    sin = np.linalg.norm(np.cross(vx, vy)) / (np.linalg.norm(vx) * np.linalg.norm(vy))
    assert 0.0 < sin < 1e-3


def test_float64_statement_equals_the_float32_oracle_on_the_plain_row(flame_consts):
    from oracle import flame_ref

    names, params = be.edge_params()
    p = torch.from_numpy(params[:1])
    c64 = be.oracle64(flame_consts)
    for zr, t2 in CONFIGS:
        v32 = flame_ref.vertices_3d(flame_consts, p.clone(), zero_rotation=zr)
        v64 = flame_ref.vertices_3d(c64, p.double(), zero_rotation=zr)
        assert v64.dtype == torch.float64
        assert float((v32.double() - v64).abs().max()) <= 2e-6 * float(v64.abs().max())
        pr32 = flame_ref.reprojected_vertices(flame_consts, p.clone(), to_2d=t2)
        pr64 = flame_ref.reprojected_vertices(c64, p.double(), to_2d=t2)
        assert pr64.dtype == torch.float64 and pr64.shape[-1] == (2 if t2 else 3)
        assert float((pr32.double() - pr64).abs().max()) <= 2e-6 * float(pr64.abs().max())
        wv, wp = be.weights(1, t2)
        g32, _ = be.oracle_grad(flame_consts, params[:1], wv, wp, zr, t2, torch.float32)
        g64, _ = be.oracle_grad(c64, params[:1], wv, wp, zr, t2, torch.float64)
        assert float(be.row_errors(g32, g64)[0]) <= 2e-6


def test_every_edge_row_has_finite_reference_gradients(edge_grads):
    names, grads = edge_grads
    for (zr, t2), (g32, g64, v32, v64) in grads.items():
        for i, n in enumerate(names):
            assert bool(torch.isfinite(g32[i]).all()) and bool(torch.isfinite(g64[i]).all()), (zr, t2, n)
            assert float(g64[i].abs().max()) > 0.0
        assert float(g64[:, be.TZ].abs().max()) == 0.0 and float(g32[:, be.TZ].abs().max()) == 0.0
        scale = dict(zip(names, zip(g32[:, be.SCALE].tolist(), g64[:, be.SCALE].tolist())))
        # clamp(scale + 1, 1e-8): nothing passes below the floor, and scale = -1 IS below it (0 < 1e-8) in both precisions
        assert scale["scale_clamped"] == (0.0, 0.0) and scale["scale_at_clamp"] == (0.0, 0.0)
        assert all(abs(g) > 1e-3 for g in scale["scale_above_clamp"])


def test_only_the_two_ill_conditioned_rows_get_a_bar_above_rtol(edge_grads):
    """The cap that keeps the reference-derived bar from hiding a failure: a row's bar is max(RTOL, 4 e32), and e32 (the
    float32 oracle's own error) may lift it only where the reference is ill-conditioned -- sin / cos of an angle near 1e6
    whose float32 norm is already 0.06 rad off, and Gram-Schmidt on two vectors 1e-4 from parallel."""
    names, grads = edge_grads
    for (zr, t2), (g32, g64, _, _) in grads.items():
        e32, bars = be.row_errors(g32, g64), be.row_bars(g32, g64)
        for n, e, bar in zip(names, e32.tolist(), bars.tolist()):
            print(f"zero_rot={zr} to_2d={t2} {n:20s} e32 = {e:.2e}  bar = {bar:.2e}")
            assert bar == max(be.RTOL, 4.0 * e)
            if n in be.ILL_CONDITIONED:
                assert be.RTOL / 4.0 < e < 2e-2, (n, e)  # lifted, and still a bar that means something (< 8 %)
            else:
                assert bar == be.RTOL, (n, e)
            if n not in be.ILL_CONDITIONED and n not in ("jaw_8191", "jaw_8193"):
                assert e <= 5e-6, (n, e)


def test_row_bars_judge_each_row_by_its_own_maximum():
    g64 = torch.tensor([[1.0, -2.0, 0.0], [1e13, 1.0, 0.0]], dtype=torch.float64)
    g32 = g64.clone()
    g32[0, 0] += 2e-3  # 1e-3 of row 0's maximum: against the batch maximum it would vanish
    assert be.row_errors(g32, g64).tolist() == pytest.approx([1e-3, 0.0])
    assert be.row_bars(g32, g64).tolist() == pytest.approx([4e-3, be.RTOL])
    g32[1, 2] = float("nan")
    assert be.row_errors(g32, g64)[1] == float("inf")


def _routing(v, dtype):
    """Where torch sends the gradients of normalize_to_cube's three reductions on v [n,3]: the (position, axis) of the scale,
    the positions of the minima and of the maxima of `v - min` per axis."""
    v = torch.as_tensor(v).to(dtype)[None].requires_grad_(True)
    lo = v.min(1, True)[0]
    v1 = v - lo
    hi = v1.max(1, True)[0]
    v2 = v1 - 0.5 * hi
    v1.retain_grad(), v2.retain_grad()
    s = v2.max(-1, True)[0].max(-2, True)[0]
    (g_lo,) = torch.autograd.grad(lo.sum(), v, retain_graph=True)
    (g_hi,) = torch.autograd.grad(hi.sum(), v1, retain_graph=True)
    (g_s,) = torch.autograd.grad(s.sum(), v2)
    assert g_s.sum() == 1 and (g_lo.sum(1) == 1).all() and (g_hi.sum(1) == 1).all()  # one element each: no split among ties
    at = lambda g: [int(x) for x in g[0].argmax(0)]  # noqa: E731
    star = int(g_s[0].flatten().argmax())
    return (star // 3, star % 3), at(g_lo), at(g_hi)


def test_torch_routes_ties_alike_in_float32_and_float64():
    """The tie cases are small integers so that both precisions tie; what the kernels are held to is then one rule, the one
    torch documents: the first maximal (minimal) value. For the scale that is the first POSITION whose row maximum is the
    global one, then that vertex's first axis -- not the first axis of largest extent."""
    cases = {name: (regions, pred) for name, _, regions, pred in be.tie_cases()}
    for name, (regions, pred) in cases.items():
        for r in regions:
            assert _routing(pred[r], torch.float32) == _routing(pred[r], torch.float64), name
            for dtype in (torch.float32, torch.float64):  # no difference NEAR 0
                p = torch.as_tensor(pred[r]).to(dtype)
                t = torch.as_tensor(be.tie_target(pred)[r]).to(dtype)
                d = (normalize_to_cube(p) - normalize_to_cube(t)).abs()
                assert bool(((d == 0.0) | (d > 1e-3)).all()), name  # exactly on L1's kink (both normalised maxima are 1) or well off it
    regions, pred = cases["two_axes_equal"]
    star, lo, hi = _routing(pred[regions[0]], torch.float32)
    assert star == (1, 1) and hi == [2, 1, 4]  # extents 4, 4, 2: x's maximum is at position 2, yet (position 1, y) gets the scale
    regions, pred = cases["three_axes_equal"]
    assert _routing(pred[regions[0]], torch.float32)[0] == (3, 2)
    regions, pred = cases["minimum_twice"]
    assert _routing(pred[regions[0]], torch.float32)[1] == [1, 1, 1]
    regions, pred = cases["maximum_twice"]
    star, lo, hi = _routing(pred[regions[0]], torch.float32)
    assert star == (1, 0) and hi == [1, 1, 1]
    regions, pred = cases["extremum_listed_twice"]
    star, lo, hi = _routing(pred[regions[0]], torch.float32)
    assert star == (1, 0) and lo == [2, 2, 2] and hi == [1, 1, 1]  # the first of the two listings
    regions, pred = cases["overlapping_regions"]
    assert [_routing(pred[r], torch.float32)[0] for r in regions] == [(1, 1), (0, 2), (0, 0)]
