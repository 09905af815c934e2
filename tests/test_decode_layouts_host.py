"""CPU: the yardstick of tests/test_gpu_decode_layouts.py, held on its own before any kernel is held to it -- the rows of
tests/decode_layouts.py are what the module says, the float64 statement is finite on every one of them, every layout's floor
(4 x the float32 oracle's own error on ordinary rows) stays under the suite's TOL_V / TOL_PX, and a bar exceeds its floor only
on the rows that may: an angle of 8191 rad and more, the near-parallel 6-DoF halves, the x4 coefficients."""
import numpy as np
import pytest
import torch

import backward_edges as be
import decode_layouts as dl
from oracle import flame_ref


@pytest.fixture(scope="module")
def refs(flame_consts):
    return {layout: dl.reference(flame_consts, layout) for layout in dl.LAYOUTS}


def test_layouts_and_rows_are_what_the_module_says(refs, static):
    assert {k: dl.n_params(c) for k, c in dl.LAYOUTS.items()} == {"D": 413, "F": 422, "N": 163, "FN": 172, "J0": 410}
    base = {k: dl.synthetic.synthetic_params(dl.N_ORDINARY, seed=dl.SEEDS[k]) for k in dl.LAYOUTS}
    for layout, ref in refs.items():
        c = ref.consts
        assert ref.params.dtype == np.float32 and ref.params.shape == (len(ref.names), dl.n_params(c))
        assert len(set(ref.names)) == len(ref.names)
        fp = flame_ref.split_3dmm(torch.from_numpy(ref.params[:dl.N_ORDINARY]), c)
        b = base[layout]
        assert np.array_equal(fp["shape"].numpy(), b[:, :c["shape"]]) and np.array_equal(fp["expression"].numpy(), b[:, 300:300 + c["expression"]])
        assert np.array_equal(fp["jaw"].numpy(), b[:, 400:400 + c["jaw"]]) and np.array_equal(fp["rotation"].numpy(), b[:, 403:409])
        assert np.array_equal(fp["translation"].numpy(), b[:, 409:412]) and np.array_equal(fp["scale"].numpy(), b[:, 412:])
        assert np.array_equal(fp["eyeballs"].numpy(), dl.extras(dl.N_ORDINARY)[:, :c["eyeballs"]])
        assert np.array_equal(fp["neck"].numpy(), dl.extras(dl.N_ORDINARY)[:, 6:6 + c["neck"]])
        assert float(np.abs(fp["translation"].numpy()[:, 2]).min()) > 0.0  # tz := 0 is a change on every ordinary row
    assert np.array_equal(refs["D"].params, base["D"])
    for batch in sorted({b for bs in dl.BATCHES.values() for b in bs}):
        rows = dl.launch_rows(batch)
        assert rows.shape == (batch,) and np.array_equal(rows[:64], np.arange(min(batch, 64)))
        for i in range(64, batch):  # a repeat sits in another row block, another 16-row MFMA block and another lane
            assert rows[i] == (i - 64 + dl.ROTATE) % 64 and rows[i] // 16 != (i % 64) // 16 and rows[i] % 16 != i % 16
    assert np.array_equal(dl.launch_rows(130)[:65], dl.launch_rows(65))  # the two launches share their first 65 rows
    lm = dl.landmark_list(static)
    assert lm.size > 445 and np.unique(lm).size < lm.size and lm.min() >= 0 and lm.max() < 5023
    # edge rows: F sweeps four joints and carries the scale / 6-DoF / zero / x4 rows, N carries all of edge_params()
    f, n = refs["F"], refs["N"]
    e_names = be.edge_params()[0]
    assert n.names[dl.N_ORDINARY:] == e_names
    row = dict(zip(f.names, f.params))
    off = dl.offsets(f.consts)
    for joint, at in (("neck", off["neck"].start), ("jaw", off["jaw"].start), ("eye0", off["eyeballs"].start), ("eye1", off["eyeballs"].start + 3)):
        assert not row[f"{joint}_0"][at:at + 3].any()
        assert 0.0 < float(row[f"{joint}_1e-40"][at]) < np.finfo(np.float32).tiny  # a denormal, not a flushed zero
        for name, angle in be.ANGLES:
            r = row[f"{joint}_{name}"]
            assert abs(float(np.linalg.norm(r[at:at + 3].astype(np.float64))) - angle) <= 1e-7 * angle, (joint, name)
            other = np.ones(r.size, bool)
            other[at:at + 3] = False
            assert np.array_equal(r[other], row["unchanged"][other])  # the other joints keep their ordinary values
    assert not row["all_zero"].any() and not dict(zip(n.names, n.params))["all_zero"].any()
    for name in e_names:
        if name.startswith(("scale_", "rot6_", "shape_expr_x4")):
            assert name in row and np.array_equal(row[name][off["eyeballs"].start:off["neck"].stop], row["unchanged"][off["eyeballs"].start:off["neck"].stop])
    assert float(row["scale_at_clamp"][off["scale"]][0]) + 1.0 == 0.0
    for ref in (f, n):
        rows = dl.edge_launch_rows(ref)
        assert len(rows) == dl.EDGE_LAUNCH and len(set(rows.tolist())) == len(rows)
        assert set(range(ref.first_edge, len(ref.names))) <= set(rows.tolist())
    assert len(f.names) - f.first_edge == 70 and len(n.names) - n.first_edge == len(e_names)


def test_float64_statement_is_finite_everywhere_and_agrees_with_float32_on_ordinary_rows(refs):
    for layout, ref in refs.items():
        for t in (ref.v64, ref.v064, ref.p64):
            assert t.dtype == torch.float64 and t.shape == (len(ref.names), 5023, 3)
            bad = [n for n, ok in zip(ref.names, torch.isfinite(t).flatten(1).all(dim=1)) if not bool(ok)]
            assert not bad, (layout, bad)
        assert bool(torch.isfinite(ref.e32_v).all()) and bool(torch.isfinite(ref.e32_px).all())
        assert bool(torch.isfinite(ref.cond_v).all()) and bool(torch.isfinite(ref.cond_px).all())
        assert float(ref.v64[:dl.N_ORDINARY].abs().max()) > 0.05  # a head, in model units


def test_every_floor_stays_under_the_bars_of_the_suite(refs):
    for layout, ref in refs.items():
        e_v, e_px = float(ref.e32_v[:dl.N_ORDINARY].max()), float(ref.e32_px[:dl.N_ORDINARY].max())
        print(f"{layout:2s}  e32 on 64 ordinary rows: {e_v:.2e} model units, {e_px:.2e} px   floors: {ref.floor_v:.2e}, {ref.floor_px:.2e}")
        if layout not in dl.RAISED_FLOORS:
            assert ref.floor_v == 4.0 * e_v and ref.floor_px == 4.0 * e_px
        assert 0.0 < ref.floor_v <= dl.TOL_V and 0.0 < ref.floor_px <= dl.TOL_PX, layout
        assert float(ref.bar_v[:dl.N_ORDINARY].max()) == ref.floor_v and float(ref.bar_px[:dl.N_ORDINARY].max()) == ref.floor_px
    for layout, (v, px, reason) in dl.RAISED_FLOORS.items():
        assert v <= dl.TOL_V and px <= dl.TOL_PX and reason


def test_only_the_named_rows_get_a_bar_above_the_floor(refs):
    """bar(row) = max(floor, 4 e32(row), cond(row)); the float32 oracle's own error or the conditioning of an angle may lift it
    only at 8191 rad and beyond (the float32 norm of the vector is 2e-4 rad and more off there), on the near-parallel 6-DoF
    halves and on the x4 coefficients. cond is nonzero on swept rows only and stays under the floor below 8191 rad."""
    for layout in ("F", "N"):
        ref, withheld = refs[layout], []
        for i in range(ref.first_edge, len(ref.names)):
            n = ref.names[i]
            e_v, e_px, c_v, c_px = float(ref.e32_v[i]), float(ref.e32_px[i]), float(ref.cond_v[i]), float(ref.cond_px[i])
            bar_v, bar_px = float(ref.bar_v[i]), float(ref.bar_px[i])
            may = n.endswith(dl.LIFTED)
            assert bar_v == max(ref.floor_v, 4.0 * e_v, c_v if may else 0.0) and bar_px == max(ref.floor_px, 4.0 * e_px, c_px if may else 0.0)
            if not may and (c_v > ref.floor_v or c_px > ref.floor_px):
                withheld.append(n)
            lifted = bar_v > ref.floor_v or bar_px > ref.floor_px
            print(f"{layout:2s} {n:20s} e32 {e_v:.2e} {e_px:.2e}  cond {c_v:.2e} {c_px:.2e}  bar {bar_v:.2e} {bar_px:.2e}{'  LIFTED' if lifted else ''}")
            swept = n.split("_")[0] in ("neck", "jaw", "eye0", "eye1")
            assert swept or (c_v == 0.0 and c_px == 0.0), n
            if swept and not n.endswith(("_0", "_1e-40")):
                assert c_v > 0.0, n
            assert not lifted or n.endswith(dl.LIFTED), (layout, n, bar_v, ref.floor_v, bar_px, ref.floor_px)
        print(f"{layout}: conditioning over the floor and NOT granted: {withheld}")
        assert all(n.endswith("_100") for n in withheld), withheld  # the next angle down; nothing below it comes near the floor
    for layout in ("D", "FN", "J0"):
        assert len(refs[layout].names) == dl.N_ORDINARY and float(refs[layout].cond_v.max()) == 0.0


def test_the_rows_can_tell_a_wrong_kernel_from_a_right_one(refs, flame_consts):
    """What the layouts mean, in float64, and that the ordinary rows depend on it by far more than a bar: a narrow row IS the
    default row with zeros in the padding, a row without a jaw input IS the default row with a zero jaw; a joint input ignored,
    the two eyeballs swapped, or the first entry past a narrow width read instead of a zero each move some vertex by more than
    100 floors on every one of the first four rows."""
    c64 = be.oracle64(flame_consts)
    n = 4

    def moved(layout, params):
        ref = refs[layout]
        v, v0, p = dl.statement(c64, ref.consts, params, torch.float64)
        return torch.minimum(dl.row_max(v - ref.v64[:n]) / ref.floor_v, dl.row_max(p - ref.p64[:n]) / ref.floor_px)

    for layout in ("N", "FN"):
        ref = refs[layout]
        wide = dict(ref.consts, shape=300, expression=100)
        fp = flame_ref.split_3dmm(torch.from_numpy(ref.params[:n]), ref.consts)
        z = lambda k: torch.zeros((n, k))  # noqa: E731
        padded = torch.cat([fp["shape"], z(200), fp["expression"], z(50), fp["jaw"], fp["rotation"], fp["eyeballs"], fp["neck"],
                            fp["translation"], fp["scale"]], dim=1)
        v, v0, p = dl.statement(c64, wide, padded, torch.float64)
        assert torch.equal(v, ref.v64[:n]) and torch.equal(v0, ref.v064[:n]) and torch.equal(p, ref.p64[:n])
        leaked = padded.clone()
        leaked[:, 100] = fp["expression"][:, 0]  # what sits behind the last shape entry in the narrow row
        v, v0, p = dl.statement(c64, wide, leaked, torch.float64)
        assert float((dl.row_max(v - ref.v64[:n]) / ref.floor_v).min()) > 100.0, layout
    j0 = refs["J0"]
    with_jaw = np.insert(j0.params[:n], [400, 400, 400], 0.0, axis=1)
    v, v0, p = dl.statement(c64, dl.LAYOUTS["D"], with_jaw, torch.float64)
    assert torch.equal(v, j0.v64[:n]) and torch.equal(p, j0.p64[:n])
    for layout in ("F", "FN"):
        ref = refs[layout]
        off = dl.offsets(ref.consts)
        eyes = off["eyeballs"].start
        for name, at in (("neck", off["neck"].start), ("jaw", off["jaw"].start), ("eye0", eyes), ("eye1", eyes + 3)):
            p = ref.params[:n].copy()
            p[:, at:at + 3] = 0.0
            assert float(moved(layout, p).min()) > 100.0, (layout, name)
        p = ref.params[:n].copy()
        p[:, eyes:eyes + 3], p[:, eyes + 3:eyes + 6] = ref.params[:n, eyes + 3:eyes + 6], ref.params[:n, eyes:eyes + 3]
        assert float(moved(layout, p).min()) > 100.0, layout
    for layout in ("D", "N"):
        ref = refs[layout]
        p = ref.params[:n].copy()
        p[:, dl.offsets(ref.consts)["jaw"]] = 0.0
        assert float(moved(layout, p).min()) > 100.0, layout
