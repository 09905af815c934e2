"""CPU: certifies the cases of tests/train_objective_cases.py that tests/test_gpu_train_objective_edges.py feeds to the kernels of
csrc/train_objective.hip. (a) every exact case sums to the same float64 bits forward, reversed and permuted, and to the integer
expectation; (b) the reference's formulas as one-line torch statements, in float32 and float64 on the CPU, agree with the expectation --
to the bit where the case is exact in float32 too (rates, visibility values, Pythagorean errors); (c) every family tells the truth from
the mutants of the restatement that apply to it; (d) the three expf facts and the tie arithmetic the cases lean on.

Mutants and the families they apply to: last element dropped / first element counted twice (IoU, visibility, keypoints); presence on one
side only (visibility, keypoints); the sum divided by n_points - 1 (keypoints); `<` turned into `<=` (the ties)."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import train_objective_cases as tc
import train_objective_restatement as rs

F = np.float32


def _orders(a, seed=0):
    """Row sums of a [rows, n] float64 array taken strictly in sequence: forward, reversed, in a seeded permutation."""
    perm = np.random.default_rng(seed).permutation(a.shape[1])
    return [np.cumsum(v, axis=1)[:, -1] for v in (a, a[:, ::-1], a[:, perm])]


# ---- (d) the facts the cases lean on ------------------------------------------------------------------------------------------------
def test_expf_facts_and_tie_arithmetic():
    with np.errstate(over="ignore"):
        e = np.exp(-tc.LOGITS)  # float32
        assert e.dtype == F and e[0] == 1.0 and e[1] == 0.0 and e[2] == np.inf and e[3] == 0.0 and e[4] == np.inf
        s = F(1) / (F(1) + e)
    assert np.array_equal(s * 256, tc.LOGIT_S256) and np.all(s * (1 - s) * (s != 0.5) == 0)
    assert np.array_equal((np.array([0, 255], np.uint8).astype(F) / F(255.0)), [0.0, 1.0])
    assert 0.05 * 100.0 == 5.0 and 0.1 * 100.0 == 10.0 and 0.25 * 2.0 == 0.5 and np.sqrt(np.float64(100) * np.float64(100)) == 100.0
    for kind in ("bbox", "plain"):
        case = tc.kp_tie_case(kind)
        lim = np.array([t * case["norm"][0] for t in case["thresholds"]])
        assert set(case["limit"]) == set(lim)
        assert np.array_equal(np.sign(case["err"] - case["limit"]), case["side"])
        assert np.array_equal(case["err"].astype(F), case["err"])  # the neighbours are float32's


# ---- IoU -----------------------------------------------------------------------------------------------------------------------------------
def _iou_from_arrays(x, t, sigmoid, mutant=None):
    """[channels, 3] float64 sums from the arrays the kernel reads, the kernel's way: fp32 sigmoid and target, float64 products."""
    n = x.shape[0] * x.shape[1]
    with np.errstate(over="ignore"):
        s = (F(1) / (F(1) + np.exp(-x))) if sigmoid else x
    s, t = s.reshape(n, -1).astype(np.float64), rs.target64(t).reshape(n, -1).astype(np.float64)
    terms = np.stack([t * s, t * t, s * s], 1)  # [channels, 3, hw]
    if mutant == "drop_last":
        terms = terms[..., :-1]
    if mutant == "first_twice":
        terms = np.concatenate([terms, terms[..., :1]], -1)
    return terms.sum(-1)


@pytest.mark.parametrize("sigmoid", [False, True])
def test_iou_cases_are_exact_in_any_order_and_catch_the_mutants(sigmoid):
    for k, (bc, hw) in enumerate(tc.IOU_SHAPES):
        case = tc.iou_case(bc, hw, sigmoid, 1000 + k)
        assert case["x"].shape[:2] == bc and case["x"][0, 0].size == hw
        for t_arr, t256 in ((case["t_f"], case["tf256"]), (case["t_u8"], case["tu256"])):
            want = tc.iou_sums(case["s256"], t256)
            for col, prod in enumerate(tc.iou_products(case["s256"], t256)):
                for got in _orders(prod, k):
                    assert np.array_equal(got, want[:, col])
            assert np.array_equal(_iou_from_arrays(case["x"], t_arr, sigmoid), want)
            for mutant in ("drop_last", "first_twice"):
                moved = _iou_from_arrays(case["x"], t_arr, sigmoid, mutant) != want
                assert moved[:, 2].all() and moved.all(1).sum() >= len(want) - 1, (bc, hw, mutant)  # all but the zero-target channel
            if not sigmoid:  # the reference's statement (keypoint_losses.py:11-23, metrics/iou.py:15-31) on probabilities
                n, d, iou32 = tc.iou_channels(want)
                exact = tc.exact_ratio_mean(n, d)
                for dtype, eps in ((torch.float64, 2.0 ** -53), (torch.float32, 2.0 ** -24)):
                    y, t = torch.from_numpy(case["x"]).to(dtype), torch.from_numpy(rs.target64(t_arr)).to(dtype)
                    op_sum = lambda v: v.view(v.shape[0], v.shape[1], -1).sum(2)  # noqa: E731
                    st, tt, ss = op_sum(t * y), op_sum(t ** 2), op_sum(y ** 2)
                    sums = torch.stack([st, tt, ss], -1).reshape(-1, 3).double().numpy()
                    if dtype == torch.float64:
                        assert np.array_equal(sums, want)
                    assert np.all(np.abs(sums - want) <= hw * eps * want)
                    iou = (st + 1e-6) / (tt + ss - st + 1e-6)
                    assert abs(float(iou.mean()) - float(exact)) <= (hw + len(want) + 4) * eps
    assert {hw for _, hw in tc.IOU_SHAPES} == set(tc.IOU_HW) and {b * c for (b, c), _ in tc.IOU_SHAPES} == {1, 6, 255, 256, 257}


def test_iou_gradient_replay_is_the_float64_restatement():
    """The replay of the kernel's lines is the restated gradient up to float64 rounding, and exactly 0 at the saturated logits."""
    case = tc.iou_case((2, 3), 257, True, 77)
    sums = tc.iou_sums(case["s256"], case["tu256"])
    got = tc.iou_grad_replay((case["s256"] / 256.0).astype(F), case["tu256"] / 256.0, sums, 3.0).reshape(case["x"].shape)
    with np.errstate(over="ignore", invalid="ignore"):
        _, _, ref = rs.iou_loss(np.clip(case["x"], -200, 200), case["t_u8"])
    assert np.all(np.abs(got - 3.0 * ref) <= 2.0 ** -22 * np.abs(3.0 * ref).max())
    sat = case["x"] != 0
    assert np.all(got[sat] == 0) and np.all(got[~sat] != 0) and np.isfinite(got).all()


# ---- visibility loss -----------------------------------------------------------------------------------------------------------------------
def _vis_from_arrays(case, crit, mutant=None):
    """The exact sum of the loss's addends from the arrays, the kernel's way: d in fp32, the criterion in float64."""
    pp, tp = case["pp"][..., None], case["tp"][..., None]
    d = (case["pred"] * pp - case["target"] * (F(1) if mutant == "one_side" else tp)).astype(F).reshape(-1).astype(np.float64)
    val, _ = rs._crit(crit, d)
    if mutant == "drop_last":
        val = val[:-1]
    if mutant == "first_twice":
        val = np.concatenate([val, val[:1]])
    return val.sum()


@pytest.mark.parametrize("shape", tc.VIS_SHAPES)
def test_visibility_cases_are_exact_in_any_order_and_catch_the_mutants(shape):
    fn = {"l1": torch.nn.L1Loss, "l2": torch.nn.MSELoss, "smooth_l1": torch.nn.SmoothL1Loss}
    for crit in tc.CRITERIA:
        killed = set()
        for k, pattern in enumerate(tc.VIS_PATTERNS):
            case = tc.vis_case(*shape, pattern, 2000 + k)
            m = case["d1024"].size
            assert np.abs(case["pred"]).max() <= 4 and np.abs(case["target"]).max() <= 4
            if pattern == "ones":
                assert set(tc.VIS_D[:m]) <= set(case["d1024"].tolist())
            addends, total = tc.vis_addends(case["d1024"], crit)
            want = total / 2.0 ** 21
            for got in _orders(addends[None], k):
                assert got[0] == want
            assert _vis_from_arrays(case, crit) == want
            killed |= {mu for mu in ("drop_last", "first_twice", "one_side") if _vis_from_arrays(case, crit, mu) != want}
            loss32, grad32 = tc.vis_expected(case, crit)
            for dtype in (torch.float64, torch.float32):  # landmarks_loss_w_visibility.py:17-26
                x = torch.from_numpy(case["pred"]).to(dtype).requires_grad_(True)
                pp, tp, t = (torch.from_numpy(case[key]).to(dtype) for key in ("pp", "tp", "target"))
                each = fn[crit](reduction="none")(x * pp[..., None], t * tp[..., None])
                assert np.array_equal(each.detach().double().numpy().reshape(-1), addends)  # exact in float32 too
                loss = fn[crit]()(x * pp[..., None], t * tp[..., None])
                loss.backward()
                rel = 2.0 ** -52 if dtype == torch.float64 else m * 2.0 ** -24
                assert abs(float(loss.detach()) - want / m) <= rel * want / m
                g64 = grad32.astype(np.float64)  # two float32 roundings apart at the most
                assert np.abs(x.grad.double().numpy() - g64).max() <= 2.0 ** -23 * np.abs(g64).max()
        assert killed == {"drop_last", "first_twice", "one_side"}, (shape, crit, killed)


# ---- keypoint errors -----------------------------------------------------------------------------------------------------------------------
def _kp_from_arrays(case, cube=False, mutant=None):
    """err [B] float64 from the arrays, by the reference's formula (metrics/keypoints.py:28 after _step_fn's scaling) in float64."""
    p, q = case["pred"].astype(np.float64) * case["scale"], case["target"].astype(np.float64) * case["scale"]
    if case["presence"] is not None:
        pr = case["presence"].astype(np.float64)[..., None]
        p, q = p * pr, (q if mutant == "one_side" else q * pr)
    if case["index"] is not None:
        p, q = p[:, case["index"]], q[:, case["index"]]
    with np.errstate(invalid="ignore", divide="ignore"):
        if cube:
            p, q = rs.normalize_to_cube(p), rs.normalize_to_cube(q)
        lengths = np.sqrt(((p - q) ** 2).sum(-1))
        if mutant == "drop_last":
            lengths = lengths[:, :-1]
        if mutant == "first_twice":
            lengths = np.concatenate([lengths, lengths[:, :1]], 1)
        return lengths, lengths.sum(1) / (case["n_points"] - (mutant == "n_minus_1"))


def _kp_torch(case, dtype, cube=False):
    """The reference's statement on the CPU: _step_fn's scaling, normalize_to_cube, keypoints.py:28-30."""
    from dad_3dheads_amd.losses import normalize_to_cube

    p, q = torch.from_numpy(case["pred"]).to(dtype) * case["scale"], torch.from_numpy(case["target"]).to(dtype) * case["scale"]
    if case["presence"] is not None:
        pr = torch.from_numpy(case["presence"]).to(dtype)[..., None]
        p, q = p * pr, q * pr
    if case["index"] is not None:
        idx = torch.from_numpy(case["index"])
        p, q = p[:, idx], q[:, idx]
    if cube:
        p, q = normalize_to_cube(p), normalize_to_cube(q)
    err = (p - q).norm(2, -1).mean(-1)
    norm = torch.sqrt(torch.from_numpy(case["bbox"])[:, 2] * torch.from_numpy(case["bbox"])[:, 3]).to(dtype) if case["bbox"] is not None else 2.0
    return err, norm


def _check_kp_case(case, cube, seed):
    n, b = case["n_points"], len(case["err"])
    lengths, err = _kp_from_arrays(case, cube)
    assert np.array_equal(err, case["err"], equal_nan=True)
    if np.isnan(case["err"]).all():  # the degenerate cube of one point
        assert cube and n == 1
        return
    assert np.array_equal(lengths, case["lengths"])
    for got in _orders(case["lengths"], seed):
        assert np.array_equal(got / n, case["err"])
    mutants = ["drop_last", "first_twice", "n_minus_1"] + (["one_side"] if case["presence"] is not None else [])
    for mutant in mutants:
        with np.errstate(divide="ignore", invalid="ignore"):
            moved = _kp_from_arrays(case, cube, mutant)[1] != case["err"]
        if mutant == "one_side":  # shows wherever a gathered point is absent: in every item once there are more points than the ends
            idx = slice(None) if case["index"] is None else case["index"]
            absent = (case["presence"][:, idx] == 0).any(1)
            assert np.array_equal(moved, absent) and (absent.all() or n <= 2), (n, b, mutant)
        else:
            assert moved.all(), (n, b, mutant)
    # the reference's statement: float64 to the bit; float32 to the bit too, as the correctly rounded quotient of an exact sum
    e64, norm = _kp_torch(case, torch.float64, cube)
    assert np.array_equal(e64.numpy(), case["err"])
    e32, norm32 = _kp_torch(case, torch.float32, cube)
    total = case["lengths"].sum(1)
    assert np.array_equal(total.astype(F), total) and np.array_equal(e32.numpy(), total.astype(F) / F(n))
    thresholds = case.get("thresholds", (0.05, 0.1))
    for below in (True, False):
        nme, rates = tc.kp_finish(case["err"], case["norm"], thresholds, below)
        for k, thr in enumerate(thresholds):  # keypoints.py:47-52
            hit = (e64 < thr * norm) if below else (e64 > thr * norm)
            assert F(hit.sum() / b) == rates[k]
            hit = (e32 < thr * norm32) if below else (e32 > thr * norm32)
            assert F(hit.sum() / b) == rates[k]
    nme, rates = tc.kp_finish(case["err"], case["norm"], thresholds)
    assert abs(float(torch.mean(e64 / norm)) - float(nme)) <= tc.mean_bar(b, 0.0)
    return rates


@pytest.mark.parametrize("n", tc.KP_POINTS)
def test_keypoint_cases_are_exact_in_any_order_and_catch_the_mutants(n):
    seen = []
    for b in tc.KP_BATCHES:
        for k, (dims, indexed, presence) in enumerate((d, i, p) for d in (2, 3) for i in (False, True) for p in (False, True)):
            case = tc.kp_case(b, n, dims, indexed, presence, 3000 + 10 * b + k)
            assert case["pred"].shape == (b, n + 7 * indexed, dims)
            if indexed:
                assert (case["index"] < 0).any() and len(set((case["index"] % (n + 7)).tolist())) < n or n == 1
            rates = _check_kp_case(case, False, k)
            if b == 257:
                seen.append(rates)
        for k, (indexed, presence) in enumerate((i, p) for i in (False, True) for p in (False, True)):
            _check_kp_case(tc.kp_cube_case(b, n, indexed, presence, 4000 + 10 * b + k), True, k)
    assert all(0 < r[0] < r[1] < 1 for r in seen)  # a large batch lies on both sides of both thresholds


@pytest.mark.parametrize("kind", ["bbox", "plain"])
def test_the_ties_tell_less_from_less_or_equal(kind):
    case = tc.kp_tie_case(kind)
    _check_kp_case(case, False, 0)
    for k, thr in enumerate(case["thresholds"]):
        lim = thr * case["norm"]
        mine = case["limit"] == lim[0]
        below = np.count_nonzero(case["err"] < lim)
        assert below == np.count_nonzero((case["side"] < 0) & mine) + np.count_nonzero(case["limit"] < lim[0])
        assert np.count_nonzero(case["err"] <= lim) == below + 1  # the mutant `<=` counts the tie
        assert np.count_nonzero(case["err"] >= lim) == np.count_nonzero(case["err"] > lim) + 1
        assert below + np.count_nonzero(case["err"] > lim) == len(lim) - 1  # the tie counts under neither


def test_mean_bar_is_the_derived_bound():
    """Half a float32 spacing at the output plus (n^2 + n + 4) 2^-53: the bound of the docstring, not a chosen number."""
    assert tc.mean_bar(6, F(0.75)) == 2.0 ** -25 + 46 * 2.0 ** -53
    assert tc.mean_bar(257, F(0.03)) == 0.5 * float(np.spacing(F(0.03))) + (257 * 257 + 257 + 4) * 2.0 ** -53
    assert tc.exact_ratio_mean(np.array([1.0, 1.0]), np.array([3.0, 6.0])) == Fraction(1, 4)


def test_encode_cases_leave_every_chunk_remainder():
    for size, batches in tc.ENCODE_BATCHES.items():
        totals = [b * c * size * size for b, c in batches]
        assert size * size % 16 and size * size % 4  # the crossing branch, in both element sizes
        assert {t % 4 for t in totals} == {0, 1, 2, 3} and len({t % 16 for t in totals}) == len(totals)  # float and uint8 tails
    for size in (3, 5):
        kp, pr, bad = tc.encode_invalid_case(size, tc.ENCODE_STRIDE[size])
        flat = kp.reshape(-1, 2)
        assert all(not np.isfinite(flat[ch]).all() and pr.reshape(-1)[ch] for ch in bad)
        assert np.count_nonzero(~np.isfinite(flat).all(1)) == len(bad) + 3 and np.count_nonzero(~pr) == 3
        with pytest.raises(ValueError):
            rs.encode(kp, pr, size, tc.ENCODE_STRIDE[size], tc.ENCODE_RADIUS[size], "uint8")
