"""Shared by tests/test_train_objective_cases_host.py and tests/test_gpu_train_objective_edges.py: inputs of the training-objective
kernels (csrc/train_objective.hip) whose sums are exact in float64 IN ANY ORDER, each with its expected values from integer or
rational arithmetic. Pure NumPy. The CPU test certifies the cases (order independence, the reference's torch statements, a table of
mutated restatements that every family must tell from the truth); the GPU test feeds the same arrays to the kernels and compares bits.

Why any order: every input lies on a dyadic grid, so every product and every partial sum is an integer multiple of one power of two
and far below 2^53 of them. A kernel that sums in another order gives the same bits; one that drops, doubles or misplaces an element
moves the result by at least one grid step.

The only rounded quantities are single float64 operations on exact operands (`acc / n`, `acc * (1.0 / m)`, `n / d`, `thr * norm`),
replayed here as the same single NumPy float64 operation, and the means of ratios (`mean_bar`)."""
from fractions import Fraction

import numpy as np

F = np.float32
EPS = 1e-6  # kIouEps

# ---- encode ------------------------------------------------------------------------------------------------------------------------
# (name, img_size, stride, radius): S = 3 (a 16-byte chunk spans up to three uint8 channels; the radius exceeds the map), 5, 9, 25, 25
ENCODE_SIZES = (("s3_r5", 12, 4, 5), ("s5_r2", 15, 3, 2), ("s9_pw", 36, 4, "pointwise"), ("s25_r5", 100, 4, 5), ("s25_r0", 50, 2, 0))
# S -> (B, C): B*C*S*S leaves every remainder of a 16-byte chunk the size allows (S = 5: 25, 75, 150, 375, 11900 elements;
# S = 3: 9, 18, 315, 39168 -- the last a multiple of 16 whose planes are not)
ENCODE_BATCHES = {5: ((1, 1), (1, 3), (2, 3), (3, 5), (7, 68)), 3: ((1, 1), (1, 2), (5, 7), (64, 68))}
ENCODE_RADIUS = {5: 2, 3: 5}
ENCODE_STRIDE = {5: 3, 3: 4}


def encode_batch(size, stride, b, c, seed):
    """Random keypoints around the map (some outside, some absent) for rs.encode."""
    rng = np.random.default_rng(seed)
    kp = rng.uniform(-2 * stride, (size + 2) * stride, (b, c, 2)).astype(F)
    pr = rng.random((b, c)) < 0.85
    pr[0, 0] = True
    kp[0, 0] = (0.5 * stride, 0.5 * stride)  # the first element of the output is a stamp's centre
    pr[-1, -1] = True
    kp[-1, -1] = ((size - 0.5) * stride, (size - 0.5) * stride)  # and so is the last one: the scalar tail writes non-zero bytes
    return kp, pr


def encode_invalid_case(size, stride):
    """B = 2, C = 20 -> 40 flat channels. Present NaN/inf points in channels that start a 16-byte chunk in both element sizes (0, 16),
    in channels that start in the middle of one (1, 3, 7, 21) and in the last channel (39); absent NaN points beside them (2, 17, 38).
    Returns kp, presence, the flat channels that must come out zero and be counted."""
    plane = size * size
    bad = (0, 16, 1, 3, 7, 21, 39)
    absent = (2, 17, 38)
    assert all(plane * ch % 16 == 0 and plane * ch % 4 == 0 for ch in bad[:2])
    assert all(plane * ch % 16 != 0 and plane * ch % 4 != 0 for ch in bad[2:])
    kp = np.full((40, 2), 0.5 * stride * size, dtype=F)
    pr = np.ones(40, dtype=bool)
    for k, ch in enumerate(bad):
        kp[ch, k % 2] = (np.nan, np.inf, -np.inf)[k % 3]
    for ch in absent:
        kp[ch, 0], pr[ch] = np.nan, False
    return kp.reshape(2, 20, 2), pr.reshape(2, 20), bad


# ---- heatmap IoU -----------------------------------------------------------------------------------------------------------------------
IOU_HW = {1: (1, 1), 3: (1, 3), 4: (2, 2), 255: (15, 17), 256: (16, 16), 257: (1, 257), 1020: (30, 34), 1024: (32, 32), 1028: (4, 257),
          4096: (64, 64), 4112: (16, 257)}
IOU_BC = {1: (1, 1), 6: (2, 3), 255: (3, 85), 256: (4, 64), 257: (1, 257)}
IOU_SHAPES = tuple((IOU_BC[6], hw) for hw in IOU_HW) + tuple((IOU_BC[n], 4) for n in (1, 255, 256, 257))  # ((B, C), hw)
LOGITS = np.array([0.0, 200.0, -200.0, np.inf, -np.inf], dtype=F)
LOGIT_S256 = np.array([128, 256, 0, 256, 0], dtype=np.int64)  # 256 * sigmoid of each, if expf(0) = 1, expf(-200) = 0, expf(200) = inf


def iou_case(bc, hw, sigmoid, seed):
    """x [B,C,H,W] float32 (probabilities on the 2^-8 grid, or logits of LOGITS), t_f float32 on the 2^-8 grid, t_u8 in {0, 255}, and
    s256 / tf256 / tu256 int64 [B*C, hw]: 256 x the values the kernel multiplies. First and last element of every channel are non-zero
    in s and in both targets, so that a dropped or doubled end moves all three sums."""
    rng = np.random.default_rng(seed)
    (b, c), (h, w) = bc, IOU_HW[hw]
    n = b * c
    if sigmoid:
        pick = rng.integers(0, len(LOGITS), (n, hw))
        pick[:, 0], pick[:, -1] = 0, 1  # sigmoid 0.5 and 1
        x, s256 = LOGITS[pick], LOGIT_S256[pick]
    else:
        s256 = rng.integers(0, 257, (n, hw))
        s256[:, 0], s256[:, -1] = 1 + rng.integers(0, 256, n), 1 + rng.integers(0, 256, n)
        x = (s256 / 256.0).astype(F)
    tf256 = rng.integers(0, 257, (n, hw)) * (rng.random((n, hw)) < 0.6)
    tu = rng.random((n, hw)) < 0.4
    tf256[:, 0], tf256[:, -1], tu[:, 0], tu[:, -1] = 1 + rng.integers(0, 256, n), 256, True, True
    if n > 1:  # one channel with an all-zero target (IoU = eps / (ss + eps)), one with s = t (IoU = 1)
        tf256[1], tu[1] = 0, False
    if n > 2 and not sigmoid:
        s256[2] = tf256[2]
        x = (s256 / 256.0).astype(F)
    shape = (b, c, h, w)
    return {"x": x.reshape(shape), "t_f": (tf256 / 256.0).astype(F).reshape(shape), "t_u8": (tu * np.uint8(255)).astype(np.uint8).reshape(shape),
            "s256": s256.astype(np.int64), "tf256": tf256.astype(np.int64), "tu256": tu.astype(np.int64) * 256, "channels": n, "hw": hw}


def iou_products(s256, t256):
    """The three addend arrays of a channel set, as exact float64 (multiples of 2^-16)."""
    s, t = s256 / 256.0, t256 / 256.0
    return t * s, t * t, s * s


def iou_sums(s256, t256):
    """[channels, 3] float64 (sum t s, sum t^2, sum s^2) from int64 arithmetic."""
    ints = np.stack([(t256 * s256).sum(1), (t256 * t256).sum(1), (s256 * s256).sum(1)], 1)
    assert ints.max() < 2 ** 53
    return ints / 65536.0  # exact: an integer below 2^53 times a power of two


def iou_channels(sums):
    """(n, d, iou float32) per channel: lines 184-185 of the kernel, one float64 operation each on exact sums."""
    st, tt, ss = sums[:, 0], sums[:, 1], sums[:, 2]
    n, d = st + EPS, tt + ss - st + EPS
    return n, d, (n / d).astype(F)


def exact_ratio_mean(num, den):
    """The mean of num_i / den_i (float64 arrays, read exactly) as a Fraction."""
    return sum(Fraction(float(a)) / Fraction(float(b)) for a, b in zip(num, den)) / len(num)


def mean_bar(count, got32, scale=1.0):
    """How far a float32 output may lie from the exact mean of `count` ratios in [0, scale]: the float64 work (count divisions, count
    additions of partial sums up to count * scale, the division or product by the count, `1.0 - mean`) errs by at most
    (count^2 + count + 4) * scale * 2^-53, and the cast to float32 by half the spacing of float32 at the output."""
    return 0.5 * float(np.spacing(F(abs(float(got32))))) + (count * count + count + 4) * max(scale, 1.0) * 2.0 ** -53


def iou_grad_replay(x_s, t, sums, g):
    """Lines 216-219 and 206-209 in float64, in the order written (no FMA: the unit is built with -ffp-contract=off).
    x_s [channels, hw]: the float32 sigmoids; t [channels, hw] float32 targets; g: the upstream gradient (float32)."""
    n, d, _ = iou_channels(sums)
    k = -np.float64(F(g)) / (np.float64(len(sums)) * d * d)
    ca, cb = (k * (d + n))[:, None], (-2.0 * k * n)[:, None]
    sd, td = x_s.astype(np.float64), t.astype(np.float64)
    return ((ca * td + cb * sd) * (sd * (1.0 - sd))).astype(F)


# ---- landmark loss with visibility -------------------------------------------------------------------------------------------------
VIS_SHAPES = ((1, 1), (1, 511), (1, 512), (1, 513), (16, 64), (3, 683), (64, 68))  # 2 B N = 2, 1022, 1024, 1026, 2048, 4098, 8704
VIS_PATTERNS = ("ones", "zeros", "alternating", "different")
VIS_D = (1024, -1024, 0, 1025, 1023, -1025, -1023)  # d = +1, -1 (the smooth-L1 joint), 0 and the grid neighbours of +-1, in 2^-10
CRITERIA = ("l1", "l2", "smooth_l1")


def vis_case(b, n, pattern, seed):
    """pred, target [B,N,2] float32 on the 2^-10 grid in [-4, 4]; pp, tp [B,N] float32 in {0, 1}; d1024 int64 [B*N*2]: 1024 d.
    The special differences VIS_D open the array and, reversed, close it, wherever both presences are 1."""
    rng = np.random.default_rng(seed)
    m = b * n * 2
    t = 32 * rng.integers(-64, 65, m)  # multiples of 2^-5: d^2 of an ordinary element is exact in float32 too
    p = np.clip(t + 32 * rng.integers(-93, 94, m), -4096, 4096)
    t[t == 0] = 224  # a value of 0 would hide `presence on one side only`
    p[p == 0] = -288
    k = min(len(VIS_D), m)
    p[:k] = t[:k] + np.array(VIS_D[:k])
    if m >= 2 * len(VIS_D):
        p[-k:] = t[-k:] + np.array(VIS_D[::-1])
    pp = {"ones": np.ones(b * n), "zeros": np.zeros(b * n), "alternating": np.arange(b * n) % 2 == 0,
          "different": rng.random(b * n) < 0.7}[pattern].astype(np.int64)
    tp = (rng.random(b * n) < 0.7).astype(np.int64) if pattern == "different" else pp.copy()
    d = p * np.repeat(pp, 2) - t * np.repeat(tp, 2)
    return {"pred": (p / 1024.0).astype(F).reshape(b, n, 2), "target": (t / 1024.0).astype(F).reshape(b, n, 2),
            "pp": pp.astype(F).reshape(b, n), "tp": tp.astype(F).reshape(b, n), "d1024": d}


def vis_addends(d1024, crit):
    """The addends of the loss as exact float64, and their exact sum as an int in units of 2^-21."""
    ad = np.abs(d1024)
    if crit == "l1":
        units = ad * 2 ** 11
    elif crit == "l2":
        units = d1024 * d1024 * 2
    else:
        units = np.where(ad < 1024, d1024 * d1024, (2 * ad - 1024) * 2 ** 10)
    assert int(units.sum()) < 2 ** 53
    return units / 2.0 ** 21, int(units.sum())


def vis_expected(case, crit, g=1.0):
    """(loss float32, grad float32 [B,N,2]): `(float)(acc * (1.0 / m))` and `(float)(slope * inv * pp)`, times the upstream g in fp32."""
    pp = np.repeat(case["pp"].reshape(-1), 2)
    # d as the kernel forms it in fp32, so that an absent point's -0.0 keeps its sign through the slope
    d = (case["pred"].reshape(-1) * pp - case["target"].reshape(-1) * np.repeat(case["tp"].reshape(-1), 2)).astype(np.float64)
    assert np.array_equal(d, case["d1024"] / 1024.0)
    _, total = vis_addends(case["d1024"], crit)
    inv = 1.0 / np.float64(d.size)
    slope = {"l1": np.where(d > 0, 1.0, np.where(d < 0, -1.0, 0.0)), "l2": 2.0 * d,
             "smooth_l1": np.where(d < -1.0, -1.0, np.where(d > 1.0, 1.0, d))}[crit]
    grad = (slope * inv * pp.astype(np.float64)).astype(F)
    return F((total / 2.0 ** 21) * inv), (grad * F(g)).reshape(case["pred"].shape)


# ---- keypoint errors -------------------------------------------------------------------------------------------------------------------
KP_POINTS = (1, 63, 64, 65, 255, 256, 257, 300)
KP_BATCHES = (1, 2, 257)
PAIRS = ((3, 4, 5), (5, 12, 13), (8, 15, 17))  # (dx, dy, |d|)
TRIPLES = ((1, 2, 2, 3), (2, 3, 6, 7), (4, 4, 7, 9))
THRESHOLDS_8 = (0.05, 0.1, 0.02, 0.04, 0.08, 0.16, 0.0, 1.0)


def _diffs(rng, dims, shape):
    """Integer differences [*shape, dims] with integer lengths [*shape]: Pythagorean tuples, permuted, signed, times 1, 2 or 4."""
    table = np.array(PAIRS if dims == 2 else TRIPLES)
    pick = table[rng.integers(0, len(table), shape)]
    comp, length = pick[..., :dims], pick[..., dims]
    comp = np.take_along_axis(comp, np.argsort(rng.random(comp.shape), -1), -1) * rng.choice([-1, 1], comp.shape)
    mult = 2 ** rng.integers(0, 3, shape)
    return comp * mult[..., None], length * mult


def kp_index(n, v, seed):
    """[n] int64 into V = n + 7 with duplicates and negative entries (python-style)."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, v, n)
    idx[::3] -= v
    if n > 1:
        idx[-1] = idx[0] + (v if idx[0] < 0 else 0)  # a duplicate, once negative and once not
    return idx


def kp_case(b, n, dims, indexed, with_presence, seed):
    """The plain path. pred, target [B,V,dims] float32 for pred_scale = target_scale = 256; presence [B,V] in {0, 1} or None;
    bbox [B,4] int64 with w = h (dims 2) or None (dims 3: the norm is 2); index or None; err, norm float64 [B] expected to the bit.
    After the scale the targets are integers in [1, 256) (never 0: `presence on one side only` shows) and the differences are Pythagorean
    integers times the item's power of two (2^-3 .. 1 in dims 2, 2^-8 .. 2^-5 in dims 3: the ratios lie on both sides of 0.05 and 0.1),
    so every point's error is exact and so is their sum. With presence the first and last gathered point are present and, from three
    points on, one in the middle is absent."""
    rng = np.random.default_rng(seed)
    v = n + 7 if indexed else n
    unit = 2.0 ** (rng.integers(-3, 1, b) if dims == 2 else rng.integers(-8, -4, b))  # ratios on both sides of 0.05 and 0.1
    q = rng.integers(1, 256, (b, v, dims)).astype(np.float64)
    diff, length = _diffs(rng, dims, (b, v))
    p = q + diff * unit[:, None, None]
    pres = (rng.random((b, v)) < 0.8).astype(np.int64) if with_presence else np.ones((b, v), np.int64)
    idx = kp_index(n, v, seed + 1) if indexed else np.arange(n)
    if with_presence:
        pres[:, idx[0]], pres[:, idx[-1]] = 1, 1  # the ends count
        if n > 2:
            pres[:, idx[n // 2]] = 0
            pres[:, idx[0]], pres[:, idx[-1]] = 1, 1
    total = (length * pres)[:, idx].sum(1)  # integers
    err = np.array([float(Fraction(int(s), n) * Fraction(float(u))) for s, u in zip(total, unit)])
    if dims == 2:
        side = rng.choice([64, 100, 128, 200], b)
        bbox = np.stack([rng.integers(0, 50, b), rng.integers(0, 50, b), side, side], 1).astype(np.int64)
        norm = side.astype(np.float64)
    else:
        bbox, norm = None, np.full(b, 2.0)
    return {"pred": (p / 256.0).astype(F), "target": (q / 256.0).astype(F), "presence": pres.astype(F) if with_presence else None,
            "bbox": bbox, "index": idx if indexed else None, "err": err, "norm": norm, "n_points": n,
            "lengths": (length * pres)[:, idx] * unit[:, None], "scale": 256.0}


def kp_cube_case(b, n, indexed, with_presence, seed):
    """The cube path (dims 3, scales 1). Item i has the extent E = 2^e_i in x, E/2 in y and 3E/8 in z. Its target points lie on the grid
    E/256 inside the box, two of the gathered points are the box's corners (difference 0), and the prediction is
    alpha (target + difference) + shift with alpha a power of two: both sets then have power-of-two scales (E/2 and alpha E/2, so a
    kernel that mixes them up is caught), the normalised difference is the integer one / 128, and every error is exact. With presence the
    shift is 0 and the box holds the origin, so an absent point (0 on both sides) stays inside and normalises to the same place.
    n = 1 is the degenerate set: 0 / 0, NaN as in the reference."""
    rng = np.random.default_rng(seed)
    v = n + 7 if indexed else n
    idx = kp_index(n, v, seed + 1) if indexed else np.arange(n)
    e = 2.0 ** rng.integers(-1, 3, b)
    alpha = 2.0 ** rng.integers(-1, 2, b)
    shift = np.zeros((b, 1, 3)) if with_presence else rng.integers(-8, 9, (b, 1, 3)) / 2.0
    lo, hi = np.array([-64, -32, -32]), np.array([192, 96, 64])
    q = rng.integers(lo + 32, hi - 31, (b, v, 3))
    diff, length = _diffs(rng, 3, (b, v))  # at most 28 units: inside the margin of 32
    pres = (rng.random((b, v)) < 0.8).astype(np.int64) if with_presence else np.ones((b, v), np.int64)
    if n > 1:  # the corners: two gathered vertices, not the first or last gathered one (those carry a length, for the mutants)
        distinct = list(dict.fromkeys(int(i) % v for i in idx))
        inner = [i for i in distinct if i not in (int(idx[0]) % v, int(idx[-1]) % v)]
        first, last = (inner[0], inner[len(inner) // 2]) if len(inner) >= 2 else (distinct[0], distinct[-1])
        assert first != last
        q[:, first], q[:, last] = lo, hi
        diff[:, first], diff[:, last], length[:, first], length[:, last] = 0, 0, 0, 0
        if with_presence and len(inner) >= 3:
            pres[:, inner[-1]] = 0
        pres[:, [first, last, int(idx[0]) % v, int(idx[-1]) % v]] = 1
    out_of_set = np.ones(v, bool)
    out_of_set[idx % v] = False
    u = (e / 256.0)[:, None, None]
    qf, pf = q * u, alpha[:, None, None] * ((q + diff) * u) + shift
    qf[:, out_of_set], pf[:, out_of_set] = 1000.0, -1000.0  # vertices outside the subset must not reach the min / max
    total = (length * pres)[:, idx].sum(1)
    err = np.array([float(Fraction(int(s), n * 128)) for s in total]) if n > 1 else np.full(b, np.nan)
    assert np.array_equal(qf.astype(F), qf) and np.array_equal(pf.astype(F), pf)
    return {"pred": pf.astype(F), "target": qf.astype(F), "presence": pres.astype(F) if with_presence else None, "bbox": None,
            "index": idx if indexed else None, "err": err, "norm": np.full(b, 2.0), "n_points": n,
            "lengths": (length * pres)[:, idx] / 128.0, "scale": 1.0}


def kp_finish(err, norm, thresholds, below=True):
    """(exact NME as a Fraction or NaN, rates float32 [T]): the finish kernel's `thr * norm` in float64 and `(float)(cnt * (1.0 / B))`."""
    with np.errstate(invalid="ignore"):
        lim = [np.float64(t) * norm for t in thresholds]
        cnt = [np.count_nonzero(err < l_ if below else err > l_) for l_ in lim]
    inv = 1.0 / np.float64(len(err))
    nme = exact_ratio_mean(err, norm) if np.all(np.isfinite(err)) else float("nan")
    return nme, np.array([F(np.float64(c) * inv) for c in cnt], dtype=F)


def kp_tie_case(kind):
    """Items whose mean error sits exactly on `thr * norm`, and on its float32 neighbours below and above.
    "bbox": dims 2, scales 256, w = h = 100, thresholds (0.05, 0.1) -> ties at 5.0 and 10.0. "plain": dims 3, scales 1, no bbox (norm 2),
    threshold 0.25 -> the tie at 0.5. Four points per item; the last one's difference runs along one axis from a target of 0, and
    carries four times the offset. Returns the case and `side` [B]: -1 below, 0 on, +1 above its threshold's limit."""
    items, side, lims = [], [], []
    if kind == "bbox":
        for lim, base in ((5.0, [(3, 4), (0, 5), (5, 0)]), (10.0, [(6, 8), (0, 10), (10, 0)])):
            lim32 = F(lim)
            for s, val in ((-1, np.nextafter(lim32, F(0))), (0, lim32), (1, np.nextafter(lim32, F(100)))):
                last = 4.0 * np.float64(val) - 3.0 * lim  # exact: a few bits around 5 or 10
                items.append(base + [(0.0, last)])
                side.append(s), lims.append(lim)
        diff = np.array(items, np.float64)  # [6,4,2], after the scale of 256
        q = np.tile(np.array([[17.0, 200.0], [255.0, 1.0], [64.0, 64.0], [0.0, 0.0]]), (len(items), 1, 1))
        p = q + diff
        pred, target, scale = p / 256.0, q / 256.0, 256.0
        bbox = np.tile(np.array([[3, 9, 100, 100]], np.int64), (len(items), 1))
        norm, thresholds = np.full(len(items), 100.0), (0.05, 0.1)
    else:
        for s, val in ((-1, np.nextafter(F(0.5), F(0))), (0, F(0.5)), (1, np.nextafter(F(0.5), F(1)))):
            last = 4.0 * np.float64(val) - 1.5
            items.append([(0.125, 0.25, 0.25), (-0.5, 0.25, 0.5), (0.0, 0.0, -0.375), (0.0, last, 0.0)])  # 3/8 + 3/4 + 3/8 + 1/2
            side.append(s), lims.append(0.5)
        diff = np.array(items, np.float64)
        q = np.tile(np.array([[0.25, 0.5, 0.75], [0.5, 0.125, 0.25], [0.375, 0.375, 0.5], [0.0, 0.0, 0.0]]), (len(items), 1, 1))
        pred, target, scale, bbox = q + diff, q, 1.0, None
        norm, thresholds = np.full(len(items), 2.0), (0.25,)
    assert np.array_equal(pred.astype(F), pred) and np.array_equal((pred.astype(F).astype(np.float64) * scale), pred * scale)
    lengths = np.sqrt((diff ** 2).sum(-1))
    err = lengths.sum(1) / 4.0
    expect = np.array([np.float64(F(l_)) if s == 0 else np.float64(np.nextafter(F(l_), F(0) if s < 0 else F(100))) for l_, s in zip(lims, side)])
    assert np.array_equal(err, expect), (err, expect)
    return {"pred": pred.astype(F), "target": target.astype(F), "presence": None, "bbox": bbox, "index": None, "err": err, "norm": norm,
            "n_points": 4, "lengths": lengths, "scale": scale, "thresholds": thresholds, "side": np.array(side), "limit": np.array(lims)}
