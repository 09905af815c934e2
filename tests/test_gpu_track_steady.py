"""GPU: steady tracks -- csrc/track_steady.hip (`dad3d_one_euro_rows`, `dad3d_track_suppress_duplicates`), `steady.OneEuroFilter`,
`FaceMeshPredictor.next_boxes(merge_iou=)` and `HeadTracker(steady=, merge_iou=)`.

Both kernels are held bit for bit to the host statements of their rules (`steady.one_euro_rows`, `boxes.suppress_duplicates`, pinned
by hand in test_track_steady_host.py). The loop is held to the same loop with the filter run in numpy on the host and the
duplicates taken by `boxes.suppress_duplicates`."""
import itertools

import numpy as np
import pytest
import torch

from dad_3dheads_amd import _lib, boxes, steady
from guarded import SENTINEL_F, Guarded

pytestmark = pytest.mark.gpu

P, DUP, EMPTY = _lib.TRACK_FLAG_PREVIOUS, _lib.TRACK_FLAG_DUPLICATE, _lib.BOX_FLAG_EMPTY
F, NAN, INF = np.float32, float("nan"), float("inf")
CAP = _lib.TRACK_MAX_SLOTS


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. the filter kernel ------------------------------------------------------------------------------------------------------
def _walk(n, d, steps, seed):
    """`steps` samples of a random walk `[n,d]` with what the rule branches on: subnormal elements that stay subnormal, a NaN at the
    first, the last and a middle position of a row and an infinity (step 2), an element that jumps to 3e38 and back to -3e38 (rule 5,
    steps 3 and 4), and flagged rows (steps 2 and 4; at step 4 row 0 is flagged, which for n == 1 is the overflowing row too)."""
    rng = np.random.default_rng(seed)
    i, c = np.meshgrid(np.arange(n), np.arange(d), indexing="ij")
    tiny = (i + c) % 7 == 3
    x = np.where(tiny, rng.integers(-9, 10, (n, d)) * 1e-40, rng.normal(0.0, 50.0, (n, d))).astype(F)
    xs, flags = [], []
    for t in range(steps):
        x = (x + np.where(tiny, rng.integers(-9, 10, (n, d)) * 1e-41, rng.normal(0.0, 2.0, (n, d))).astype(F)).astype(F)
        s, f = x.copy(), np.zeros(n, np.int32)
        if t == 2:
            s[0, 0], s[1 % n, d - 1], s[2 % n, d // 2], s[5 % n, d // 3] = NAN, NAN, NAN, -INF
            f[1::4] = EMPTY
        if t >= 3:
            s[n - 1, d // 4] = 3e38 if t == 3 else -3e38
        if t == 4:
            f[0::5] = -3
        xs.append(s)
        flags.append(f)
    return xs, flags


def _filter_steps(n, d, form, seed, steps=5):
    """The kernel over `steps` samples against the numpy rule, every buffer between guard words. `form`: "contiguous", "strided" (x
    and out with different row strides, sentinels in between) or "in-place" (out is x, strided)."""
    lib = _lib.load()
    rng = np.random.default_rng(seed + 1)
    mc, be = rng.uniform(0.05, 3.0, d).astype(F), rng.choice(np.array([0.0, 0.007, 0.5], F), d)
    xs, flags = _walk(n, d, steps, seed)
    x_stride = d if form == "contiguous" else d + 5
    out_stride = d if form == "contiguous" else x_stride if form == "in-place" else d + 3
    sx, sdx, age = np.zeros((n, d), F), np.zeros((n, d), F), np.zeros(n, np.int32)
    g_x, g_out = Guarded(n * x_stride, torch.float32), Guarded(n * out_stride, torch.float32)
    g_sx, g_sdx, g_age = Guarded(n * d, torch.float32), Guarded(n * d, torch.float32), Guarded(n, torch.int32)
    for g in (g_sx, g_sdx, g_age):
        g.body.zero_()
    d_mc, d_be = torch.from_numpy(mc).cuda(), torch.from_numpy(be).cuda()
    ages = []
    for t, (x, f) in enumerate(zip(xs, flags)):
        scalars = steady.one_euro_scalars(1 / 30 if t != 3 else 1 / 24, 1.0)  # dt may change from call to call
        use_flags = t != 1
        want = steady.one_euro_rows(x, sx, sdx, age, mc, be, scalars, f if use_flags else None)
        g_x.body.view(n, x_stride)[:, :d] = torch.from_numpy(x).cuda()
        g_out.body.fill_(float(SENTINEL_F))
        d_flags = torch.from_numpy(f).cuda()
        dst = g_x if form == "in-place" else g_out
        status = lib.dad3d_one_euro_rows(g_x.ptr(), x_stride, dst.ptr(), out_stride, n, d, d_flags.data_ptr() if use_flags else None,
                                         d_mc.data_ptr(), d_be.data_ptr(), *(float(s) for s in scalars), g_sx.ptr(), g_sdx.ptr(), g_age.ptr(), 0, None)
        torch.cuda.synchronize()
        assert status == _lib.OK, lib.dad3d_last_error()
        rows = dst.host().reshape(n, out_stride)
        assert np.array_equal(_bits(rows[:, :d]), _bits(want)), (t, np.argwhere(_bits(rows[:, :d]) != _bits(want))[:4])
        assert (rows[:, d:] == SENTINEL_F).all(), "a word between two rows was written"
        if form != "in-place":
            got_x = g_x.host().reshape(n, x_stride)
            assert np.array_equal(_bits(got_x[:, :d]), _bits(x)) and (got_x[:, d:] == SENTINEL_F).all(), "the input was written"
        assert np.array_equal(_bits(g_sx.host().reshape(n, d)), _bits(sx)), t
        assert np.array_equal(_bits(g_sdx.host().reshape(n, d)), _bits(sdx)), t
        assert g_age.host().tolist() == age.tolist(), t
        assert np.isfinite(sx).all() and np.isfinite(sdx).all()
        ages.append(age.copy())
    return np.stack(ages), sdx


@pytest.mark.parametrize("d", [1, 63, 64, 65, 413, 1000])
def test_filter_kernel_equals_the_numpy_rule_bit_for_bit(d):
    for n, form in itertools.product((1, 3, 70), ("contiguous", "strided", "in-place")):
        ages, sdx = _filter_steps(n, d, form, seed=d + n)
        assert ages[2, 0] == 0 and ages[4, 0] == 0  # rule 2; rule 1
        assert n == 1 or (ages[3:, n - 1] == 1).all()  # rule 5: filtered, the row would be 2 samples old (for n == 1 rule 1 comes first)
        if n == 70:
            assert ages.max() == 5 and sdx.any() and (ages[2, 1::4] == 0).all()  # rows that were filtered at every step; flagged rows


def test_filter_argument_contract_writes_no_word():
    lib = _lib.load()
    n, d = 3, 5
    bufs = [Guarded(n * d, torch.float32) for _ in range(6)] + [Guarded(n, torch.int32)]
    x, out, mc, be, sx, sdx, age = bufs

    def call(**kw):
        a = {"x": x.ptr(), "xs": d, "out": out.ptr(), "os": d, "n": n, "d": d, "mc": mc.ptr(), "be": be.ptr(), "rate": 30.0, "tpd": 0.2, "ad": 0.2,
             "sx": sx.ptr(), "sdx": sdx.ptr(), "age": age.ptr()}
        a.update(kw)
        return lib.dad3d_one_euro_rows(a["x"], a["xs"], a["out"], a["os"], a["n"], a["d"], None, a["mc"], a["be"], a["rate"], a["tpd"], a["ad"],
                                       a["sx"], a["sdx"], a["age"], 0, None)

    for kw in ({"x": None}, {"out": None}, {"mc": None}, {"be": None}, {"sx": None}, {"sdx": None}, {"age": None}, {"d": 0}, {"n": -1},
               {"xs": d - 1}, {"os": d - 1}, {"rate": 0.0}, {"rate": NAN}, {"tpd": -1.0}, {"tpd": INF}, {"ad": 0.0}, {"ad": 1.5}, {"ad": NAN}):
        assert call(**kw) == _lib.E_INVALID, kw
    assert call(n=0) == _lib.OK
    torch.cuda.synchronize()
    for g in bufs:
        assert (g.host() == g.sentinel).all(), "a refused call wrote"


def test_one_euro_filter_object_steps_resets_and_keeps_its_state_on_the_device():
    n, d = 6, 40
    rng = np.random.default_rng(9)
    mc, be = rng.uniform(0.1, 2.0, d).astype(F), np.full(d, 0.3, F)
    filt = steady.OneEuroFilter(n, d, mc, be, d_cutoff=1.5, device="cuda:0")
    sx, sdx, age = np.zeros((n, d), F), np.zeros((n, d), F), np.zeros(n, np.int32)
    x = rng.normal(0, 10, (n, d)).astype(F)
    for t in range(5):
        x = (x + rng.normal(0, 1, (n, d))).astype(F)
        wide = torch.full((n, d + 3), NAN, device="cuda")
        wide[:, :d] = torch.from_numpy(x).cuda()
        flags = np.zeros(n, np.int32)
        flags[4] = t == 2
        if t == 3:
            filt.reset(torch.tensor([1, 77, -1], device="cuda"))  # 77 and -1 name no row
            filt.reset([2])
            age[[1, 2]] = 0
        want = steady.one_euro_rows(x, sx, sdx, age, mc, be, steady.one_euro_scalars(1 / 25, 1.5), flags)
        got = filt.step(wide[:, :d], torch.from_numpy(flags).cuda(), dt=1 / 25)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)) and filt.age.tolist() == age.tolist(), t
        assert np.array_equal(_bits(filt.state_x.cpu().numpy()), _bits(sx)) and np.array_equal(_bits(filt.state_dx.cpu().numpy()), _bits(sdx))
    assert age.tolist() == [5, 2, 2, 5, 2, 5]
    filt.reset()
    assert filt.age.tolist() == [0] * n
    for bad in (torch.zeros((n, d), device="cuda", dtype=torch.float64), torch.zeros((n, d + 1), device="cuda"), torch.zeros((n, d)),
                torch.zeros((d, n), device="cuda").t()):
        with pytest.raises(ValueError):
            filt.step(bad)


def test_one_euro_filter_with_the_default_device_takes_steps():
    """`device="cuda"` names the current device; the tensors the filter is given name it by index."""
    n, d = 3, 7
    filt = steady.OneEuroFilter(n, d, 1.0, 0.25)
    assert filt.device == torch.device("cuda", torch.cuda.current_device()) == filt.state_x.device
    rng = np.random.default_rng(4)
    sx, sdx, age = np.zeros((n, d), F), np.zeros((n, d), F), np.zeros(n, np.int32)
    for t in range(3):
        x = rng.normal(0, 5, (n, d)).astype(F)
        want = steady.one_euro_rows(x, sx, sdx, age, [1.0] * d, [0.25] * d, steady.one_euro_scalars(1 / 30 + t / 1000))
        d_x = torch.from_numpy(x).cuda()
        got = filt.step(d_x, dt=1 / 30 + t / 1000) if t else filt.step(d_x, torch.zeros(n, dtype=torch.int32, device="cuda"), out=d_x)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)) and filt.age.tolist() == age.tolist() == [t + 1] * n
    assert not hasattr(filt, "_scalars")  # a measured dt differs at every step: nothing is kept per dt


# ---- 2. the duplicate kernel ---------------------------------------------------------------------------------------------------
def _clustered(n, seed):
    """Boxes about 40 wide around a few centres per frame, shifted by up to half a box, so that IoUs lie on both sides of 0.5 and
    chains form; some slots flagged, some with a zero or negative side. -> (boxes, flags, image_index)."""
    rng = np.random.default_rng(seed)
    clusters = max(1, n // 6)
    centres = rng.integers(0, 60 * clusters + 1, (clusters, 2))
    which = rng.integers(0, clusters, n)
    size = rng.integers(30, 51, (n, 2))
    xy = centres[which] + rng.integers(-20, 21, (n, 2))
    bx = np.concatenate([xy, size], axis=1).astype(np.int32)
    index = rng.integers(0, 3, n).astype(np.int32)
    flags = np.where(rng.random(n) < 0.1, rng.choice([1, 2, 8, 16], n), 0).astype(np.int32)
    dead = rng.random(n) < 0.1
    bx[dead, 2 + (np.arange(n)[dead] & 1)] = rng.integers(-5, 1, int(dead.sum()))
    if n >= 3:  # and one chain for certain, away from the clusters: A kept, B gone, C kept although it overlaps B
        at = [n // 5, n // 2, n - 2]
        bx[at] = [(5000, 5000, 10, 10), (5003, 5000, 10, 10), (5006, 5000, 10, 10)]
        flags[at], index[at] = 0, 1
    return bx, flags, index


def _has_greedy_chain(bx, flags, index, out_flags, iou):
    """Is there a slot that was kept although it overlaps an earlier slot that was itself suppressed?"""
    b = bx.astype(np.int64)
    part = (flags == 0) & (b[:, 2] > 0) & (b[:, 3] > 0)
    x0, y0, x1, y1 = b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]
    iw = np.maximum(0, np.minimum(x1[:, None], x1[None]) - np.maximum(x0[:, None], x0[None]))
    ih = np.maximum(0, np.minimum(y1[:, None], y1[None]) - np.maximum(y0[:, None], y0[None]))
    inter = iw * ih
    area = b[:, 2] * b[:, 3]
    union = area[:, None] + area[None] - inter
    hit = (inter > 0) & (inter.astype(np.float64) >= iou * union.astype(np.float64)) & (index[:, None] == index[None]) & part[:, None] & part[None]
    gone = out_flags == DUP
    earlier = np.arange(len(b))[:, None] < np.arange(len(b))[None]
    return bool((hit & earlier & gone[:, None] & (part & ~gone)[None]).any())


def _suppress(bx, flags, index, iou, expect=_lib.OK, n=None):
    lib = _lib.load()
    count = len(bx) if n is None else n
    g_b, g_f = Guarded(len(bx) * 4, torch.int32), Guarded(len(bx), torch.int32)
    g_b.body.copy_(torch.from_numpy(bx.reshape(-1)).cuda())
    g_f.body.copy_(torch.from_numpy(flags).cuda())
    d_index = torch.from_numpy(index).cuda()
    status = lib.dad3d_track_suppress_duplicates(g_b.ptr(), g_f.ptr(), d_index.data_ptr(), count, iou, 0, None)
    torch.cuda.synchronize()
    assert status == expect, lib.dad3d_last_error()
    return g_b.host().reshape(-1, 4), g_f.host()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, CAP])
def test_suppress_kernel_equals_the_numpy_rule(n):
    for seed, iou in ((n, 0.5), (n + 1, 0.3), (n + 2, 1.0)):
        bx, flags, index = _clustered(n, seed)
        if iou == 1.0 and n > 1:
            bx[n // 2:] = bx[: n - n // 2]  # exact copies, or nothing is a duplicate at 1.0
        want_b, want_f = boxes.suppress_duplicates(bx, flags, index, iou)
        got_b, got_f = _suppress(bx, flags, index, iou)
        assert got_f.tolist() == want_f.tolist(), np.flatnonzero(got_f != want_f)[:8]
        assert np.array_equal(got_b, want_b)
        if n >= 63:
            assert (want_f == DUP).any() and ((want_f == 0) & (bx[:, 2] > 0) & (bx[:, 3] > 0)).sum() > 1
        if n >= 63 and iou < 1.0:
            assert _has_greedy_chain(bx, flags, index, want_f, iou), "no greedy chain in the input: the case is vacuous"


def test_suppress_by_hand_on_the_device():
    a, b, c = (0, 0, 10, 10), (3, 0, 10, 10), (6, 0, 10, 10)
    bx = np.array([a, b, c, (0, 0, 10, 10), (0, 0, 10, 5), a, (0, 0, 10, 10), (0, 0, 10, 5)], np.int32)
    index = np.array([0, 0, 0, 1, 1, 2, 3, 3], np.int32)
    flags = np.array([0, 0, 0, 0, 0, 0, 8, 0], np.int32)
    got_b, got_f = _suppress(bx, flags, index, 0.5)
    assert got_f.tolist() == [0, DUP, 0, 0, DUP, 0, 8, 0]  # the chain; the boundary IoU of 1/2; another frame; a flagged slot suppresses nobody
    assert got_b.tolist() == [list(a), [0] * 4, list(c), [0, 0, 10, 10], [0] * 4, list(a), [0, 0, 10, 10], [0, 0, 10, 5]]
    big = 2 ** 31 - 1
    wide = np.array([(-5, -5, big, big), (-5, -5, big, big), (-5, -5, big, big - 1), (-(2 ** 31), -(2 ** 31), big, big)], np.int32)
    assert _suppress(wide, np.zeros(4, np.int32), np.zeros(4, np.int32), 1.0)[1].tolist() == [0, DUP, 0, 0]


def test_suppress_argument_contract_writes_no_word():
    bx, flags, index = _clustered(8, 1)
    bx[1] = bx[0]
    flags[:2], index[:2] = 0, 0
    for iou in (0.0, -0.1, 1.0000001, NAN, INF):
        got_b, got_f = _suppress(bx, flags, index, iou, expect=_lib.E_INVALID)
        assert np.array_equal(got_b, bx) and np.array_equal(got_f, flags)
    for n in (-1, CAP + 1):
        got_b, got_f = _suppress(bx, flags, index, 0.5, expect=_lib.E_INVALID, n=n)
        assert np.array_equal(got_b, bx) and np.array_equal(got_f, flags)
    got_b, got_f = _suppress(bx, flags, index, 0.5, n=0)
    assert np.array_equal(got_b, bx) and np.array_equal(got_f, flags)
    lib, p = _lib.load(), torch.zeros(64, dtype=torch.int32, device="cuda").data_ptr()
    for null in range(3):
        a = [None if k == null else p for k in range(3)]
        assert lib.dad3d_track_suppress_duplicates(a[0], a[1], a[2], 1, 0.5, 0, None) == _lib.E_INVALID, null


# ---- 3. the loop ---------------------------------------------------------------------------------------------------------------
class Stub(torch.nn.Module):
    """A small deterministic model whose params depend on its input and on the call: the translation is shifted by the mean of a
    4 x 4 grid of the crop's pixels (summed in a fixed order, element by element, so a row's bits do not depend on the batch it stands
    in) plus an offset that changes from call to call -- the jitter the filter is for -- and the first expression and shape
    coefficients move with the call too; the 68 landmarks follow the crop. The rest is fixed so that a head about fills its crop."""

    def __init__(self):
        super().__init__()
        from dad_3dheads_amd import synthetic
        from dad_3dheads_amd.config import load_default_config
        from dad_3dheads_amd.predictor import find_3dmm_idx

        consts = load_default_config()["constants"]
        self.t0, self.s0, self.e0 = (find_3dmm_idx(k, consts) for k in ("translation", "scale", "expression"))
        base = torch.from_numpy(synthetic.synthetic_params(1, seed=8))[0]
        base[self.t0:self.t0 + 2] = 0.0
        base[self.s0] = 7.0
        self.register_buffer("base", base)
        self.register_buffer("k", torch.linspace(0.5, 2.0, 136))
        self.calls = 0

    def forward(self, x):
        s = x.float()[:, :, 32::64, 32::64]
        acc = s[:, :, 0, 0]
        for i, j in list(itertools.product(range(4), range(4)))[1:]:
            acc = acc + s[:, :, i, j]
        m = acc / 16.0  # [B,3]
        params = self.base[None].repeat(x.shape[0], 1)
        jitter = (0.03, -0.02, 0.025, -0.035, 0.01, 0.0, -0.015, 0.02)[self.calls % 8]
        params[:, self.t0:self.t0 + 2] += 0.02 * torch.tanh(m[:, :2]) + jitter
        params[:, self.e0] += 4.0 * jitter
        params[:, 0] += 10.0 * jitter
        self.calls += 1
        return {"OUTPUT_3DMM_PARAMS": params, "OUTPUT_2D_LANDMARKS": 0.5 + 0.3 * torch.tanh(m[:, :2].repeat(1, 68) * self.k)}


FRAME_SHAPES = [(96, 128), (120, 100)]
START = [np.array([[20, 15, 50, 55], [62, 30, 48, 52]], np.int32), np.array([[25, 30, 50, 60]], np.int32)]  # three slots
TWICE = [np.array([[20, 15, 50, 55], [62, 30, 48, 52], [20, 15, 50, 55]], np.int32), START[1]]  # slot 2 stands on slot 0's head; slot 3 is START's 2
KEYS = ("bbox", "flags", "3dmm_params", "projected_vertices", "points")
ALL_KEYS = KEYS + ("track_flags", "image_index", "3d_vertices")


@pytest.fixture(scope="module")
def pred(flame_model):
    from dad_3dheads_amd.config import load_default_config
    from dad_3dheads_amd.predictor import FaceMeshPredictor

    return FaceMeshPredictor(load_default_config(), cuda_id=0, model=Stub(), flame_model=flame_model)


@pytest.fixture(scope="module")
def frames():
    rng = np.random.default_rng(31)
    return [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda() for h, w in FRAME_SHAPES]


def _config():
    return steady.SteadyConfig(rate=30.0, groups={"translation": (0.8, 0.3)})


def _track(pred, frames, start, steps, **kw):
    from dad_3dheads_amd.tracking import HeadTracker

    pred.model.calls = 0
    tracker = HeadTracker(pred, **kw)
    tracker.start(frames, start)
    return tracker, [tracker.step(frames) for _ in range(steps)]


def _host_loop(pred, frames, start, steps, config, merge_iou):
    """The comparison loop: the params cross the host and are filtered there in numpy, and so do the boxes.
    -> [(batched tensors, next boxes, track flags, ages) of each step]."""
    pred.model.calls = 0
    flat, index = boxes.flatten_boxes(len(frames), start)
    shapes = [tuple(f.shape[:2]) for f in frames]
    n = len(flat)
    mc, be = config.expand()
    sx, sdx, age = np.zeros((n, 413), F), np.zeros((n, 413), F), np.zeros(n, np.int32)
    scalars = steady.one_euro_scalars(config.dt, config.d_cutoff)

    def hook(params, flags):
        out = steady.one_euro_rows(params.cpu().numpy(), sx, sdx, age, mc, be, scalars, flags.cpu().numpy())
        return torch.from_numpy(out).to(params.device)

    out = []
    staged = pred._stage_frames(frames)
    for _ in range(steps):
        d_boxes, d_index = torch.from_numpy(flat.astype(np.int32)).cuda(), torch.from_numpy(index).cuda()
        batched = pred._predict_boxes_batched(staged, d_boxes, d_index, boxes.offset_factors(0.1), params_hook=hook)
        flat, track = boxes.next_boxes(batched["projected_vertices"].cpu().numpy(), shapes, index, prev_flags=batched["flags"].cpu().numpy())
        flat, track = boxes.suppress_duplicates(flat, track, index, merge_iou)
        out.append((batched, flat, track, age.copy()))
    return out


def test_tracker_equals_the_loop_filtered_and_merged_on_the_host(pred, frames):
    tracker, steps = _track(pred, frames, TWICE, 4, steady=_config(), merge_iou=0.5)
    want = _host_loop(pred, frames, TWICE, 4, _config(), 0.5)
    for t, (got, (batched, next_flat, track, age)) in enumerate(zip(steps, want)):
        assert len(got) == 4
        for k, g in enumerate(got):
            assert set(g) == set(ALL_KEYS) | {"3dmm_params_raw"} and all(torch.is_tensor(v) and v.is_cuda for v in g.values())
            for key, mine in (("3dmm_params", "3dmm_params"), ("3dmm_params_raw", "3dmm_params_raw"), ("projected_vertices", "projected_vertices"),
                              ("3d_vertices", "3d_vertices"), ("points", "points"), ("bbox", "bbox"), ("flags", "flags")):
                a, b = g[key].reshape(-1), batched[mine][k].reshape(-1)
                assert a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32)), (t, k, key)
            assert int(g["track_flags"]) == track[k], (t, k)
        if t >= 1:  # the filter filters: live rows differ from what the network gave, and the state is the loop's
            t0 = pred.model.t0
            assert float(got[0]["3dmm_params"][0, t0]) != float(got[0]["3dmm_params_raw"][0, t0]) and float(got[0]["3dmm_params"][0, 0]) != float(got[0]["3dmm_params_raw"][0, 0])
    assert [int(r["track_flags"]) for r in steps[0]] == [0, 0, DUP, 0]
    assert tracker.boxes().cpu().numpy().tolist() == want[-1][1].tolist()
    assert tracker.age().tolist() == want[-1][3].tolist() == [4, 4, 0, 4]


def test_two_slots_on_one_head_the_second_goes_and_the_others_do_not_notice(pred, frames):
    kw = {"steady": _config(), "merge_iou": 0.5}
    tracker, steps = _track(pred, frames, TWICE, 4, **kw)
    assert [[int(r["track_flags"]) for r in res] for res in steps] == [[0, 0, DUP, 0]] + [[0, 0, P, 0]] * 3
    assert [[int(r["flags"]) for r in res] for res in steps] == [[0, 0, 0, 0]] + [[0, 0, EMPTY, 0]] * 3
    assert [[int(r["image_index"]) for r in res] for res in steps] == [[0, 0, -1, 1]] * 4  # never drawn
    assert tracker.boxes()[2].tolist() == [0, 0, 0, 0] and tracker.lost().tolist() == [0, 0, P, 0]
    _, alone = _track(pred, frames, START, 4, **kw)
    for t in range(4):
        for k_all, k_alone in ((0, 0), (1, 1), (3, 2)):
            for key in ALL_KEYS + ("3dmm_params_raw",):
                assert torch.equal(steps[t][k_all][key], alone[t][k_alone][key]), (t, k_all, key)
    # without merge_iou both slots live on, on the same head
    _, both = _track(pred, frames, TWICE, 2, steady=_config())
    assert [int(r["track_flags"]) | int(r["flags"]) for r in both[1]] == [0] * 4 and torch.equal(both[1][0]["bbox"], both[1][2]["bbox"])


def test_a_reseeded_slot_restarts_its_filter(pred, frames):
    tracker, steps = _track(pred, frames, TWICE, 3, steady=_config(), merge_iou=0.5)
    tz = pred.model.t0 + 2
    assert tracker.age().tolist() == [3, 3, 0, 3]
    tracker.reseed(torch.tensor([1, 2], device="cuda"), torch.tensor([[62, 30, 48, 52], [20, 15, 50, 55]], device="cuda"))
    assert tracker.age().tolist() == [3, 0, 0, 3] and tracker.lost().tolist() == [0] * 4
    res = tracker.step(frames)
    assert tracker.age().tolist() == [4, 1, 1, 4]
    for k, fresh in enumerate((False, True, True, False)):
        raw, out = res[k]["3dmm_params_raw"].clone(), res[k]["3dmm_params"]
        assert float(out[0, tz]) == 0.0  # tz := 0 from the decode, as without the filter; raw keeps the network's
        raw[0, tz] = 0.0
        assert torch.equal(raw, out) == fresh, k
    assert [int(r["flags"]) for r in res] == [0] * 4 and [int(r["track_flags"]) for r in res] == [0, 0, DUP, 0]  # and slot 2 found slot 0's head again
    tracker.reset()
    assert tracker.age().tolist() == [0] * 4
    assert tracker.step(frames, dt=1 / 15)[0]["3dmm_params"].shape == (1, 413) and tracker.age().tolist() == [1, 1, 0, 1]


def test_with_both_options_off_the_results_are_the_plain_loops(pred, frames):
    """Same keys, same bits as `predict_boxes` with the boxes taken on the host, which is what the tracker was before."""
    _, steps = _track(pred, frames, START, 3, steady=None, merge_iou=None)
    pred.model.calls = 0
    flat, index = boxes.flatten_boxes(len(frames), START)
    host_frames = [f.cpu().numpy() for f in frames]
    for t, got in enumerate(steps):
        res = pred.predict_boxes(host_frames, flat, image_index=index)
        proj = np.concatenate([r["projected_vertices"].numpy() for r in res])
        flat, track = boxes.next_boxes(proj, FRAME_SHAPES, index, prev_flags=[r["flags"] for r in res])
        for k, (g, w) in enumerate(zip(got, res)):
            assert set(g) == set(ALL_KEYS) == set(w) | {"track_flags"}  # no new key
            for key in KEYS + ("3d_vertices",):
                gv, wv = g[key].cpu().numpy(), np.asarray(w[key].numpy() if torch.is_tensor(w[key]) else w[key])
                assert gv.shape == wv.shape and np.array_equal(gv, wv.astype(gv.dtype)) and gv.tobytes() == wv.astype(gv.dtype).tobytes(), (t, k, key)
            assert int(g["track_flags"]) == track[k] == 0 and int(g["image_index"]) == w["image_index"]


def test_step_reseed_and_next_boxes_make_no_host_wait(pred, frames, monkeypatch):
    from dad_3dheads_amd.tracking import HeadTracker

    flat, index = boxes.flatten_boxes(len(frames), TWICE)
    d_boxes, d_index = torch.from_numpy(flat).cuda(), torch.from_numpy(index).cuda()
    slots, fresh = torch.tensor([2], device="cuda"), torch.tensor([[20, 15, 50, 55]], device="cuda")
    _, want = _track(pred, frames, TWICE, 3, steady=_config(), merge_iou=0.5)
    pred.model.calls = 0
    tracker = HeadTracker(pred, steady=_config(), merge_iou=0.5)
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError("a host wait")

    with monkeypatch.context() as m:
        for name in ("cpu", "item", "tolist", "numpy"):
            m.setattr(torch.Tensor, name, refuse)
        m.setattr(torch.cuda, "synchronize", refuse)
        tracker.start(frames, d_boxes, d_index)
        got = [tracker.step(frames) for _ in range(3)]
        age = tracker.age()
        tracker.reseed(slots, fresh)
        tracker.reset()
        pred.model.calls = 0  # the stub's params depend on the call: the host values below come from the same call
        res = pred.predict_boxes(frames, d_boxes, d_index, device_outputs=True, points_on_device=True)
        merged = pred.next_boxes(res, frames, merge_iou=0.5)
        plain = pred.next_boxes(res, frames)
    for g_step, w_step in zip(got, want):
        for g, w in zip(g_step, w_step):
            for key in ALL_KEYS + ("3dmm_params_raw",):
                assert g[key].is_cuda and torch.equal(g[key], w[key]), key
    assert age.is_cuda and tracker.boxes()[2].tolist() == [20, 15, 50, 55]
    # FaceMeshPredictor.next_boxes(merge_iou=): the launch for device values, the numpy rule for host values, the same integers
    pred.model.calls = 0
    host = pred.predict_boxes([f.cpu().numpy() for f in frames], flat, image_index=index)
    want_pair = pred.next_boxes(host, frames, merge_iou=0.5)
    assert isinstance(want_pair[0], np.ndarray) and want_pair[1].tolist() == [0, 0, DUP, 0] and plain[1].tolist() == [0] * 4
    assert np.array_equal(merged[0].cpu().numpy(), want_pair[0]) and np.array_equal(merged[1].cpu().numpy(), want_pair[1])
    with pytest.raises(ValueError, match="merge_iou"):
        pred.next_boxes(res, frames, merge_iou=1.5)
