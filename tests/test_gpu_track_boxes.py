"""GPU: tracking heads from frame to frame -- csrc/track_boxes.hip (`dad3d_boxes_from_heads`), `FaceMeshPredictor.next_boxes` and
`tracking.HeadTracker`.

The kernel is held bit for bit to the host statement of its rule, `boxes.next_boxes` (pinned by hand in test_track_boxes_host.py):
integers, so equal or wrong. The loop is held to the same loop with the boxes taken on the host: `predict_boxes` with host boxes,
numpy `next_boxes` on the copied vertices, host boxes back in."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from dad_3dheads_amd import _lib, boxes

pytestmark = pytest.mark.gpu

P, R, NF, S, O = (_lib.TRACK_FLAG_PREVIOUS, _lib.TRACK_FLAG_RANGE, _lib.TRACK_FLAG_NONFINITE, _lib.TRACK_FLAG_SMALL,
                  _lib.TRACK_FLAG_OUTSIDE)
NAN, INF = float("nan"), float("inf")
THREADS = 256  # the kernel's workgroup (csrc/track_boxes.hip: kTrackThreads)
SHAPES = [(100, 200), (1080, 1920), (1, 1)]  # (h, w)
SENTINEL, GUARD = -7777, 8


def _launch(proj, index, shapes=SHAPES, prev=None, subset=None, min_side=1, min_visible=0.5, pad_floats=0, addresses=None, expect=_lib.OK,
            n_verts=None, vertex_stride=None, n_subset=None):
    """The kernel on `proj` float32 [N,V,C] (C = 2 or 3 is the vertex stride; `pad_floats` of NaN follow every head, so the head stride
    is V*C + pad_floats) -> (boxes [N,4], flags [N]) as numpy. Both outputs lie between guard words in buffers filled with a sentinel:
    every word of theirs must have been written, and no other."""
    lib = _lib.load()
    proj = np.asarray(proj, np.float32)
    n, v, c = proj.shape
    rows = np.full((n, v * c + pad_floats), NAN, np.float32)
    rows[:, :v * c] = proj.reshape(n, -1)
    d_proj = torch.from_numpy(rows).cuda()
    anchor = torch.zeros(4, dtype=torch.uint8, device="cuda")  # no pixel is read: the address only has to be there
    addresses = [anchor.data_ptr()] * len(shapes) if addresses is None else addresses
    table = torch.tensor([[a, h, w, 3 * w] for a, (h, w) in zip(addresses, shapes)], dtype=torch.int64).cuda()
    d_index = torch.tensor(np.asarray(index), dtype=torch.int32).cuda()
    d_prev = None if prev is None else torch.tensor(np.asarray(prev), dtype=torch.int32).cuda()
    d_subset = None if subset is None else torch.tensor(np.asarray(subset), dtype=torch.int32).cuda()
    out_boxes = torch.full((n * 4 + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    out_flags = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    status = lib.dad3d_boxes_from_heads(d_proj.data_ptr(), n, v if n_verts is None else n_verts, rows.shape[1], c if vertex_stride is None else vertex_stride,
                                        None if d_subset is None else d_subset.data_ptr(),
                                        (0 if d_subset is None else len(d_subset)) if n_subset is None else n_subset,
                                        table.data_ptr(), len(shapes), d_index.data_ptr(), None if d_prev is None else d_prev.data_ptr(),
                                        min_side, min_visible, out_boxes.data_ptr() + 4 * GUARD, out_flags.data_ptr() + 4 * GUARD, 0, None)
    torch.cuda.synchronize()
    assert status == expect, (status, lib.dad3d_last_error())
    got_boxes, got_flags = out_boxes.cpu().numpy(), out_flags.cpu().numpy()
    for got in (got_boxes, got_flags):
        assert (got[:GUARD] == SENTINEL).all() and (got[-GUARD:] == SENTINEL).all(), "a guard word was written"
    got_boxes, got_flags = got_boxes[GUARD:-GUARD].reshape(n, 4), got_flags[GUARD:-GUARD]
    if expect == _lib.OK:
        assert not (got_boxes == SENTINEL).any() and not (got_flags == SENTINEL).any(), "an output word was not written"
    else:
        assert (got_boxes == SENTINEL).all() and (got_flags == SENTINEL).all(), "a refused call wrote"
    return got_boxes, got_flags


def _check(proj, index, shapes=SHAPES, prev=None, subset=None, min_side=1, min_visible=0.5, pad_floats=0):
    """Kernel == host rule, bit for bit -> (boxes, flags)."""
    proj = np.asarray(proj, np.float32)
    want_boxes, want_flags = boxes.next_boxes(proj, shapes, index, prev, subset, min_side, min_visible)
    got_boxes, got_flags = _launch(proj, index, shapes, prev, subset, min_side, min_visible, pad_floats)
    assert got_flags.tolist() == want_flags.tolist(), np.flatnonzero(got_flags != want_flags)
    assert np.array_equal(got_boxes, want_boxes), np.flatnonzero((got_boxes != want_boxes).any(1))
    return got_boxes, got_flags


def _heads(n, v, seed, c=2):
    """Random heads around random centres, some inside their frames and some over an edge; frame numbers over all of SHAPES."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-40.0, 240.0, (n, 1, c))
    proj = (centre + rng.uniform(-30.0, 30.0, (n, v, c))).astype(np.float32)
    return proj, rng.integers(0, len(SHAPES), n).astype(np.int32)


# ---- 1. the reduction ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", [1, 63, 64, 65, THREADS - 1, THREADS, THREADS + 1, 5023])
def test_vertex_counts_at_lane_wave_and_workgroup_seams(v):
    seen = set()
    for n in (1, 3, 70):
        proj, index = _heads(n, v, seed=v + n)
        _, flags = _check(proj, index, min_side=0 if v == 1 else 1)
        seen |= set(flags.tolist())
    assert 0 in seen and (v == 1 or O in seen)  # live heads and lost ones


def test_every_position_of_the_reduction_wins_once():
    v = THREADS + 44
    positions = [0, 63, THREADS - 1, THREADS, v - 1]  # first, last of the first wave, last lane, second trip, last element
    rng = np.random.default_rng(1)
    heads, want = [], []
    for pos, which in itertools.product(positions, range(4)):
        xy = rng.uniform(40.0, 60.0, (v, 2)).astype(np.float32)
        xy[pos, which & 1] = 10.5 if which < 2 else 90.5  # xmin, ymin, xmax, ymax in turn
        lo, hi = np.floor(xy.min(0)).astype(int), np.ceil(xy.max(0)).astype(int)
        assert (lo[which & 1] == 10) if which < 2 else (hi[which & 1] == 91)
        heads.append(xy)
        want.append([lo[0], lo[1], hi[0] - lo[0], hi[1] - lo[1]])
    got, flags = _check(np.stack(heads), np.zeros(len(heads), np.int32))
    assert not flags.any() and got.tolist() == np.array(want).tolist()


def test_ties_negatives_exact_integers_and_signed_zero():
    v = 70
    tie = np.tile(np.array([[3.0, 4.0], [9.0, 8.0]], np.float32), (v // 2, 1))  # every value 35 times
    neg = np.tile(np.array([[-0.5, -7.25], [12.0, 13.0]], np.float32), (v // 2, 1))
    zero = np.tile(np.array([[-0.0, 0.0], [0.0, -0.0], [5.0, 5.0], [5.0, 5.0]], np.float32), (v // 2, 1))[:v]
    tiny = np.tile(np.array([[-1e-40, 1e-40], [6.0, 6.0]], np.float32), (v // 2, 1))  # subnormals are numbers: floor -1, ceil of the other 6
    one = np.full((v, 2), 17.0, np.float32)  # all vertices in one point
    got, flags = _check(np.stack([tie, neg, zero, tiny, one]), np.zeros(5, np.int32), min_side=0, min_visible=0.25)
    assert got.tolist() == [[3, 4, 6, 4], [-1, -8, 13, 21], [0, 0, 5, 5], [-1, 0, 7, 6], [17, 17, 0, 0]] and not flags.any()
    assert _check(one[None], [0])[1].tolist() == [S]


# ---- 2. layouts and subsets ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c, pad", [(2, 0), (3, 0), (2, 7), (3, 5)], ids=["nv2", "nv3", "nv2-padded", "nv3-padded"])
def test_layouts(c, pad):
    """[N,V,2], [N,V,3] with a z that must not be read (NaN), and a head stride beyond V * vertex_stride (NaN in between)."""
    proj, index = _heads(9, 300, seed=5, c=c)
    if c == 3:
        proj[:, :, 2] = NAN
    flat, _ = _heads(9, 300, seed=5, c=c)
    want = boxes.next_boxes(np.ascontiguousarray(flat[:, :, :2]), SHAPES, index)
    got = _check(proj, index, pad_floats=pad)
    assert np.array_equal(got[0], want[0]) and got[1].tolist() == want[1].tolist() and NF not in got[1]


@pytest.mark.parametrize("k", [1, 445])
def test_subset_with_duplicates_reads_only_its_vertices(k):
    n, v = 4, 5023
    rng = np.random.default_rng(k)
    picked = rng.choice(v, size=max(1, k - k // 5), replace=False)
    subset = np.concatenate([picked, picked[: k - len(picked)]]).astype(np.int32)  # a fifth of them twice
    rng.shuffle(subset)
    assert len(subset) == k
    proj = np.empty((n, v, 2), np.float32)
    proj[:] = np.array([NAN, 1e30, -1e30, INF], np.float32)[rng.integers(0, 4, (n, v, 2))]  # what must not reach the result
    proj[:, picked] = (rng.uniform(20.0, 80.0, (n, 1, 2)) + rng.uniform(-15.0, 15.0, (n, len(picked), 2))).astype(np.float32)
    got, flags = _check(proj, np.zeros(n, np.int32), subset=subset, min_side=0)
    assert not flags.any() and (np.abs(got) < 200).all()
    assert _check(proj, np.zeros(n, np.int32), min_side=0)[1].tolist() == [NF] * n  # and without the subset they do


@pytest.mark.parametrize("bad", ["n_verts", -1])
def test_subset_index_outside_the_vertices_is_range(bad):
    v = 300
    proj, _ = _heads(3, v, seed=2)
    for at in (0, 150, 299):
        subset = np.arange(v, dtype=np.int32)
        subset[at] = v if bad == "n_verts" else -1
        got, flags = _check(proj, np.zeros(3, np.int32), subset=subset)
        assert flags.tolist() == [R] * 3 and not got.any()


# ---- 3. every flag -------------------------------------------------------------------------------------------------------------
def _inside(n, v, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(40.0, 60.0, (n, 1, 2)) + rng.uniform(-20.0, 20.0, (n, v, 2))).astype(np.float32)


@pytest.mark.parametrize("bad", [NAN, INF, -INF], ids=["nan", "+inf", "-inf"])
def test_nonfinite_in_one_coordinate_anywhere(bad):
    v = 5023
    where = [0, 63, 64, THREADS - 1, THREADS, 2500, v - 2, v - 1]  # v - 1: the last lane's last element
    proj = _inside(2 * len(where) + 1, v, seed=3)
    for k, at in enumerate(where):
        proj[2 * k, at, 0] = bad
        proj[2 * k + 1, at, 1] = bad
    got, flags = _check(proj, np.zeros(len(proj), np.int32))
    assert flags.tolist() == [NF] * (2 * len(where)) + [0] and not got[:-1].any() and got[-1].any()


def test_magnitude_two_to_the_thirty_and_the_float_below():
    below = float(np.nextafter(np.float32(2 ** 30), np.float32(0)))
    proj = _inside(9, 100, seed=4)
    for k, (axis, value) in enumerate([(0, 2.0 ** 30), (0, -(2.0 ** 30)), (1, 2.0 ** 30), (1, -(2.0 ** 30)), (0, 3e38)]):
        proj[k, 99 - k, axis] = value
    for k, (axis, value) in enumerate([(0, below), (0, -below), (1, below), (1, -below)]):
        proj[5 + k, 50 + k, axis] = value
    got, flags = _check(proj, np.zeros(9, np.int32), min_visible=0.0)
    assert flags.tolist() == [R] * 5 + [0] * 4
    assert got[5, 2] > 2 ** 30 - 200 and got[6, 0] == -(2 ** 30 - 64) and got[7, 3] > 2 ** 30 - 200 and got[8, 1] == -(2 ** 30 - 64)
    assert _check(proj, np.zeros(9, np.int32))[1].tolist() == [R] * 5 + [O] * 4


def test_image_index_and_frame_entries_outside_the_range():
    proj = _inside(6, 100, seed=6)
    got, flags = _check(proj, [-1, len(SHAPES), 0, 1, 2 ** 31 - 1, -(2 ** 31)])
    assert flags.tolist() == [R, R, 0, 0, R, R]
    # frame entries that dad3d_preprocess_boxes flags RANGE: a null address, a side of 0, a side of 2^30
    anchor = torch.zeros(4, dtype=torch.uint8, device="cuda")
    shapes = [(100, 200), (100, 200), (0, 200), (100, 0), (2 ** 30, 200), (100, 2 ** 30 - 1)]
    got, flags = _launch(proj, np.arange(6), shapes=shapes, addresses=[anchor.data_ptr(), 0] + [anchor.data_ptr()] * 4, min_visible=0.0)
    assert flags.tolist() == [0, R, R, R, R, 0] and not got[1:5].any() and got[0].any() and got[5].any()
    want = boxes.next_boxes(proj, shapes, np.arange(6), min_visible=0.0)
    assert want[1].tolist() == [0, 0, R, R, R, 0] and np.array_equal(want[0][[0, 5]], got[[0, 5]])


def test_previous_reads_no_vertex():
    proj = _inside(5, 300, seed=7)
    proj[[0, 2, 4]] = NAN
    got, flags = _check(proj, [0, 0, 7, -1, 0], prev=[_lib.BOX_FLAG_EMPTY, 0, -1, 2 ** 30, 0])
    assert flags.tolist() == [P, 0, P, P, NF] and not got[[0, 2, 3, 4]].any() and got[1].any()


def test_small_outside_and_both():
    flat = np.zeros((4, 10, 2), np.float32)
    flat[0] = [(30.0, 5.0), (50.0, 7.0)] * 5      # 20 x 2 inside
    flat[1] = [(-30.0, 5.0), (-10.0, 7.0)] * 5    # 20 x 2 outside
    flat[2] = [(-30.0, 5.0), (-10.0, 47.0)] * 5   # 20 x 42 outside
    flat[3] = [(30.0, 5.0), (50.0, 47.0)] * 5     # 20 x 42 inside
    got, flags = _check(flat, np.zeros(4, np.int32), min_side=3)
    assert flags.tolist() == [S, S | O, O, 0] and got.tolist() == [[0] * 4] * 3 + [[30, 5, 20, 42]]
    assert _check(flat, np.zeros(4, np.int32), min_side=2)[1].tolist() == [0, O, O, 0]
    assert _check(flat, np.zeros(4, np.int32), min_side=43)[1].tolist() == [S, S | O, S | O, S]


def test_frames_of_mixed_sizes_and_the_min_visible_boundary():
    half = np.array([(-10.0, 10.0), (10.0, 30.0)] * 3, np.float32)       # 20 x 20, half of it left of the frame
    pixel = np.array([(0.0, 0.0), (2.0, 1.0)] * 3, np.float32)           # 2 x 1 over the 1 x 1 frame: half visible
    corner = np.array([(1900.0, 1070.0), (1940.0, 1090.0)] * 3, np.float32)  # 40 x 20 over the large frame's corner: a quarter
    proj, index = np.stack([half, half, pixel, pixel, corner, corner]), [0, 1, 2, 1, 1, 0]
    up = float(np.nextafter(0.5, 1))
    assert _check(proj, index, min_visible=0.5)[1].tolist() == [0, 0, 0, 0, O, O]
    assert _check(proj, index, min_visible=up)[1].tolist() == [O, O, O, 0, O, O]
    assert _check(proj, index, min_visible=0.25)[1].tolist() == [0, 0, 0, 0, 0, O]
    assert _check(proj, index, min_visible=float(np.nextafter(0.25, 1)))[1].tolist() == [0, 0, 0, 0, O, O]
    assert _check(proj, index, min_visible=0.0)[1].tolist() == [0] * 6
    assert _check(proj, index, min_visible=1.0)[1].tolist() == [O, O, O, 0, O, O]


def test_argument_contract_leaves_the_outputs_untouched():
    proj = _inside(2, 10, seed=8)
    index = np.zeros(2, np.int32)
    for kw in ({"n_verts": 0}, {"n_verts": 65536}, {"vertex_stride": 1}, {"vertex_stride": 0}, {"min_side": -1}, {"min_visible": -0.5},
               {"min_visible": 1.5}, {"min_visible": NAN}, {"subset": [0, 1], "n_subset": 0}, {"subset": [0, 1], "n_subset": 65536}, {"n_subset": 2},
               {"shapes": []}):
        _launch(proj, index, expect=_lib.E_INVALID, **kw)
    lib, p = _lib.load(), torch.zeros(64, dtype=torch.int32, device="cuda").data_ptr()
    for null in range(5):
        a = [None if k == null else p for k in range(5)]
        assert lib.dad3d_boxes_from_heads(a[0], 1, 1, 2, 2, None, 0, a[1], 1, a[2], None, 1, 0.5, a[3], a[4], 0, None) == _lib.E_INVALID, null
    assert lib.dad3d_boxes_from_heads(None, 0, 1, 2, 2, None, 0, None, 1, None, None, 1, 0.5, None, None, 0, None) == _lib.OK
    assert lib.dad3d_boxes_from_heads(p, 65536, 1, 2, 2, None, 0, p, 1, p, None, 1, 0.5, p, p, 0, None) == _lib.E_INVALID


# ---- 4. the loop ---------------------------------------------------------------------------------------------------------------
class Stub(torch.nn.Module):
    """A small deterministic model whose params depend on its input: the translation is shifted by the mean of a 4 x 4 grid of the
    crop's pixels (summed in a fixed order, element by element, so a row's bits do not depend on the batch it stands in), the 68
    landmarks likewise; the rest is fixed so that a head about fills its crop. `off` = (row, first call): from that call on the
    row's translation is sent eight crop widths to the right, off every frame here."""

    def __init__(self):
        super().__init__()
        from dad_3dheads_amd import synthetic
        from dad_3dheads_amd.config import load_default_config
        from dad_3dheads_amd.predictor import find_3dmm_idx

        consts = load_default_config()["constants"]
        self.t0, self.s0 = find_3dmm_idx("translation", consts), find_3dmm_idx("scale", consts)
        base = torch.from_numpy(synthetic.synthetic_params(1, seed=8))[0]
        base[self.t0:self.t0 + 2] = 0.0
        base[self.s0] = 7.0  # the head spans about 0.85 of the crop's long side: its box, widened by 0.1 a side, is about the crop again
        self.register_buffer("base", base)
        self.register_buffer("k", torch.linspace(0.5, 2.0, 136))
        self.calls, self.off = 0, None

    def forward(self, x):
        s = x.float()[:, :, 32::64, 32::64]
        acc = s[:, :, 0, 0]
        for i, j in list(itertools.product(range(4), range(4)))[1:]:
            acc = acc + s[:, :, i, j]
        m = acc / 16.0  # [B,3]
        params = self.base[None].repeat(x.shape[0], 1)
        params[:, self.t0:self.t0 + 2] += 0.02 * torch.tanh(m[:, :2])
        if self.off is not None and self.calls >= self.off[1]:
            params[self.off[0], self.t0] += 8.0
        self.calls += 1
        return {"OUTPUT_3DMM_PARAMS": params, "OUTPUT_2D_LANDMARKS": 0.5 + 0.3 * torch.tanh(m[:, :2].repeat(1, 68) * self.k)}


FRAME_SHAPES = [(96, 128), (120, 100)]
START = [np.array([[20, 15, 50, 55], [62, 30, 48, 52]], np.int32), np.array([[25, 30, 50, 60]], np.int32)]  # three slots
KEYS = ("bbox", "flags", "3dmm_params", "projected_vertices", "points")


@pytest.fixture(scope="module")
def pred(flame_model):
    from dad_3dheads_amd.config import load_default_config
    from dad_3dheads_amd.predictor import FaceMeshPredictor

    return FaceMeshPredictor(load_default_config(), cuda_id=0, model=Stub(), flame_model=flame_model)


@pytest.fixture(scope="module")
def frames():
    rng = np.random.default_rng(31)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in FRAME_SHAPES]


def _reset(pred, off=None):
    pred.model.calls, pred.model.off = 0, off


def _track(pred, frames, start, steps, off=None, **kw):
    """`steps` steps of a fresh tracker -> (tracker, [results of each step])."""
    from dad_3dheads_amd.tracking import HeadTracker

    _reset(pred, off)
    tracker = HeadTracker(pred, **kw)
    tracker.start(frames, start)
    d_frames = [torch.from_numpy(f).cuda() for f in frames]
    return tracker, [tracker.step(d_frames) for _ in range(steps)]


def _host_loop(pred, frames, start, steps, **kw):
    """The comparison loop: every box crosses the host. -> [(results, track boxes, track flags) of each step]."""
    _reset(pred)
    flat, index = boxes.flatten_boxes(len(frames), start)
    shapes = [f.shape[:2] for f in frames]
    out = []
    for _ in range(steps):
        res = pred.predict_boxes(frames, flat, image_index=index)
        proj = np.concatenate([r["projected_vertices"].numpy() for r in res])
        flat, track = boxes.next_boxes(proj, shapes, index, prev_flags=[r["flags"] for r in res], **kw)
        out.append((res, flat, track))
    return out


def _same(got, want, key):
    g = got[key].cpu().numpy()
    w = want[key].numpy() if torch.is_tensor(want[key]) else np.asarray(want[key])
    return g.shape == w.shape and g.tobytes() == w.astype(g.dtype).tobytes() and np.array_equal(g, w)


@pytest.mark.parametrize("subset", [None, "face"], ids=["all-vertices", "subset"])
def test_tracker_equals_the_loop_with_the_boxes_taken_on_the_host(pred, frames, subset):
    kw = {} if subset is None else {"subset": np.arange(0, 5023, 11, dtype=np.int64), "min_side": 2, "min_visible": 0.4}
    tracker, steps = _track(pred, frames, START, 4, **kw)
    want = _host_loop(pred, frames, START, 4, **kw)
    previous = None
    for t, (got, (res, next_flat, track)) in enumerate(zip(steps, want)):
        assert len(got) == len(res) == 3
        for k, (g, w) in enumerate(zip(got, res)):
            assert set(g) == set(w) | {"track_flags"} and all(torch.is_tensor(v) and v.is_cuda for v in g.values())
            for key in KEYS:
                assert _same(g, w, key), (t, k, key)
            assert int(g["track_flags"]) == track[k] == 0 and int(g["flags"]) == 0, (t, k)  # the scene keeps every head in its frame
            assert int(g["image_index"]) == w["image_index"]
            assert torch.equal(g["3d_vertices"].cpu(), w["3d_vertices"])
        if t == 1:
            assert [g["bbox"].tolist() for g in got] != previous  # the feedback is real: the crops are not the first step's
        previous = [g["bbox"].tolist() for g in got]
    assert tracker._boxes.cpu().numpy().tolist() == want[-1][1].tolist()
    assert tracker.lost().tolist() == [0, 0, 0]


def test_a_lost_slot_stays_lost_until_it_is_reseeded_and_the_others_do_not_notice(pred, frames):
    from dad_3dheads_amd import overlay

    d_frames = [torch.from_numpy(f).cuda() for f in frames]
    tracker, steps = _track(pred, frames, START, 4, off=(1, 2))  # slot 1 leaves its frame at step 2
    flags = [[int(r["flags"]) for r in res] for res in steps]
    track = [[int(r["track_flags"]) for r in res] for res in steps]
    assert track == [[0, 0, 0], [0, 0, 0], [0, O, 0], [0, P, 0]]
    assert flags == [[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, _lib.BOX_FLAG_EMPTY, 0]]
    assert [[int(r["image_index"]) for r in res] for res in steps] == [[0, 0, 1], [0, 0, 1], [0, -1, 1], [0, -1, 1]]
    assert steps[3][1]["bbox"].tolist() == [0, 0, 0, 0] and tracker._boxes[1].tolist() == [0, 0, 0, 0]
    # the other slots, bit for bit, are those of a run that never had slot 1
    _, alone = _track(pred, frames, [START[0][:1], START[1]], 4)
    for t in range(4):
        for k_all, k_alone in ((0, 0), (2, 1)):
            for key in KEYS + ("track_flags", "image_index", "3d_vertices"):
                assert torch.equal(steps[t][k_all][key], alone[t][k_alone][key]), (t, k_all, key)
    # the lost head is not drawn: the frames are those of drawing the live slots alone
    for res in (steps[2], steps[3]):
        drawn = overlay.draw_heads(res, d_frames, head_mesh=pred.head_mesh)
        live = overlay.draw_heads([res[0], res[2]], d_frames, head_mesh=pred.head_mesh)
        for a, b, src in zip(drawn, live, d_frames):
            assert torch.equal(a, b) and not torch.equal(a, src)
    # lost at every later step, until the caller's detector finds it again
    assert [int(r["track_flags"]) for r in tracker.step(d_frames)] == [0, P, 0]
    assert tracker.lost().tolist() == [0, P, 0]
    pred.model.off = None
    tracker.reseed(torch.tensor([1, 99], device="cuda"), torch.tensor([[62, 30, 48, 52], [1, 2, 3, 4]], device="cuda"))  # 99 names no slot
    assert tracker.lost().tolist() == [0, 0, 0] and tracker._boxes[1].tolist() == [62, 30, 48, 52]
    for _ in range(2):
        res = tracker.step(d_frames)
        assert [int(r["flags"]) | int(r["track_flags"]) for r in res] == [0, 0, 0] and [int(r["image_index"]) for r in res] == [0, 0, 1]
    assert tracker._boxes[1, 2:].min() > 20  # a head's box again


def test_step_reseed_and_next_boxes_make_no_host_wait(pred, frames, monkeypatch):
    from dad_3dheads_amd.tracking import HeadTracker

    d_frames = [torch.from_numpy(f).cuda() for f in frames]
    flat, index = boxes.flatten_boxes(len(frames), START)
    d_boxes, d_index = torch.from_numpy(flat).cuda(), torch.from_numpy(index).cuda()
    slots, fresh = torch.tensor([2], device="cuda"), torch.tensor([[25, 30, 50, 60]], device="cuda")
    subset = torch.arange(0, 5023, 7, device="cuda")
    _, want = _track(pred, frames, START, 3)
    _reset(pred)
    tracker = HeadTracker(pred)
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError("a host wait")

    with monkeypatch.context() as m:
        for name in ("cpu", "item", "tolist", "numpy"):
            m.setattr(torch.Tensor, name, refuse)
        m.setattr(torch.cuda, "synchronize", refuse)
        tracker.start(d_frames, d_boxes, d_index)
        got = [tracker.step(d_frames) for _ in range(3)]
        lost = tracker.lost()
        tracker.reseed(slots, fresh)
        res = pred.predict_boxes(d_frames, d_boxes, d_index, device_outputs=True, points_on_device=True)
        from_dicts = pred.next_boxes(res, d_frames)
        from_proj = pred.next_boxes(torch.cat([r["projected_vertices"] for r in res]), FRAME_SHAPES, image_index=d_index, subset=subset,
                                    min_side=2, min_visible=0.3)
    for g_step, w_step in zip(got, want):
        for g, w in zip(g_step, w_step):
            for key in KEYS + ("track_flags", "image_index"):
                assert g[key].is_cuda and torch.equal(g[key], w[key]), key
    assert lost.is_cuda and tracker._boxes[2].tolist() == [25, 30, 50, 60]
    # FaceMeshPredictor.next_boxes: the kernel for device values, the numpy rule for host values, the same integers
    host = pred.predict_boxes(frames, flat, image_index=index)
    for got_pair, kw in ((from_dicts, {}), (from_proj, {"subset": subset.cpu().numpy(), "min_side": 2, "min_visible": 0.3})):
        assert all(t.is_cuda and t.dtype == torch.int32 for t in got_pair)
        want_pair = pred.next_boxes(host, frames, **kw)
        assert isinstance(want_pair[0], np.ndarray) and want_pair[0].any()
        assert np.array_equal(got_pair[0].cpu().numpy(), want_pair[0]) and np.array_equal(got_pair[1].cpu().numpy(), want_pair[1])
