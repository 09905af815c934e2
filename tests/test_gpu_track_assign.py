"""GPU: detections into tracks -- csrc/track_assign.hip (`dad3d_track_assign_detections`), `FaceMeshPredictor.assign_detections`,
`HeadTracker.start(n_slots=)` / `update` / `misses`, `OneEuroFilter.reset(mask=)` and `TextureAccumulator.reset(mask=)`.

The kernel is held word for word to the host statement of its rule (`boxes.assign_detections`, pinned by hand and against an
independent walk in test_track_assign_host.py), every buffer between guard words. The loop is held to the same loop whose state
crosses the host and goes through the statement."""
import numpy as np
import pytest
import torch

from dad_3dheads_amd import _lib, boxes, steady, synthetic
from guarded import Guarded

pytestmark = pytest.mark.gpu

I32 = np.int32
P, RETIRED = _lib.TRACK_FLAG_PREVIOUS, _lib.TRACK_FLAG_RETIRED
PAD, INV, COV, SPAWN, FULL = (_lib.ASSIGN_FLAG_PADDING, _lib.ASSIGN_FLAG_INVALID, _lib.ASSIGN_FLAG_COVERED, _lib.ASSIGN_FLAG_SPAWNED,
                              _lib.ASSIGN_FLAG_FULL)
CAP = _lib.TRACK_MAX_SLOTS
SIZES = [(1, 1), (3, 70), (64, 64), (65, 33), (1, 1024), (1024, 1), (0, 5), (5, 0), (1024, 1024)]


# ---- 1. the kernel against the statement ---------------------------------------------------------------------------------------
def _guarded(values):
    g = Guarded(values.size, torch.int32)
    if values.size:
        g.body.copy_(torch.from_numpy(np.ascontiguousarray(values, I32).reshape(-1)).cuda())
    return g


def _launch(slots, flags, index, misses, dets, det_index, n_frames, iou, count=None, searched=None, refresh=False, max_misses=None,
            expect=_lib.OK):
    """One launch with every buffer between guard words -> the seven arrays in the statement's order. The detections, their frames,
    the count and the mask are checked to be unwritten."""
    lib = _lib.load()
    n, m = len(slots), len(dets)
    g_b, g_f, g_i = _guarded(slots), _guarded(flags), _guarded(index)
    g_m = None if misses is None else _guarded(misses)
    g_db, g_di = _guarded(dets), _guarded(det_index)
    g_c = None if count is None else _guarded(np.array([count], I32))
    g_s = None if searched is None else _guarded(np.asarray(searched, I32))
    g_a, g_df, g_sp = Guarded(m, torch.int32), Guarded(m, torch.int32), Guarded(n, torch.int32)
    ptr = lambda g: None if g is None else g.ptr()  # noqa: E731
    status = lib.dad3d_track_assign_detections(g_b.ptr(), g_f.ptr(), g_i.ptr(), ptr(g_m), n, g_db.ptr(), g_di.ptr(), ptr(g_c), m, ptr(g_s), n_frames,
                                               iou, int(refresh), -1 if max_misses is None else max_misses, g_a.ptr(), g_df.ptr(), g_sp.ptr(), 0, None)
    torch.cuda.synchronize()
    assert status == expect, lib.dad3d_last_error()
    assert np.array_equal(g_db.host().reshape(-1, 4), dets) and np.array_equal(g_di.host(), det_index), "the detections were written"
    assert g_c is None or g_c.host().tolist() == [count]
    assert g_s is None or g_s.host().tolist() == list(searched)
    return (g_b.host().reshape(-1, 4), g_f.host(), g_i.host(), None if g_m is None else g_m.host(), g_a.host(), g_df.host(), g_sp.host())


def _case(n, m, seed, n_frames):
    """The tie-heavy grid of the host test, widened with the number of boxes so that a box meets a handful of others: sides 1 .. 4 on
    integer positions, a few empty or negative sides, flagged slots, frames out of 0 .. n_frames - 1 with some outside."""
    rng = np.random.default_rng(seed)
    span = max(3, int(2 * np.sqrt(max(n, m) / n_frames)))

    def some(k):
        b = np.concatenate([rng.integers(0, span, (k, 2)), rng.integers(1, 5, (k, 2))], axis=1).astype(I32)
        empty = rng.random(k) < 0.06
        b[empty, 2 + (np.arange(k)[empty] & 1)] = rng.integers(-3, 1, int(empty.sum()))
        return b

    def frames(k):
        f = rng.integers(0, n_frames, k)
        out = rng.random(k) < 0.05
        f[out] = rng.choice([-1, n_frames, n_frames + 7, -(2 ** 31)], int(out.sum()))
        return f.astype(I32)

    flags = np.where(rng.random(n) < 0.25, rng.choice([1, 2, 8, 16, 32, 64, -5], n), 0).astype(I32)
    misses = rng.choice([0, 0, 1, 2, 3, 2 ** 30 - 1, 2 ** 30], n).astype(I32)
    return some(n), flags, frames(n), misses, some(m), frames(m)


@pytest.mark.parametrize("n,m", SIZES)
def test_kernel_equals_the_numpy_statement_word_for_word(n, m):
    outcomes, matched, retired = set(), 0, 0
    variants = (  # (frames, match_iou, count, misses, mask, refresh, max_misses)
        (1, 0.02, None, True, False, False, 1), (3, 0.3, "device", True, True, True, 0), (8, 0.1, "negative", True, True, False, 2),
        (2, 0.5, "beyond", False, False, True, None), (1, 1.0, "device", True, False, False, None), (5, 0.05, None, False, True, False, None))
    for k, (n_frames, iou, how, with_misses, with_mask, refresh, max_misses) in enumerate(variants):
        slots, flags, index, misses, dets, det_index = _case(n, m, 1000 * n + m + 17 * k, n_frames)
        if iou == 1.0 and n and m:  # exact copies, or nothing passes at 1.0
            take = min(n, m) // 2 + 1
            dets[:take], det_index[:take] = slots[:take], index[:take]
        count = {None: None, "device": (3 * m) // 4, "negative": -3, "beyond": m + 9}[how]
        searched = (np.arange(n_frames) % 3 != 1).astype(I32) if with_mask else None
        want = boxes.assign_detections(slots, flags, index, misses if with_misses else None, dets, det_index, n_frames, iou, count, searched, refresh,
                                       max_misses)
        got = _launch(slots, flags, index, misses if with_misses else None, dets, det_index, n_frames, iou, count, searched, refresh, max_misses)
        for name, g, w in zip(want._fields, got, want):
            assert (g is None) == (w is None), name
            assert w is None or np.array_equal(g, w), (k, name, np.argwhere(np.asarray(g) != np.asarray(w))[:6].tolist())
        outcomes.update(want.det_flags.tolist())
        matched += int(((want.det_flags == 0) & (want.assign >= 0)).sum())
        retired += int(((want.flags == RETIRED) & (flags != RETIRED)).sum())
    if n >= 64 and m >= 33:  # the cases are not vacuous
        assert outcomes == {0, PAD, INV, COV, SPAWN, FULL}, outcomes
        assert matched > 10 and retired > 0


def test_by_hand_on_the_device():
    """The hand cases of the host test that the kernel could get wrong on its own: the exact comparison where the double quotients are
    equal, the int32 extremes, ties, a retired slot not reused, and the two empty extents."""
    side, big, low = 2 ** 30, 2 ** 31 - 1, -(2 ** 31)
    z, one = np.zeros(1, I32), np.ones(1, I32)
    slot = np.array([[0, 0, side, side]], I32)
    close = np.array([[24, 27, 1073741786, 1073741776], [6, 11, 1073741784, 1073741778]], I32)  # equal in float64, the second larger
    got = _launch(slot, z, z, z, close, np.zeros(2, I32), 1, 0.9)
    assert got[4].tolist() == [-1, 0] and got[5].tolist() == [COV, 0]
    got = _launch(close, np.zeros(2, I32), np.zeros(2, I32), np.zeros(2, I32), slot, z, 1, 0.9)
    assert got[4].tolist() == [1] and got[3].tolist() == [1, 0]
    slots = np.array([[2 ** 30, 2 ** 30, big, big], [low, low, big, big], [0, 0, 0, 0]], I32)
    dets = np.array([[low, low, big, big - 1], [2 ** 30, 2 ** 30, big, big], [big, big, big, big]], I32)
    got = _launch(slots, np.array([0, 0, P], I32), np.zeros(3, I32), None, dets, np.zeros(3, I32), 1, 1.0)
    assert got[4].tolist() == [2, 0, -1] and got[5].tolist() == [SPAWN, 0, FULL] and got[0][2].tolist() == [low, low, big, big - 1]
    a = np.array([[0, 0, 10, 10]] * 2, I32)
    got = _launch(a, np.zeros(2, I32), np.zeros(2, I32), np.zeros(2, I32), a, np.zeros(2, I32), 1, 0.3)
    assert got[4].tolist() == [0, 1]
    got = _launch(a, np.zeros(2, I32), np.zeros(2, I32), np.zeros(2, I32), a[:1], z, 1, 0.3)
    assert got[4].tolist() == [0] and got[3].tolist() == [0, 1]
    far = np.array([[100, 0, 5, 5]], I32)
    got = _launch(a[:1], z, z, z, far, z, 1, 0.3, max_misses=0)
    assert got[1].tolist() == [RETIRED] and got[0].tolist() == [[0] * 4] and got[5].tolist() == [FULL] and got[6].tolist() == [0]
    got = _launch(got[0], got[1], got[2], got[3], far, one, 2, 0.3, max_misses=0)
    assert got[4].tolist() == [0] and got[5].tolist() == [SPAWN] and got[2].tolist() == [1] and got[6].tolist() == [1] and got[3].tolist() == [0]
    none = np.zeros((0, 4), I32)
    got = _launch(none, np.zeros(0, I32), np.zeros(0, I32), None, np.array([[0, 0, 10, 10], [0, 0, 0, 10], [5, 5, 5, 5]], I32), np.zeros(3, I32), 1, 0.3, count=2)
    assert got[4].tolist() == [-1] * 3 and got[5].tolist() == [FULL, INV, PAD]
    got = _launch(np.array([[0, 0, 10, 10], [0, 0, 0, 0]], I32), np.array([0, P], I32), np.zeros(2, I32), np.zeros(2, I32), none, np.zeros(0, I32), 1, 0.3,
                  max_misses=3)
    assert got[3].tolist() == [1, 0] and got[6].tolist() == [0, 0] and got[1].tolist() == [0, P]


def test_argument_contract_writes_no_word():
    slots, flags, index, misses, dets, det_index = _case(6, 7, 3, 2)
    for kw in ({"iou": 0.0}, {"iou": float("nan")}, {"iou": 1.5}, {"n_frames": 0}, {"refresh": 2}):
        args = {"n_frames": 2, "iou": 0.3, "refresh": False}
        args.update(kw)
        got = _launch(slots, flags, index, misses, dets, det_index, args["n_frames"], args["iou"], refresh=args["refresh"], expect=_lib.E_INVALID)
        for g, w in zip(got[:4], (slots, flags, index, misses)):
            assert np.array_equal(g, w)
        assert all((g == -7777).all() for g in got[4:])
    got = _launch(slots, flags, index, None, dets, det_index, 2, 0.3, max_misses=0, expect=_lib.E_INVALID)
    assert np.array_equal(got[0], slots) and (got[4] == -7777).all()


# ---- 2. the all-identical chain ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, CAP])
def test_all_identical_boxes_in_one_frame_take_one_pair_a_round(n):
    """Every pair ties at the ratio 1, so a round finds one mutual pair, (k, k) in round k: min(n, m) rounds, the most the kernel
    runs. The words are stated: detection k goes to slot k. The time limit is sized from the round count: a round is two looks that
    each stop at their first candidate (ratio 1), two barriers and a few LDS words, which 50 microseconds a round covers many times
    over on any clock this part runs at; 20 ms stand for the launch itself."""
    lib = _lib.load()
    same = np.tile(np.array([[5, 7, 40, 30]], I32), (n, 1))
    zeros = np.zeros(n, I32)
    warm = _launch(same[:1], zeros[:1], zeros[:1], zeros[:1], same[:1], zeros[:1], 1, 0.3)  # the code object is loaded
    assert warm[4].tolist() == [0]
    dev = [torch.from_numpy(a.copy()).cuda() for a in (same, zeros, zeros, np.full(n, 3, I32), same, zeros)]
    out = [torch.full((n,), -9, dtype=torch.int32, device="cuda") for _ in range(3)]
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    begin.record()
    status = lib.dad3d_track_assign_detections(*(t.data_ptr() for t in dev[:4]), n, dev[4].data_ptr(), dev[5].data_ptr(), None, n, None, 1, 0.3, 0, 0,
                                               *(t.data_ptr() for t in out), 0, torch.cuda.current_stream().cuda_stream)
    end.record()
    torch.cuda.synchronize()
    assert status == _lib.OK, lib.dad3d_last_error()
    elapsed_ms = begin.elapsed_time(end)
    print(f"identical chain {n} x {n}: {elapsed_ms:.3f} ms")
    assert out[0].tolist() == list(range(n)) and out[1].tolist() == [0] * n and out[2].tolist() == [0] * n
    assert dev[3].tolist() == [0] * n and dev[1].tolist() == [0] * n and np.array_equal(dev[0].cpu().numpy(), same)
    assert elapsed_ms < 20.0 + n * 0.05, elapsed_ms


# ---- 3. the loop ---------------------------------------------------------------------------------------------------------------
FRAME_SHAPES = [(150, 200), (180, 140)]
START = [np.array([[10, 20, 90, 100], [95, 30, 100, 110]], I32), np.array([[20, 40, 100, 120]], I32)]  # three heads
TEX = 64


@pytest.fixture(scope="module")
def pred(flame_model):
    from dad_3dheads_amd.predictor import FaceMeshPredictor

    return FaceMeshPredictor.random_init(cuda_id=0, flame_model=flame_model)


@pytest.fixture(scope="module")
def frames():
    rng = np.random.default_rng(77)
    return [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda() for h, w in FRAME_SHAPES]


@pytest.fixture(scope="module")
def creator(flame_model, static):
    from dad_3dheads_amd.uv_texture import UVTextureCreator

    atlas = dict(synthetic.synthetic_texture_data(TEX, seed=0, static=static, duplicates=50))
    atlas.update(synthetic.synthetic_texcoords(TEX, static))
    return UVTextureCreator(texture_data=atlas, flame_model=flame_model, static=static, device=0)


def _config():
    return steady.SteadyConfig(rate=30.0, groups={"translation": (0.8, 0.3)})


def _started(pred, frames, **kw):
    from dad_3dheads_amd.tracking import HeadTracker

    tracker = HeadTracker(pred, steady=_config(), **kw)
    tracker.start(frames, START, n_slots=5)
    return tracker


def _detections(state_boxes, state_flags):
    """Detections that match slot 0 (its own box, one pixel to the right), miss slot 1 (nothing near it), and add a head in a corner
    of frame 1 where no slot stands; two rows of padding behind them. -> (boxes [5,4], frames [5], count)."""
    assert state_flags[0] == 0 and state_flags[1] == 0, "the scenario needs slots 0 and 1 tracked after the first step"
    x, y, w, h = (int(v) for v in state_boxes[0])
    new = [0, 0, 24, 24]
    bx, by, bw, bh = (int(v) for v in state_boxes[2])
    assert state_flags[2] != 0 or not (bx < 24 and by < 24 and bx + bw > 0 and by + bh > 0), "the corner of frame 1 is taken"
    dets = np.array([[x + 1, y, w, h], new, [3, 3, 0, 9], [1, 2, 3, 4], [5, 6, 7, 8]], I32)
    return dets, np.array([0, 1, 1, 0, 0], I32), 3


def test_update_equals_the_loop_whose_state_crosses_the_host(pred, frames, creator):
    from dad_3dheads_amd.uv_texture import TextureAccumulator

    # the device loop
    tracker = _started(pred, frames)
    acc = TextureAccumulator(creator, 5)
    assert tracker.n_slots == 5 and tracker.lost().tolist() == [0, 0, 0, P, P] and tracker.misses().tolist() == [0] * 5
    first = tracker.step(frames)
    assert [int(r["flags"]) for r in first[3:]] == [_lib.BOX_FLAG_EMPTY] * 2 and [int(r["image_index"]) for r in first[3:]] == [-1, -1]
    acc.add(first, frames)
    state = [t.cpu().numpy().copy() for t in (tracker.boxes(), tracker.lost(), tracker._index, tracker.misses())]
    dets, det_index, count = _detections(state[0], state[1])
    acc.textures.fill_(7)  # whatever the heads baked: a reset is seen on every texel
    acc.score.fill_(0.5)
    assert tracker.age().tolist()[:2] == [1, 1]
    d_dets, d_index, d_count = torch.from_numpy(dets).cuda(), torch.from_numpy(det_index).cuda(), torch.tensor([count], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    honoured = _sync_debug_is_honoured()
    print("torch.cuda.set_sync_debug_mode is honoured:", honoured)
    if honoured:
        torch.cuda.set_sync_debug_mode("error")
    try:
        result = tracker.update(d_dets, d_index, d_count, match_iou=0.3, max_misses=0, accumulator=acc)
    finally:
        if honoured:
            torch.cuda.set_sync_debug_mode("default")
    assert all(t.is_cuda and t.dtype == torch.int32 for t in result) and result._fields == ("assign", "det_flags", "spawned")
    # the statement on the state that was copied to the host
    want = boxes.assign_detections(state[0], state[1], state[2], state[3], dets, det_index, 2, 0.3, count=count, max_misses=0)
    for name, got, w in (("boxes", tracker.boxes(), want.boxes), ("flags", tracker.lost(), want.flags), ("frames", tracker._index, want.image_index),
                         ("misses", tracker.misses(), want.misses), ("assign", result.assign, want.assign), ("det_flags", result.det_flags, want.det_flags),
                         ("spawned", result.spawned, want.spawned)):
        assert np.array_equal(got.cpu().numpy(), w), name
    assert want.assign.tolist() == [0, 3, -1, -1, -1] and want.det_flags.tolist() == [0, SPAWN, INV, PAD, PAD]
    assert want.flags[1] == RETIRED and want.spawned.tolist() == [0, 0, 0, 1, 0] and want.image_index[3] == 1
    # the spawned slot's filter track and texture restart; the matched slot's do not
    assert tracker.age().tolist()[0] == 1 and tracker.age().tolist()[3] == 0
    tex, score = acc.textures.cpu().numpy(), acc.score.cpu().numpy()
    assert (tex[3] == 0).all() and (score[3] == -1.0).all()
    assert all((tex[k] == 7).all() and (score[k] == 0.5).all() for k in (0, 1, 2, 4))
    second = tracker.step(frames)
    assert tracker.age().tolist()[3] == 1 and tracker.age().tolist()[0] == 2

    # the host loop: the same start and step, the state through the statement, the same step again
    other = _started(pred, frames)
    other.step(frames)
    for t, before, after in zip((other._boxes, other._track_flags, other._index, other._misses), state, (want.boxes, want.flags, want.image_index, want.misses)):
        assert np.array_equal(t.cpu().numpy(), before)  # the same start and the same step
        t.copy_(torch.from_numpy(after).cuda())
    other._filter.reset(np.flatnonzero(want.spawned))
    again = other.step(frames)
    for k, (g, w) in enumerate(zip(second, again)):
        for key in ("track_flags", "image_index", "flags", "bbox"):
            assert torch.equal(g[key], w[key]), (k, key)
    assert [int(r["image_index"]) for r in second][1] == -1 and int(second[1]["flags"]) == _lib.BOX_FLAG_EMPTY  # the retired slot is an ordinary lost slot
    assert int(second[3]["flags"]) == 0  # the spawned slot read its crop from frame 1
    assert np.array_equal(tracker.boxes().cpu().numpy(), other.boxes().cpu().numpy()) and tracker.lost().tolist() == other.lost().tolist()
    assert tracker.lost().tolist()[1] == P and tracker.misses().tolist() == want.misses.tolist()


def _sync_debug_is_honoured():
    """Does this build raise for a synchronising call under `set_sync_debug_mode("error")`?"""
    probe = torch.zeros(1, device="cuda")
    torch.cuda.set_sync_debug_mode("error")
    try:
        probe.item()
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return False


def test_update_in_its_host_forms_and_no_call_waits(pred, frames, monkeypatch):
    """Per-frame lists and a flat array with an index give what device tensors give; with device tensors nothing touches the host."""
    outs = []
    dets = [np.array([[11, 20, 90, 100]], I32), np.array([[0, 0, 24, 24], [30, 30, 0, 5]], np.float64)]
    flat, index = np.concatenate([d.astype(np.float64) for d in dets]), np.array([0, 1, 1], I32)
    for form in ("lists", "flat", "device"):
        tracker = _started(pred, frames)
        if form == "lists":
            outs.append((tracker, tracker.update(dets, refresh=True, frame_searched=[1, 0])))
        elif form == "flat":
            outs.append((tracker, tracker.update(flat, index, refresh=True, frame_searched=np.array([True, False]))))
        else:
            args = (torch.from_numpy(flat).cuda(), torch.from_numpy(index).cuda(), torch.tensor(3, device="cuda"))
            mask = torch.tensor([1, 0], device="cuda")
            torch.cuda.synchronize()

            def refuse(*a, **k):
                raise AssertionError("a host wait")

            with monkeypatch.context() as mp:
                for name in ("cpu", "item", "tolist", "numpy"):
                    mp.setattr(torch.Tensor, name, refuse)
                mp.setattr(torch.cuda, "synchronize", refuse)
                outs.append((tracker, tracker.update(*args, refresh=True, frame_searched=mask)))
    for tracker, result in outs:
        assert result.assign.tolist() == [0, 3, -1] and result.det_flags.tolist() == [0, SPAWN, INV] and result.spawned.tolist() == [0, 0, 0, 1, 0]
        assert tracker.boxes().tolist() == [[11, 20, 90, 100], [95, 30, 100, 110], [20, 40, 100, 120], [0, 0, 24, 24], [0] * 4]
        assert tracker.misses().tolist() == [0, 1, 0, 0, 0] and tracker.lost().tolist() == [0, 0, 0, 0, P]  # frame 1 was not searched: slot 2 counts no miss
        assert tracker._index.tolist() == [0, 0, 1, 1, 0]
    tracker = outs[0][0]
    tracker.reseed([1], [[95, 30, 100, 110]])
    assert tracker.misses().tolist() == [0] * 5
    full = tracker.update([np.zeros((0, 4), I32), np.array([[100, 100, 20, 20], [60, 150, 20, 20]], I32)], count=2)
    assert full.det_flags.tolist() == [SPAWN, FULL] and full.assign.tolist() == [4, -1]


def test_a_tracker_without_spare_slots_that_is_never_updated_is_the_plain_loop(flame_model, frames):
    """No `n_slots`, no `update`: the keys and bits of `predict_boxes` with the boxes taken by `boxes.next_boxes` on the host, as
    test_gpu_track_boxes.py compares them, on its deterministic stub model (a row's bits do not depend on the call it stands in)."""
    from dad_3dheads_amd.config import load_default_config
    from dad_3dheads_amd.predictor import FaceMeshPredictor
    from dad_3dheads_amd.tracking import HeadTracker
    from test_gpu_track_boxes import Stub

    pred = FaceMeshPredictor(load_default_config(), cuda_id=0, model=Stub(), flame_model=flame_model)
    tracker = HeadTracker(pred)
    tracker.start(frames, START)
    assert tracker.n_slots == 3 and tracker.misses().tolist() == [0, 0, 0]
    flat, index = boxes.flatten_boxes(len(frames), START)
    host_frames = [f.cpu().numpy() for f in frames]
    keys = ("bbox", "flags", "3dmm_params", "projected_vertices", "points", "3d_vertices")
    for t in range(2):
        got = tracker.step(frames)
        res = pred.predict_boxes(host_frames, flat, image_index=index)
        proj = np.concatenate([r["projected_vertices"].numpy() for r in res])
        flat, track = boxes.next_boxes(proj, FRAME_SHAPES, index, prev_flags=[r["flags"] for r in res])
        for k, (g, w) in enumerate(zip(got, res)):
            assert set(g) == set(keys) | {"track_flags", "image_index"} == set(w) | {"track_flags"}  # no new key
            for key in keys:
                gv, wv = g[key].cpu().numpy(), np.asarray(w[key].numpy() if torch.is_tensor(w[key]) else w[key])
                assert gv.shape == wv.shape and gv.tobytes() == wv.astype(gv.dtype).tobytes(), (t, k, key)
            assert int(g["track_flags"]) == track[k] and int(g["image_index"]) == (w["image_index"] if track[k] == 0 and w["flags"] == 0 else -1)
        assert np.array_equal(tracker.boxes().cpu().numpy(), flat.astype(I32)) and tracker.lost().tolist() == track.tolist()
    assert tracker.misses().tolist() == [0, 0, 0]
