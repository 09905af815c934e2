"""CPU: detections into tracks -- `dad3d_track_assign_detections` (csrc/track_assign.hip) is exported, bound, mirrors the header and
refuses bad calls before any device work; the host statement of its rule (`boxes.assign_detections`) pinned by hand, one small case
each, and held to an independent sorted walk in `fractions.Fraction` and to the round form the kernel runs, on random cases from a
coordinate grid small enough for ties and chains; `HeadTracker.start(n_slots=)` and `HeadTracker.update` refuse bad calls before
anything is launched."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from dad_3dheads_amd import _lib, boxes
from dad_3dheads_amd.tracking import HeadTracker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD, INV, COV, SPAWN, FULL = (_lib.ASSIGN_FLAG_PADDING, _lib.ASSIGN_FLAG_INVALID, _lib.ASSIGN_FLAG_COVERED, _lib.ASSIGN_FLAG_SPAWNED,
                              _lib.ASSIGN_FLAG_FULL)
P, RETIRED = _lib.TRACK_FLAG_PREVIOUS, _lib.TRACK_FLAG_RETIRED
I32 = np.int32


def _assign(slots, dets, flags=None, index=None, misses=None, det_index=None, n_frames=1, iou=0.3, **kw):
    slots, dets = np.asarray(slots, I32).reshape(-1, 4), np.asarray(dets, I32).reshape(-1, 4)
    n, m = len(slots), len(dets)
    flags = np.zeros(n, I32) if flags is None else np.asarray(flags, I32)
    index = np.zeros(n, I32) if index is None else np.asarray(index, I32)
    misses = np.zeros(n, I32) if misses is None else np.asarray(misses, I32)
    det_index = np.zeros(m, I32) if det_index is None else np.asarray(det_index, I32)
    before = [a.copy() for a in (slots, flags, index, misses, dets, det_index)]
    out = boxes.assign_detections(slots, flags, index, misses, dets, det_index, n_frames, iou, **kw)
    for a, b in zip((slots, flags, index, misses, dets, det_index), before):
        assert np.array_equal(a, b), "the statement works on copies"
    assert all(v.dtype == I32 for v in out) and out.assign.shape == (m,) and out.spawned.shape == (n,)
    return out


# ---- the library ---------------------------------------------------------------------------------------------------------------
def test_entry_is_exported_and_constants_mirror_the_header():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "dad3d_track_assign_detections")
    assert len(_lib.SIGNATURES["dad3d_track_assign_detections"][1]) == 19
    text = open(os.path.join(ROOT, "include", "dad3d.h")).read()

    def define(name):
        found = re.findall(r"#define\s+" + name + r"\s+\(?(0x[0-9a-fA-F]+|\d+)\)?\s*$", text, re.M)
        assert len(found) == 1, (name, found)
        return int(found[0], 0)

    assert re.search(r"#define\s+DAD3D_TRACK_FLAG_RETIRED\s+\(0x40\)", text)  # parenthesised: not one of the five plain flags
    assert define("DAD3D_TRACK_FLAG_RETIRED") == _lib.TRACK_FLAG_RETIRED == 0x40
    assert define("DAD3D_TRACK_MAX_DETECTIONS") == _lib.TRACK_MAX_DETECTIONS == 1024 == _lib.TRACK_MAX_SLOTS
    bits = [define("DAD3D_ASSIGN_FLAG_" + k) for k in ("PADDING", "INVALID", "COVERED", "SPAWNED", "FULL")]
    assert bits == [PAD, INV, COV, SPAWN, FULL]
    assert all(b > 0 and b & (b - 1) == 0 for b in bits) and len(set(bits)) == 5  # distinct powers of two
    others = (_lib.TRACK_FLAG_PREVIOUS, _lib.TRACK_FLAG_RANGE, _lib.TRACK_FLAG_NONFINITE, _lib.TRACK_FLAG_SMALL, _lib.TRACK_FLAG_OUTSIDE,
              _lib.TRACK_FLAG_DUPLICATE)
    assert all(RETIRED & v == 0 for v in others)  # a seventh bit


def test_argument_errors_come_before_any_device_work():
    """No GPU is needed to be refused."""
    lib = _lib.load()
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.addressof(buf)

    def call(b=p, f=p, ix=p, mi=p, n=1, db=p, di=p, dc=None, m=1, fs=None, nf=1, iou=0.5, refresh=0, mm=-1, a=p, df=p, sp=p):
        return lib.dad3d_track_assign_detections(b, f, ix, mi, n, db, di, dc, m, fs, nf, iou, refresh, mm, a, df, sp, 0, None)

    nan, inf = float("nan"), float("inf")
    for kw in ({"iou": 0.0}, {"iou": -0.5}, {"iou": float(np.nextafter(1.0, 2.0))}, {"iou": nan}, {"iou": inf}, {"n": -1}, {"m": -1},
               {"n": _lib.TRACK_MAX_SLOTS + 1}, {"m": _lib.TRACK_MAX_DETECTIONS + 1}, {"nf": 0}, {"nf": -3}, {"refresh": 2}, {"refresh": -1},
               {"mm": 0, "mi": None}, {"mm": 5, "mi": None}, {"b": None}, {"f": None}, {"ix": None}, {"sp": None}, {"db": None}, {"di": None},
               {"a": None}, {"df": None}, {"n": 0, "m": 0, "iou": nan}, {"n": 0, "m": 0, "nf": 0}, {"n": 0, "db": None}, {"m": 0, "sp": None}):
        assert call(**kw) == _lib.E_INVALID, kw
        assert b"dad3d_track_assign_detections" in lib.dad3d_last_error(), kw
    # both extents zero: valid, and nothing to launch; a pointer whose extent is zero may be null
    assert call(n=0, m=0) == _lib.OK
    assert call(n=0, m=0, b=None, f=None, ix=None, mi=None, sp=None, db=None, di=None, a=None, df=None) == _lib.OK
    assert not any(buf)  # nothing was written


# ---- the rule, by hand ---------------------------------------------------------------------------------------------------------
def test_best_first_keeps_the_identities_of_two_neighbouring_heads():
    """Two heads side by side whose boxes overlap, detected in the other order. "The first slot that passes" would give detection 0
    to slot 0 (IoU 60/140 passes 0.3) and swap the two heads; best-first gives each detection its own head."""
    slots = [(0, 0, 10, 10), (4, 0, 10, 10)]
    out = _assign(slots, [(4, 0, 10, 10), (0, 0, 10, 10)])
    assert out.assign.tolist() == [1, 0] and out.det_flags.tolist() == [0, 0]
    assert out.boxes.tolist() == [list(b) for b in slots] and out.spawned.tolist() == [0, 0] and out.misses.tolist() == [0, 0]
    # and a detection between the two goes to the nearer head: 80/120 against 70/130
    out = _assign(slots, [(2, 0, 10, 10)], misses=[3, 4])
    assert out.assign.tolist() == [0] and out.misses.tolist() == [0, 5]
    out = _assign(slots, [(3, 0, 10, 10)], misses=[3, 4])
    assert out.assign.tolist() == [1] and out.misses.tolist() == [4, 0]


def test_ties_go_to_the_lower_detection_then_to_the_lower_slot():
    a = (0, 0, 10, 10)
    out = _assign([a, a], [a, a])
    assert out.assign.tolist() == [0, 1] and out.det_flags.tolist() == [0, 0]
    out = _assign([a], [a, a])
    assert out.assign.tolist() == [0, -1] and out.det_flags.tolist() == [0, COV]  # the lower detection
    out = _assign([a, a], [a])
    assert out.assign.tolist() == [0] and out.misses.tolist() == [0, 1]  # the lower slot
    # equal ratios that are no equal boxes: 1/2 three times
    slots, dets = [(0, 0, 10, 10), (0, 5, 10, 10)], [(0, 0, 10, 5), (0, 5, 10, 5)]
    out = _assign(slots, dets, iou=0.5)  # detection 1 lies in both slots at 50/100: it ties, detection 0 passes with slot 0 only
    assert out.assign.tolist() == [0, 1]
    out = _assign(slots, dets[::-1], iou=0.5)  # now detection 0 ties: (0, 0) is the first pair of the list and detection 1 is left covered
    assert out.assign.tolist() == [0, -1] and out.det_flags.tolist() == [0, COV]


def test_ratios_are_compared_exactly_where_their_double_quotients_are_equal():
    """Found by search: against the slot (0, 0, 2^30, 2^30) these two detections have different IoUs, the second the larger, whose
    float64 quotients are the same number, and so are the float64 cross products."""
    side = 2 ** 30
    slot, d0, d1 = (0, 0, side, side), (24, 27, 1073741786, 1073741776), (6, 11, 1073741784, 1073741778)

    def areas(d):
        inter = (min(d[0] + d[2], side) - d[0]) * (min(d[1] + d[3], side) - d[1])
        return inter, d[2] * d[3] + side * side - inter

    (i0, u0), (i1, u1) = areas(d0), areas(d1)
    assert float(i0) / float(u0) == float(i1) / float(u1) and float(i0) * float(u1) == float(i1) * float(u0)
    assert i1 * u0 > i0 * u1 and Fraction(i1, u1) > Fraction(i0, u0)
    out = _assign([slot], [d0, d1], iou=0.9)
    assert out.assign.tolist() == [-1, 0] and out.det_flags.tolist() == [COV, 0]
    out = _assign([slot], [d1, d0], iou=0.9)
    assert out.assign.tolist() == [0, -1]
    out = _assign([d0, d1], [slot], iou=0.9)  # and from the slots' side: the higher slot is the better one
    assert out.assign.tolist() == [1] and out.misses.tolist() == [1, 0]


def test_boxes_at_the_int32_extremes_do_not_overflow():
    big, low = 2 ** 31 - 1, -(2 ** 31)
    slots = [(2 ** 30, 2 ** 30, big, big), (low, low, big, big)]  # x + w beyond 2^31; areas of nearly 2^62
    dets = [(low, low, big, big - 1), (2 ** 30, 2 ** 30, big, big), (big, big, big, big)]
    out = _assign(slots + [(0, 0, 0, 0)], dets, flags=[0, 0, P], iou=1.0)
    # detection 0 is not slot 1's box exactly (IoU (2^31 - 2) / (2^31 - 1) < 1); it overlaps it, but does not pass at 1.0: it spawns
    assert out.assign.tolist() == [2, 0, -1] and out.det_flags.tolist() == [SPAWN, 0, FULL]
    out = _assign(slots + [(0, 0, 0, 0)], dets, flags=[0, 0, P], iou=float(np.nextafter(1.0, 0.0)) - 2.0 ** -31)
    assert out.assign.tolist() == [1, 0, 2] and out.det_flags.tolist() == [0, 0, SPAWN]
    assert out.boxes[2].tolist() == [big] * 4
    # wrapped to int32, slot 0's far corner would be negative and nothing would meet it
    out = _assign([(2 ** 30, 2 ** 30, big, big)], [(2 ** 31 - 10, 2 ** 31 - 10, 5, 5)], iou=1e-18)
    assert out.assign.tolist() == [0]
    out = _assign([(2 ** 30, 2 ** 30, big, big)], [(2 ** 31 - 10, 2 ** 31 - 10, 5, 5)], iou=1e-17)  # 25 / (2^31 - 1)^2 is 5.4e-18
    assert out.det_flags.tolist() == [FULL]


def test_covered_by_a_slot_that_is_matched_to_another_detection():
    a = (0, 0, 10, 10)
    out = _assign([a, (0, 0, 0, 0)], [a, (1, 0, 10, 10)], flags=[0, P])
    assert out.assign.tolist() == [0, -1] and out.det_flags.tolist() == [0, COV]  # a free slot is there, and stays free
    assert out.spawned.tolist() == [0, 0] and out.flags.tolist() == [0, P] and out.boxes.tolist() == [list(a), [0] * 4]
    # the slot's flag and its empty box each make it free: the same detections then spawn
    out = _assign([a, (0, 0, 0, 0)], [(1, 0, 10, 10)], flags=[8, P])
    assert out.assign.tolist() == [0] and out.det_flags.tolist() == [SPAWN] and out.flags.tolist() == [0, P]
    out = _assign([(0, 0, 10, 0), (0, 0, -3, 10)], [(1, 0, 10, 10), a])
    assert out.assign.tolist() == [0, 1] and out.det_flags.tolist() == [SPAWN, SPAWN]  # overlapping each other: both spawn


def test_full_spawn_order_and_invalid_detections():
    slots = [(0, 0, 10, 10), (0, 0, 0, 0), (50, 50, 10, 10), (7, 7, 7, 7)]
    dets = [(100, 0, 5, 5), (200, 0, 0, 5), (300, 0, 5, 5), (400, 0, 5, 5), (500, 0, 5, -1), (600, 0, 5, 5), (0, 0, 10, 10)]
    det_index = [0, 0, 0, 2, 0, -1, 0]
    out = _assign(slots, dets, flags=[0, P, 0, 16], det_index=det_index, n_frames=2, misses=[0, 9, 0, 9])
    assert out.assign.tolist() == [1, -1, 3, -1, -1, -1, 0]
    assert out.det_flags.tolist() == [SPAWN, INV, SPAWN, INV, INV, INV, 0]  # an empty side, a frame beyond the frames, a negative side and frame
    assert out.spawned.tolist() == [0, 1, 0, 1] and out.flags.tolist() == [0, 0, 0, 0] and out.misses.tolist() == [0, 0, 1, 0]
    assert out.boxes.tolist() == [[0, 0, 10, 10], [100, 0, 5, 5], [50, 50, 10, 10], [300, 0, 5, 5]]
    out = _assign(slots, [d for d, f in zip(dets, det_index) if f == 0 and d[2] > 0 and d[3] > 0] + [(700, 0, 5, 5)], flags=[0, P, 0, 16])
    assert out.assign.tolist() == [1, 3, 0, -1] and out.det_flags.tolist() == [SPAWN, SPAWN, 0, FULL]


def test_padding_by_count():
    a, far = (0, 0, 10, 10), (100, 0, 5, 5)
    slots, dets = [a, (0, 0, 0, 0), (0, 0, 0, 0)], [a, far, (200, 0, 5, 5)]
    for count, assign, how in ((-5, [-1] * 3, [PAD] * 3), (0, [-1] * 3, [PAD] * 3), (1, [0, -1, -1], [0, PAD, PAD]),
                               (2, [0, 1, -1], [0, SPAWN, PAD]), (3, [0, 1, 2], [0, SPAWN, SPAWN]), (4, [0, 1, 2], [0, SPAWN, SPAWN]),
                               (2 ** 31 - 1, [0, 1, 2], [0, SPAWN, SPAWN]), (None, [0, 1, 2], [0, SPAWN, SPAWN])):
        out = _assign(slots, dets, flags=[0, P, P], count=count)
        assert out.assign.tolist() == assign and out.det_flags.tolist() == how, count
        assert out.misses.tolist() == [0 if assign[0] == 0 else 1, 0, 0]  # padding confirms nobody
    out = _assign(slots, [(0, 0, 0, 0), a], flags=[0, P, P], count=1)
    assert out.det_flags.tolist() == [INV, PAD]  # padding is said first


def test_refresh_on_and_off():
    slots, dets = [(0, 0, 10, 10), (50, 0, 10, 10)], [(51, 1, 10, 10), (1, 0, 11, 10)]
    off = _assign(slots, dets)
    on = _assign(slots, dets, refresh=True)
    assert off.assign.tolist() == on.assign.tolist() == [1, 0]
    assert off.boxes.tolist() == [list(b) for b in slots] and on.boxes.tolist() == [[1, 0, 11, 10], [51, 1, 10, 10]]
    assert on.image_index.tolist() == [0, 0] and on.flags.tolist() == [0, 0]


def test_retirement_over_consecutive_calls():
    a, none = (0, 0, 10, 10), np.zeros((0, 4), I32)
    out = _assign([a], none, max_misses=0)  # more than 0 misses: the first unconfirmed call retires
    assert out.flags.tolist() == [RETIRED] and out.boxes.tolist() == [[0] * 4] and out.misses.tolist() == [1]
    state = _assign([a], none, max_misses=1)
    assert state.flags.tolist() == [0] and state.misses.tolist() == [1] and state.boxes.tolist() == [list(a)]
    again = _assign(state.boxes, [a], flags=state.flags, misses=state.misses, max_misses=1)  # a match in between
    assert again.misses.tolist() == [0] and again.assign.tolist() == [0]
    for calls, (flag, count) in enumerate(((0, 1), (RETIRED, 2)), 1):
        again = _assign(again.boxes, none, flags=again.flags, misses=again.misses, max_misses=1)
        assert again.flags.tolist() == [flag] and again.misses.tolist() == [count], calls
    gone = _assign(again.boxes, none, flags=again.flags, misses=again.misses, max_misses=1)
    assert gone.flags.tolist() == [RETIRED] and gone.misses.tolist() == [2]  # a retired slot is free: it counts nothing more
    # never: a negative limit, or None
    for never in (None, -1, -7):
        out = _assign([a], none, misses=[5], max_misses=never)
        assert out.flags.tolist() == [0] and out.misses.tolist() == [6]
    out = _assign([a, a], none, misses=[2 ** 30 - 1, 2 ** 30], max_misses=2 ** 30)
    assert out.misses.tolist() == [2 ** 30, 2 ** 30] and out.flags.tolist() == [0, 0]  # saturated, never beyond the largest limit
    out = _assign([a], none, misses=[2 ** 31 - 1])
    assert out.misses.tolist() == [2 ** 30]
    # without misses nothing is counted, nothing retires, and a limit has nothing to compare
    out = boxes.assign_detections([a], [0], [0], None, none, [], 1, 0.3)
    assert out.misses is None and out.flags.tolist() == [0]
    with pytest.raises(ValueError, match="max_misses"):
        boxes.assign_detections([a], [0], [0], None, none, [], 1, 0.3, max_misses=0)


def test_a_slot_of_a_frame_that_was_not_searched_is_untouched():
    a = (0, 0, 10, 10)
    slots, index = [a, a, a, a], [0, 1, 2, 7]
    out = _assign(slots, [a], index=index, det_index=[2], n_frames=3, frame_searched=[0, 5, 1], max_misses=0, misses=[4, 4, 4, 4])
    assert out.assign.tolist() == [2]
    assert out.misses.tolist() == [4, 5, 0, 4] and out.flags.tolist() == [0, RETIRED, 0, 0]  # frame 7 is no frame of the mask: not searched
    out = _assign(slots, [a], index=index, det_index=[2], n_frames=3, max_misses=0, misses=[4, 4, 4, 4])
    assert out.misses.tolist() == [5, 5, 0, 5] and out.flags.tolist() == [RETIRED, RETIRED, 0, RETIRED]  # no mask: every slot was searched
    with pytest.raises(ValueError, match="frame_searched"):
        _assign(slots, [a], index=index, n_frames=3, frame_searched=[1, 1])


def test_a_spawn_moves_the_slot_to_the_detections_frame():
    out = _assign([(0, 0, 10, 10), (3, 3, 3, 3)], [(0, 0, 10, 10)], flags=[0, 2], index=[0, 0], det_index=[1], n_frames=2, misses=[0, 6])
    assert out.assign.tolist() == [1] and out.det_flags.tolist() == [SPAWN]  # the same box in another frame is another head
    assert out.image_index.tolist() == [0, 1] and out.boxes[1].tolist() == [0, 0, 10, 10] and out.flags.tolist() == [0, 0]
    assert out.misses.tolist() == [1, 0] and out.spawned.tolist() == [0, 1]


def test_a_slot_retired_in_a_call_is_not_reused_in_that_call():
    far = (100, 0, 5, 5)
    out = _assign([(0, 0, 10, 10)], [far], max_misses=0)
    assert out.flags.tolist() == [RETIRED] and out.det_flags.tolist() == [FULL] and out.assign.tolist() == [-1] and out.spawned.tolist() == [0]
    nxt = _assign(out.boxes, [far], flags=out.flags, misses=out.misses, max_misses=0)
    assert nxt.assign.tolist() == [0] and nxt.det_flags.tolist() == [SPAWN] and nxt.flags.tolist() == [0] and nxt.misses.tolist() == [0]
    assert nxt.boxes.tolist() == [list(far)] and nxt.spawned.tolist() == [1]


def test_no_slots_and_no_detections():
    dets = [(0, 0, 10, 10), (0, 0, 0, 10), (5, 5, 5, 5)]
    out = _assign(np.zeros((0, 4), I32), dets, count=2)
    assert out.assign.tolist() == [-1] * 3 and out.det_flags.tolist() == [FULL, INV, PAD] and out.spawned.shape == (0,)
    out = _assign([(0, 0, 10, 10), (0, 0, 0, 0)], np.zeros((0, 4), I32), flags=[0, P], max_misses=3)
    assert out.assign.shape == (0,) and out.misses.tolist() == [1, 0] and out.spawned.tolist() == [0, 0] and out.flags.tolist() == [0, P]
    out = _assign(np.zeros((0, 4), I32), np.zeros((0, 4), I32))
    assert out.assign.shape == out.spawned.shape == (0,)
    for bad in ({"iou": 0.0}, {"iou": 1.5}, {"iou": float("nan")}, {"n_frames": 0}):
        with pytest.raises(ValueError):
            _assign([(0, 0, 1, 1)], [(0, 0, 1, 1)], **bad)
    with pytest.raises(ValueError):
        boxes.assign_detections(np.zeros((2, 4)), [0], [0, 0], [0, 0], np.zeros((0, 4)), [], 1, 0.5)


# ---- an independent statement --------------------------------------------------------------------------------------------------
def _passing(slots, flags, index, dets, det_index, real, n_frames, iou):
    """{(d, s): Fraction} of the passing pairs, and which slots are live and which detections valid, in plain Python."""
    live = [flags[s] == 0 and slots[s][2] > 0 and slots[s][3] > 0 for s in range(len(slots))]
    valid = [d < real and dets[d][2] > 0 and dets[d][3] > 0 and 0 <= det_index[d] < n_frames for d in range(len(dets))]
    ratio = {}
    for d, (x, y, w, h) in enumerate(dets):
        for s, (sx, sy, sw, sh) in enumerate(slots):
            if valid[d] and live[s] and index[s] == det_index[d]:
                inter = max(0, min(x + w, sx + sw) - max(x, sx)) * max(0, min(y + h, sy + sh) - max(y, sy))
                union = w * h + sw * sh - inter
                if inter > 0 and float(inter) >= iou * float(union):
                    ratio[d, s] = Fraction(inter, union)
    return ratio, live, valid


def _walk(ratio):
    """The sorted walk: {d: s}."""
    taken_d, taken_s = {}, set()
    for d, s in sorted(ratio, key=lambda k: (-ratio[k], k[0], k[1])):
        if d not in taken_d and s not in taken_s:
            taken_d[d] = s
            taken_s.add(s)
    return taken_d


def _rounds(ratio):
    """The round form of the kernel: every unmatched detection's best unmatched slot, every unmatched slot's best unmatched detection
    over all of them, mutual pairs taken, until a round takes nothing. -> ({d: s}, rounds that took something)."""
    taken_d, taken_s, rounds = {}, set(), 0
    while True:
        best_s, best_d = {}, {}
        for d, s in sorted(ratio):  # ascending, and replaced only by a strictly better ratio: ties stay with the lower index
            if d in taken_d or s in taken_s:
                continue
            if d not in best_s or ratio[d, s] > ratio[d, best_s[d]]:
                best_s[d] = s
            if s not in best_d or ratio[d, s] > ratio[best_d[s], s]:
                best_d[s] = d
        mutual = [(d, s) for d, s in best_s.items() if best_d[s] == d]
        if not mutual:
            return taken_d, rounds
        rounds += 1
        for d, s in mutual:
            taken_d[d] = s
            taken_s.add(s)


def _independent(slots, flags, index, misses, dets, det_index, n_frames, iou, count, searched, refresh, max_misses):
    n, m = len(slots), len(dets)
    real = m if count is None else min(max(count, 0), m)
    ratio, live, valid = _passing(slots, flags, index, dets, det_index, real, n_frames, iou)
    match = _walk(ratio)
    by_rounds, rounds = _rounds(ratio)
    assert by_rounds == match, "the round form is not the sorted walk"
    slots, flags, index, misses = [list(b) for b in slots], list(flags), list(index), list(misses)
    assign, how, spawned = [-1] * m, [0] * m, [0] * n
    vacant = [s for s in range(n) if not live[s]]
    for d in range(m):
        if d >= real:
            how[d] = PAD
        elif not valid[d]:
            how[d] = INV
        elif d in match:
            assign[d] = match[d]
            misses[match[d]] = 0
            if refresh:
                slots[match[d]] = list(dets[d])
        elif any(k[0] == d for k in ratio):
            how[d] = COV
        elif vacant:
            s = vacant.pop(0)
            assign[d], how[d], spawned[s] = s, SPAWN, 1
            slots[s], index[s], flags[s], misses[s] = list(dets[d]), det_index[d], 0, 0
        else:
            how[d] = FULL
    for s in range(n):
        if live[s] and s not in match.values() and (searched is None or (0 <= index[s] < n_frames and searched[index[s]])):
            misses[s] = min(misses[s] + 1, 2 ** 30)
            if max_misses is not None and 0 <= max_misses < misses[s]:
                flags[s], slots[s] = RETIRED, [0] * 4
    return (slots, flags, index, misses, assign, how, spawned), rounds


def grid_case(rng, n, m, n_frames=2, span=4):
    """Boxes on a grid of `span` positions with sides 1 .. 4 (a few empty), most of them in frame 0, so that equal ratios and chains of
    preferences are common; some slots flagged, some frames outside the frames. -> (slots, flags, index, misses, dets, det_index)."""
    def some(k):
        b = np.concatenate([rng.integers(0, span, (k, 2)), rng.integers(1, 5, (k, 2))], axis=1).astype(I32)
        b[rng.random(k) < 0.05, 2 + (k & 1)] = rng.integers(-2, 1)
        return b

    def frames(k):
        return np.where(rng.random(k) < 0.7, 0, rng.integers(-1, n_frames + 1, k)).astype(I32)

    flags = np.where(rng.random(n) < 0.1, rng.choice([1, 8, 32, 64], n), 0).astype(I32)
    return some(n), flags, frames(n), rng.integers(0, 3, n).astype(I32), some(m), frames(m)


def test_statement_equals_an_independent_walk_in_fractions_and_the_round_form():
    rng = np.random.default_rng(2024)
    most_rounds, ties, outcomes = 0, 0, set()
    for case in range(3000):
        n, m = (int(v) for v in rng.integers(0, 12, 2))
        slots, flags, index, misses, dets, det_index = grid_case(rng, n, m)
        iou = float(rng.choice([0.02, 0.1, 0.3, 0.5, 1.0], p=[0.3, 0.25, 0.2, 0.15, 0.1]))
        count = None if case % 3 else int(rng.integers(-1, m + 2))
        searched = None if case % 4 else rng.integers(0, 2, 2).tolist()
        refresh, max_misses = bool(case & 1), (None, 0, 1, 2)[case % 4]
        got = boxes.assign_detections(slots, flags, index, misses, dets, det_index, 2, iou, count, searched, refresh, max_misses)
        want, rounds = _independent(slots.tolist(), flags.tolist(), index.tolist(), misses.tolist(), dets.tolist(), det_index.tolist(), 2, iou,
                                    count, searched, refresh, max_misses)
        assert [v.tolist() for v in got] == list(want), case
        most_rounds = max(most_rounds, rounds)
        outcomes.update(want[5])
        ratio = _passing(slots.tolist(), flags.tolist(), index.tolist(), dets.tolist(), det_index.tolist(), m if count is None else count, 2, iou)[0]
        ties += len(set(ratio.values())) < len(ratio)
    assert outcomes == {0, PAD, INV, COV, SPAWN, FULL}
    assert ties > 300 and most_rounds >= 3, (ties, most_rounds)  # the cases are not vacuous: equal ratios, and chains of several rounds


# ---- HeadTracker's argument errors ---------------------------------------------------------------------------------------------
class _NoLaunch:
    """A predictor on the CPU whose every launch is an error: what the tracker may touch before it refuses a call."""
    device = torch.device("cpu")
    _img_size = 256

    def __getattr__(self, name):
        raise AssertionError(f"the tracker reached for predictor.{name} before it refused the call")


def test_head_tracker_refuses_bad_slots_and_updates_before_anything_is_launched():
    frames = [np.zeros((400, 400, 3), np.uint8), np.zeros((300, 300, 3), np.uint8)]
    start = [np.array([[10, 10, 200, 200]], I32), np.array([[20, 20, 100, 100], [150, 150, 100, 100]], I32)]
    det = np.array([[10, 10, 50, 50]], I32)
    tracker = HeadTracker(_NoLaunch())
    with pytest.raises(ValueError, match="start"):
        tracker.update([det, det])
    with pytest.raises(ValueError, match="start"):
        tracker.misses()
    for bad in (2, -1, 2.5, "5", True):
        with pytest.raises(ValueError, match="n_slots"):
            tracker.start(frames, start, n_slots=bad)
    assert tracker.n_slots == 0
    tracker.start(frames, start, n_slots=5)
    assert tracker.n_slots == 5 and tracker.boxes().tolist() == [[10, 10, 200, 200], [20, 20, 100, 100], [150, 150, 100, 100], [0] * 4, [0] * 4]
    assert tracker.lost().tolist() == [0, 0, 0, P, P] and tracker.misses().tolist() == [0] * 5 and tracker._index.tolist() == [0, 1, 1, 0, 0]
    tracker.start(frames, start, n_slots=3)
    assert tracker.n_slots == 3 and tracker.lost().tolist() == [0, 0, 0]
    tracker.start(frames, start)
    assert tracker.n_slots == 3 and tracker.lost().tolist() == [0, 0, 0]
    nan = float("nan")
    many = np.tile(det, (_lib.TRACK_MAX_DETECTIONS + 1, 1))
    for args, kw, what in (
            (([det, det],), {"match_iou": 0.0}, "match_iou"), (([det, det],), {"match_iou": 1.01}, "match_iou"), (([det, det],), {"match_iou": nan}, "match_iou"),
            (([det, det],), {"max_misses": 1.5}, "max_misses"), (([det, det],), {"max_misses": True}, "max_misses"),
            (([det],), {}, "per frame"), ((det,), {"det_index": [0, 1]}, "image_index"), ((det[:, :3],), {"det_index": [0]}, "expected"),
            ((det,), {"det_index": [0.5]}, "integers"), (([many, det],), {}, "detections"), ((many, np.zeros(len(many), I32)), {}, "detections"),
            (([det, det],), {"count": 1.5}, "count"), (([det, det],), {"count": torch.tensor([1, 2])}, "count"), (([det, det],), {"count": torch.tensor(1.0)}, "count"),
            (([det, det],), {"frame_searched": [1]}, "frame_searched"), (([det, det],), {"frame_searched": [1, 0, 1]}, "frame_searched"),
            (([det, det],), {"accumulator": object()}, "accumulator"),
            ((torch.zeros((1, 4)),), {"det_index": None}, "det_index"), ((torch.zeros((1, 4)), torch.zeros(2, dtype=torch.int32)), {}, "det_index"),
            ((torch.zeros((4,)), torch.zeros(4, dtype=torch.int32)), {}, "det_boxes")):
        with pytest.raises(ValueError, match=what):
            tracker.update(*args, **kw)
    crowd = HeadTracker(_NoLaunch())
    crowd.start(frames, start, n_slots=_lib.TRACK_MAX_SLOTS + 1)  # without merge_iou start has no cap; update has the launch's
    with pytest.raises(ValueError, match="slots"):
        crowd.update([det, det])
    with pytest.raises(ValueError, match="slots"):
        HeadTracker(_NoLaunch(), merge_iou=0.5).start(frames, start, n_slots=_lib.TRACK_MAX_SLOTS + 1)
