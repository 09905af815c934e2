"""Host: the cases of tests/raster_cases.py certified on the CPU, with the reference alone (`sim3dr_oracle`) -- what the GPU tests of
test_gpu_frames_fuzz.py claim to reach is reached, and the flags they predict follow from the reference's box and the documented pool.
Every claim is a count above zero; `pytest -s` prints the counts (they are quoted in the docstrings of the GPU tests)."""
import json
import math
import os

import numpy as np
import pytest

import raster_cases as RC
import render_frames_restatement as RF
import texture_occlusion_restatement as TO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raster_cases_digest.json")


def _c(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _unrolled_flat(v, t, seed=0):
    """One vertex per triangle corner and one flat random colour per triangle: the image shows which triangle won."""
    vu = _c(np.asarray(v)[np.asarray(t).reshape(-1)])
    tri = np.arange(3 * len(t), dtype=np.int32).reshape(-1, 3)
    col = np.repeat(np.random.default_rng(seed).uniform(0.05, 0.95, (len(t), 3)).astype(np.float32), 3, 0)
    return vu, tri, np.ascontiguousarray(col)


def tie_pixels(oracle, v, t, h, w):
    """Pixels of `_rasterize` whose winner changes when the triangles are listed in reverse: at least two triangles reach the winning
    depth there, and the index decides. The depth buffers of the two runs must agree."""
    vu, tri, col = _unrolled_flat(v, t)
    with np.errstate(all="ignore"):
        a, da = oracle.rasterize(vu, tri, col, height=h, width=w, channel=3, return_depth=True)
        b, db = oracle.rasterize(vu, np.ascontiguousarray(tri[::-1]), col, height=h, width=w, channel=3, return_depth=True)
    assert np.array_equal(da, db, equal_nan=True)
    return int((a != b).any(-1).sum())


def edge_pixels(oracle, v, t, h, w):
    """Pixels where the strict interior test of `_rasterize` and the `>=` of `_rasterize_triangles` disagree on the winning depth: the
    pixel's centre lies on an edge (u == 0 or v == 0) of a triangle that would otherwise win or cover it."""
    with np.errstate(all="ignore"):
        _, strict = oracle.rasterize(_c(v), t, np.zeros_like(_c(v)), height=h, width=w, channel=3, return_depth=True)
        loose, _, _ = oracle.rasterize_triangles(_c(v), t, h, w)
    return int((strict != loose).sum())


def mixed_sign_pixels(oracle, v, t, h, w):
    """Pixels where a fragment of positive and one of negative depth compete: the largest depth is > 0 and the smallest < 0."""
    neg = _c(v).copy()
    neg[:, 2] = -neg[:, 2]
    with np.errstate(all="ignore"):
        hi, cover, _ = oracle.rasterize_triangles(_c(v), t, h, w)
        lo, cover2, _ = oracle.rasterize_triangles(neg, t, h, w)
    return int(((cover >= 0) & (cover2 >= 0) & (hi > 0) & (-lo < 0)).sum())


def zero_area_triangles(v, t):
    """Triangles whose `dot00 * dot11 - dot01 * dot01` is exactly 0 in the reference's float32 arithmetic (inverDeno = 0)."""
    p = _c(v)[np.asarray(t)][:, :, :2]
    a, b = p[:, 2] - p[:, 0], p[:, 1] - p[:, 0]
    with np.errstate(all="ignore"):
        d00 = a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]
        d01 = a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]
        d11 = b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]
        return int((d00 * d11 - d01 * d01 == 0).sum())


def test_build_case_returns_what_it_returned_before_the_move():
    with open(GOLDEN) as f:
        pinned = json.load(f)
    assert sorted(pinned) == sorted(f"{p}:{s}" for p in RC.PROFILES for s in RC.DIGEST_SEEDS)
    for key, digest in pinned.items():
        profile, seed = key.split(":")
        assert RC.case_digest(RC.build_case(int(seed), profile)) == digest, key


def test_each_profile_shows_what_it_claims(sim3dr_oracle):
    counts = {p: dict(ties=0, edges=0, zero_area=0, over32=0, over64=0, mixed=0) for p in RC.PROFILES}
    for p in RC.PROFILES:
        for seed in RC.SEEDS:
            v, t, _, _, h, w, _ = RC.build_case(seed, p)
            c = counts[p]
            _, o32, o64 = RC.tile_entries(v, t, h, w)
            c["over32"] += o32
            c["over64"] += o64
            c["zero_area"] += zero_area_triangles(v, t)
            c["mixed"] += mixed_sign_pixels(sim3dr_oracle, v, t, h, w)
            if p in ("tie_planes", "layers", "pixel_centres"):
                c["ties"] += tie_pixels(sim3dr_oracle, v, t, h, w)
                c["edges"] += edge_pixels(sim3dr_oracle, v, t, h, w)
        print(p, counts[p])
    assert counts["tie_planes"]["ties"] > 0 and counts["layers"]["ties"] > 0
    assert counts["pixel_centres"]["edges"] > 0
    assert counts["slivers"]["zero_area"] > 0
    assert all(c["over32"] > 0 and c["over64"] > 0 for c in counts.values())
    assert sum(c["mixed"] > 0 for c in counts.values()) > 0


def test_the_scenes_meet_the_admission_conditions():
    flagged, with_capacity, capacity_then_admitted = {p: 0 for p in RC.PROFILES}, 0, 0
    for p in RC.PROFILES:
        for seed in RC.SEEDS:
            sc = RC.scene(seed, p)
            shapes = [b.shape for b in sc["bgs"]]
            assert len(set(shapes)) == 3 and shapes[1] == (64, 64, 3) and shapes[0][0] % 64 and shapes[0][1] % 64
            assert all(max(s[:2]) <= 280 for s in shapes) and len(sc["t"]) <= 1536 and len(sc["verts"]) == 3
            assert len(set(sc["image_index"])) == 2  # two heads share a frame
            flags = RC.scene_flags(sc)
            assert RC.FRAME_FLAG_INDEX not in flags
            flagged[p] += any(flags)
            cap = [k for k, f in enumerate(flags) if f == RC.FRAME_FLAG_CAPACITY]
            with_capacity += bool(cap)
            capacity_then_admitted += bool(cap) and any(f == 0 for f in flags[cap[0] + 1:])
    print("scenes with a flagged head per profile", flagged, "with CAPACITY", with_capacity, "then a later head admitted", capacity_then_admitted)
    assert all(2 * n <= len(RC.SEEDS) for n in flagged.values())
    assert with_capacity >= 2 and capacity_then_admitted >= 1


def test_admitted_states_the_documented_rule():
    I, C = RC.FRAME_FLAG_INDEX, RC.FRAME_FLAG_CAPACITY
    assert RC.admitted([5, 5, 5], [0, 1, 0], 2, 15) == [0, 0, 0]               # all fit together
    assert RC.admitted([5, 5, 6], [0, 1, 0], 2, 15) == [0, 0, C]               # ascending order
    assert RC.admitted([9, 7, 6], [0, 1, 0], 2, 15) == [0, C, 0]               # a later head still fits
    assert RC.admitted([16, 7, 6], [0, 1, 0], 2, 15) == [C, 0, 0]
    assert RC.admitted([99, 7, 6], [2, -1, 0], 2, 15) == [I, I, 0]             # a head without a frame needs nothing
    assert RC.admitted([5, 99, 11], [0, 7, 0], 2, 15) == [0, I, C]
    assert RC.admitted([], [], 2, 0) == []


def _brute_force(v, t, h, w):
    """Per triangle the pixels of its clipped box, one by one, with Python's own ceil / floor: tiles touched, pixels per tile."""
    entries = over32 = over64 = 0
    for tri in np.asarray(t):
        xs, ys = [float(v[i, 0]) for i in tri], [float(v[i, 1]) for i in tri]
        x0, x1 = max(math.ceil(min(xs)), 0), min(math.floor(max(xs)), w - 1)
        y0, y1 = max(math.ceil(min(ys)), 0), min(math.floor(max(ys)), h - 1)
        per_tile = {}
        for y in range(y0, y1 + 1):
            for x in range(x0, x1 + 1):
                per_tile[(x // 64, y // 64)] = per_tile.get((x // 64, y // 64), 0) + 1
        entries += len(per_tile)
        over32 += bool(per_tile) and max(per_tile.values()) > 32
        over64 += bool(per_tile) and max(per_tile.values()) > 64
    return entries, over32, over64


@pytest.mark.parametrize("seed,profile,shape", [(5, "tile_straddle", None), (6, "slivers", (70, 130)), (7, "mixed_sizes", (64, 64))])
def test_tile_entries_agrees_with_a_brute_force_count(seed, profile, shape):
    v, t, _, _, h, w, _ = RC.build_case(seed, profile)
    h, w = shape or (h, w)
    want = _brute_force(v, t[:60], h, w)
    assert RC.tile_entries(v, t[:60], h, w) == want and want[0] > 0 and want[1] >= want[2] > 0


def test_tile_entries_on_coordinates_no_int_holds():
    v = np.array([[3e38, 5, 0], [-3e38, 9, 0], [7, 1e7, 0], [10.5, 10.5, 0], [20.5, 3.25, 0], [float("nan"), 4, 0]], np.float32)
    # 3e38 as the maximum converts to INT_MIN (no box); -3e38 as the minimum clips to 0; 1e7 clips to the frame; NaN: std::min / std::max
    # keep their first argument unless the comparison holds
    t = np.array([[0, 3, 4], [1, 3, 4], [2, 3, 4], [5, 3, 4], [3, 4, 5]], np.int32)
    x0, x1, y0, y1, vis = RC.tri_boxes(v, t, 100, 100)
    assert vis.tolist() == [False, True, True, False, True]
    assert (x0[1], x1[1], y0[1], y1[1]) == (0, 20, 4, 10) and (x0[2], x1[2], y0[2], y1[2]) == (7, 20, 4, 99)
    assert (x0[4], x1[4], y0[4], y1[4]) == (11, 20, 4, 10)
    assert RC.tile_entries(v, t, 100, 100) == (1 + 2 + 1, 3, 3)


def test_whole_box_frames_are_covered_by_the_reference(sim3dr_oracle):
    wb = RC.whole_box_frames()
    shapes = wb["shapes"]
    assert len(shapes) == 4 * 64 and {s for s in shapes if s[0] != 64 or s[1] <= 64} == {(bh, bw) for bh in (1, 63, 64) for bw in range(1, 65)}
    assert {s[1] for s in shapes if s[1] > 64} == set(range(65, 129))
    bgs = [np.full((h, w, 3), RC.WHOLE_BOX_BG, np.uint8) for h, w in shapes]
    want = RF.expected_frames(sim3dr_oracle, bgs, wb["verts"], wb["t"], wb["cols"], wb["image_index"])
    assert all((f != RC.WHOLE_BOX_BG).all() for f in want)  # every byte of every frame is drawn
    maps, window, flags = TO.expected_depth_frames(sim3dr_oracle, shapes, wb["verts"], wb["t"], wb["image_index"], 128)
    assert not flags.any() and all(np.isfinite(m).all() and m.shape == shapes[f] for m, f in zip(maps, wb["image_index"]))
    needs = [RC.tile_entries(v, wb["t"], *shapes[f]) for v, f in zip(wb["verts"], wb["image_index"])]
    assert all(n[0] == (2 if shapes[f][1] > 64 else 1) for n, f in zip(needs, wb["image_index"]))
    assert not any(RC.admitted([n[0] for n in needs], wb["image_index"], len(shapes), RC.pool_entries(1, len(needs))))
    later = [k for k in range(len(shapes), len(wb["verts"]))]
    assert len(later) >= 30 and all(wb["verts"][k][:, 2].max() < wb["verts"][wb["image_index"][k]][:, 2].min() for k in later)
    print("whole boxes: frames", len(shapes), "heads", len(needs), "boxes over 32 pixels", sum(n[1] for n in needs), "over 64", sum(n[2] for n in needs))


def test_directed_pairs_overlap_in_the_reference(sim3dr_oracle):
    h, w = RC.PAIR_FRAME
    for table in (RC.DEPTH_PAIRS, RC.FRAME_PAIRS):
        for name, v, col in RC.directed_pairs(table):
            x0, x1, y0, y1, vis = RC.tri_boxes(v, RC.PAIR_TRIANGLES, h, w)
            side = int(name.split("side ")[1].split()[0])
            if "zero_area" not in name:
                assert vis.all() and ((x1 - x0 + 1) * (y1 - y0 + 1)).tolist() == [side * side] * 2, name
            # both triangles cover a pixel: each alone under the depth raster's test
            cover = [sim3dr_oracle.rasterize_triangles(_c(v * [1, 1, 0]), np.ascontiguousarray(RC.PAIR_TRIANGLES[i:i + 1]), h, w)[1] >= 0 for i in (0, 1)]
            assert (cover[0] & cover[1]).sum() >= 1, name
            assert zero_area_triangles(v, RC.PAIR_TRIANGLES) == ("zero_area" in name), name


def test_directed_pairs_show_their_winner_in_the_reference(sim3dr_oracle):
    h, w = RC.PAIR_FRAME
    # depth maps: the smaller z wins, whatever the order of the triangles
    pairs = RC.directed_pairs(RC.DEPTH_PAIRS)
    maps, _, flags = TO.expected_depth_frames(sim3dr_oracle, [RC.PAIR_FRAME], np.stack([v for _, v, _ in pairs]), RC.PAIR_TRIANGLES,
                                              [0] * len(pairs), 32)
    assert not flags.any()
    by_name = {name: wm for (name, _, _), wm in zip(pairs, maps)}
    for name, wm in by_name.items():
        values = set(np.round(wm[np.isfinite(wm)].astype(np.float64), 3).tolist())  # a flat plane's depth rounds in the last place
        expect = {"mixed_signs": {-1.0, 1.0}, "both_negative": {-3.0, -2.0}, "two_zeros": {0.0},
                  "zero_area": {1.5, float(name.split()[3]) if name.startswith("zero_area") else 0.0}}
        for key, want in expect.items():
            if name.startswith(key):
                assert values == want, (name, values)
        if name.startswith("threshold"):  # the plane at 1e8f is covered where its products round down, the one below it nearly everywhere
            assert values and max(values) < 1e8 and np.isinf(wm[4:6, :2]).any(), name
        if "swap False" in name:
            assert np.array_equal(wm, by_name[name.replace("swap False", "swap True")]), name
    # frames: the larger z wins; only the tie depends on the order
    pairs = RC.directed_pairs(RC.FRAME_PAIRS)
    bgs = [np.full((h, w, 3), 255, np.uint8) for _ in pairs]
    want = RF.expected_frames(sim3dr_oracle, bgs, np.stack([v for _, v, _ in pairs]), RC.PAIR_TRIANGLES, np.stack([c for _, _, c in pairs]),
                              list(range(len(pairs))))
    by_name = {name: f for (name, _, _), f in zip(pairs, want)}
    for name, f in by_name.items():
        assert (f != 255).any(), name
        if "swap False" in name and not name.startswith("threshold"):  # the two planes at the threshold round onto each other: ties too
            assert np.array_equal(f, by_name[name.replace("swap False", "swap True")]) != name.startswith("two_zeros"), name
