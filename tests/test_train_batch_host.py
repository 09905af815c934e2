"""CPU: the host half of the device-built training batch (dataset.py) -- bbox math and RNG order, the restatement against the
reference's own FlameDataset (tests/golden/train_batch_golden.npz), collate packing and its refill rule, config parsing,
refusal of empty crops, and a loader path that never imports HIP."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import train_batch_restatement as rs
from dad_3dheads_amd import synthetic
from dad_3dheads_amd.dataset import FlameDataset, RawBatchCollate, ensure_bbox_boundaries, extend_bbox
from dad_3dheads_amd.resize_geometry import longest_max_size

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "train_batch_golden.npz")


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def st():
    return synthetic.load_static()


def test_bbox_math_and_rng_order(z):
    for name in z["cases"]:
        p = str(name) + "_"
        np.random.seed(int(z[p + "rng_seed"]))
        got = []
        for bbox, shape in zip(z[p + "anno_bbox"], z[p + "image_shapes"]):
            off = tuple(0.1 * np.random.uniform(size=4) + 0.05)
            got.append(ensure_bbox_boundaries(extend_bbox(np.array(bbox), off), tuple(shape[:2])))
        got = np.stack(got)
        assert got.dtype == np.int32 and np.array_equal(got, z[p + "bbox"]), name
    assert (z["lms_mean_68_edges_bbox"][:, 2] == 1).any()  # a 1-px-wide crop
    assert (z["lms_imagenet_68_anno_bbox"][:, :2] < 0).any()  # a negative corner


def test_restatement_against_golden(z, st):
    for name in z["cases"]:
        name = str(name)
        p = name + "_"
        kw = dict(zip(("corners", "weights"), rs.lmk68_tables(st))) if str(z[p + "subset"]) == "68" else {"index": st["lmk_445"]}
        for i, it in enumerate(rs.case_items(z, name, st)):
            frame = (it["image_shape"][0], *it["bbox"])
            full, px, norm, pres = rs.chain(it["vertices"], it["model_view"], it["projection"], frame, 256, str(z[p + "mode"]), **kw)
            w, h = it["bbox"][2:]
            mag = max(1.0, 256 / w, 256 / h) if str(z[p + "mode"]) == "resize" else max(1.0, 256 / max(w, h))
            assert np.abs(px - z[p + "subset_px"][i]).max() <= 1e-3 * mag, (name, i)
            assert np.abs(full[:: int(z["full_stride"])] - z[p + "full"][i]).max() <= 1e-3 * mag, (name, i)
            assert np.abs(norm - z[p + "landmarks"][i]).max() <= 1e-3 * mag / 256, (name, i)
            assert np.array_equal(pres, z[p + "presence"][i]), (name, i)
            # ... and a bound measured against the reference, not a constant: the restatement lies no further from the float64
            # chain than 3x the golden does (both sum the same 4-term products, in different orders: the same error distribution,
            # not the same maximum over ~5000 points; DESIGN.md 4.10 holds the measured ratios, 1.8 at the worst)
            full64, px64, _, _ = rs.chain64(it["vertices"], it["model_view"], it["projection"], frame, 256, str(z[p + "mode"]), **kw)
            stride = int(z["full_stride"])
            for what, mine, gold, exact in (("full", full[::stride], z[p + "full"][i], full64[::stride]), ("subset_px", px, z[p + "subset_px"][i], px64)):
                d_mine, d_gold = np.abs(mine - exact).max(), np.abs(gold - exact).max()
                print(f"{name} item {i} {what}: restated {d_mine:.3g} px, golden {d_gold:.3g} px, ratio {d_mine / d_gold if d_gold else 0:.2f}")
                assert d_mine <= 3 * d_gold, (name, i, what, d_mine, d_gold)


# ---- the cases of tests/gt_keypoints_cases.py can tell a wrong kernel from a right one --------------------------------------------
def _fused_mat_points(m, p):
    """(b): product and add in float64, rounded once."""
    return (np.float64(p) @ np.float64(m).T).astype(np.float32)


def mutated_chain(mutation):
    """`rs.chain` with one plausible mistake of a kernel restated into it (the letters of MUTATIONS)."""
    F = np.float32

    def chain(vertices, model_view, projection, frame, size, mode, index=None, corners=None, weights=None):
        height, cx, cy, w, h, top, left = (int(v) for v in frame[:7])
        mat = _fused_mat_points if mutation == "b" else rs._mat_points
        v = np.asarray(vertices, F)
        wh = mat(model_view, np.concatenate([v, np.ones_like(v[:, :1])], 1))

        def project(pts):
            c = mat(projection, pts)
            x, y = c[:, 0] / c[:, 3], c[:, 1] / c[:, 3]
            y = F(height) - (y + F(cy)) if mutation == "i" else (F(height) - y) - F(cy)
            return np.stack([x - F(cx), y], -1).astype(F)

        if index is None and corners is None:
            xy_sub = np.zeros((0, 2), F)
        elif index is not None:
            xy_sub = project(rs.rows(wh, index))
        else:
            wt, tri = weights.astype(F), rs.rows(wh, corners)  # [K,3 corners,4]
            if mutation == "a":  # the combination of the projections
                p = [project(tri[:, j]) for j in range(3)]
                xy_sub = ((p[0] * wt[:, 0, None] + p[1] * wt[:, 1, None]) + p[2] * wt[:, 2, None]).astype(F)
            else:
                if mutation == "b":
                    sub = (np.float64(tri) * np.float64(wt)[:, :, None]).sum(1).astype(F)
                else:
                    sub = ((tri[:, 0] * wt[:, 0, None] + tri[:, 1] * wt[:, 1, None]) + tri[:, 2] * wt[:, 2, None]).astype(F)
                if mutation != "j":
                    sub[:, 3] = 1
                xy_sub = project(sub)

        def resize(xy):
            x, y = xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64)
            if mode == "longest_max_size":
                s = size / max(h, w)
                s = np.float64(F(s)) if mutation == "c" else s
                px, py = (top, left) if mutation == "g" else (left, top)
                return np.stack([x * s + px, y * s + py], -1).astype(F)
            sx, sy = size / w, size / h
            if mutation == "c":
                sx, sy = np.float64(F(sx)), np.float64(F(sy))
            if mutation == "h":
                sx, sy = sy, sx
            return np.stack([x * sx, y * sy], -1).astype(F)

        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            sub_px = resize(xy_sub)
            if mutation == "e":
                pres = (0 <= xy_sub[:, 0]) & (xy_sub[:, 0] <= w) & (0 <= xy_sub[:, 1]) & (xy_sub[:, 1] <= h)
            elif mutation == "f":
                pres = rs.presence(sub_px, size, size)
            else:
                pres = rs.presence(xy_sub, w, h)
            norm = sub_px * (F(1) / F(size)) if mutation == "d" else sub_px / F(size)
            return resize(project(wh)), sub_px, norm.astype(F), pres

    return chain


# mutation -> (what a kernel would have got wrong, the cases that must catch it, the outputs in which they do)
MUTATIONS = {
    None: ("nothing: the mutant machinery itself restates rs.chain", (), ()),
    "a": ("the barycentric combination after the projection, not before", ("posed-barycentric-longest_max_size-256-5023-68",), (1, 2)),
    "b": ("4-term sums and the barycentric sum fused", ("posed-index-resize-255-300-445", "posed-barycentric-resize-300-189-68"), (0, 1, 2)),
    "c": ("the resize scale held in fp32", ("posed-index-longest_max_size-256-188-68", "posed-barycentric-resize-300-5023-445"), (0, 1, 2)),
    "d": ("subset_norm as a multiply by the reciprocal", ("posed-index-longest_max_size-255-5023-68", "posed-barycentric-resize-300-5023-68"), (2,)),
    "e": ("presence with <=", ("edges-index-longest_max_size-256", "edges-barycentric-resize-255"), (3,)),
    "f": ("presence on the resized point against out_size", ("edges-index-longest_max_size-256", "edges-barycentric-longest_max_size-255"), (3,)),
    "g": ("pad_top and pad_left swapped", ("posed-index-longest_max_size-256-1-1", "edges-barycentric-longest_max_size-256"), (0, 1, 2)),
    "h": ("sx and sy swapped in resize mode", ("posed-barycentric-resize-255-1-1", "edges-index-resize-256"), (0, 1, 2)),
    "i": ("y = H - (y + crop_y) instead of (H - y) - crop_y", ("posed-index-longest_max_size-256-5023-445", "batch-70"), (0, 1, 2)),
    "j": ("w := 1 omitted after the combination", ("homogeneous-barycentric",), (1, 2)),
}


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_cases_tell_a_mutated_chain_from_the_chain(mutation):
    """For every mistake, the cases named for it have an output word that differs from rs.chain -- in each of the outputs named.
    The GPU test holds the kernel to rs.chain on these very inputs, so a kernel with that mistake fails it."""
    import gt_keypoints_cases as gk

    _, names, outputs = MUTATIONS[mutation]
    chain = mutated_chain(mutation)
    if mutation is None:  # every case, bad ids and infinities included
        for case in gk.all_cases():
            for got, want in zip(gk.evaluate(case, chain), gk.expected(case)):
                assert gk.same_bits(got, want), case["name"]
        return
    for name in names:
        case = gk.by_name(name)
        got, want = gk.evaluate(case, chain), gk.expected(case)
        for o in outputs:
            assert not gk.same_bits(got[o], want[o]), (mutation, name, o)


def test_gt_keypoints_cases_hold_what_they_are_for():
    """The properties of the shared inputs that the GPU test relies on, certified here."""
    import gt_keypoints_cases as gk

    names = [c["name"] for c in gk.all_cases()]
    assert len(set(names)) == len(names) and len(gk.posed_cases()) == 2 * 2 * 3 * 8
    for case in gk.posed_cases():
        fr = case["frames"]
        assert (fr[:, 1:3] < 0).any() and (fr[:, 3] == 1).any() and (fr[:, 3] > fr[:, 4]).any() and (fr[:, 3] < fr[:, 4]).any()
        assert (fr[:, 5] > 0).any() and (fr[:, 6] > 0).any()  # pads on either side
    full, px, norm, pres = gk.expected(gk.by_name("posed-barycentric-longest_max_size-256-5023-68"))
    assert np.isfinite(full).all() and pres[0].any() and not pres[0].all() and pres[2].any() and not pres[2].all()
    for case in gk.posed_cases():  # no vertex: every id is out of range
        if case["vertices"].shape[1] == 0:
            out = gk.expected(case)
            assert out[0].shape == (3, 0, 2) and np.isnan(out[1]).all() and np.isnan(out[2]).all() and not out[3].any()
    pres = gk.expected(gk.batch_case())[3]
    assert len(pres) == 70 and pres.any(1).sum() > 20 and (~pres).any(1).sum() > 20
    for case in gk.edge_cases():  # the restatement agrees with the table written by hand
        assert np.array_equal(gk.expected(case)[3], case["presence"]), case["name"]
        pts = case["points"]
        for edge in (0.0, gk.up(0), gk.down(0), gk.EDGE_W, gk.up(gk.EDGE_W), gk.down(gk.EDGE_W)):
            assert (pts[:, 0] == np.float32(edge)).any(), edge
        for edge in (0.0, gk.up(0), gk.down(0), gk.EDGE_H, gk.up(gk.EDGE_H), gk.down(gk.EDGE_H)):
            assert (pts[:, 1] == np.float32(edge)).any(), edge
        assert np.signbit(pts[:, 0]).any() and np.signbit(pts[pts[:, 1] == 0, 1]).any()  # -0.0 among them
    for case in gk.bad_id_cases():
        full, px, norm, pres = gk.expected(case)
        clean = gk.evaluate(case, sub=case["clean"])
        bad = case["bad"]
        assert bad.sum() == 4 and not bad[0] and not bad[-1] and not (bad[1:] & bad[:-1]).any()  # between good neighbours
        assert np.isnan(px[:, bad]).all() and np.isnan(norm[:, bad]).all() and not pres[:, bad].any()
        assert np.isfinite(clean[1]).all() and clean[3][:, bad].any()  # a good id there gives a point, some of them present
        for o in range(1, 4):
            assert gk.same_bits(np.ascontiguousarray(clean[o][:, ~bad]), np.ascontiguousarray(gk.expected(case)[o][:, ~bad]))
    for case in gk.special_cases():
        if case["name"].startswith("camera-plane"):
            _, px, _, pres = gk.expected(case)
            k = 5  # the subset runs backwards: row 5 is the mirrored point (w = -0.5), row 6 the one in front
            assert np.isfinite(px[0, k:]).all() and pres[0, k:].all(), "the mirrored point is finite and inside its crop"
            assert np.isinf(px[0, 4]).all() and np.isneginf(px[0, 3, 0]) and np.isnan(px[0, 3, 1]) and np.isnan(px[0, 2]).all()
            assert not pres[0, :k].any() and not pres[1:].any()  # w = 2^-23 (far outside), w = 0, and the items with an infinity in a matrix: absent


def test_exact_edges_are_absent(z):
    p = "resize_mean_445_"
    i = list(z[p + "kinds"]).index("ortho_edges")
    # the first four subset points sit exactly on the left, right, top and bottom edges; the next two one pixel inside
    assert list(z[p + "presence"][i][:6]) == [False, False, False, False, True, True]


def _items(z, st, name="lms_imagenet_68"):
    return rs.case_items(z, name, st)


def test_collate_packing_and_refill(z, st):
    items = _items(z, st)
    raw = RawBatchCollate(256)([items[0], None, items[1], items[2], None])
    b = 5
    assert raw["crops"].dtype == torch.uint8 and raw["crop_descs"].shape == (b, 8) and raw["frames"].shape == (b, 8)
    order = [items[0], items[1], items[2], items[0], items[1]]  # collate_skip_none: refilled from the front
    assert raw["SAMPLE_INDEX_KEY"].tolist() == [it["SAMPLE_INDEX_KEY"] for it in order]
    assert raw["IMAGE_FILENAME_KEY"] == [it["IMAGE_FILENAME_KEY"] for it in order]
    for i, it in enumerate(order):
        off, h, w, nh, nw, top, left, stride = raw["crop_descs"][i].tolist()
        assert (h, w, stride) == (it["image"].shape[0], it["image"].shape[1], 3 * it["image"].shape[1])
        assert (nh, nw, top, left) == longest_max_size(h, w, 256)
        assert np.array_equal(raw["crops"][off: off + h * w * 3].numpy().reshape(h, w, 3), it["image"])
        assert raw["frames"][i].tolist() == [int(it["image_shape"][0]), *it["bbox"].tolist(), top, left, 0]
        assert torch.equal(raw["vertices"][i], torch.from_numpy(it["vertices"]))
    assert raw["INPUT_BBOX_KEY"].dtype == torch.int32 and raw["SAMPLE_INDEX_KEY"].dtype == torch.int64
    resize = RawBatchCollate(256, "resize")([items[0]])
    assert resize["crop_descs"][0, 3:7].tolist() == [256, 256, 0, 0]
    with pytest.raises(ValueError):
        RawBatchCollate(256)([None, None])


def test_config_parsing(z, st, tmp_path):
    cfg68 = rs.case_config(z, "lms_imagenet_68", str(tmp_path / "a"), st)
    assert FlameDataset([], cfg68).keypoints_indices is None
    cfg445 = rs.case_config(z, "resize_mean_445", str(tmp_path / "b"), st)
    ds = FlameDataset([], cfg445)
    assert ds.keypoints_indices == [int(v) for v in st["lmk_445"]] and ds.resize_mode == "resize" and ds.normalize == "mean"
    with pytest.raises(ValueError, match="num_classes"):
        FlameDataset([], dict(cfg445, num_classes=68))
    with pytest.raises(KeyError):
        FlameDataset([], dict(cfg68, transform={"resize_mode": "crop"}))
    with pytest.raises(KeyError):
        FlameDataset([], dict(cfg68, transform={"normalize": "none"}))


def _write_item(tmp_path, st, bbox, shape=(120, 90, 3)):
    import json

    from PIL import Image

    Image.fromarray(rs.image(3, *shape[:2])).save(tmp_path / "a.png")
    with open(tmp_path / "a.json", "w") as f:
        json.dump({"vertices": st["template_geo"].tolist(), "model_view_matrix": np.eye(4).tolist(),
                   "projection_matrix": np.eye(4).tolist()}, f)
    return [{"img_path": "a.png", "bbox": bbox, "annotation_path": "a.json"}]


def test_empty_crop_is_refused(st, tmp_path):
    cfg = {"dataset_root": str(tmp_path), "img_size": 256, "stride": 4, "num_classes": 68,
           "keypoints": {"2d_subset_name": "multipie_keypoints"}}
    ds = FlameDataset(_write_item(tmp_path, st, [200.0, 10.0, 20.0, 30.0]), cfg)  # right of the 90-px-wide image
    with pytest.raises(ValueError, match="item 0"):
        ds[0]
    ok = FlameDataset(_write_item(tmp_path, st, [10.5, 12.25, 40.0, 50.0]), cfg)[0]
    assert ok["image"].flags["C_CONTIGUOUS"] and ok["image"].shape[:2] == tuple(ok["bbox"][[3, 2]])


def test_a_forked_child_destroys_no_device_handle():
    """A DataLoader worker is a fork of the training process: when its collector meets garbage of the parent that holds a native
    handle, `__del__` must not free device state the child does not own. In the creating process it still does, once."""
    from dad_3dheads_amd.flame import FLAMELayer
    from dad_3dheads_amd.rccl import RcclAllGather
    from dad_3dheads_amd.Sim3DR.mesh import Mesh
    from dad_3dheads_amd.uv_texture import UVMap

    calls = []

    class Lib:
        def __getattr__(self, name):
            return lambda h: calls.append((name, h))

    for cls, destroy in ((FLAMELayer, "dad3d_flame_destroy"), (Mesh, "dad3d_mesh_destroy"), (UVMap, "dad3d_uvmap_destroy")):
        for pid, want in ((os.getpid() + 1, []), (os.getpid(), [(destroy, 77)])):
            obj = object.__new__(cls)
            obj.__dict__.update(_handle=77, _lib=Lib(), _owner_pid=pid)
            del calls[:]
            obj.__del__()
            obj.__del__()  # the handle is gone after the first call
            assert calls == want, (cls.__name__, pid)
    for pid, want in ((os.getpid() + 1, 0), (os.getpid(), 1)):
        gather = object.__new__(RcclAllGather)
        del calls[:]
        gather.__dict__.update(_owner_pid=pid, destroy=lambda: calls.append("destroy"))
        gather.__del__()
        assert len(calls) == want, pid


def test_loader_path_never_imports_hip(st, tmp_path):
    """__getitem__ and the collate in a process where importing the HIP library or initialising the GPU fails."""
    _write_item(tmp_path, st, [10.5, 12.25, 40.0, 50.0])
    code = f"""
import sys, importlib.abc
class Block(importlib.abc.MetaPathFinder):
    def find_spec(self, name, path, target=None):
        if name.endswith("._lib") or name.endswith(".coder") or name.endswith(".predictor"):
            raise ImportError("HIP is not available in a loader worker: " + name)
sys.meta_path.insert(0, Block())
sys.path[:0] = [{ROOT!r}]
import torch
torch.cuda._lazy_init = lambda: (_ for _ in ()).throw(RuntimeError("GPU initialised in a loader worker"))
from dad_3dheads_amd.dataset import FlameDataset
ds = FlameDataset([{{"img_path": "a.png", "bbox": [10.5, 12.25, 40.0, 50.0], "annotation_path": "a.json"}}] * 3,
                  {{"dataset_root": {str(tmp_path)!r}, "img_size": 256, "num_classes": 68,
                    "keypoints": {{"2d_subset_name": "multipie_keypoints"}}}})
raw = ds.get_collate_fn()([ds[i] for i in range(3)])
assert raw["crops"].numel() > 0 and not any(m.endswith("._lib") for m in sys.modules)
print("ok")
"""
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr[-2000:]
