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
