"""CPU: the lifting rule of the device annotation reader as tests/annotation_restatement.py states it, against `FlameDataset._load_mesh`,
and the host half of the file form: `FileBatchCollate`'s packing and the bboxes of a `"files"` dataset."""
import json

import numpy as np
import pytest
import torch

import annotation_restatement as R
from dad_3dheads_amd import _lib
from dad_3dheads_amd.dataset import FileBatchCollate, FlameDataset

SWEEP = [(1, 160), (7, 120), (85, 40), (5023, 4)]  # (n_verts, documents): a few hundred in all


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("n_verts,count", SWEEP)
def test_must_lift_sweep_lifts_and_equals_load_mesh(lib, n_verts, count):
    """Every document of the seeded sweep lifts (a condition, not a measurement: zero may be flagged), and what lifts is `_load_mesh`."""
    flagged = 0
    for doc in R.sweep(100 + n_verts, n_verts, count):
        status, v, m, p = R.restate(doc, n_verts, lib)
        flagged += status != 0
        if status == 0:
            rv, rm, rp = R.load_mesh_of(doc)
            assert _same(v, rv) and _same(m, rm) and _same(p, rp)
    assert flagged == 0


def test_load_mesh_of_is_load_mesh(tmp_path):
    doc = R.sweep(3, 7, 1)[0]
    path = tmp_path / "a.json"
    path.write_bytes(doc)
    for a, b in zip(FlameDataset._load_mesh(str(path)), R.load_mesh_of(doc)):
        assert _same(a, b)


def test_special_numbers_are_numpys(lib):
    """ints above 2^24, -0.0 and the int -0, 1e300 (inf in float32): the cast `np.array(list, float32)` makes."""
    v = "[[16777217,-0.0,1e300],[-0,9007199254740992,-1e300],[0.1,1.0000000596046448,5e-324e0]]".replace("5e-324e0", "1e-46")
    doc = ('{"vertices":%s,"model_view_matrix":%s,"projection_matrix":%s}' % ((v,) + R.base_parts()[1:])).encode()
    status, got, _, _ = R.restate(doc, 3, lib)
    assert status == 0
    ref = R.load_mesh_of(doc)[0]
    assert _same(got, ref)
    assert np.isinf(ref[0, 2]) and np.signbit(ref[0, 1]) and not np.signbit(ref[1, 0]) and ref[0, 0] == 16777216.0 and ref[2, 2] == 0.0


@pytest.mark.parametrize("n_verts", [1, 2, 7])
def test_named_bad_documents_are_flagged(lib, n_verts):
    docs = R.bad_documents(n_verts)
    for must in ("duplicate key", "duplicate extra key", "escaped key", "nested object", "one row fewer", "one row more", "row of 2", "row of 4", "flat matrix",
                 "NaN", "20 digits", "trailing comma in array", "bare word", "high byte", "top-level array", "truncated"):
        assert must in docs
    for name, doc in docs.items():
        assert R.restate(doc, n_verts, lib)[0] != 0, name


def test_the_flag_says_what_is_wrong(lib):
    docs = R.bad_documents(2)
    for name, flag in (("duplicate key", R.KEYS), ("duplicate extra key", R.KEYS), ("long key", R.KEYS), ("too many keys", R.KEYS),
                       ("nested object", R.GRAMMAR), ("row of 4", R.SHAPE), ("20 digits", R.NUMBER),
                       ("high byte", R.STRING), ("bare word", R.GRAMMAR), ("flat matrix", R.SHAPE), ("trailing comma in object", R.GRAMMAR)):
        assert R.restate(docs[name], 2, lib)[0] == flag, name
    for name in ("GRAMMAR", "KEYS", "SHAPE", "NUMBER", "STRING", "RANGE"):
        assert getattr(R, name) == getattr(_lib, "ANNOTATION_FLAG_" + name)
    assert (R.MAX_RUN, R.MAX_WORD) == (_lib.ANNOTATION_MAX_BACKSLASH_RUN, _lib.ANNOTATION_MAX_WORD_BYTES)
    assert (R.MAX_KEY, R.MAX_KEYS) == (_lib.ANNOTATION_MAX_KEY_BYTES, _lib.ANNOTATION_MAX_KEYS)


def test_a_lifted_document_never_differs_from_json_load(lib):
    """Random damage to a good document: wherever the restatement still lifts, json.load reads the same arrays."""
    rng = np.random.default_rng(9)
    good = R.sweep(4, 3, 1)[0]
    lifted = 0
    for _ in range(400):
        doc = bytearray(good)
        for _ in range(int(rng.integers(1, 3))):
            at = int(rng.integers(len(doc)))
            kind = int(rng.integers(3))
            if kind == 0:
                doc[at] = int(rng.choice(list(b'[]{},:"\\ 0123456789.-eE\n\x00\xe9tn')))
            elif kind == 1:
                del doc[at]
            else:
                doc.insert(at, int(rng.choice(list(b'[]{},:"\\ 0.-e'))))
        status, v, m, p = R.restate(bytes(doc), 3, lib)
        if status == 0:
            lifted += 1
            rv, rm, rp = R.load_mesh_of(bytes(doc))
            assert _same(v, rv) and _same(m, rm) and _same(p, rp)
    assert lifted > 0


def test_entry_validates_before_device_work(lib):
    assert lib.dad3d_annotation_parse(None, 0, None, None, 0, 5023, None, None, None, None, 0, None) == _lib.OK  # an empty batch
    assert lib.dad3d_annotation_parse(None, 16, None, None, 1, 5023, None, None, None, None, 0, None) == _lib.E_INVALID
    assert b"null" in lib.dad3d_last_error()
    buf = np.zeros(64, np.uint8)
    ptr = buf.ctypes.data + (-buf.ctypes.data % 16)
    assert lib.dad3d_annotation_parse(ptr + 1, 16, ptr, ptr, 1, 5023, ptr, ptr, ptr, ptr, 0, None) == _lib.E_INVALID
    assert b"aligned" in lib.dad3d_last_error()
    assert lib.dad3d_annotation_parse(ptr, 16, ptr, ptr, 1, 0, ptr, ptr, ptr, ptr, 0, None) == _lib.E_INVALID
    assert lib.dad3d_annotation_parse(ptr, 16, ptr, ptr, 70000, 1, ptr, ptr, ptr, ptr, 0, None) == _lib.E_INVALID
    assert lib.dad3d_annotation_parse(ptr, -1, ptr, ptr, 1, 1, ptr, ptr, ptr, ptr, 0, None) == _lib.E_INVALID


# ---- the file form on the host -------------------------------------------------------------------------------------------------------

CFG = {"img_size": 256, "stride": 4, "num_classes": 68, "keypoints": {"2d_subset_name": "multipie_keypoints"},
       "transform": {"resize_mode": "longest_max_size"}}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from PIL import Image

    root = tmp_path_factory.mktemp("files")
    rng = np.random.default_rng(1)
    anno = []
    for i, ((h, w), bbox) in enumerate([((40, 50), [5, 6, 30, 20]), ((64, 33), [20, 30, 30, 60]), ((7, 90), [-3, 0, 40, 7]), ((30, 30), [2, 2, 9, 9])]):
        img = Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        if i == 3:
            img = img.convert("P")  # a palette: the worker decodes it
        img.save(root / f"img_{i}.png")
        (root / f"mesh_{i}.json").write_bytes(R.sweep(i, 2, 1)[0])
        anno.append({"img_path": f"img_{i}.png", "bbox": bbox, "annotation_path": f"mesh_{i}.json"})
    return dict(CFG, dataset_root=str(root)), anno


def test_files_dataset_gives_the_raw_bboxes(files):
    cfg, anno = files
    raw, by_file = FlameDataset(anno, cfg), FlameDataset(anno, cfg, item_form="files")
    assert isinstance(by_file.get_collate_fn(), FileBatchCollate) and not isinstance(raw.get_collate_fn(), FileBatchCollate)
    np.random.seed(7)
    a = [raw[i] for i in range(len(anno))]
    np.random.seed(7)
    b = [by_file[i] for i in range(len(anno))]
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x["bbox"], y["bbox"]) and y["bbox"].dtype == np.int32
        assert np.array_equal(x["image_shape"], y["image_shape"])
        assert (x["SAMPLE_INDEX_KEY"], x["IMAGE_FILENAME_KEY"]) == (y["SAMPLE_INDEX_KEY"], y["IMAGE_FILENAME_KEY"])
        assert y["annotation"].tobytes() == open(cfg["dataset_root"] + f"/mesh_{i}.json", "rb").read()
        if i == 3:  # decoded by the worker, whole: the crop is the device's
            assert y["png"].size == 0 and y["decoded"].shape == (30, 30, 3)
            bx, by, bw, bh = x["bbox"]
            assert np.array_equal(y["decoded"][by:by + bh, bx:bx + bw], x["image"])
        else:
            assert y["decoded"] is None and y["png"].tobytes() == open(cfg["dataset_root"] + f"/img_{i}.png", "rb").read()
    # both forms draw the same count: the next draw is the same
    np.random.seed(7)
    [raw[i] for i in range(2)]
    after_raw = np.random.uniform()
    np.random.seed(7)
    [by_file[i] for i in range(2)]
    assert np.random.uniform() == after_raw
    with pytest.raises(ValueError, match="item_form"):
        FlameDataset(anno, cfg, item_form="jpeg")
    empty = [dict(anno[0], bbox=[60, 60, 5, 5])]
    for form in ("raw", "files"):
        with pytest.raises(ValueError, match="crops an empty image"):
            FlameDataset(empty, cfg, item_form=form)[0]


def test_file_collate_offsets_alignment_and_refill(files):
    cfg, anno = files
    ds = FlameDataset(anno, cfg, item_form="files")
    np.random.seed(3)
    items = [ds[i] for i in range(len(anno))]
    collate = ds.get_collate_fn()
    batch = collate(items)
    for key in ("png_files", "decoded_images", "annotations"):
        assert batch[key].dtype == torch.uint8 and batch[key].dim() == 1 and batch[key].numel() % 16 == 0
    assert all(isinstance(v, torch.Tensor) for k, v in batch.items() if k != "IMAGE_FILENAME_KEY")
    for table, key, field in (("png_table", "png_files", "png"), ("annotation_table", "annotations", "annotation")):
        t = batch[table].numpy()
        assert t.dtype == np.int64 and (t[:, 0] % 16 == 0).all()
        ends = t[:, 0] + (t[:, 1] + 15) // 16 * 16
        assert (t[1:, 0] == ends[:-1]).all() and ends[-1] == batch[key].numel()
        for i, it in enumerate(items):
            got = batch[key][t[i, 0]:t[i, 0] + t[i, 1]].numpy()
            assert got.tobytes() == it[field].tobytes()
            assert not batch[key][t[i, 0] + t[i, 1]:ends[i]].any()  # zero between the files
    assert batch["png_table"][3, 1] == 0 and batch["decoded_table"][3, 1] == 30 * 30 * 3 and (batch["decoded_table"][:3, 1] == 0).all()
    assert batch["png_table"][:3, 2:].tolist() == [[40, 50, 3], [64, 33, 3], [7, 90, 3]]
    off = int(batch["decoded_table"][3, 0])
    assert np.array_equal(batch["decoded_images"][off:off + 2700].numpy().reshape(30, 30, 3), items[3]["decoded"])
    raw_collate = FlameDataset(anno, cfg).get_collate_fn()
    for i, it in enumerate(items):
        x, y, w, h = (int(v) for v in it["bbox"])
        H, W = (int(v) for v in it["image_shape"][:2])
        nh, nw, top, left = raw_collate._geometry(h, w)
        assert batch["crop_descs"][i].tolist() == [(y * W + x) * 3, h, w, nh, nw, top, left, W * 3]
        assert batch["frames"][i].tolist() == [H, x, y, w, h, top, left, 0]
    assert np.array_equal(batch["INPUT_BBOX_KEY"].numpy(), np.stack([it["bbox"] for it in items]))
    assert batch["SAMPLE_INDEX_KEY"].tolist() == [0, 1, 2, 3] and batch["IMAGE_FILENAME_KEY"] == [a["img_path"] for a in anno]
    # None items are dropped and the batch is refilled with copies of its first valid items, as RawBatchCollate does
    holes = collate([None, items[1], None, items[2]])
    assert holes["SAMPLE_INDEX_KEY"].tolist() == [1, 2, 1, 2] and holes["annotation_table"].shape == (4, 2)
    t = holes["annotation_table"].numpy()
    assert holes["annotations"][t[2, 0]:t[2, 0] + t[2, 1]].numpy().tobytes() == items[1]["annotation"].tobytes()
    with pytest.raises(ValueError, match="every item of the batch is None"):
        collate([None, None])
    with pytest.raises(ValueError, match="does not lie"):
        collate([dict(items[0], bbox=np.array([0, 0, 51, 10], np.int32))])


def test_default_item_form_is_raw(files):
    cfg, anno = files
    ds = FlameDataset(anno, cfg)
    assert ds.item_form == "raw"
    np.random.seed(0)
    assert set(ds[0]) == {"image", "bbox", "image_shape", "vertices", "model_view", "projection", "SAMPLE_INDEX_KEY", "IMAGE_FILENAME_KEY"}
