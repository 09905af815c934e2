"""GPU: training batches built on the device (dataset.FlameBatchBuilder: dad3d_preprocess_images, dad3d_gt_keypoints,
dad3d_heatmap_encode) against the reference's own FlameDataset (tests/golden/train_batch_golden.npz), the NumPy restatement
(tests/train_batch_restatement.py) and the preprocessing oracle (oracle/preprocess_ref.py)."""
import os

import numpy as np
import pytest
import torch

import train_batch_restatement as rs
from dad_3dheads_amd import synthetic
from dad_3dheads_amd.dataset import NORMALIZE, FlameBatchBuilder, FlameDataset, RawBatchCollate
from oracle import preprocess_ref as pp

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_batch_golden.npz")
TL, TH, TF, TP, TB = ("TARGET_2D_LANDMARKS", "TARGET_LANDMARKS_HEATMAP", "TARGET_2D_FULL_LANDMARKS", "TARGET_2D_LANDMARKS_PRESENCE",
                      "INPUT_BBOX_KEY")


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def st():
    return synthetic.load_static()


def _case(z, st, name, tmp):
    cfg = rs.case_config(z, name, str(tmp), st)
    items = rs.case_items(z, name, st)
    return cfg, items, RawBatchCollate(256, cfg["transform"]["resize_mode"])


def _magnification(z, name, i):
    """How much the resize step magnifies an fp32 rounding of a crop-pixel point (1-px crops in resize mode: 256x)."""
    _, _, w, h = (int(v) for v in z[name + "_bbox"][i])
    if str(z[name + "_mode"]) == "resize":
        return max(1.0, 256 / w, 256 / h)
    return max(1.0, 256 / max(w, h))


@pytest.mark.parametrize("name", ["lms_imagenet_68", "resize_mean_445", "lms_mean_68_edges"])
def test_batch_against_golden_and_oracle(z, st, name, tmp_path):
    cfg, items, collate = _case(z, st, name, tmp_path)
    builder = FlameBatchBuilder(cfg, 0)
    raw = collate(items)
    images, t = builder(raw)
    torch.cuda.synchronize()
    p = name + "_"
    mean, std = NORMALIZE[cfg["transform"]["normalize"]]
    for i, it in enumerate(items):  # images: bit-equal to the oracle on each crop
        img = it["image"]
        if cfg["transform"]["resize_mode"] == "resize":
            small = pp.resize_linear_u8(img, 256, 256)
            m = np.array(mean, np.float32) * np.float32(255)
            den = np.reciprocal(np.array(std, np.float32) * np.float32(255), dtype=np.float32)
            ref = np.transpose((small.astype(np.float32) - m) * den, (2, 0, 1))
        else:
            ref = pp.transform(img, 256, mean, std)
        assert np.array_equal(images[i].cpu().numpy(), ref), (name, i)
    sub_px = builder.last_subset_px.cpu().numpy()
    full = t[TF].cpu().numpy()
    for i in range(len(items)):
        tol = 1e-3 * _magnification(z, name, i)
        assert np.abs(sub_px[i] - z[p + "subset_px"][i]).max() <= tol, (name, i)
        assert np.abs(full[i, ::int(z["full_stride"])] - z[p + "full"][i]).max() <= tol, (name, i)
        assert np.abs(t[TL][i].cpu().numpy() - z[p + "landmarks"][i]).max() <= tol / 256, (name, i)
    # ... and every geometric target equals the restatement of the kernel's fixed order to the bit (tests/test_gpu_gt_keypoints.py
    # holds the entry itself to it; here it is the builder's tables, uploads and frame rows that are held)
    pres = t[TP].cpu().numpy()
    kw = dict(zip(("corners", "weights"), rs.lmk68_tables(st))) if str(z[p + "subset"]) == "68" else {"index": st["lmk_445"]}
    for i, it in enumerate(items):
        want = rs.chain(it["vertices"], it["model_view"], it["projection"], (it["image_shape"][0], *it["bbox"]), 256, str(z[p + "mode"]), **kw)
        for what, got, ref in zip(("full", "subset_px", "landmarks", "presence"), (full[i], sub_px[i], t[TL][i].cpu().numpy(), pres[i]), want):
            assert got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(got.view(np.uint8), ref.view(np.uint8)), (name, i, what)
    # presence: the golden's on every point, the ones on a crop edge included
    assert np.array_equal(pres, z[p + "presence"])
    # heatmaps: byte-equal to the restated reference coder (tests/train_objective_restatement.encode) on the kernel's own
    # subset and presence ...
    import train_objective_restatement as tors

    heat = t[TH].cpu().numpy()
    assert np.array_equal(heat, tors.encode(sub_px, pres, 64, 4, 5, "uint8"))
    # ... and equal to the golden except channels whose cell differs from the golden's
    cell = np.floor(sub_px / 4) != np.floor(z[p + "subset_px"] / 4)
    same = ~cell.any(-1) & (pres == z[p + "presence"])
    assert np.array_equal(heat[same], z[p + "heatmap"][same])
    assert builder.coder.num_classes == heat.shape[1]


def _oracle_image(img, mode, mean, std):
    """The preprocessing oracle's network input of one crop, as test_batch_against_golden_and_oracle states it."""
    if mode == "resize":
        small = pp.resize_linear_u8(img, 256, 256)
        m = np.array(mean, np.float32) * np.float32(255)
        den = np.reciprocal(np.array(std, np.float32) * np.float32(255), dtype=np.float32)
        return np.transpose((small.astype(np.float32) - m) * den, (2, 0, 1))
    return pp.transform(img, 256, mean, std)


def test_double_transform_bit_equal(st):
    """Identity matrices, H = 0, crop corner 0: the kernel's crop-pixel points are the fed points (x, -y) exactly, so the
    float64 keypoint transform meets the restatement bit for bit, for both modes and odd crop shapes; so do the 68 landmarks, their
    normalised form and their presence, and the images of these shapes are the preprocessing oracle's."""
    rng = np.random.default_rng(5)
    kw = dict(zip(("corners", "weights"), rs.lmk68_tables(st)))
    for mode in ("longest_max_size", "resize"):
        items = []
        for i, (h, w) in enumerate([(1, 300), (255, 257), (256, 256), (611, 97), (3, 1)]):
            xy = (rng.uniform(-0.2, 1.2, (rs.N_VERTS, 2)) * (w, h)).astype(np.float32)
            verts = np.stack([xy[:, 0], -xy[:, 1], rng.uniform(-1, 1, rs.N_VERTS).astype(np.float32)], -1).astype(np.float32)
            items.append({"image": rs.image(40 + i, h, w), "bbox": np.array([0, 0, w, h], np.int32),
                          "image_shape": np.array([0, w, 3]), "vertices": verts, "model_view": np.eye(4, dtype=np.float32),
                          "projection": np.eye(4, dtype=np.float32), "SAMPLE_INDEX_KEY": i, "IMAGE_FILENAME_KEY": str(i)})
        cfg = {"img_size": 256, "stride": 4, "num_classes": 68, "keypoints": {"2d_subset_name": "multipie_keypoints"},
               "transform": {"resize_mode": mode}}
        builder = FlameBatchBuilder(cfg, 0)
        images, t = builder(RawBatchCollate(256, mode)(items))
        mean, std = NORMALIZE[builder.normalize]
        full, sub_px, norm, pres = t[TF].cpu().numpy(), builder.last_subset_px.cpu().numpy(), t[TL].cpu().numpy(), t[TP].cpu().numpy()
        present = 0
        for i, it in enumerate(items):
            h, w = it["image"].shape[:2]
            assert it["image"].any() and np.array_equal(images[i].cpu().numpy(), _oracle_image(it["image"], mode, mean, std)), (mode, i)
            ref = rs.albu_keypoints(np.stack([it["vertices"][:, 0], -it["vertices"][:, 1]], -1), h, w, 256, mode)
            assert np.array_equal(full[i].view(np.uint32), ref.view(np.uint32)), (mode, i)
            want = rs.chain(it["vertices"], it["model_view"], it["projection"], (0, 0, 0, w, h), 256, mode, **kw)
            assert np.array_equal(want[0].view(np.uint32), ref.view(np.uint32))
            for what, got, r in zip(("subset_px", "subset_norm", "presence"), (sub_px[i], norm[i], pres[i]), want[1:]):
                assert got.dtype == r.dtype and got.shape == r.shape and np.array_equal(got.view(np.uint8), r.view(np.uint8)), (mode, i, what)
            present += int(pres[i].sum())
        assert 0 < present < pres.size  # the landmarks fall on both sides of the crops' edges


def test_batch_of_one_equals_batch_of_64(z, st, tmp_path):
    name = "lms_imagenet_68"
    cfg, items, collate = _case(z, st, name, tmp_path)
    builder = FlameBatchBuilder(cfg, 0)
    big = [items[i % len(items)] for i in range(64)]
    img64, t64 = builder(collate(big))
    for i in (0, 3, 63):
        img1, t1 = builder(collate([big[i]]))
        assert torch.equal(img1[0], img64[i])
        for k in (TL, TH, TF, TP):
            assert torch.equal(t1[k][0], t64[k][i]), (k, i)


def test_non_finite_input_poisons_only_its_item(z, st, tmp_path):
    name = "lms_imagenet_68"
    cfg, items, collate = _case(z, st, name, tmp_path)
    builder = FlameBatchBuilder(cfg, 0)
    _, clean = builder(collate(items))
    bad = [dict(it) for it in items]
    bad[1]["vertices"] = np.full_like(items[1]["vertices"], np.nan)
    mv = items[2]["model_view"].copy()
    mv[0, 3] = np.inf
    bad[2]["model_view"] = mv
    pm = items[3]["projection"].copy()
    pm[0, 0] = -np.inf
    bad[3]["projection"] = pm
    _, t = builder(collate(bad))
    for i in (1, 2, 3):
        assert not t[TP][i].any(), i
        assert int(t[TH][i].max()) == 0, i
    for i in (0, 4, 5):
        for k in (TL, TH, TF, TP):
            assert torch.equal(t[k][i], clean[k][i]), (k, i)


def test_whole_step_matches_golden_targets(z, st, tmp_path):
    """builder -> LossModule (train_loss.yaml) and StepMetrics on seeded network outputs: the loss terms and metrics of the
    golden's own targets (a clean case: no subset point near a crop edge or a stride-cell boundary)."""
    from dad_3dheads_amd.head_mesh import HeadMesh
    from dad_3dheads_amd.loss_module import LossModule
    from dad_3dheads_amd.metrics import StepMetrics

    name = "lms_imagenet_68"
    assert bool(z[name + "_clean"])
    cfg, items, collate = _case(z, st, name, tmp_path)
    images, t = FlameBatchBuilder(cfg, 0)(collate(items))
    p, b, dev = name + "_", len(items), torch.device("cuda", 0)
    gold = {TL: torch.from_numpy(z[p + "landmarks"]).to(dev), TH: torch.from_numpy(z[p + "heatmap"]).to(dev),
            TP: torch.from_numpy(z[p + "presence"]).to(dev), TB: t[TB], "TARGET_3D_MODEL_VERTICES": t["TARGET_3D_MODEL_VERTICES"]}
    assert torch.equal(t[TP], gold[TP]) and torch.equal(t[TH], gold[TH])
    # the golden stores every other vertex of the full landmarks: compare the metric on those
    stride = int(z["full_stride"])
    model = synthetic.synthetic_flame_model(0, st)
    rng = np.random.default_rng(9)
    params = torch.from_numpy(synthetic.synthetic_params(b, seed=9)).to(dev)
    outputs = {"OUTPUT_LANDMARKS_HEATMAP": torch.from_numpy(rng.normal(0, 2, t[TH].shape).astype(np.float32)).to(dev),
               "OUTPUT_2D_LANDMARKS": torch.from_numpy(rng.uniform(0.2, 0.8, (b, 68, 2)).astype(np.float32)).to(dev),
               "OUTPUT_3DMM_PARAMS": params}
    face = np.arange(0, rs.N_VERTS, stride)[::3]
    regions = {"face": face, "face_w_ears": face[::2], "head": face[::4]}
    folder = tmp_path / "regions"
    folder.mkdir()
    for k, v in regions.items():
        np.save(folder / (k + ".npy"), v)
    fi = {"folder": str(folder), "files": {k: k + ".npy" for k in regions}}
    loss_cfg = {"reduction": "sum", "criterions": [
        {"name": "heatmap_loss", "target_key": TH, "output_key": "OUTPUT_LANDMARKS_HEATMAP", "weight": 1.0,
         "loss": {"_target_": "model_training.losses.IoULoss"}},
        {"name": "landmarks_loss", "target_key": [TL, TP], "output_key": ["OUTPUT_2D_LANDMARKS", TP], "weight": 100.0,
         "loss": {"_target_": "model_training.losses.LandmarksLossWVisibility", "criterion": "smooth_l1"}}]}
    module = LossModule.from_config(loss_cfg)
    total, terms = module(outputs, {**t}, 0)
    total_g, terms_g = module(outputs, {**t, **gold}, 0)
    assert abs(float(total) - float(total_g)) <= 1e-5 * max(1.0, abs(float(total_g)))
    for k in terms:
        assert abs(float(terms[k]) - float(terms_g[k])) <= 1e-5 * max(1.0, abs(float(terms_g[k]))), k
    hm = HeadMesh(flame_model=model, static=st, device=0)
    full_t = dict(t)
    full_t[TF] = t[TF][:, ::stride].contiguous()
    full_g = {**full_t, **gold, TF: torch.from_numpy(z[p + "full"]).to(dev)}
    sub_face = {"face": np.arange(0, full_t[TF].shape[1], 3)}

    class _Sub:  # the metric's mesh reprojection, thinned to the stored vertices
        def reprojected_vertices(self, params_3dmm, to_2d=True):
            return hm.reprojected_vertices(params_3dmm=params_3dmm, to_2d=to_2d)[:, ::stride].contiguous()

        def vertices_3d(self, params_3dmm, zero_rotation=True):
            return hm.vertices_3d(params_3dmm=params_3dmm, zero_rotation=zero_rotation)[:, ::stride].contiguous()

    m1, m2 = StepMetrics(_Sub(), sub_face, 256), StepMetrics(_Sub(), sub_face, 256)
    full_t["TARGET_3D_MODEL_VERTICES"] = full_g["TARGET_3D_MODEL_VERTICES"] = t["TARGET_3D_MODEL_VERTICES"][:, ::stride].contiguous()
    outputs["OUTPUT_3DMM_PARAMS"] = params
    r1, r2 = m1(outputs, full_t), m2(outputs, full_g)
    for k in r2:
        if k.endswith("3d"):
            continue  # the 3-D metrics read the raw vertices, the same tensor on both sides
        a, g = float(r1[k]), float(r2[k])
        assert abs(a - g) <= 1e-5 * max(abs(g), 1e-6), (k, a, g)


def test_stream_order_without_sync(z, st, tmp_path):
    """Built and consumed on a side stream with no synchronisation: the same bits as on the default stream."""
    name = "resize_mean_445"
    cfg, items, collate = _case(z, st, name, tmp_path)
    builder = FlameBatchBuilder(cfg, 0)
    ref_img, ref = builder(collate(items))
    raw = collate(items)
    raw = {k: (v.pin_memory() if torch.is_tensor(v) else v) for k, v in raw.items()}
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        img, t = builder(raw)
        img_sum = img.double().sum()
        heat_sum = t[TH].to(torch.int64).sum()
        full_copy = t[TF].clone()
    side.synchronize()
    assert float(img_sum) == float(ref_img.double().sum())
    assert int(heat_sum) == int(ref[TH].to(torch.int64).sum())
    assert torch.equal(full_copy, ref[TF])


def test_dataloader_workers_pinned_loop(z, st, tmp_path):
    """FlameDataset -> DataLoader(num_workers=2, pin_memory=True) -> FlameBatchBuilder on files written from a golden case:
    the targets are the golden's."""
    from PIL import Image
    import json

    name = "lms_imagenet_68"
    p = name + "_"
    cfg = rs.case_config(z, name, str(tmp_path / "kp"), st)
    anno = []
    for i, seed in enumerate(z[p + "seeds"]):
        shape = tuple(int(v) for v in z[p + "image_shapes"][i])
        Image.fromarray(rs.image(int(seed), *shape[:2])).save(tmp_path / f"img_{seed}.png")
        verts = rs.mesh(int(seed), st["template_geo"])
        with open(tmp_path / f"mesh_{seed}.json", "w") as f:
            json.dump({"vertices": verts.tolist(), "model_view_matrix": z[p + "model_view"][i].tolist(),
                       "projection_matrix": z[p + "projection"][i].tolist()}, f)
        anno.append({"img_path": f"img_{seed}.png", "bbox": z[p + "anno_bbox"][i].tolist(), "annotation_path": f"mesh_{seed}.json"})
    cfg["dataset_root"] = str(tmp_path)
    ds = FlameDataset(anno, cfg)
    seed = int(z[p + "rng_seed"])

    def init(worker_id):  # one worker sees the whole batch: the reference's RNG stream, seeded
        np.random.seed(seed)

    loader = torch.utils.data.DataLoader(ds, batch_size=len(anno), num_workers=2, pin_memory=True,
                                         collate_fn=ds.get_collate_fn(), worker_init_fn=init, multiprocessing_context="fork")
    builder = FlameBatchBuilder(cfg, 0)
    for raw in loader:
        assert raw["crops"].is_pinned()
        assert np.array_equal(raw[TB].numpy(), z[p + "bbox"])
        _, t = builder(raw)
        assert torch.equal(t[TP].cpu(), torch.from_numpy(z[p + "presence"]))
        assert torch.equal(t[TH].cpu(), torch.from_numpy(z[p + "heatmap"]))
        assert np.abs(t[TL].cpu().numpy() - z[p + "landmarks"]).max() <= 1e-3 / 256
        break
