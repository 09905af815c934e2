"""GPU: the file form of the training loader. A `FlameDataset(item_form="files")`, `FileBatchCollate` and
`FlameBatchBuilder` give every image and every target of the raw chain over the same files and the same seed, bit for bit: the same
kernels read the same bytes, so there is no tolerance. Covered: both resize modes, the 68 landmarks and an index subset, B = 3 and 5,
crops of odd shapes and one bbox that clips at two borders; a grey + alpha PNG, a palette PNG (decoded by the worker), an Adam7 PNG
(decoded by PIL for the builder), an annotation with a nested object (parsed by the host), a truncated annotation (the host's error), a
batch already on the device, and the caller's batch left as it was."""
import io
import json
import os
import struct
import zlib

import numpy as np
import pytest
import torch

from dad_3dheads_amd import synthetic
from dad_3dheads_amd.dataset import FileBatchCollate, FlameBatchBuilder, FlameDataset

pytestmark = pytest.mark.gpu
N_VERTS = 5023
# the crop shapes of test_gpu_train_batch.test_double_transform_bit_equal as image sizes (H, W), each with a bbox inside it; the second
# bbox grows past the right and the bottom border whatever the jitter draws
SIZES = [(255, 257), (256, 256), (1, 300), (611, 97), (3, 1)]
BBOXES = [[20, 30, 200, 190], [150, 160, 120, 110], [10, 0, 200, 1], [5, 40, 80, 500], [0, 0, 1, 3]]
CASES = [(mode, subset) for mode in ("longest_max_size", "resize") for subset in ("68", "445")]


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def adam7_png(arr):
    """An interlaced 8-bit RGB PNG of `arr` [H,W,3] (PIL writes none): the seven passes, filter 0 on every row."""
    h, w, _ = arr.shape
    raw = b""
    for x0, y0, dx, dy in [(0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)]:
        sub = arr[y0::dy, x0::dx]
        if sub.shape[0] and sub.shape[1]:
            raw += b"".join(b"\x00" + np.ascontiguousarray(row).tobytes() for row in sub)
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 1)) + _chunk(b"IDAT", zlib.compress(raw))
            + _chunk(b"IEND", b""))


def annotation(rng, extra=None):
    verts = rng.uniform(-1, 1, (N_VERTS, 3)).astype(np.float32)
    mv = np.eye(4, dtype=np.float32)
    mv[:3, :3] += rng.uniform(-0.1, 0.1, (3, 3)).astype(np.float32)
    mv[:3, 3] = rng.uniform(-0.2, 0.2, 3).astype(np.float32) + np.float32([0, 0, -5])  # column vectors: the head 5 units in front
    pm = np.array([[300, 0, -128, 0], [0, 300, -128, 0], [0, 0, -1.002, -0.2002], [0, 0, -1, 0]], dtype=np.float32)  # pixels, w = -z
    doc = {"vertices": verts.astype(np.float64).tolist(), "model_view_matrix": mv.astype(np.float64).tolist(),
           "projection_matrix": pm.astype(np.float64).tolist(), "bbox": [1, 2, 3, 4]}
    doc.update(extra or {})
    return json.dumps(doc).encode("ascii")


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from PIL import Image

    root = tmp_path_factory.mktemp("train_files")
    rng = np.random.default_rng(11)
    anno = []
    for i, ((h, w), bbox) in enumerate(zip(SIZES, BBOXES)):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(root / f"img_{i}.png")
        (root / f"mesh_{i}.json").write_bytes(annotation(rng))
        anno.append({"img_path": f"img_{i}.png", "bbox": bbox, "annotation_path": f"mesh_{i}.json"})
    h, w = SIZES[0]
    Image.fromarray(rng.integers(0, 256, (h, w, 2), dtype=np.uint8), "LA").save(root / "grey_alpha.png")
    Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).convert("P").save(root / "palette.png")
    pixels = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    (root / "adam7.png").write_bytes(adam7_png(pixels))
    with Image.open(root / "adam7.png") as im:
        assert im.info.get("interlace") == 1 and np.array_equal(np.asarray(im.convert("RGB")), pixels)
    (root / "nested.json").write_bytes(annotation(rng, {"attributes": {"quality": 1, "tags": ["a", "b"]}}))
    (root / "truncated.json").write_bytes((root / "mesh_0.json").read_bytes()[:100000])
    os.makedirs(root / "kp")
    np.save(root / "kp" / "keypoints_445.npy", {"all": [int(v) for v in synthetic.load_static()["lmk_445"]]})
    return str(root), anno


_builders = {}


def config(root, mode, subset):
    kp = ({"2d_subset_name": "multipie_keypoints", "2d_subset_path": os.path.join(root, "kp")} if subset == "68" else
          {"2d_subset_name": "keypoints_445", "2d_subset_path": os.path.join(root, "kp")})
    return {"img_size": 256, "stride": 4, "num_classes": 68 if subset == "68" else 445, "keypoints": kp, "dataset_root": root,
            "transform": {"normalize": "imagenet" if mode == "resize" else "mean", "resize_mode": mode}}


def builder(root, mode, subset):
    if (mode, subset) not in _builders:
        _builders[mode, subset] = FlameBatchBuilder(config(root, mode, subset), 0)
    return _builders[mode, subset]


def batch(anno, cfg, form, seed):
    np.random.seed(seed)
    ds = FlameDataset(anno, cfg, item_form=form)
    return ds.get_collate_fn()([ds[i] for i in range(len(anno))])


def same(a, b):
    (img_a, t_a), (img_b, t_b) = a, b
    assert img_a.dtype == img_b.dtype and torch.equal(img_a, img_b)
    assert set(t_a) == set(t_b)
    for k in t_a:
        if isinstance(t_a[k], torch.Tensor):
            assert t_a[k].dtype == t_b[k].dtype and t_a[k].shape == t_b[k].shape, k
            assert torch.equal(t_a[k].cpu(), t_b[k].cpu()), k
            assert not t_a[k].is_floating_point() or bool(torch.isfinite(t_a[k]).all()), k  # equal, and not equal NaNs
        else:
            assert t_a[k] == t_b[k], k


def both_chains(root, anno, mode="longest_max_size", subset="68", seed=3, to_device=False):
    cfg, build = config(root, mode, subset), builder(root, mode, subset)
    want = build(batch(anno, cfg, "raw", seed))
    assert build.last_fallbacks is None
    files = batch(anno, cfg, "files", seed)
    assert isinstance(FlameDataset(anno, cfg, item_form="files").get_collate_fn(), FileBatchCollate)
    if to_device:
        files = {k: v.cuda() if isinstance(v, torch.Tensor) else v for k, v in files.items()}
    kept = {k: v.clone() if isinstance(v, torch.Tensor) else list(v) for k, v in files.items()}
    got = build(files)
    torch.cuda.synchronize()
    same(want, got)
    for k, v in kept.items():  # the caller's batch is as it was
        assert torch.equal(files[k], v) if isinstance(v, torch.Tensor) else files[k] == v, k
    return dict(build.last_fallbacks)


NONE = {"annotation_host": 0, "png_host": 0, "png_worker": 0}


@pytest.mark.parametrize("b", [3, 5])
@pytest.mark.parametrize("mode,subset", CASES)
def test_file_chain_equals_raw_chain(data, mode, subset, b):
    root, anno = data
    assert both_chains(root, anno[:b], mode, subset, seed=b) == NONE


def test_grey_alpha_png(data):
    root, anno = data
    assert both_chains(root, [dict(anno[0], img_path="grey_alpha.png")] + anno[1:3]) == NONE


def test_palette_png_is_decoded_by_the_worker(data):
    root, anno = data
    assert both_chains(root, anno[1:3] + [dict(anno[0], img_path="palette.png")]) == dict(NONE, png_worker=1)
    assert both_chains(root, [dict(anno[0], img_path="palette.png")]) == dict(NONE, png_worker=1)  # no PNG reaches the device


def test_adam7_png_is_decoded_by_pil(data):
    root, anno = data
    assert both_chains(root, [anno[1], dict(anno[0], img_path="adam7.png"), anno[2]], "resize", "445") == dict(NONE, png_host=1)


def test_nested_object_annotation_is_parsed_by_the_host(data):
    root, anno = data
    mixed = [anno[0], dict(anno[1], annotation_path="nested.json"), dict(anno[2], img_path="palette.png"), anno[3]]
    assert both_chains(root, mixed) == {"annotation_host": 1, "png_host": 0, "png_worker": 1}


def test_decoded_images_larger_than_the_output_twice_in_a_row(data, tmp_path):
    """600 x 600 files: the decoded images of a batch (1.08 MB each) outweigh its output (0.79 MB each), so a decoded block freed before
    the preprocess launch is the allocator's best fit for that launch's output. The builder holds the images until the launch is
    enqueued; from the second call on the pool is full of such blocks."""
    from PIL import Image

    root, anno = data
    rng = np.random.default_rng(21)
    yy, xx = np.mgrid[0:600, 0:600]
    big = []
    for i in range(3):
        img = np.stack([(xx + 40 * i) % 256, (yy * 3) % 256, (xx + yy) % 256], -1) + rng.integers(0, 8, (600, 600, 3))
        Image.fromarray((img % 256).astype(np.uint8)).save(os.path.join(root, f"big_{i}.png"))
        big.append(dict(anno[i], img_path=f"big_{i}.png", bbox=[40 + 10 * i, 60, 480, 450]))
    assert 3 * 600 * 600 * 3 > 3 * 3 * 256 * 256 * 4
    for seed in (1, 2, 3):
        assert both_chains(root, big, seed=seed) == NONE
    assert both_chains(root, big + [dict(big[0], img_path="adam7.png", bbox=anno[0]["bbox"])], "resize", seed=4) == dict(NONE, png_host=1)


def test_truncated_annotation_raises_the_hosts_error(data):
    root, anno = data
    cfg = config(root, "longest_max_size", "68")
    files = batch([anno[0], dict(anno[1], annotation_path="truncated.json")], cfg, "files", 1)
    with pytest.raises(json.JSONDecodeError):
        builder(root, "longest_max_size", "68")(files)
    with pytest.raises(json.JSONDecodeError):
        FlameDataset._load_mesh(os.path.join(root, "truncated.json"))


def test_batch_already_on_the_device(data):
    root, anno = data
    mixed = [anno[0], dict(anno[1], annotation_path="nested.json"), dict(anno[0], img_path="adam7.png")]
    assert both_chains(root, mixed, to_device=True) == {"annotation_host": 1, "png_host": 1, "png_worker": 0}


def test_decode_packed_is_decode(data):
    """`PngDecoder.decode` is packing + `decode_packed`: the same tensors from a buffer the caller packed, on the host or on the device."""
    from dad_3dheads_amd.png_reader import PngDecoder, _align

    root, _ = data
    files = [open(os.path.join(root, n), "rb").read() for n in ("img_0.png", "grey_alpha.png", "palette.png", "adam7.png", "img_4.png")]
    dec = PngDecoder(0)
    want = dec.decode([io.BytesIO(f).getvalue() for f in files], 3)
    offsets, at = [], 0
    for f in files:
        offsets.append(at)
        at += _align(len(f))
    buf = torch.zeros(at, dtype=torch.uint8)
    for o, f in zip(offsets, files):
        buf[o:o + len(f)] = torch.frombuffer(bytearray(f), dtype=torch.uint8)
    for buffer in (buf, buf.cuda()):
        got = dec.decode_packed(buffer, offsets, [len(f) for f in files], 3)
        assert np.array_equal(got.flags, want.flags) and got.shapes == want.shapes
        assert all(torch.equal(a, b) for a, b in zip(got.tensors(), want.tensors()))
    assert want.flags.tolist()[0] == 0 and want.flags[2] == -1 and want.flags[3] != 0
    with pytest.raises(ValueError, match="multiple of 16"):
        dec.decode_packed(buf, [8], [len(files[0])], 3)
