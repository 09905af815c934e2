"""DAD-3DNet training batches built on the GPU from raw image crops: a drop-in for the reference's
`model_training/data/flame_dataset.py` `FlameDataset` and `collate_skip_none`.

The loader is split at the host / device boundary:

* `FlameDataset.__getitem__` runs in the DataLoader workers and stays CPU-only (no HIP, safe in a forked worker). It reads
  the image, draws the reference's bbox jitter from the global NumPy RNG, crops, and loads the annotation mesh. It returns a
  RAW item: the uint8 crop, the int32 bbox, the full image shape, the vertices [5023,3], the model-view and projection
  matrices [4,4] (float32), the index and the file name. The reference's per-sample dict (the resized, normalised image,
  the 2-D keypoints, presence and heatmap) exists only batched, on the device: that is the one interface difference.
* `RawBatchCollate` (`FlameDataset.get_collate_fn()`) packs raw items into CPU tensors: one uint8 buffer for every crop,
  with per-item descriptors, and stacked arrays, so `DataLoader(pin_memory=True)` pins the whole batch.
* `FlameBatchBuilder` uploads a raw batch and launches three kernels on the current stream, with no host sync:
  `dad3d_preprocess_images` (resize, pad, normalise, CHW), `dad3d_gt_keypoints` (model-view, projection, 68 landmarks or
  the index subset, crop shift, presence, albumentations' keypoint geometry) and `dad3d_heatmap_encode`.

Images are read with PIL by default (cv2 is not a dependency); pass `reader=` to use another decoder. DAD-3DHeads images
are PNG, a lossless format, so the decoder does not change the pixels; for JPEG inputs, decoders may differ and parity with
the reference's cv2.imread is unpinned.
"""
from __future__ import annotations

import json
import os
from typing import Any, Callable, Dict, List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .landmarks import load_2d_indices
from .resize_geometry import longest_max_size

__all__ = ["FlameDataset", "RawBatchCollate", "FlameBatchBuilder", "extend_bbox", "ensure_bbox_boundaries", "read_as_rgb",
           "NORMALIZE", "RESIZE_MODES"]

# model_training/data/config.py keys
SAMPLE_INDEX_KEY, IMAGE_FILENAME_KEY = "SAMPLE_INDEX_KEY", "IMAGE_FILENAME_KEY"
INPUT_IMAGE_KEY, INPUT_BBOX_KEY, INPUT_SIZE_KEY = "INPUT_IMAGE_KEY", "INPUT_BBOX_KEY", "INPUT_SIZE_KEY"
TARGET_3D_MODEL_VERTICES, TARGET_2D_FULL_LANDMARKS = "TARGET_3D_MODEL_VERTICES", "TARGET_2D_FULL_LANDMARKS"
TARGET_2D_LANDMARKS, TARGET_LANDMARKS_HEATMAP = "TARGET_2D_LANDMARKS", "TARGET_LANDMARKS_HEATMAP"
TARGET_2D_LANDMARKS_PRESENCE = "TARGET_2D_LANDMARKS_PRESENCE"

# data/transforms.py:26-32 (A.Normalize's [0,1]-scale constants)
NORMALIZE = {"imagenet": ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)), "mean": ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))}
RESIZE_MODES = {"longest_max_size": 0, "resize": 1}  # DAD3D_RESIZE_LONGEST_MAX_SIZE / DAD3D_RESIZE_RESIZE

# keys of a raw item / raw batch
IMAGE, BBOX, IMAGE_SHAPE, VERTICES, MODEL_VIEW, PROJECTION = "image", "bbox", "image_shape", "vertices", "model_view", "projection"
CROPS, CROP_DESCS, FRAMES = "crops", "crop_descs", "frames"


def read_as_rgb(path: str) -> np.ndarray:
    """uint8 RGB [H,W,3] with PIL (data/utils.py:18-34 reads with cv2, then scikit-image)."""
    from PIL import Image

    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


def extend_bbox(bbox: np.ndarray, offset: Union[Tuple[float, ...], float] = 0.1) -> np.ndarray:
    """data/utils.py:73-103: grow [x, y, w, h] by offset * 100 % per side -- (left, right, top, bottom), (w, h) or one value --
    and truncate to int32."""
    x, y, w, h = bbox
    if isinstance(offset, tuple) and len(offset) == 4:
        left, right, top, bottom = offset
    elif isinstance(offset, tuple) and len(offset) == 2:
        left = right = offset[0]
        top = bottom = offset[1]
    else:
        left = right = top = bottom = offset
    return np.array([x - w * left, y - h * top, w * (1.0 + right + left), h * (1.0 + top + bottom)]).astype("int32")


def ensure_bbox_boundaries(bbox: np.ndarray, img_shape: Tuple[int, int]) -> np.ndarray:
    """data/utils.py:106-115: clip [x, y, w, h] to an image of shape (h, w); int32."""
    x1, y1, w, h = bbox
    x1, y1 = min(max(0, x1), img_shape[1]), min(max(0, y1), img_shape[0])
    x2, y2 = min(max(0, x1 + w), img_shape[1]), min(max(0, y1 + h), img_shape[0])
    return np.array([x1, y1, x2 - x1, y2 - y1]).astype("int32")


def _transform_config(config: Mapping[str, Any]) -> Tuple[str, str]:
    tr = config.get("transform") or {}
    normalize, resize = tr.get("normalize", "imagenet"), tr.get("resize_mode", "longest_max_size")
    if normalize not in NORMALIZE:
        raise KeyError(f"normalize must be one of {sorted(NORMALIZE)}, not {normalize!r}")
    if resize not in RESIZE_MODES:
        raise KeyError(resize)  # get_resize_fn raises KeyError(mode)
    return normalize, resize


def _subset(config: Mapping[str, Any]) -> Optional[List[int]]:
    """The subset: None for the 68 landmarks (get_68_landmarks), else the vertex ids of `keypoints`; num_classes must match."""
    indices = load_2d_indices(config["keypoints"])
    n = config.get("num_classes")
    k = 68 if indices is None else len(indices)
    if n != k:
        raise ValueError(f"num_classes is {n}, but the keypoints config gives {k} points"
                         + (" (multipie_keypoints: the 68 landmarks)" if indices is None else ""))
    return indices


class FlameDataset(torch.utils.data.Dataset):
    """model_training/data/flame_dataset.py:46-205 with a CPU-only `__getitem__` that returns the RAW item (see the module
    docstring); `FlameBatchBuilder` makes the reference's targets from a collated batch of them, on the device.
    `data`: the annotation list (img_path, bbox, annotation_path per item); `config`: the `train` / `val` block of
    config/dataset/dad_3d_heads.yaml (dataset_root, img_size, num_classes, keypoints, transform, stride)."""

    def __init__(self, data: List[Dict[str, Any]], config: Mapping[str, Any],
                 reader: Optional[Callable[[str], np.ndarray]] = None) -> None:
        self.data = data
        self.config = config
        self.img_size = config["img_size"]
        self.filename_key = "img_path"
        self.num_classes = config.get("num_classes")
        self.keypoints_indices = _subset(config)
        self.normalize, self.resize_mode = _transform_config(config)
        self.reader = reader or read_as_rgb

    def __len__(self) -> int:
        return len(self.data)

    @classmethod
    def from_config(cls, config: Mapping[str, Any], reader: Optional[Callable[[str], np.ndarray]] = None) -> "FlameDataset":
        with open(config["ann_path"]) as f:
            anno = json.load(f)
        return cls(data=anno, config=config, reader=reader)

    def get_collate_fn(self) -> "RawBatchCollate":
        return RawBatchCollate(self.img_size, self.resize_mode)

    def __getitem__(self, idx: int) -> Dict[str, Any]:
        anno = self.data[idx]
        root = self.config.get("dataset_root", "")
        img = self.reader(os.path.join(root, anno["img_path"]))
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
            raise ValueError(f"item {idx} ({anno['img_path']}): expected a uint8 RGB image [H,W,3], got {img.dtype} {img.shape}")
        # _parse_anno (flame_dataset.py:100-104): the same draw from the global NumPy RNG, the same int32 bbox
        offset = tuple(0.1 * np.random.uniform(size=4) + 0.05)
        x, y, w, h = ensure_bbox_boundaries(extend_bbox(np.array(anno["bbox"]), offset), img.shape[:2])
        if w == 0 or h == 0:
            raise ValueError(f"item {idx} ({anno['img_path']}): the bbox {anno['bbox']} crops an empty image ({w} x {h})")
        vertices, model_view, projection = self._load_mesh(os.path.join(root, anno["annotation_path"]))
        return {IMAGE: np.ascontiguousarray(img[y: y + h, x: x + w]), BBOX: np.array([x, y, w, h], dtype=np.int32),
                IMAGE_SHAPE: np.array(img.shape, dtype=np.int64), VERTICES: vertices, MODEL_VIEW: model_view,
                PROJECTION: projection, SAMPLE_INDEX_KEY: idx, IMAGE_FILENAME_KEY: anno[self.filename_key]}

    @staticmethod
    def _load_mesh(mesh_path: str) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The arrays of `_load_mesh` (flame_dataset.py:115-127); its model-view product runs on the device."""
        with open(mesh_path) as f:
            data = json.load(f)
        vertices = np.ascontiguousarray(np.array(data["vertices"], dtype=np.float32).reshape(-1, 3))
        model_view = np.ascontiguousarray(np.array(data["model_view_matrix"], dtype=np.float32).reshape(4, 4))
        projection = np.ascontiguousarray(np.array(data["projection_matrix"], dtype=np.float32).reshape(4, 4))
        return vertices, model_view, projection


class RawBatchCollate:
    """`collate_skip_none` (flame_dataset.py:37-43) for raw items: `None` items are dropped and the batch is refilled with
    copies of its first valid items. Packs into CPU tensors:
      crops       uint8 [sum h*w*3]   every crop, back to back
      crop_descs  int64 [B,8]         dad3d_preprocess_images' descriptor rows with the crop's byte OFFSET in column 0
                                      (the builder adds the device address): offset, h, w, new_h, new_w, pad_top, pad_left,
                                      row stride
      frames      int32 [B,8]         dad3d_gt_keypoints' rows: image height, crop x, y, w, h, pad_top, pad_left, 0
      vertices    f32 [B,N,3], model_view / projection f32 [B,4,4], image_shape int64 [B,3], INPUT_BBOX_KEY int32 [B,4],
      SAMPLE_INDEX_KEY int64 [B], IMAGE_FILENAME_KEY list of str (as default_collate delivers them)."""

    def __init__(self, img_size: int, resize_mode: str = "longest_max_size") -> None:
        if resize_mode not in RESIZE_MODES:
            raise KeyError(resize_mode)
        self.img_size = int(img_size)
        self.resize_mode = resize_mode

    def _geometry(self, h: int, w: int) -> Tuple[int, int, int, int]:
        if self.resize_mode == "resize":  # A.Resize(S, S): no pad
            return self.img_size, self.img_size, 0, 0
        return longest_max_size(h, w, self.img_size)

    def __call__(self, batch: Sequence[Optional[Mapping[str, Any]]]) -> Dict[str, Any]:
        n = len(batch)
        items = [b for b in batch if b is not None]
        if not items:
            raise ValueError("every item of the batch is None")
        items = items + items[: n - len(items)]
        b = len(items)
        sizes = [int(it[IMAGE].size) for it in items]
        offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        crops = torch.empty(int(sum(sizes)), dtype=torch.uint8)
        flat = crops.numpy()
        descs = np.zeros((b, 8), dtype=np.int64)
        frames = np.zeros((b, 8), dtype=np.int32)
        for i, it in enumerate(items):
            img = it[IMAGE]
            h, w = img.shape[:2]
            if h == 0 or w == 0:
                raise ValueError(f"item {it.get(SAMPLE_INDEX_KEY)}: empty crop ({w} x {h})")
            flat[offsets[i]: offsets[i] + sizes[i]] = np.ascontiguousarray(img, dtype=np.uint8).reshape(-1)
            nh, nw, top, left = self._geometry(h, w)
            descs[i] = (offsets[i], h, w, nh, nw, top, left, w * 3)
            x, y, bw, bh = (int(v) for v in it[BBOX])
            if (bw, bh) != (w, h):
                raise ValueError(f"item {it.get(SAMPLE_INDEX_KEY)}: bbox {bw} x {bh} does not match its {w} x {h} crop")
            frames[i] = (int(it[IMAGE_SHAPE][0]), x, y, w, h, top, left, 0)
        stack = lambda k, dt: torch.from_numpy(np.stack([np.asarray(it[k], dtype=dt) for it in items]))  # noqa: E731
        return {CROPS: crops, CROP_DESCS: torch.from_numpy(descs), FRAMES: torch.from_numpy(frames),
                VERTICES: stack(VERTICES, np.float32), MODEL_VIEW: stack(MODEL_VIEW, np.float32),
                PROJECTION: stack(PROJECTION, np.float32), IMAGE_SHAPE: stack(IMAGE_SHAPE, np.int64),
                INPUT_BBOX_KEY: stack(BBOX, np.int32),
                SAMPLE_INDEX_KEY: torch.tensor([int(it[SAMPLE_INDEX_KEY]) for it in items], dtype=torch.int64),
                IMAGE_FILENAME_KEY: [it[IMAGE_FILENAME_KEY] for it in items]}


class FlameBatchBuilder:
    """A raw batch (CPU, ideally pinned, or already on the device) -> (images [B,3,S,S] float32, targets), on the current
    stream of `device`, with no host sync. `targets` holds what KeypointsDataMixin.get_input keeps (train/mixins.py:30-52):
    TARGET_2D_LANDMARKS [B,K,2] (/ img_size), TARGET_LANDMARKS_HEATMAP [B,K,S/stride,S/stride] (uint8 by default, the
    dataset's bytes: losses.py fuses the / 255; "float" gives get_input's uint8 / 255), TARGET_3D_MODEL_VERTICES [B,N,3],
    TARGET_2D_FULL_LANDMARKS [B,N,2] (S pixels), TARGET_2D_LANDMARKS_PRESENCE bool [B,K], INPUT_BBOX_KEY int32 [B,4]; plus
    SAMPLE_INDEX_KEY and IMAGE_FILENAME_KEY as the collate delivers them."""

    def __init__(self, config: Mapping[str, Any], device: Union[int, str, torch.device, None] = None,
                 heatmap_form: str = "uint8") -> None:
        from . import _lib
        from .benchmark_export import Landmarks68
        from .coder import HeatmapCoder
        from .synthetic import load_static

        if heatmap_form not in ("uint8", "float"):
            raise ValueError(f"heatmap_form must be 'uint8' or 'float', not {heatmap_form!r}")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise ValueError(f"FlameBatchBuilder builds on a GPU, not {dev}")
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        self.img_size = int(config["img_size"])
        self.num_classes = int(config["num_classes"])
        self.normalize, self.resize_mode = _transform_config(config)
        self.heatmap_form = heatmap_form
        self._lib = _lib.load()
        self._check = _lib.check
        self.coder = HeatmapCoder(config, self.num_classes, device=self.device)
        indices = _subset(config)
        self.index = self.corners = self.weights = None
        if indices is None:  # get_68_landmarks: the packaged embedding on the FLAME faces (benchmark_export.Landmarks68)
            lmk = Landmarks68(load_static()["faces"], device=self.device)
            self.corners = lmk.corners.to(torch.int32).contiguous()
            self.weights = lmk.weights.to(torch.float32).contiguous()
        else:
            self.index = torch.tensor(indices, dtype=torch.int32, device=self.device)
        mean, std = NORMALIZE[self.normalize]
        import ctypes as C

        self._mean, self._std = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)

    def _up(self, t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
        return t.to(self.device, dtype, non_blocking=True).contiguous()

    def __call__(self, raw: Mapping[str, Any]) -> Tuple[torch.Tensor, Dict[str, Any]]:
        dev, s = self.device, self.img_size
        crops = self._up(raw[CROPS], torch.uint8)
        descs = raw[CROP_DESCS].to(dev, torch.int64, non_blocking=True)
        descs = (descs.clone() if descs is raw[CROP_DESCS] else descs).contiguous()  # never edit the caller's batch
        descs[:, 0] += crops.data_ptr()
        frames = self._up(raw[FRAMES], torch.int32)
        verts = self._up(raw[VERTICES], torch.float32)
        mv, pm = self._up(raw[MODEL_VIEW], torch.float32), self._up(raw[PROJECTION], torch.float32)
        b, n = verts.shape[:2]
        if descs.shape != (b, 8) or frames.shape != (b, 8) or mv.shape != (b, 4, 4) or pm.shape != (b, 4, 4) or verts.shape[2] != 3:
            raise ValueError("inconsistent raw batch: " + ", ".join(f"{k} {tuple(raw[k].shape)}" for k in
                                                                    (CROP_DESCS, FRAMES, VERTICES, MODEL_VIEW, PROJECTION)))
        stream = torch.cuda.current_stream(dev).cuda_stream
        k = self.num_classes
        images = torch.empty((b, 3, s, s), dtype=torch.float32, device=dev)
        full = torch.empty((b, n, 2), dtype=torch.float32, device=dev)
        subset_px = torch.empty((b, k, 2), dtype=torch.float32, device=dev)
        subset = torch.empty((b, k, 2), dtype=torch.float32, device=dev)
        presence = torch.empty((b, k), dtype=torch.uint8, device=dev)
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        self._check(self._lib.dad3d_preprocess_images(descs.data_ptr(), b, s, self._mean, self._std, images.data_ptr(),
                                                      dev.index, stream))
        self._check(self._lib.dad3d_gt_keypoints(
            verts.data_ptr(), mv.data_ptr(), pm.data_ptr(), frames.data_ptr(), b, n, ptr(self.index), ptr(self.corners),
            ptr(self.weights), k, s, RESIZE_MODES[self.resize_mode], full.data_ptr(), subset_px.data_ptr(), subset.data_ptr(),
            presence.data_ptr(), dev.index, stream))
        heatmap = self.coder.encode(subset_px, presence, form=self.heatmap_form)
        targets = {TARGET_2D_LANDMARKS: subset, TARGET_LANDMARKS_HEATMAP: heatmap, TARGET_3D_MODEL_VERTICES: verts,
                   TARGET_2D_FULL_LANDMARKS: full, TARGET_2D_LANDMARKS_PRESENCE: presence.view(torch.bool),
                   INPUT_BBOX_KEY: self._up(raw[INPUT_BBOX_KEY], torch.int32)}
        for key in (SAMPLE_INDEX_KEY, IMAGE_FILENAME_KEY):
            if key in raw:
                targets[key] = raw[key]
        self.last_subset_px = subset_px  # the heatmap coder's input (S pixels) of the last call, for inspection
        return images, targets
