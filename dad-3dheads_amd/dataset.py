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

`FlameDataset(..., item_form="files")` moves the decoding to the device as well: `__getitem__` only reads the bytes
of the PNG and of the annotation file, `FileBatchCollate` packs them, and `FlameBatchBuilder` decodes the PNGs (png_reader), parses
the annotations (`dad3d_annotation_parse`) and crops by address, then runs the same three kernels. That form waits for the device once
per batch, to read the PNG flags and the annotation status together; the default "raw" form stays free of host syncs.

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

__all__ = ["FlameDataset", "RawBatchCollate", "FileBatchCollate", "FlameBatchBuilder", "extend_bbox", "ensure_bbox_boundaries", "read_as_rgb",
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
# keys of a file item / file batch
PNG, DECODED, ANNOTATION = "png", "decoded", "annotation"
PNG_FILES, PNG_TABLE, DECODED_IMAGES, DECODED_TABLE, ANNOTATIONS, ANNOTATION_TABLE = ("png_files", "png_table", "decoded_images",
                                                                                      "decoded_table", "annotations", "annotation_table")
ITEM_FORMS = ("raw", "files")


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
    config/dataset/dad_3d_heads.yaml (dataset_root, img_size, num_classes, keypoints, transform, stride).
    `item_form="files"`: `__getitem__` decodes nothing. The item carries the bytes of the PNG and of the annotation file (uint8
    arrays), the bbox from the same draw and the image shape from the file's IHDR; `get_collate_fn()` gives the matching
    `FileBatchCollate`, and the builder decodes both on the device. A file the worker cannot size (not a PNG, a palette, 16 bits)
    is decoded here with `reader` and travels as a full decoded image; the crop is still taken on the device."""

    def __init__(self, data: List[Dict[str, Any]], config: Mapping[str, Any],
                 reader: Optional[Callable[[str], np.ndarray]] = None, item_form: str = "raw") -> None:
        if item_form not in ITEM_FORMS:
            raise ValueError(f"item_form must be one of {ITEM_FORMS}, not {item_form!r}")
        self.item_form = item_form
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
    def from_config(cls, config: Mapping[str, Any], reader: Optional[Callable[[str], np.ndarray]] = None,
                    item_form: str = "raw") -> "FlameDataset":
        with open(config["ann_path"]) as f:
            anno = json.load(f)
        return cls(data=anno, config=config, reader=reader, item_form=item_form)

    def get_collate_fn(self) -> Union["RawBatchCollate", "FileBatchCollate"]:
        if self.item_form == "files":
            return FileBatchCollate(self.img_size, self.resize_mode)
        return RawBatchCollate(self.img_size, self.resize_mode)

    def _read_checked(self, idx: int, path: str) -> np.ndarray:
        img = self.reader(path)
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
            raise ValueError(f"item {idx} ({self.data[idx]['img_path']}): expected a uint8 RGB image [H,W,3], got {img.dtype} {img.shape}")
        return img

    def _file_item(self, idx: int) -> Dict[str, Any]:
        from .png_reader import _header

        anno = self.data[idx]
        root = self.config.get("dataset_root", "")
        path = os.path.join(root, anno["img_path"])
        with open(path, "rb") as f:
            png = f.read()
        head = _header(png)
        decoded = None
        if head is None:  # the worker cannot size it: decoded here, cropped on the device
            decoded = np.ascontiguousarray(self._read_checked(idx, path))
            png, shape = b"", decoded.shape
        else:
            shape = (head[0], head[1], 3)
        offset = tuple(0.1 * np.random.uniform(size=4) + 0.05)  # the same single draw as the raw form
        x, y, w, h = ensure_bbox_boundaries(extend_bbox(np.array(anno["bbox"]), offset), shape[:2])
        if w == 0 or h == 0:
            raise ValueError(f"item {idx} ({anno['img_path']}): the bbox {anno['bbox']} crops an empty image ({w} x {h})")
        with open(os.path.join(root, anno["annotation_path"]), "rb") as f:
            text = f.read()
        return {PNG: np.frombuffer(png, dtype=np.uint8), DECODED: decoded, ANNOTATION: np.frombuffer(text, dtype=np.uint8),
                BBOX: np.array([x, y, w, h], dtype=np.int32), IMAGE_SHAPE: np.array(shape, dtype=np.int64),
                SAMPLE_INDEX_KEY: idx, IMAGE_FILENAME_KEY: anno[self.filename_key]}

    def __getitem__(self, idx: int) -> Dict[str, Any]:
        if self.item_form == "files":
            return self._file_item(idx)
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
            return FlameDataset._mesh_of(f)

    @staticmethod
    def _mesh_of(f) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """`_load_mesh` on an open text file."""
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


class FileBatchCollate(RawBatchCollate):
    """`RawBatchCollate` for the items of `FlameDataset(item_form="files")`: the same `None` dropping and refill. Everything is
    a CPU tensor, so `DataLoader(pin_memory=True)` pins the batch whole:
      png_files         uint8   every PNG file, each at a multiple of 16 bytes (_packed_files.pack), zero between them
      png_table         int64 [B,5]   offset, size (0: the item came decoded), and the IHDR's height, width, channels
      decoded_images    uint8   every image a worker had to decode (HWC RGB), each at a multiple of 16 bytes
      decoded_table     int64 [B,2]   offset, size (0: the item is a PNG)
      annotations       uint8   every annotation file, each at a multiple of 16 bytes
      annotation_table  int64 [B,2]   offset, size
      crop_descs        int64 [B,8]   dad3d_preprocess_images' rows for a crop read in place from the full image: the crop's byte
                                      offset in its image (y W + x) 3 in column 0 (the builder adds the image's device address),
                                      h, w, new_h, new_w, pad_top, pad_left, row stride W 3
      frames, image_shape, INPUT_BBOX_KEY, SAMPLE_INDEX_KEY, IMAGE_FILENAME_KEY as in the raw form."""

    @staticmethod
    def _pack(arrays: Sequence[np.ndarray]) -> Tuple[torch.Tensor, np.ndarray]:
        from ._packed_files import pack

        return pack(arrays)  # not pinned: `DataLoader(pin_memory=True)` pins the batch whole

    def __call__(self, batch: Sequence[Optional[Mapping[str, Any]]]) -> Dict[str, Any]:
        from .png_reader import _header_of

        n = len(batch)
        items = [b for b in batch if b is not None]
        if not items:
            raise ValueError("every item of the batch is None")
        items = items + items[: n - len(items)]
        b = len(items)
        none = np.zeros(0, dtype=np.uint8)
        png_files, png_at = self._pack([it[PNG] for it in items])
        decoded, decoded_table = self._pack([none if it.get(DECODED) is None else it[DECODED] for it in items])
        annotations, annotation_table = self._pack([it[ANNOTATION] for it in items])
        png_table = np.zeros((b, 5), dtype=np.int64)
        png_table[:, :2] = png_at
        descs = np.zeros((b, 8), dtype=np.int64)
        frames = np.zeros((b, 8), dtype=np.int32)
        for i, it in enumerate(items):
            H, W = (int(v) for v in it[IMAGE_SHAPE][:2])
            if png_table[i, 1]:
                head = _header_of(bytes(it[PNG][:33]), int(png_table[i, 1]))
                if head is None or head[:2] != (H, W):
                    raise ValueError(f"item {it.get(SAMPLE_INDEX_KEY)}: the PNG's header does not give the item's {H} x {W} image")
                png_table[i, 2:] = head
            elif decoded_table[i, 1] != H * W * 3:
                raise ValueError(f"item {it.get(SAMPLE_INDEX_KEY)}: neither a PNG nor a decoded {H} x {W} RGB image")
            x, y, w, h = (int(v) for v in it[BBOX])
            if w <= 0 or h <= 0 or x < 0 or y < 0 or x + w > W or y + h > H:
                raise ValueError(f"item {it.get(SAMPLE_INDEX_KEY)}: bbox {(x, y, w, h)} does not lie in its {W} x {H} image")
            nh, nw, top, left = self._geometry(h, w)
            descs[i] = ((y * W + x) * 3, h, w, nh, nw, top, left, W * 3)
            frames[i] = (H, x, y, w, h, top, left, 0)
        stack = lambda k, dt: torch.from_numpy(np.stack([np.asarray(it[k], dtype=dt) for it in items]))  # noqa: E731
        return {PNG_FILES: png_files, PNG_TABLE: torch.from_numpy(png_table), DECODED_IMAGES: decoded,
                DECODED_TABLE: torch.from_numpy(decoded_table), ANNOTATIONS: annotations,
                ANNOTATION_TABLE: torch.from_numpy(annotation_table), CROP_DESCS: torch.from_numpy(descs),
                FRAMES: torch.from_numpy(frames), IMAGE_SHAPE: stack(IMAGE_SHAPE, np.int64), INPUT_BBOX_KEY: stack(BBOX, np.int32),
                SAMPLE_INDEX_KEY: torch.tensor([int(it[SAMPLE_INDEX_KEY]) for it in items], dtype=torch.int64),
                IMAGE_FILENAME_KEY: [it[IMAGE_FILENAME_KEY] for it in items]}


class FlameBatchBuilder:
    """A raw batch (CPU, ideally pinned, or already on the device) -> (images [B,3,S,S] float32, targets), on the current
    stream of `device`, with no host sync. A file batch (`FileBatchCollate`) gives the same images and targets, to the bit, from
    the files' bytes: upload, PNG decode to RGB on the device, crops read in place from the decoded images, the annotations
    through `dad3d_annotation_parse`, then the same kernels. The file form waits for the device ONCE per batch: it reads the PNG
    flags and the annotation status together (its small tables go up from pinned memory without blocking; a batch that is not
    pinned blocks in its uploads, as in the raw form). An annotation with a nonzero status is parsed on the host with `_load_mesh`'s code from
    the bytes still in the batch (which raises its own error for a bad file) and its rows are uploaded before
    `dad3d_gt_keypoints` runs; a PNG the device flags is decoded by PIL. `last_fallbacks` counts, for the last call, the items
    that took each: {"annotation_host", "png_host", "png_worker"} (None after a raw batch). A file batch already on the device
    costs one more small copy back, of its tables. `targets` holds what KeypointsDataMixin.get_input keeps (train/mixins.py:30-52):
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
        self.n_verts = int(load_static()["faces"].max()) + 1  # the annotation's vertex count: the packaged FLAME topology's
        self.last_fallbacks: Optional[Dict[str, int]] = None
        self._png = None
        self._range_flag = _lib.ANNOTATION_FLAG_RANGE

    def _up(self, t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
        return t.to(self.device, dtype, non_blocking=True).contiguous()

    def _from_files(self, raw: Mapping[str, Any]):
        """The front of a file batch: (descs, frames, verts, mv, pm) on the device, as the raw form uploads them, and the owners of
        the memory the descriptors point into. The caller holds those until `dad3d_preprocess_images` is enqueued: a block freed
        before that launch could be handed to the very output the launch writes."""
        import io

        from ._packed_files import read_back
        from .png_reader import PngDecoder

        dev = self.device
        if self._png is None:
            self._png = PngDecoder(dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        png_table, decoded_table, ann_table = (raw[k].cpu().numpy() for k in (PNG_TABLE, DECODED_TABLE, ANNOTATION_TABLE))
        b, n = len(ann_table), self.n_verts
        if png_table.shape != (b, 5) or decoded_table.shape != (b, 2) or ann_table.shape != (b, 2) or raw[CROP_DESCS].shape != (b, 8):
            raise ValueError("inconsistent file batch: " + ", ".join(f"{k} {tuple(raw[k].shape)}" for k in
                                                                     (PNG_TABLE, DECODED_TABLE, ANNOTATION_TABLE, CROP_DESCS)))
        text = self._up(raw[ANNOTATIONS], torch.uint8)
        offsets = self._up(raw[ANNOTATION_TABLE][:, 0], torch.int64)
        sizes = self._up(raw[ANNOTATION_TABLE][:, 1], torch.int64)
        decoded = self._up(raw[DECODED_IMAGES], torch.uint8)
        pngs = [i for i in range(b) if png_table[i, 1]]  # the others came decoded
        pending = self._png._launch_packed(raw[PNG_FILES], png_table[pngs, 0], png_table[pngs, 1], 3,
                                           heads=[tuple(int(v) for v in png_table[i, 2:]) for i in pngs])
        verts = torch.empty((b, n, 3), dtype=torch.float32, device=dev)
        mv = torch.empty((b, 4, 4), dtype=torch.float32, device=dev)
        pm = torch.empty((b, 4, 4), dtype=torch.float32, device=dev)
        status = torch.empty(b, dtype=torch.int32, device=dev)
        if text.numel():
            self._check(self._lib.dad3d_annotation_parse(text.data_ptr(), text.numel(), offsets.data_ptr(), sizes.data_ptr(), b, n,
                                                         verts.data_ptr(), mv.data_ptr(), pm.data_ptr(), status.data_ptr(), dev.index, stream))
        else:  # nothing but empty files: the host's parser says so
            status.fill_(self._range_flag)
        (got,), (words,) = read_back([pending], [status])  # the one sync of the file form
        images = pending.finish(*words)
        self.last_fallbacks = {"annotation_host": int((got != 0).sum()),
                               "png_host": int((images.flags != 0).sum()),
                               "png_worker": int((png_table[:, 1] == 0).sum())}
        for i in np.nonzero(got)[0]:  # the host's parser, from the bytes still in the batch
            off, size = (int(v) for v in ann_table[i])
            data = raw[ANNOTATIONS][off:off + size].cpu().numpy().tobytes()
            v, m, p = FlameDataset._mesh_of(io.TextIOWrapper(io.BytesIO(data)))
            if v.shape != (n, 3):
                raise ValueError(f"item {i} of the batch: {v.shape[0]} vertices in the annotation, {n} expected")
            verts[i], mv[i], pm[i] = (torch.from_numpy(t).to(dev) for t in (v, m, p))
        tensors = dict(zip(pngs, images.tensors()))
        bases = []
        for i in range(b):
            if i in tensors:
                H, W = (int(v) for v in png_table[i, 2:4])
                if tuple(tensors[i].shape) != (H, W, 3) or not tensors[i].is_contiguous():
                    raise ValueError(f"item {i} of the batch decoded to {tuple(tensors[i].shape)}, not {(H, W, 3)}")
                bases.append(tensors[i].data_ptr())
            else:
                bases.append(decoded.data_ptr() + int(decoded_table[i, 0]))
        descs = raw[CROP_DESCS].to(dev, torch.int64, non_blocking=True)
        descs = (descs.clone() if descs is raw[CROP_DESCS] else descs).contiguous()  # never edit the caller's batch
        descs[:, 0] += torch.tensor(bases, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
        return (descs, self._up(raw[FRAMES], torch.int32), verts, mv, pm), (pending, images, tensors, decoded)

    def __call__(self, raw: Mapping[str, Any]) -> Tuple[torch.Tensor, Dict[str, Any]]:
        if ANNOTATIONS in raw:
            front, owners = self._from_files(raw)
            built = self._build(raw, *front)
            del owners  # alive up to here: the preprocess launch that reads the decoded images is on the stream
            return built
        self.last_fallbacks = None
        dev = self.device
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
        return self._build(raw, descs, frames, verts, mv, pm)

    def _build(self, raw, descs, frames, verts, mv, pm) -> Tuple[torch.Tensor, Dict[str, Any]]:
        dev, s = self.device, self.img_size
        b, n = verts.shape[:2]
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
