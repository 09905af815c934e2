"""Drop-in for the reference's `predictor.FaceMeshPredictor` (predictor.py:68-211) on the MI355X.

Same constructor (`config` dict with `model_path`, `img_size`, `stride`, `constants`; `cuda_id`), same
`__call__(image) -> dict` with the reference's keys, shapes, dtypes and side effects:

    "points"             int ndarray [68,2]     68 2-D landmarks re-adjusted to the input frame (predictor.py:147-152)
    "projected_vertices" Tensor [1,5023,2]      HeadMesh.reprojected_vertices                      (predictor.py:137)
    "3d_vertices"        Tensor [5023,3]        HeadMesh.vertices_3d(...)[0].squeeze()             (predictor.py:136)
    "3dmm_params"        Tensor [1,413]         scale/translation re-adjusted, tz zeroed           (predictor.py:154-176, head_mesh.py:41)

What is different underneath: the CNN runs on PyTorch-ROCm, its 413-vector never leaves HBM
(the reference does `.detach().cpu()`, predictor.py:104), the re-adjustment is a HIP kernel and the TWO
CPU decodes of predictor.py:136-137 are ONE fused HIP launch. `predict_batch` is the batched entry the
reference lacks. Third-party preprocessing (albumentations / cv2, absent here) is ONE HIP kernel for a batch of images
of any sizes (`dad3d_preprocess_images`, csrc/preprocess.hip): LongestMaxSize (cv2 INTER_LINEAR, the 8-bit fixed-point
path) -> PadIfNeeded(centre, 0) -> Normalize(imagenet) -> CHW (predictor.py:80-95,195-203).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, boxes as _boxes
from .head_mesh import HeadMesh
from .heatmap_points import points_from_heatmap, points_from_landmarks
from .resize_geometry import calculate_paddings, py3round  # noqa: F401  (public names of this module)

# keys of the CNN's output dict (model_training/data/config.py:16-23: every constant's value is its own name)
OUTPUT_3DMM_PARAMS = "OUTPUT_3DMM_PARAMS"
OUTPUT_2D_LANDMARKS = "OUTPUT_2D_LANDMARKS"
OUTPUT_LANDMARKS_HEATMAP = "OUTPUT_LANDMARKS_HEATMAP"
_MEAN = (0.485, 0.456, 0.406)
_STD = (0.229, 0.224, 0.225)


def find_3dmm_idx(key: str, consts: Dict[str, int]) -> int:
    idx = 0
    for k, v in consts.items():
        if k == key:
            break
        idx += v
    return idx


class FaceMeshPredictor:
    def __init__(self, config: Dict[str, Any], cuda_id: int = 0, model: Optional[Callable] = None,
                 flame_model: Any = None, flame_path: Optional[str] = None, landmarks: Optional[Sequence[int]] = None):
        self.cuda_id = cuda_id
        self.device = torch.device("cuda", cuda_id)
        self.flame_constants = config["constants"]
        if model is None:  # the reference's path: a TorchScript file under $HOME (predictor.py:72)
            path = os.path.join(os.path.expanduser("~"), config["model_path"])
            if not os.path.isfile(path):
                raise FileNotFoundError(
                    f"{path} not found. The reference downloads it on first use (predictor.py:29-65); there is no "
                    "network here -- place the file there or pass model=<module returning the output dict>.")
            model = torch.jit.load(path)
        self.model = model.to(self.device).eval() if hasattr(model, "to") else model
        self.head_mesh = HeadMesh(self.flame_constants, flame_model=flame_model, flame_path=flame_path,
                                  device=cuda_id, image_size=config["img_size"], landmarks=landmarks)
        self._img_size = config["img_size"]
        self._stride = config.get("stride", 2)
        self._lib = _lib.load()

    @classmethod
    def dad_3dnet(cls, tail: str = "framework", **kwargs):
        """`tail` reaches a `model` that is an `InferenceNet` built for it; the TorchScript checkpoint has no such choice."""
        from .config import load_default_config

        if tail not in ("framework", "hip"):
            raise ValueError(f"dad_3dnet: tail must be 'framework' or 'hip', not {tail!r}")
        if tail == "hip" and kwargs.get("model") is None:
            raise ValueError("dad_3dnet: tail='hip' needs model=InferenceNet(DAD3DNet, tail='hip'): a TorchScript file runs the framework's ops")
        return cls(config=load_default_config(), **kwargs)

    @classmethod
    def random_init(cls, dtype: torch.dtype = torch.bfloat16, seed: int = 0, tune: bool = False, graph: bool = False,
                    tail: str = "framework", **kwargs):
        """DAD-3DNet architecture declared in `network.py` with seeded random weights (no checkpoint offline):
        the real compute and memory footprint of the front half for throughput and plumbing tests. `tail`: InferenceNet's."""
        from .config import load_default_config
        from .network import DAD3DNet, GraphedNet, InferenceNet

        net = InferenceNet(DAD3DNet(seed=seed), dtype, tune=tune, tail=tail)
        device = torch.device("cuda", kwargs.get("cuda_id", 0))
        model = GraphedNet(net.to(device)) if graph else net  # graph=True: one hipGraph per input shape
        return cls(config=load_default_config(), model=model, **kwargs)

    # -- preprocess (predictor.py:86-95,195-203) ---------------------------------------------------------
    def _geometry(self, hw: Tuple[int, int]) -> Tuple[List[int], float, Tuple[int, int]]:
        h, w = hw
        scale = self._img_size / float(max(h, w))
        new_h, new_w = (py3round(d * scale) for d in (h, w))
        return calculate_paddings(new_h, new_w), scale, (new_h, new_w)

    def _preprocess_launch(self, sources: Sequence[Tuple[int, int, int, int]]) -> torch.Tensor:
        """sources: (device address, h, w, row stride in bytes) per image -> float32 [B,3,S,S] on the device, one launch."""
        rows = []
        for ptr, h, w, stride in sources:
            pads, _, (nh, nw) = self._geometry((h, w))
            rows.append([ptr, h, w, nh, nw, pads[0], pads[2], stride])
        descs = torch.tensor(rows, dtype=torch.int64).to(self.device, non_blocking=False)
        out = torch.empty((len(rows), 3, self._img_size, self._img_size), dtype=torch.float32, device=self.device)
        mean, std = (C.c_float * 3)(*_MEAN), (C.c_float * 3)(*_STD)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._lib.dad3d_preprocess_images(descs.data_ptr(), len(rows), self._img_size, mean, std, out.data_ptr(),
                                                     self.cuda_id, stream))
        return out

    def preprocess(self, x: np.ndarray, cache: Dict[str, Any]) -> torch.Tensor:
        cache["input_shape"] = x.shape[:2]
        if x.ndim != 3 or x.shape[2] != 3 or x.dtype != np.uint8:
            raise ValueError(f"expected a uint8 RGB image [H,W,3], got {x.dtype} {x.shape}")
        img = torch.from_numpy(np.ascontiguousarray(x)).to(self.device)
        out = self._preprocess_launch([(img.data_ptr(), x.shape[0], x.shape[1], x.shape[1] * 3)])
        cache["_staged"] = img  # keeps the upload alive until the launch has consumed it (stream order)
        return out

    def process(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        with torch.no_grad():
            return self.model(x)

    # -- postprocess (predictor.py:102-176,188-193) -------------------------------------------------------
    def _landmarks_68(self, out: Dict[str, torch.Tensor], geometry: Any) -> Optional[torch.Tensor]:
        """The 68 points in the input frame, int32 `[B,68,2]` on the device, or None where the model has no 2-D output:
        predictor.py:106-112,132-133,147-152 on the device (heatmap_points.py), with no host wait.
        `geometry`: one (pad_left, pad_top, scale) triple, a float64 `[B,3]` device tensor of them, or the float64 `[B,5]` geometry of
        crops (pad_left, pad_top, scale, x, y), whose points land in the frame."""
        if OUTPUT_2D_LANDMARKS in out:
            return points_from_landmarks(out[OUTPUT_2D_LANDMARKS], geometry, self._img_size)
        if OUTPUT_LANDMARKS_HEATMAP in out:  # unravel_index(sigmoid(heatmap)).flip(-1) * stride (predictor.py:108-112)
            return points_from_heatmap(out[OUTPUT_LANDMARKS_HEATMAP], geometry, self._img_size, self._stride, sigmoid=True)
        return None

    def _readjust(self, params: torch.Tensor, geometry: torch.Tensor) -> None:
        """predictor.py:154-176 in place on the device. `geometry`: float32 `[B,3]` (pad_left, pad_top, scale) of whole images, or the
        float64 `[B,5]` (pad_left, pad_top, scale, x, y) of crops, whose origin `adjust_3dmm_to_paddings` (head_mesh.py:48-60) adds."""
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if geometry.dtype == torch.float64:
            assert tuple(geometry.shape) == (params.shape[0], 5) and geometry.is_contiguous()
            _lib.check(self._lib.dad3d_flame_readjust_params_frame(self.head_mesh.flame._handle, params.data_ptr(), params.shape[0],
                                                                   geometry.data_ptr(), stream))
        else:
            _lib.check(self._lib.dad3d_flame_readjust_params(self.head_mesh.flame._handle, params.data_ptr(), params.shape[0],
                                                             geometry.data_ptr(), 0.0, 0.0, 1.0, stream))

    def _readjust_and_decode(self, params: torch.Tensor, pads_scale: torch.Tensor, device_outputs: bool):
        self._readjust(params, pads_scale)
        out = self.head_mesh.decode(params, verts3d=True, proj=True, to_2d=True, landmarks=False, mutate=True)
        v3d, proj = out["verts3d"], out["proj"]
        if not device_outputs:
            v3d, proj, params = v3d.cpu(), proj.cpu(), params.cpu()
        return v3d, proj, params

    def __call__(self, x: Any) -> Dict[str, Any]:
        res = self.predict_batch([x])[0]
        return res

    def predict_tensor(self, images: torch.Tensor, landmarks_px: bool = True, pose: bool = False) -> Dict[str, torch.Tensor]:
        """Device-resident batch entry: uint8 RGB `[B, H, W, 3]` on this GPU, all images of one size -> device tensors
        `3dmm_params [B,413]`, `3d_vertices [B,5023,3]`, `projected_vertices [B,5023,2]`, `points [B,68,2]` int32
        and, when the head mesh was built with a landmark list, `landmarks [B,n,2]` int32. Nothing is copied to the
        host and nothing synchronises: normalisation, CNN, re-adjustment kernel and the fused decode are queued on
        the current stream (the reference does `.cpu()` after the CNN, predictor.py:104, then decodes twice on the CPU).
        `pose=True` adds `rotation_matrix [B,3,3]` float32, `rpy [B,3]` float64 (roll, pitch, yaw in degrees) and `pose_flags [B]`
        int32 (`_lib.POSE_FLAG_*`) from the returned params: one more launch (`pose.head_pose`), still no wait."""
        assert images.ndim == 4 and images.shape[-1] == 3 and images.dtype == torch.uint8 and images.is_cuda
        b, h, w = images.shape[:3]
        pads, scale, (nh, nw) = self._geometry((h, w))
        images = images.contiguous()
        x = self._preprocess_launch([(images.data_ptr() + i * h * w * 3, h, w, w * 3) for i in range(b)])
        out = self.process(x)
        params = out[OUTPUT_3DMM_PARAMS].detach().to(torch.float32).contiguous().clone()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        # one (pad_left, pad_top, scale) triple for the whole batch: pads_scale == NULL
        _lib.check(self._lib.dad3d_flame_readjust_params(self.head_mesh.flame._handle, params.data_ptr(), b, None,
                                                         float(pads[2]), float(pads[0]), float(scale), stream))
        want_lmk = landmarks_px and self.head_mesh.flame.n_landmarks > 0
        dec = self.head_mesh.decode(params, verts3d=True, proj=True, to_2d=True, landmarks=False, landmarks_px=want_lmk,
                                    mutate=True)
        res = {"3dmm_params": params, "3d_vertices": dec["verts3d"], "projected_vertices": dec["proj"]}
        if want_lmk:
            res["landmarks"] = dec["lmk_px"]
        pts = self._landmarks_68(out, (pads[2], pads[0], scale))  # predictor.py:106-112,147-152 on the device
        if pts is not None:
            res["points"] = pts
        if pose:
            res.update(self._pose_of(params))
        return res

    @staticmethod
    def _pose_of(params: torch.Tensor) -> Dict[str, torch.Tensor]:
        """`rotation_matrix`, `rpy` and `pose_flags` of params rows on the device (`dad3d_head_pose`, one launch, no wait):
        `rot_mat_from_6dof` as the reference computes it and `calculate_rpy`'s angles."""
        from .pose import head_pose

        hp = head_pose(params, want=("rotation", "rpy"))
        return {"rotation_matrix": hp.rotation, "rpy": hp.rpy, "pose_flags": hp.flags}

    def predict_batch(self, images: Sequence[np.ndarray], device_outputs: bool = False,
                      points_on_device: bool = False, pose: bool = False) -> List[Dict[str, Any]]:
        """Batched predictor: list of HxWx3 uint8 RGB arrays (any sizes) -> list of the reference's result dicts. With
        `points_on_device` the `points` are int32 `[68,2]` device tensors; together with `device_outputs` the call makes no
        host wait after the upload. `pose=True`: every dict gains `rotation_matrix` (float32 `[3,3]`, `rot_mat_from_6dof` of the
        returned params), `rpy` (float64 `[3]`: roll, pitch, yaw in degrees, `calculate_rpy`'s values) and `pose_flags`
        (`_lib.POSE_FLAG_*`), computed on the device: device tensors under `device_outputs`, else they come in the params' copy."""
        staged = []
        for im in images:
            if im.ndim != 3 or im.shape[2] != 3 or im.dtype != np.uint8:
                raise ValueError(f"expected uint8 RGB images [H,W,3], got {im.dtype} {im.shape}")
            staged.append(torch.from_numpy(np.ascontiguousarray(im)).to(self.device))
        batch = self._preprocess_launch([(t.data_ptr(), t.shape[0], t.shape[1], t.shape[1] * 3) for t in staged])
        return self._results_of(batch, [im.shape[:2] for im in images], device_outputs, points_on_device, pose)

    # -- frames and bounding boxes (model_training/data/flame_dataset.py:96-99; csrc/preprocess_boxes.hip) -------------------------
    def _input_format(self) -> int:
        """What the preprocess launch writes for `self.model`: the fp16 / bf16 channels-last tensor `InferenceNet.forward` would
        make of the float32 one (its cast and layout pass then find nothing to do), float32 planar for any other model."""
        from .network import GraphedNet, InferenceNet

        net = self.model.net if isinstance(self.model, GraphedNet) else self.model
        if isinstance(net, InferenceNet) and net.dtype in (torch.bfloat16, torch.float16):
            return _lib.PREPROCESS_OUT_BF16_NHWC if net.dtype == torch.bfloat16 else _lib.PREPROCESS_OUT_F16_NHWC
        return _lib.PREPROCESS_OUT_F32_NCHW

    def _stage_frames(self, frames: Sequence[Any]) -> List[torch.Tensor]:
        """uint8 RGB frames as device tensors `[H,W,3]` with a unit pixel stride: an array is uploaded (once, however many boxes it
        carries), a tensor on this device is read where it lies, whatever its row stride."""
        staged = []
        for f in frames:
            if isinstance(f, np.ndarray):
                if f.ndim != 3 or f.shape[2] != 3 or f.dtype != np.uint8:
                    raise ValueError(f"expected uint8 RGB frames [H,W,3], got {f.dtype} {f.shape}")
                staged.append(torch.from_numpy(np.ascontiguousarray(f)).to(self.device))
            elif torch.is_tensor(f) and f.is_cuda:
                if f.ndim != 3 or f.shape[2] != 3 or f.dtype != torch.uint8 or f.device != self.device:
                    raise ValueError(f"expected uint8 RGB frames [H,W,3] on {self.device}, got {f.dtype} {tuple(f.shape)} on {f.device}")
                staged.append(f if f.stride(2) == 1 and f.stride(1) == 3 and f.stride(0) >= 3 * f.shape[1] else f.contiguous())
            else:
                raise ValueError(f"expected numpy arrays or CUDA tensors, got {type(f).__name__}")
            if staged[-1].shape[0] < 1 or staged[-1].shape[1] < 1:
                raise ValueError(f"frame {len(staged) - 1} is empty: {tuple(staged[-1].shape)}")
        return staged

    def _frames_table(self, frames: Sequence[torch.Tensor]) -> torch.Tensor:
        """The int64 `[M,4]` device table {address, h, w, row stride in bytes} of `dad3d_preprocess_boxes` and `dad3d_boxes_from_heads`."""
        return torch.tensor([[t.data_ptr(), t.shape[0], t.shape[1], t.stride(0)] for t in frames], dtype=torch.int64).to(self.device)

    def _preprocess_boxes_launch(self, frames: Sequence[torch.Tensor], boxes: torch.Tensor, image_index: torch.Tensor,
                                 factors: Optional[Tuple[float, float, float, float]], out_format: int = _lib.PREPROCESS_OUT_F32_NCHW,
                                 table: Optional[torch.Tensor] = None):
        """One launch: device frames `[H,W,3]`, device boxes `[N,4]` (int32, int64, float32 or float64) and int32 `image_index [N]` ->
        (network input, crops int32 `[N,4]`, geometry float64 `[N,5]`, flags int32 `[N]`), all on the device; nothing waits.
        `table`: the frames' table where the caller has it already."""
        n, s = boxes.shape[0], self._img_size
        if table is None:
            table = self._frames_table(frames)
        dtype = {_lib.PREPROCESS_OUT_F32_NCHW: torch.float32, _lib.PREPROCESS_OUT_F16_NHWC: torch.float16,
                 _lib.PREPROCESS_OUT_BF16_NHWC: torch.bfloat16}[out_format]
        layout = torch.contiguous_format if out_format == _lib.PREPROCESS_OUT_F32_NCHW else torch.channels_last
        out = torch.empty((n, 3, s, s), dtype=dtype, device=self.device, memory_format=layout)
        crops = torch.empty((n, 4), dtype=torch.int32, device=self.device)
        geometry = torch.empty((n, 5), dtype=torch.float64, device=self.device)
        flags = torch.empty((n,), dtype=torch.int32, device=self.device)
        mean, std = (C.c_float * 3)(*_MEAN), (C.c_float * 3)(*_STD)
        offset = None if factors is None else (C.c_double * 4)(*factors)
        box_dtype = {torch.int32: _lib.BOX_DTYPE_I32, torch.int64: _lib.BOX_DTYPE_I64, torch.float32: _lib.BOX_DTYPE_F32,
                     torch.float64: _lib.BOX_DTYPE_F64}[boxes.dtype]
        assert boxes.is_contiguous() and image_index.is_contiguous() and image_index.dtype == torch.int32
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._lib.dad3d_preprocess_boxes(table.data_ptr(), len(frames), boxes.data_ptr(), box_dtype, image_index.data_ptr(), n,
                                                    offset, s, mean, std, out_format, out.data_ptr(), crops.data_ptr(),
                                                    geometry.data_ptr(), flags.data_ptr(), self.cuda_id, stream))
        return out, crops, geometry, flags

    def predict_boxes(self, frames: Sequence[Any], boxes: Any, image_index: Any = None, offset: Any = 0.1,
                      device_outputs: bool = False, points_on_device: bool = False, pose: bool = False) -> List[Dict[str, Any]]:
        """The heads of frames from bounding boxes, in the frames' coordinates: one result dict per box, in box order, with the
        keys and shapes of `predict_batch` plus `"bbox"` (the crop used, int32 `[4]` as (x, y, w, h)), `"image_index"` and
        `"flags"` (`_lib.BOX_FLAG_*`). No detector is part of this: the boxes are the caller's.

        `frames`: uint8 RGB numpy arrays or CUDA tensors `[H,W,3]` of any sizes; a tensor is read where it lies, with any row
        stride. `boxes` as (x, y, w, h): on the host a list with one `[k_i,4]` array per frame, or one `[N,4]` array with
        `image_index [N]`; or a CUDA tensor `[N,4]` with a CUDA `image_index`. `offset`: what `extend_bbox` takes (one value,
        (w, h) or (left, right, top, bottom)), or None for the boxes as they are.

        Every box becomes the crop the network was trained on -- `extend_bbox`, `ensure_bbox_boundaries` -- and the crops go through
        the predictor's preprocessing in ONE launch that reads them in place (`dad3d_preprocess_boxes`); behind the CNN the params
        are moved into the frame as `adjust_3dmm_to_paddings(params, [y, _, x, _])` does it and the points get (x, y) added, so
        `projected_vertices`, `points` and `3dmm_params` are the frame's; `3d_vertices` do not depend on the frame.

        A host box that the kernel would flag raises ValueError before anything is launched. Device boxes are never looked at on
        the host: flagged rows come back with their flags and with finite, meaningless values, and with `device_outputs` and
        `points_on_device` nothing waits for the device (`bbox`, `image_index` and `flags` are then device tensors too).
        `pose=True`: `predict_batch`'s pose keys, from the params moved into the frame (the move does not touch the rotation)."""
        return self._predict_boxes_staged(self._stage_frames(frames), boxes, image_index, offset, device_outputs, points_on_device, pose)

    def _predict_boxes_staged(self, frames: List[torch.Tensor], boxes: Any, image_index: Any, offset: Any, device_outputs: bool,
                              points_on_device: bool, pose: bool = False) -> List[Dict[str, Any]]:
        factors = _boxes.offset_factors(offset)
        if torch.is_tensor(boxes):
            if not boxes.is_cuda or boxes.ndim != 2 or boxes.shape[1] != 4 or boxes.dtype == torch.bool or boxes.is_complex():
                raise ValueError(f"boxes: expected a CUDA tensor [N,4] of numbers, got {boxes.dtype} {tuple(boxes.shape)} on {boxes.device}")
            if not torch.is_tensor(image_index) or not image_index.is_cuda or tuple(image_index.shape) != (boxes.shape[0],) \
                    or image_index.is_floating_point():
                raise ValueError("image_index: device boxes need a CUDA integer tensor [N]")
            known = (torch.int32, torch.int64, torch.float32, torch.float64)
            dev_boxes = (boxes if boxes.dtype in known else boxes.to(torch.float64)).to(self.device).contiguous()
            dev_index = image_index.to(self.device, torch.int32).contiguous()
        else:
            flat, index = _boxes.flatten_boxes(len(frames), boxes, image_index)
            _boxes.check_boxes([tuple(t.shape[:2]) for t in frames], flat, index, factors, self._img_size)  # ValueError, nothing launched
            dev_boxes, dev_index = torch.from_numpy(flat).to(self.device), torch.from_numpy(index).to(self.device)
        if dev_boxes.shape[0] == 0:
            return []
        batched = self._predict_boxes_batched(frames, dev_boxes, dev_index, factors)
        crops, flags = batched["bbox"], batched["flags"]
        results = self._rows_of(batched, device_outputs, points_on_device, pose)
        if device_outputs and points_on_device:  # no wait: the side outputs stay where they are
            for i, r in enumerate(results):
                r.update({"bbox": crops[i], "image_index": dev_index[i], "flags": flags[i]})
        else:
            side = torch.cat([crops, dev_index[:, None], flags[:, None]], dim=1).cpu().numpy()  # one copy
            for i, r in enumerate(results):
                r.update({"bbox": side[i, :4].copy(), "image_index": int(side[i, 4]), "flags": int(side[i, 5])})
        return results

    def predict_files(self, sources: Sequence[Any], device_outputs: bool = False, jpeg_entropy: str = "segments",
                      points_on_device: bool = False, boxes: Any = None, image_index: Any = None,
                      offset: Any = 0.1, pose: bool = False) -> List[Dict[str, Any]]:
        """`predict_batch` fed with image files (paths or bytes, any sizes): PNG files and baseline JPEG files are decoded to RGB
        on the device (png_reader.PngDecoder, jpeg_reader.JpegDecoder, channels=3) and the decoded images go to the preprocess launch
        where they lie, so no decoded pixel crosses the bus. A source that starts FF D8 goes to the JPEG decoder, every other one
        to the PNG decoder; where both kinds are present their flags are read in one wait. A file a decoder flags (a progressive
        JPEG, a palette PNG, ...) is decoded by PIL on the host and uploaded. The result dicts are those of `predict_batch` on
        `np.asarray(Image.open(f).convert("RGB"))`, in the order of `sources`; what follows the preprocess launch is
        `predict_batch`'s own code. `jpeg_entropy` is `JpegDecoder`'s `entropy`: "sync" decodes a JPEG file without restart markers
        in pieces, to the same pixels. With `boxes` (and `image_index`, `offset`) the files are frames and the call is `predict_boxes`
        on them. `pose`: as in `predict_batch`."""
        from ._packed_files import bytes_of, read_back
        from .jpeg_reader import SOI, JpegDecoder
        from .png_reader import PngDecoder

        files = [bytes_of(s) for s in sources]
        jpegs = [i for i, f in enumerate(files) if f[:2] == SOI]
        if not jpegs:
            decoded = PngDecoder(self.device).decode(files, channels=3).tensors()  # alive until the launch has consumed them
        else:
            pngs = [i for i in range(len(files)) if i not in set(jpegs)]
            jpeg = JpegDecoder(self.device, entropy=jpeg_entropy)._launch([files[i] for i in jpegs], 3)
            png = PngDecoder(self.device)._launch([files[i] for i in pngs], 3) if pngs else None
            decoded = [None] * len(files)
            for pending, words, where in zip((jpeg, png), read_back([jpeg, png])[1], (jpegs, pngs)):  # the one wait
                if pending is not None:
                    for i, t in zip(where, pending.finish(*words).tensors()):
                        decoded[i] = t
        if boxes is not None:  # the decoded frames stay on the device; the crops are read from them in place
            return self._predict_boxes_staged(self._stage_frames(decoded), boxes, image_index, offset, device_outputs, points_on_device, pose)
        batch = self._preprocess_launch([(t.data_ptr(), t.shape[0], t.shape[1], t.stride(0)) for t in decoded])
        return self._results_of(batch, [tuple(t.shape[:2]) for t in decoded], device_outputs, points_on_device, pose)

    def _results_of(self, batch: torch.Tensor, shapes: Sequence[Tuple[int, int]], device_outputs: bool,
                    points_on_device: bool = False, pose: bool = False) -> List[Dict[str, Any]]:
        """What `predict_batch` does behind its preprocess launch, for images of the sizes `shapes` = [(h, w)]."""
        geo = [self._geometry(s) for s in shapes]
        # both uploads in front of the CNN. The points need the scale as the float64 it is (predictor.py:151); the params kernel reads float32
        pads_scale = torch.tensor([[g[0][2], g[0][0], g[1]] for g in geo], dtype=torch.float32, device=self.device)
        geometry = torch.tensor([[g[0][2], g[0][0], g[1]] for g in geo], dtype=torch.float64).to(self.device)
        return self._results_from(batch, pads_scale, geometry, device_outputs, points_on_device, pose)

    def _results_from(self, batch: torch.Tensor, pads_scale: torch.Tensor, geometry: torch.Tensor, device_outputs: bool,
                      points_on_device: bool, pose: bool = False) -> List[Dict[str, Any]]:
        """The CNN and everything behind it. `pads_scale` is what `_readjust` takes and `geometry` what `_landmarks_68` takes: for
        crops both are the float64 `[B,5]` geometry of `dad3d_preprocess_boxes`."""
        return self._rows_of(self._batched_from(batch, pads_scale, geometry), device_outputs, points_on_device, pose)

    def _batched_from(self, batch: torch.Tensor, pads_scale: torch.Tensor, geometry: torch.Tensor,
                      params_hook: Optional[Callable[[torch.Tensor], torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """`_results_from` before the results are cut into rows: the device tensors `3dmm_params [N,413]` and, where the model has a
        2-D output, `points [N,68,2]` int32, `projected_vertices [N,5023,2]` and `3d_vertices [N,5023,3]`. Nothing waits.
        `params_hook` (private, for `tracking.HeadTracker`): called with the readjusted params `[N,413]` between `_readjust` and the
        decode, it returns the params to decode (a contiguous float32 device tensor; the argument itself, changed in place, is
        fine), so the decode still runs once; `3dmm_params_raw` is then the readjusted rows as the hook received them. The points
        come from the network's 2-D head and do not pass the hook."""
        out = self.process(batch)
        params = out[OUTPUT_3DMM_PARAMS].detach().to(self.device, torch.float32).contiguous().clone()
        pts = self._landmarks_68(out, geometry)
        if params_hook is not None:
            if pts is None:  # nothing to decode for: the hook's state is not advanced for a result its caller cannot use
                raise ValueError("params_hook: the predictor's model has no 2-D output, so there is no decode to stand in front of")
            self._readjust(params, pads_scale)
            raw = params.clone()
            params = params_hook(params)
            dec = self.head_mesh.decode(params, verts3d=True, proj=True, to_2d=True, landmarks=False, mutate=True)
            return {"points": pts, "projected_vertices": dec["proj"], "3d_vertices": dec["verts3d"], "3dmm_params": params, "3dmm_params_raw": raw}
        if pts is None:  # `return {"3dmm_params": ...}` branch of predictor.py:144-145
            self._readjust(params, pads_scale)
            return {"3dmm_params": params}
        v3d, proj, params = self._readjust_and_decode(params, pads_scale, True)
        return {"points": pts, "projected_vertices": proj, "3d_vertices": v3d, "3dmm_params": params}

    @classmethod
    def _rows_of(cls, batched: Dict[str, torch.Tensor], device_outputs: bool, points_on_device: bool, pose: bool = False) -> List[Dict[str, Any]]:
        """One result dict per row of `_batched_from`'s tensors, copied to the host first unless the caller keeps them on the device.
        `pose`: the rows' `rotation_matrix`, `rpy` and `pose_flags` too, computed on the device from `3dmm_params`."""
        dev_params = batched["3dmm_params"]
        n = dev_params.shape[0]
        extra: List[Dict[str, Any]] = [{} for _ in range(n)]
        if pose:
            found = cls._pose_of(dev_params)
            rot, rpy, pflags = found["rotation_matrix"], found["rpy"], found["pose_flags"]
            if device_outputs:
                params = dev_params
            else:  # the params' copy carries the pose: the rows' bytes side by side, cut apart on the host
                packed = torch.cat([dev_params.view(torch.uint8), rot.reshape(n, 9).view(torch.uint8), rpy.view(torch.uint8),
                                    pflags[:, None].view(torch.uint8)], dim=1).cpu()
                parts = [part.contiguous() for part in packed.split([dev_params.shape[1] * 4, 36, 24, 4], dim=1)]
                params = parts[0].view(torch.float32)
                rot, rpy, pflags = parts[1].view(torch.float32).reshape(n, 3, 3), parts[2].view(torch.float64), parts[3].view(torch.int32)[:, 0].tolist()
            extra = [{"rotation_matrix": rot[i], "rpy": rpy[i], "pose_flags": pflags[i]} for i in range(n)]
        else:
            params = dev_params if device_outputs else dev_params.cpu()
        if "points" not in batched:
            return [{"3dmm_params": params[i : i + 1], **extra[i]} for i in range(n)]
        pts, proj, v3d = batched["points"], batched["projected_vertices"], batched["3d_vertices"]
        if not device_outputs:
            v3d, proj = v3d.cpu(), proj.cpu()
        if not points_on_device:
            pts = pts.cpu().numpy().astype(int)  # one copy; `astype(int)` is the reference's dtype (predictor.py:152)
        return [{"points": pts[i], "projected_vertices": proj[i : i + 1], "3d_vertices": v3d[i], "3dmm_params": params[i : i + 1], **extra[i]}
                for i in range(n)]

    def _predict_boxes_batched(self, frames: List[torch.Tensor], dev_boxes: torch.Tensor, dev_index: torch.Tensor,
                               factors: Optional[Tuple[float, float, float, float]], table: Optional[torch.Tensor] = None,
                               params_hook: Optional[Callable[[torch.Tensor, torch.Tensor], torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """What stands behind `predict_boxes`, uncut: `_batched_from`'s device tensors in frame coordinates plus `bbox [N,4]` (the
        crops used), `flags [N]` and `image_index [N]`, int32. Staged frames, device boxes and index; nothing waits.
        `params_hook(params, flags)`: `_batched_from`'s hook, given the rows' box flags too."""
        batch, crops, geometry, flags = self._preprocess_boxes_launch(frames, dev_boxes, dev_index, factors, self._input_format(), table)
        batched = self._batched_from(batch, geometry, geometry, None if params_hook is None else (lambda p: params_hook(p, flags)))
        batched.update({"bbox": crops, "flags": flags, "image_index": dev_index})
        return batched

    def next_boxes(self, results_or_proj: Any, frames: Sequence[Any], image_index: Any = None, prev_flags: Any = None, subset: Any = None,
                   min_side: int = 1, min_visible: float = 0.5, merge_iou: Optional[float] = None):
        """The boxes of the next `predict_boxes` call from the heads of this one, the tracking step of 3DDFA_V2: each head's box is the
        integer bounds of its projected vertices (`subset`: vertex indices, None for all 5023, the head box the dataset's `bbox` and
        the training crop are about), zeroed and flagged `_lib.TRACK_FLAG_*` where the head is lost -- see `boxes.next_boxes` for
        the rule. -> (boxes int32 `[N,4]` as (x, y, w, h), flags int32 `[N]`).

        `results_or_proj`: the list of dicts `predict_boxes` returned (`image_index` and `prev_flags` then default to the dicts' own
        `image_index` and `flags`), or `projected_vertices` stacked as `[N,V,2]` / `[N,V,3]`. `frames`: the frames (only their sizes
        matter: arrays, tensors or (h, w) pairs). Device values go through ONE launch (`dad3d_boxes_from_heads`) and nothing waits
        for the device; host values go through the same rule in numpy. Give the boxes to the next call with the same `image_index`:
        a zeroed box comes back flagged `BOX_FLAG_EMPTY`, and with that flag as `prev_flags` the head stays lost until it gets a
        fresh box from the caller's detector.

        `merge_iou` in (0, 1]: of two boxes of one frame that overlap by at least this IoU the later one is flagged
        `TRACK_FLAG_DUPLICATE` and zeroed (`boxes.suppress_duplicates`; one more launch for device values, which takes at most
        `_lib.TRACK_MAX_SLOTS` heads -- the kernel's limit; host values have none). None: no box is compared with another."""
        if merge_iou is not None and not 0.0 < float(merge_iou) <= 1.0:
            raise ValueError(f"merge_iou {merge_iou} is outside (0, 1]")
        if isinstance(results_or_proj, (list, tuple)):
            dicts = list(results_or_proj)
            if not dicts:
                return np.zeros((0, 4), np.int32), np.zeros(0, np.int32)
            if image_index is None:
                image_index = [d["image_index"] for d in dicts]
            if prev_flags is None:
                prev_flags = [d["flags"] for d in dicts]
            proj = torch.cat([d["projected_vertices"] for d in dicts])
            on_device = proj.is_cuda
            image_index, prev_flags = (torch.stack([v.reshape(()) for v in seq])  # the dicts' 0-d device values: gathered on the device
                                       if on_device and isinstance(seq, list) and all(torch.is_tensor(v) and v.is_cuda for v in seq) else seq
                                       for seq in (image_index, prev_flags))
        else:
            proj = results_or_proj
            on_device = torch.is_tensor(proj) and proj.is_cuda
        if image_index is None:
            raise ValueError("image_index: needed with projected vertices (the result dicts carry their own)")
        if not on_device:
            shapes = [tuple(int(s) for s in (f.shape[:2] if hasattr(f, "shape") else f[:2])) for f in frames]
            host = [None if v is None else v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v) for v in (image_index, prev_flags, subset)]
            proj = proj.numpy() if torch.is_tensor(proj) else np.asarray(proj)
            found = _boxes.next_boxes(np.ascontiguousarray(proj, dtype=np.float32), shapes, host[0], host[1], host[2], min_side, min_visible)
            return found if merge_iou is None else _boxes.suppress_duplicates(found[0], found[1], host[0], merge_iou)
        # the kernel reads no pixel: a frame given by its size alone gets a placeholder address, which only says that the frame exists
        table = torch.tensor([[f.data_ptr(), f.shape[0], f.shape[1], f.stride(0)] if torch.is_tensor(f) else
                              [1, *(int(s) for s in (f.shape[:2] if hasattr(f, "shape") else f[:2])), 0] for f in frames], dtype=torch.int64).to(self.device)
        n = proj.shape[0]
        out_boxes = torch.empty((n, 4), dtype=torch.int32, device=self.device)
        out_flags = torch.empty((n,), dtype=torch.int32, device=self.device)
        if merge_iou is not None and n > _lib.TRACK_MAX_SLOTS:
            raise ValueError(f"merge_iou: {n} heads are more than the {_lib.TRACK_MAX_SLOTS} the duplicate rule compares in one launch")
        dev_index = self._dev_int32(image_index, n, "image_index")
        self._boxes_from_heads_launch(proj, table, dev_index,
                                      None if prev_flags is None else self._dev_int32(prev_flags, n, "prev_flags"),
                                      None if subset is None else self._dev_int32(subset, None, "subset"), min_side, min_visible, out_boxes, out_flags)
        if merge_iou is not None:
            self._suppress_duplicates_launch(out_boxes, out_flags, dev_index, merge_iou)
        return out_boxes, out_flags

    def _suppress_duplicates_launch(self, boxes: torch.Tensor, flags: torch.Tensor, image_index: torch.Tensor, merge_iou: float) -> None:
        """`dad3d_track_suppress_duplicates` on the current stream, in place on `boxes` int32 `[N,4]` and `flags [N]` as
        `_boxes_from_heads_launch` left them: one launch, nothing is read on the host."""
        n = boxes.shape[0]
        for t, shape in ((boxes, (n, 4)), (flags, (n,)), (image_index, (n,))):
            assert t.dtype == torch.int32 and t.is_contiguous() and t.device == self.device and tuple(t.shape) == shape, (t.dtype, tuple(t.shape))
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._lib.dad3d_track_suppress_duplicates(boxes.data_ptr(), flags.data_ptr(), image_index.data_ptr(), n, float(merge_iou),
                                                             self.cuda_id, stream))

    def assign_detections(self, boxes: torch.Tensor, flags: torch.Tensor, image_index: torch.Tensor, misses: Optional[torch.Tensor],
                          det_boxes: torch.Tensor, det_index: torch.Tensor, n_frames: int, match_iou: float,
                          count: Optional[torch.Tensor] = None, frame_searched: Optional[torch.Tensor] = None, refresh: bool = False,
                          max_misses: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """A detector's boxes against tracked slots, on the device: `dad3d_track_assign_detections` on the current stream, ONE launch,
        the rule of `boxes.assign_detections`. In place on the slot state -- `boxes` int32 `[N,4]`, `flags [N]`, `image_index [N]`
        and `misses [N]` (or None: nothing is counted, nothing retires) -- from `det_boxes` int32 `[M,4]`, `det_index [M]`, `count`
        (an int32 tensor of one element on the device: how many detections are real; None: all) and `frame_searched [n_frames]` (None:
        every frame). All contiguous int32 tensors on this device; at most `_lib.TRACK_MAX_SLOTS` slots and
        `_lib.TRACK_MAX_DETECTIONS` detections (the kernel's limits). -> (assign `[M]`, det_flags `[M]`, spawned `[N]`), new device
        tensors. Nothing is read on the host. `match_iou` and `max_misses` are the caller's choices; nobody has tuned them."""
        n, m, n_frames = boxes.shape[0], det_boxes.shape[0], int(n_frames)
        if not 0.0 < float(match_iou) <= 1.0:  # false for a NaN
            raise ValueError(f"match_iou {match_iou} is outside (0, 1]")
        if n > _lib.TRACK_MAX_SLOTS or m > _lib.TRACK_MAX_DETECTIONS:
            raise ValueError(f"{n} slots and {m} detections: one launch takes {_lib.TRACK_MAX_SLOTS} and {_lib.TRACK_MAX_DETECTIONS}")
        if n_frames < 1:
            raise ValueError(f"n_frames {n_frames} is below 1")
        if max_misses is not None and int(max_misses) >= 0 and misses is None:
            raise ValueError(f"max_misses {max_misses} needs the misses it counts")
        for name, t, shape in (("boxes", boxes, (n, 4)), ("flags", flags, (n,)), ("image_index", image_index, (n,)), ("misses", misses, (n,)),
                               ("det_boxes", det_boxes, (m, 4)), ("det_index", det_index, (m,)), ("count", count, None),
                               ("frame_searched", frame_searched, (n_frames,))):
            if t is None and name in ("misses", "count", "frame_searched"):
                continue
            if not torch.is_tensor(t) or t.dtype != torch.int32 or t.device != self.device or not t.is_contiguous() \
                    or (tuple(t.shape) != shape if shape is not None else t.numel() != 1):
                raise ValueError(f"{name}: expected a contiguous int32 tensor {list(shape) if shape else '[1]'} on {self.device}, got "
                                 f"{getattr(t, 'dtype', type(t).__name__)} {tuple(getattr(t, 'shape', ()))}")
        assign = torch.empty((m,), dtype=torch.int32, device=self.device)
        det_flags = torch.empty((m,), dtype=torch.int32, device=self.device)
        spawned = torch.empty((n,), dtype=torch.int32, device=self.device)
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._lib.dad3d_track_assign_detections(
            boxes.data_ptr(), flags.data_ptr(), image_index.data_ptr(), ptr(misses), n, det_boxes.data_ptr(), det_index.data_ptr(), ptr(count), m,
            ptr(frame_searched), n_frames, float(match_iou), int(bool(refresh)), -1 if max_misses is None else int(max_misses),
            assign.data_ptr(), det_flags.data_ptr(), spawned.data_ptr(), self.cuda_id, stream))
        return assign, det_flags, spawned

    def _dev_int32(self, values: Any, n: Optional[int], name: str) -> torch.Tensor:
        """Integers as a contiguous int32 tensor `[n]` on this device: a tensor is converted where it lies, host values are uploaded."""
        t = values if torch.is_tensor(values) else torch.from_numpy(np.asarray(values).reshape(-1).astype(np.int32))
        if t.is_floating_point() or t.ndim != 1 or (n is not None and t.shape[0] != n):
            raise ValueError(f"{name}: expected integers [{'K' if n is None else n}], got {t.dtype} {tuple(t.shape)}")
        return t.to(self.device, torch.int32).contiguous()

    def _boxes_from_heads_launch(self, proj: torch.Tensor, table: torch.Tensor, image_index: torch.Tensor, prev_flags: Optional[torch.Tensor],
                                 subset: Optional[torch.Tensor], min_side: int, min_visible: float, out_boxes: torch.Tensor,
                                 out_flags: torch.Tensor) -> None:
        """`dad3d_boxes_from_heads` on the current stream: `proj` float32 `[N,V,2|3]` on this device with a unit last stride (any
        head and vertex strides), int32 device vectors, the frames' table; writes `out_boxes [N,4]` and `out_flags [N]` in place."""
        if proj.ndim != 3 or proj.shape[2] not in (2, 3) or proj.dtype != torch.float32 or proj.device != self.device:
            raise ValueError(f"projected vertices: expected float32 [N,V,2] or [N,V,3] on {self.device}, got {proj.dtype} {tuple(proj.shape)}")
        if proj.shape[0] and (proj.stride(2) != 1 or proj.stride(1) < 2 or proj.stride(0) < 0):
            proj = proj.contiguous()
        n, v = proj.shape[:2]
        assert out_boxes.is_contiguous() and out_boxes.dtype == torch.int32 and tuple(out_boxes.shape) == (n, 4)
        assert out_flags.is_contiguous() and out_flags.dtype == torch.int32 and tuple(out_flags.shape) == (n,)
        for t, shape in ((image_index, (n,)), (prev_flags, (n,)), (subset, None)):
            assert t is None or (t.dtype == torch.int32 and t.is_contiguous() and t.device == self.device and t.ndim == 1
                                 and (shape is None or tuple(t.shape) == shape)), (t.dtype, tuple(t.shape))
        assert table.dtype == torch.int64 and table.is_contiguous() and table.ndim == 2 and table.shape[1] == 4
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._lib.dad3d_boxes_from_heads(proj.data_ptr(), n, v, proj.stride(0), proj.stride(1),
                                                    None if subset is None else subset.data_ptr(), 0 if subset is None else subset.shape[0],
                                                    table.data_ptr(), table.shape[0], image_index.data_ptr(),
                                                    None if prev_flags is None else prev_flags.data_ptr(), int(min_side), float(min_visible),
                                                    out_boxes.data_ptr(), out_flags.data_ptr(), self.cuda_id, stream))
