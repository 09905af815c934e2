"""Heads tracked from frame to frame on the device, as 3DDFA_V2 (the project Sim3DR comes from) tracks them: detect once, then take
each frame's box from the previous frame's fit. `HeadTracker.step` is `predict_boxes` on the boxes it holds on the device followed
by ONE launch (`dad3d_boxes_from_heads`, csrc/track_boxes.hip) from the heads' projected vertices to the boxes of the next step,
so a video loop never waits for the device.

A head is lost explicitly and stays lost: the launch zeroes the box of a head it flags (`_lib.TRACK_FLAG_*`: not finite, out of
range, too small, mostly outside its frame), the next `predict_boxes` flags the zero box `BOX_FLAG_EMPTY` without reading a pixel,
and that flag comes back as `TRACK_FLAG_PREVIOUS` at every later step, until `reseed` writes a box that the caller's detector found.
`start` fixes the NUMBER of slots: nothing is compacted, and no detector is part of this.

`update` is where the caller's detector meets the slots, in ONE launch and with no host read (`dad3d_track_assign_detections`,
csrc/track_assign.hip; `boxes.assign_detections` is the rule): detections are matched to live slots one to one, best IoU first; an
unmatched detection that no live slot covers takes a free slot (`start(n_slots=)` reserves spare ones), which moves to the
detection's frame; a live slot the detector has not confirmed for more than `max_misses` searched calls is retired, and lost like
any other lost slot. There is no appearance matching: a slot that drifted onto another head is that head's slot from then on.

Two options, both off by default, steady the loop with one more launch each and still no host wait. `steady` (a
`steady.SteadyConfig`) passes every slot's 3DMM row through a One-Euro filter between the CNN and the decode, in frame coordinates
(crop-space params of different crops do not compare), so the vertices, the projected vertices and with them the next crop are
steadied too; the filter's state is per slot and restarts with the slot. `points` come from the network's 2-D head and stay
unfiltered. `merge_iou` flags the later of two slots that converged on one head `TRACK_FLAG_DUPLICATE` and zeroes its box
(`boxes.suppress_duplicates`): it is then lost like any other lost slot. Which of the two is "right" cannot be known without
appearance; the lower slot wins."""
from __future__ import annotations

from collections import namedtuple
from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, boxes as _boxes
from .steady import OneEuroFilter, SteadyConfig

Assignment = namedtuple("Assignment", "assign det_flags spawned")  # what `HeadTracker.update` returns: device tensors


class HeadTracker:
    def __init__(self, predictor, offset: Any = 0.1, subset: Any = None, min_side: int = 1, min_visible: float = 0.5,
                 steady: Optional[SteadyConfig] = None, merge_iou: Optional[float] = None, pose: bool = False):
        """`predictor`: a `FaceMeshPredictor`. `offset`: what `predict_boxes` widens every box by. `subset`: the vertex indices whose
        bounds are a head's next box (an index list such as the face or head lists of the metrics; None: all vertices, the head box
        the dataset's `bbox` and the training crop are about). `min_side`, `min_visible`: see `boxes.next_boxes`. `steady`: a
        `steady.SteadyConfig` to filter the params with, or None. `merge_iou` in (0, 1]: the IoU from which two slots of one frame
        are one head, or None. With both None every result is what it is without them. `pose`: every result of `step` gains
        `predict_boxes(.., pose=True)`'s `rotation_matrix`, `rpy` and `pose_flags`, on the device. Nothing is launched here."""
        self.pose = bool(pose)
        if steady is not None and not isinstance(steady, SteadyConfig):
            raise ValueError(f"steady: expected a steady.SteadyConfig or None, got {type(steady).__name__}")
        if merge_iou is not None and not 0.0 < float(merge_iou) <= 1.0:  # false for a NaN
            raise ValueError(f"merge_iou {merge_iou} is outside (0, 1]")
        self.steady, self.merge_iou = steady, None if merge_iou is None else float(merge_iou)
        self._filter: Optional[OneEuroFilter] = None
        self.predictor = predictor
        self._factors = _boxes.offset_factors(offset)
        self._offset = offset
        if int(min_side) < 0 or not 0.0 <= float(min_visible) <= 1.0:
            raise ValueError(f"min_side {min_side} is negative or min_visible {min_visible} is outside [0, 1]")
        self.min_side, self.min_visible = int(min_side), float(min_visible)
        self._subset_host = None
        if subset is not None:
            ids = (subset.cpu().numpy() if torch.is_tensor(subset) else np.asarray(subset)).reshape(-1)
            if ids.size == 0 or ids.dtype.kind not in "iu":
                raise ValueError(f"subset: expected a list of vertex indices, got {ids.dtype} {ids.shape}")
            self._subset_host = ids.astype(np.int32)
        self._subset: Optional[torch.Tensor] = None
        self._n_frames: Optional[int] = None
        self._boxes: Optional[torch.Tensor] = None        # int32 [N,4]: the boxes of the next step
        self._index: Optional[torch.Tensor] = None        # int32 [N]: every slot's frame; update moves a spawned slot
        self._track_flags: Optional[torch.Tensor] = None  # int32 [N]: TRACK_FLAG_* of the last step
        self._misses: Optional[torch.Tensor] = None       # int32 [N]: consecutive updates that searched for a slot and did not confirm it

    @property
    def n_slots(self) -> int:
        return 0 if self._boxes is None else int(self._boxes.shape[0])

    def start(self, frames: Sequence[Any], boxes: Any, image_index: Any = None, n_slots: Optional[int] = None) -> None:
        """Fixes the slots: one per box, in box order, each in the frame its `image_index` names, and the number of frames of
        every later `step`. `boxes` and `image_index` in the forms `predict_boxes` takes them. A host box that `predict_boxes`
        would refuse raises ValueError here; device boxes are never looked at on the host (a flagged one is a slot that starts
        lost). The boxes are held as int32, converted toward zero, which is what the tracker's own boxes are.

        `n_slots >= len(boxes)` reserves spare slots behind the boxes' for the heads `update` finds later. A spare slot starts
        lost -- the zero box, `TRACK_FLAG_PREVIOUS`, frame 0 -- so no pixel is read for it. None: one slot per box, as ever."""
        device = self.predictor.device
        if n_slots is not None and (isinstance(n_slots, bool) or not isinstance(n_slots, (int, np.integer))):
            raise ValueError(f"n_slots: expected an integer or None, got {n_slots!r}")
        if torch.is_tensor(boxes):
            if boxes.ndim != 2 or boxes.shape[1] != 4 or boxes.dtype == torch.bool or boxes.is_complex():
                raise ValueError(f"boxes: expected a tensor [N,4] of numbers, got {boxes.dtype} {tuple(boxes.shape)}")
            if not torch.is_tensor(image_index) or tuple(image_index.shape) != (boxes.shape[0],) or image_index.is_floating_point():
                raise ValueError("image_index: device boxes need an integer tensor [N]")
            dev_boxes = boxes.to(device, torch.int32).contiguous().clone()
            dev_index = image_index.to(device, torch.int32).contiguous().clone()
        else:
            flat, index = _boxes.flatten_boxes(len(frames), boxes, image_index)
            shapes = [tuple(int(s) for s in f.shape[:2]) for f in frames]
            _boxes.check_boxes(shapes, flat, index, self._factors, self.predictor._img_size)  # ValueError, nothing launched
            dev_boxes = torch.from_numpy(flat.astype(np.int32)).to(device)
            dev_index = torch.from_numpy(index).to(device)
        given = dev_boxes.shape[0]
        if n_slots is not None and int(n_slots) < given:
            raise ValueError(f"n_slots {n_slots} is below the {given} boxes given")
        total = given if n_slots is None else int(n_slots)
        if self.merge_iou is not None and total > _lib.TRACK_MAX_SLOTS:
            raise ValueError(f"start: {total} slots are more than the {_lib.TRACK_MAX_SLOTS} that merge_iou compares in one launch")
        self._n_frames = len(frames)
        self._track_flags = torch.zeros(total, dtype=torch.int32, device=device)
        if total > given:  # the spare slots: lost from the start
            dev_boxes = torch.cat([dev_boxes, dev_boxes.new_zeros((total - given, 4))])
            dev_index = torch.cat([dev_index, dev_index.new_zeros(total - given)])
            self._track_flags[given:] = _lib.TRACK_FLAG_PREVIOUS
        self._boxes, self._index = dev_boxes, dev_index
        self._misses = torch.zeros(total, dtype=torch.int32, device=device)
        self._subset = None if self._subset_host is None else torch.from_numpy(self._subset_host).to(device)
        self._filter = None
        if self.steady is not None and dev_boxes.shape[0]:
            min_cutoff, beta = self.steady.expand(self.predictor.head_mesh.flame_constants)
            self._filter = OneEuroFilter(dev_boxes.shape[0], len(min_cutoff), min_cutoff, beta, self.steady.d_cutoff, device)

    def step(self, frames: Sequence[Any], dt: Optional[float] = None) -> List[Dict[str, Any]]:
        """One frame set of the video: `predict_boxes(frames, <the held boxes>, device_outputs=True, points_on_device=True)`, then the
        boxes of the next step from these heads, written over the held ones. -> `predict_boxes`'s result dicts, one per slot, all
        values on the device, plus `"track_flags"` (`_lib.TRACK_FLAG_*` of the box this head gave). `"image_index"` is the slot's
        frame for a live head and -1 for a flagged one (box flags or track flags), so `overlay.draw_heads` and `Mesh.render_frames`,
        which skip a head that names no frame, do not draw a lost head's meaningless values. The frames may change size from step
        to step; their number is `start`'s. Nothing here waits for the device.

        With `steady`: `dt` is the time since the last step in seconds (None: `1 / steady.rate`). `"3dmm_params"` is the filtered
        row (with tz := 0 from the decode, as without the filter), `"3d_vertices"`, `"projected_vertices"` and the next boxes come
        from it, and the new key `"3dmm_params_raw"` is the readjusted row before the filter (its tz as the network gave it). A row
        whose box is flagged passes unfiltered and restarts its track. `"points"` are the network's 2-D head's and are not
        filtered. The filter works in frame coordinates: if the frames change size (another video, another scale), call `reset()`.
        With `merge_iou`: a duplicate slot has `TRACK_FLAG_DUPLICATE` in `"track_flags"`, so `"image_index"` -1.
        With `pose`: the pose keys come from `"3dmm_params"`, so with `steady` from the filtered row."""
        if self._boxes is None:
            raise ValueError("step: call start(frames, boxes) first")
        if len(frames) != self._n_frames:
            raise ValueError(f"step: {len(frames)} frames, but start fixed {self._n_frames}")
        pred = self.predictor
        if self.n_slots == 0:
            return []
        staged = pred._stage_frames(frames)
        table = pred._frames_table(staged)
        hook = None
        if self._filter is not None:
            step_dt = self.steady.dt if dt is None else float(dt)
            hook = lambda params, box_flags: self._filter.step(params, box_flags, step_dt, out=params)  # noqa: E731  in place
        batched = pred._predict_boxes_batched(staged, self._boxes, self._index, self._factors, table, params_hook=hook)
        if "projected_vertices" not in batched:
            raise ValueError("step: the predictor's model has no 2-D output, so there are no projected vertices to take boxes from")
        flags = batched["flags"]
        pred._boxes_from_heads_launch(batched["projected_vertices"], table, self._index, flags, self._subset, self.min_side, self.min_visible,
                                      self._boxes, self._track_flags)
        if self.merge_iou is not None:
            pred._suppress_duplicates_launch(self._boxes, self._track_flags, self._index, self.merge_iou)
        track = self._track_flags.clone()  # the results keep this step's flags when the next step writes its own
        drawn = torch.where((flags | track) != 0, torch.full_like(self._index, -1), self._index)
        results = pred._rows_of(batched, True, True, self.pose)
        for i, r in enumerate(results):
            r.update({"bbox": batched["bbox"][i], "image_index": drawn[i], "flags": flags[i], "track_flags": track[i]})
            if hook is not None:
                r["3dmm_params_raw"] = batched["3dmm_params_raw"][i : i + 1]
        return results

    def reseed(self, slots: Any, boxes: Any) -> None:
        """Fresh boxes `[K,4]` for the slots `[K]` that the caller's detector found again: they are the slots' boxes at the next
        step, and the slots' flags are cleared. Host or device arguments; device arguments are never read on the host, so their
        slot numbers are the caller's to keep inside 0 .. n_slots - 1 (host ones outside raise ValueError)."""
        if self._boxes is None:
            raise ValueError("reseed: call start(frames, boxes) first")
        device = self._boxes.device
        if torch.is_tensor(slots):
            if slots.is_floating_point() or slots.ndim != 1:
                raise ValueError(f"slots: expected integers [K], got {slots.dtype} {tuple(slots.shape)}")
            if not slots.is_cuda and slots.numel() and not (0 <= int(slots.min()) and int(slots.max()) < self.n_slots):
                raise ValueError(f"slots: values outside 0 .. {self.n_slots - 1}")
            dev_slots = slots.to(device, torch.int64)
        else:
            ids = np.asarray(slots).reshape(-1)
            if ids.size and (ids.dtype.kind not in "iu" or ids.min() < 0 or ids.max() >= self.n_slots):
                raise ValueError(f"slots: expected integers in 0 .. {self.n_slots - 1}, got {ids.tolist()}")
            dev_slots = torch.from_numpy(ids.astype(np.int64)).to(device)
        fresh = boxes if torch.is_tensor(boxes) else torch.from_numpy(np.asarray(boxes, dtype=np.float64).reshape(-1, 4).astype(np.int32))
        if fresh.ndim != 2 or tuple(fresh.shape) != (dev_slots.shape[0], 4) or fresh.dtype == torch.bool or fresh.is_complex():
            raise ValueError(f"boxes: expected [{dev_slots.shape[0]},4] numbers, got {fresh.dtype} {tuple(fresh.shape)}")
        if dev_slots.shape[0] == 0:
            return
        # slot numbers given on the device were never seen on the host: one outside the slots goes to a spare row and moves nothing
        n = self.n_slots
        rows = torch.where((dev_slots >= 0) & (dev_slots < n), dev_slots, torch.full_like(dev_slots, n))
        spare = torch.zeros((1, 4), dtype=torch.int32, device=device)
        self._boxes.copy_(torch.cat([self._boxes, spare]).index_copy_(0, rows, fresh.to(device, torch.int32))[:n])
        self._track_flags.copy_(torch.cat([self._track_flags, spare[0, :1]]).index_fill_(0, rows, 0)[:n])
        self._misses.copy_(torch.cat([self._misses, spare[0, :1]]).index_fill_(0, rows, 0)[:n])
        if self._filter is not None:
            self._filter.reset(rows)  # a fresh box is a fresh track: the slot's next sample passes unfiltered

    def update(self, det_boxes: Any, det_index: Any = None, count: Any = None, match_iou: float = 0.3, refresh: bool = False,
               max_misses: Optional[int] = None, frame_searched: Any = None, accumulator: Any = None) -> Assignment:
        """What the caller's detector found, into the slots, in ONE launch on the tracker's own boxes, flags, frames and misses
        (`boxes.assign_detections` is the rule): a detection that overlaps a live slot of its frame by at least `match_iou` is
        matched to it, one to one and best IoU first (with `refresh` the slot takes the detection's box); an unmatched detection
        that no live slot covers takes a free slot, which moves to the detection's frame (`ASSIGN_FLAG_SPAWNED`; `ASSIGN_FLAG_FULL`
        if none is free); a live slot whose frame was searched and that no detection matched counts a miss, and with more than
        `max_misses` (None: never) it is retired -- `TRACK_FLAG_RETIRED`, the zero box, lost like any lost slot, free at the next
        update. -> `Assignment(assign, det_flags, spawned)` on the device: per detection its slot (or -1) and `_lib.ASSIGN_FLAG_*`
        (0: matched), per slot 1 where it was spawned -- for a caller that attaches the detector's own attributes to slots.

        Detections in the forms `predict_boxes` takes boxes: one `[k,4]` array per frame, or a flat `[M,4]` array with `det_index
        [M]`, or CUDA tensors `[M,4]` and `[M]` with `count`, an optional CUDA tensor of one integer (how many are real; the rest is
        padding). Host detections are uploaded as int32 (toward zero) and not validated beyond shape and dtype: a bad one comes back
        `ASSIGN_FLAG_INVALID`, as a bad device box does. `frame_searched`: `[n_frames]`, non-zero where the detector looked (None:
        everywhere); a slot of a frame that was not searched counts no miss.

        With `steady` a spawned slot's filter track restarts; with an `accumulator` (`uv_texture.TextureAccumulator`) its texture and
        scores are reset. A matched slot keeps both: it is the same head. Nothing here waits for the device or reads a device value.
        `match_iou=0.3`, and whatever `max_misses` a caller picks, are design choices that nobody has tuned."""
        if self._boxes is None:
            raise ValueError("update: call start(frames, boxes) first")
        device, n_frames = self._boxes.device, self._n_frames
        if not 0.0 < float(match_iou) <= 1.0:  # false for a NaN
            raise ValueError(f"match_iou {match_iou} is outside (0, 1]")
        if max_misses is not None and (isinstance(max_misses, bool) or not isinstance(max_misses, (int, np.integer))):
            raise ValueError(f"max_misses: expected an integer or None, got {max_misses!r}")
        if self.n_slots > _lib.TRACK_MAX_SLOTS:
            raise ValueError(f"update: {self.n_slots} slots are more than the {_lib.TRACK_MAX_SLOTS} one launch takes")
        if accumulator is not None and (not hasattr(accumulator, "reset") or int(getattr(accumulator, "n_slots", 0)) < self.n_slots):
            raise ValueError(f"accumulator: expected a TextureAccumulator of at least {self.n_slots} slots")
        if torch.is_tensor(det_boxes):
            if det_boxes.ndim != 2 or det_boxes.shape[1] != 4 or det_boxes.dtype == torch.bool or det_boxes.is_complex():
                raise ValueError(f"det_boxes: expected a tensor [M,4] of numbers, got {det_boxes.dtype} {tuple(det_boxes.shape)}")
            if not torch.is_tensor(det_index) or tuple(det_index.shape) != (det_boxes.shape[0],) or det_index.is_floating_point():
                raise ValueError("det_index: device detections need an integer tensor [M]")
            dev_dets = det_boxes.to(device, torch.int32).contiguous()
            dev_det_index = det_index.to(device, torch.int32).contiguous()
        else:
            flat, index = _boxes.flatten_boxes(n_frames, det_boxes, det_index)
            with np.errstate(invalid="ignore"):
                dev_dets = torch.from_numpy(flat.astype(np.int32)).to(device)
            dev_det_index = torch.from_numpy(index).to(device)
        if dev_dets.shape[0] > _lib.TRACK_MAX_DETECTIONS:
            raise ValueError(f"update: {dev_dets.shape[0]} detections are more than the {_lib.TRACK_MAX_DETECTIONS} one launch takes")
        dev_count = None
        if torch.is_tensor(count):
            if count.numel() != 1 or count.is_floating_point() or count.dtype == torch.bool:
                raise ValueError(f"count: expected one integer, got {count.dtype} {tuple(count.shape)}")
            dev_count = count.reshape(1).to(device, torch.int32)
        elif count is not None:
            if isinstance(count, bool) or not isinstance(count, (int, np.integer)):
                raise ValueError(f"count: expected an integer, a tensor of one or None, got {count!r}")
            dev_count = torch.tensor([min(max(int(count), -1), 2 ** 31 - 1)], dtype=torch.int32).to(device)
        dev_searched = None
        if frame_searched is not None:
            looked = frame_searched if torch.is_tensor(frame_searched) else torch.from_numpy(np.asarray(frame_searched).reshape(-1) != 0)
            if tuple(looked.shape) != (n_frames,) or looked.is_floating_point():
                raise ValueError(f"frame_searched: expected [{n_frames}] integers or bools, got {tuple(looked.shape)}")
            dev_searched = (looked.to(device) != 0).to(torch.int32)
        assign, det_flags, spawned = self.predictor.assign_detections(
            self._boxes, self._track_flags, self._index, self._misses, dev_dets, dev_det_index, n_frames, match_iou, dev_count, dev_searched,
            refresh, max_misses)
        if self._filter is not None:
            self._filter.reset(mask=spawned)  # a new head in the slot: its next sample passes unfiltered
        if accumulator is not None:
            accumulator.reset(mask=spawned)
        return Assignment(assign, det_flags, spawned)

    def misses(self) -> torch.Tensor:
        """int32 `[N]` on the device: for every slot the consecutive `update` calls that searched its frame and did not confirm it
        (0 after a match, a spawn or a reseed). The tracker's own buffer."""
        if self._misses is None:
            raise ValueError("misses: call start(frames, boxes) first")
        return self._misses

    def reset(self) -> None:
        """Every slot's filter track restarts at the next step (nothing else changes; without `steady` nothing happens). For a
        caller whose frames change size between steps: the filter's state is in the old frames' coordinates. No host wait."""
        if self._filter is not None:
            self._filter.reset()

    def age(self) -> torch.Tensor:
        """int32 `[N]` on the device: how many samples each slot's filter track has seen (0: it restarts at the next step; it stops
        counting at 2^30). The filter's own buffer; ValueError without `steady`."""
        if self._boxes is None:
            raise ValueError("age: call start(frames, boxes) first")
        if self._filter is None:
            raise ValueError("age: the tracker was built without steady")
        return self._filter.age

    def boxes(self) -> torch.Tensor:
        """int32 `[N,4]` on the device: the boxes (x, y, w, h) the next step will use, zero for a lost slot. The tracker's own buffer."""
        if self._boxes is None:
            raise ValueError("boxes: call start(frames, boxes) first")
        return self._boxes

    def lost(self) -> torch.Tensor:
        """int32 `[N]` on the device: the `_lib.TRACK_FLAG_*` of every slot after the last step, 0 for a slot that is tracked. A
        caller reads it when it chooses to wait, for instance every few frames before it runs its detector."""
        if self._track_flags is None:
            raise ValueError("lost: call start(frames, boxes) first")
        return self._track_flags
