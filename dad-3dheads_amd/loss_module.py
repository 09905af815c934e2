"""`model_training/train/loss_module.py` `LossModule`: weights, schedules and sums the training criteria. `from_config` takes
the already-resolved `loss` block of `config/loss/train_loss.yaml` (no hydra) and maps the reference's `_target_` strings to
this package's HIP criteria."""
from __future__ import annotations

from typing import Any, Dict, List, Mapping, Optional, Tuple, Union

import torch
from torch import Tensor, nn

from .losses import IoULoss, LandmarksLossWVisibility, ReprojectionLoss, Vertices3DLoss

__all__ = ["LossModule", "CRITERIA"]

CRITERIA = {
    "model_training.losses.IoULoss": IoULoss,
    "model_training.losses.Vertices3DLoss": Vertices3DLoss,
    "model_training.losses.ReprojectionLoss": ReprojectionLoss,
    "model_training.losses.LandmarksLossWVisibility": LandmarksLossWVisibility,
}
_MESH_CRITERIA = (Vertices3DLoss, ReprojectionLoss)


class LossModule(nn.Module):
    def __init__(self, names: List[str], output_keys: List[Any], target_keys: List[Any], criterions: List[nn.Module],
                 weights: List[float], schedule: List[int], reduction: str = "sum") -> None:
        super().__init__()
        self.criterions = nn.ModuleList(criterions)
        self.names = names
        self.weights = weights
        self.output_keys = output_keys
        self.target_keys = target_keys
        self.reduction = reduction
        self.schedule = schedule

    def _get_values(self, values: Union[Tensor, Dict[str, Tensor]], key: Union[None, str, List[str]]) -> Union[Tensor, List[Tensor]]:
        if torch.is_tensor(values) and key is None:
            return values
        if isinstance(values, Mapping) and isinstance(key, str):
            return values[key]
        if isinstance(values, Mapping) and isinstance(key, list):
            return [values[k] for k in key]
        raise ValueError(f"Unsupported combination of values {type(values)} and key {key}")

    def forward(self, predictions: Union[Tensor, Dict[str, Tensor]], targets: Union[Tensor, Dict[str, Tensor]],
                epoch: int) -> Tuple[Tensor, Dict[str, Tensor]]:
        losses_dict: Dict[str, Tensor] = {}
        losses: List[Tensor] = []
        for name, criterion, weight, predicted_key, target_key, epoch_start in zip(
                self.names, self.criterions, self.weights, self.output_keys, self.target_keys, self.schedule):
            if epoch >= epoch_start:
                joint = {**predictions, **targets}
                loss = criterion(self._get_values(joint, predicted_key), self._get_values(joint, target_key)) * weight
                losses_dict[name] = loss
                losses.append(loss)
        stack = torch.stack(losses)
        if self.reduction == "sum":
            total = stack.sum()
        elif self.reduction == "mean":
            total = stack.mean()
        elif self.reduction == "none":
            total = stack
        else:
            raise ValueError(f"Unsupported reduction value {self.reduction}")
        return total, losses_dict

    @staticmethod
    def from_config(config: Mapping[str, Any], head_mesh_kwargs: Optional[Mapping[str, Any]] = None) -> "LossModule":
        """loss_module.py:72-109 on a resolved dict. `head_mesh_kwargs` (flame_model, static, device, ...) go to the two mesh
        criteria, as extra keyword arguments of their HeadMesh."""
        names, output_keys, target_keys, criterions, weights, schedule = [], [], [], [], [], []
        for criterion in config["criterions"]:
            spec = dict(criterion["loss"])
            target = spec.pop("_target_")
            if target not in CRITERIA:
                raise ValueError(f"no HIP criterion for {target!r} (known: {sorted(CRITERIA)})")
            cls = CRITERIA[target]
            if cls in _MESH_CRITERIA:
                spec.update(head_mesh_kwargs or {})
            names.append(criterion["name"])
            output_keys.append(criterion.get("output_key", None))
            target_keys.append(criterion["target_key"])
            criterions.append(cls(**spec))
            weights.append(criterion.get("weight", float(1.0)))
            schedule.append(criterion.get("epoch_start", 0))
        return LossModule(names=names, output_keys=output_keys, target_keys=target_keys, weights=weights, criterions=criterions,
                          reduction=config.get("reduction", "sum"), schedule=schedule)
