"""Steady tracks: a One-Euro filter (Casiez, Roussel, Vogel 2012) over rows of float32 values whose state lives on the device, so a
tracker's 3DMM params are smoothed between the CNN and the decode with no host wait (`tracking.HeadTracker(steady=...)`).

`one_euro_rows` is the rule in numpy float32 and `OneEuroFilter` the device form, ONE launch a step (`dad3d_one_euro_rows`,
csrc/track_steady.hip), held to the numpy rule bit for bit. The rule is stated on three float32 scalars the host computes once per
call (`one_euro_scalars`), so both forms start from the same bits; include/dad3d.h has it in full. `SteadyConfig` spreads
per-group filter constants over the 413 entries of a 3DMM row."""
from __future__ import annotations

import math
from typing import Any, Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .flame import _SLICE_ORDER, FLAME_CONSTS

AGE_MAX = 2 ** 30

# Untuned design choices, not measurements: neither a video nor the trained checkpoint is at hand. (min_cutoff in Hz, beta.)
# The identity barely moves within a track, so the shape gets a very low cutoff; expression and jaw move fast and are kept
# responsive; the pose follows speed (beta > 0), which is what the One-Euro filter is for.
DEFAULT_GROUPS: Dict[str, Tuple[float, float]] = {
    "shape": (0.05, 0.0), "expression": (2.0, 0.0), "jaw": (2.0, 0.0),
    "rotation": (1.0, 0.5), "translation": (1.0, 0.5), "scale": (1.0, 0.5),
}
DEFAULT_OTHER: Tuple[float, float] = (1.0, 0.0)  # anything else: eyeballs, neck


def one_euro_scalars(dt: float, d_cutoff: float = 1.0) -> Tuple[np.float32, np.float32, np.float32]:
    """(rate, two_pi_dt, alpha_d) as float32, each computed in float64 and rounded once: `rate = 1/dt`, `two_pi_dt = 2 pi dt`,
    `alpha_d = r_d / (r_d + 1)` with `r_d = 2 pi d_cutoff dt`. ValueError unless all three are finite and positive."""
    dt, d_cutoff = float(dt), float(d_cutoff)
    if not (dt > 0.0 and math.isfinite(dt) and d_cutoff > 0.0 and math.isfinite(d_cutoff)):
        raise ValueError(f"dt {dt} and d_cutoff {d_cutoff} must be finite and positive")
    r_d = 2.0 * math.pi * d_cutoff * dt
    with np.errstate(over="ignore"):
        scalars = (np.float32(1.0 / dt), np.float32(2.0 * math.pi * dt), np.float32(r_d / (r_d + 1.0)))
    if not all(np.isfinite(s) and s > 0 for s in scalars):
        raise ValueError(f"dt {dt}: a scalar of the rule is not a positive float32 {tuple(float(s) for s in scalars)}")
    return scalars


def _constants(values: Any, d: int, name: str, positive: bool) -> np.ndarray:
    v = np.asarray(values, dtype=np.float32).reshape(-1)
    if v.size == 1:
        v = np.full(d, v[0], np.float32)
    if v.shape != (d,) or not np.all(np.isfinite(v)) or not (np.all(v > 0) if positive else np.all(v >= 0)):
        raise ValueError(f"{name}: expected {d} finite values {'> 0' if positive else '>= 0'}")
    return np.ascontiguousarray(v)


def one_euro_rows(x, state_x, state_dx, age, min_cutoff, beta, scalars, flags=None) -> np.ndarray:
    """`dad3d_one_euro_rows` in numpy float32, rule for rule: `x [N,D]` -> the output `[N,D]`; `state_x`, `state_dx` (float32 `[N,D]`)
    and `age` (int32 `[N]`) are updated in place. `scalars` from `one_euro_scalars`; `min_cutoff`, `beta` float32 `[D]`."""
    x = np.asarray(x, dtype=np.float32)
    n, d = x.shape
    rate, two_pi_dt, alpha_d = (np.float32(s) for s in scalars)
    mc, be = np.asarray(min_cutoff, np.float32).reshape(d), np.asarray(beta, np.float32).reshape(d)
    assert state_x.shape == (n, d) and state_dx.shape == (n, d) and age.shape == (n,)
    assert state_x.dtype == np.float32 and state_dx.dtype == np.float32 and age.dtype == np.int32
    out = x.copy()
    one = np.float32(1.0)
    for i in range(n):
        if (flags is not None and flags[i] != 0) or not np.all(np.isfinite(x[i])):  # rules 1 and 2
            age[i] = 0
            continue
        restart = age[i] <= 0  # rule 3
        if not restart:
            with np.errstate(all="ignore"):
                xp, dxp = state_x[i], state_dx[i]
                dx = (x[i] - xp) * rate
                dxh = dxp + alpha_d * (dx - dxp)
                fc = mc + be * np.abs(dxh)
                r = two_pi_dt * fc
                a = r / (r + one)
                o = xp + a * (x[i] - xp)
            restart = not (np.all(np.isfinite(o)) and np.all(np.isfinite(dxh)))  # rule 5
        if restart:
            state_x[i], state_dx[i], age[i] = x[i], 0.0, 1
        else:
            out[i], state_x[i], state_dx[i], age[i] = o, o, dxh, min(int(age[i]) + 1, AGE_MAX)
    return out


class OneEuroFilter:
    """The device form, for any float32 rows: the state `[n,d]` and the ages `[n]` live on `device`, a step is one launch and
    nothing waits. `min_cutoff` (> 0) and `beta` (>= 0): one value, or `d` of them."""

    def __init__(self, n: int, d: int, min_cutoff: Any, beta: Any, d_cutoff: float = 1.0, device: Any = "cuda"):
        if int(n) < 0 or int(d) < 1:
            raise ValueError(f"n {n} must be >= 0 and d {d} >= 1")
        self.n, self.d = int(n), int(d)
        one_euro_scalars(1.0, d_cutoff)  # ValueError for a bad d_cutoff
        self.d_cutoff = float(d_cutoff)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"OneEuroFilter runs on a GPU, got {self.device} (steady.one_euro_rows is the host statement)")
        if self.device.index is None:  # "cuda" is the current device; tensors name theirs by index, and so does the launch
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.min_cutoff = torch.from_numpy(_constants(min_cutoff, self.d, "min_cutoff", True)).to(self.device)
        self.beta = torch.from_numpy(_constants(beta, self.d, "beta", False)).to(self.device)
        self.state_x = torch.zeros((self.n, self.d), dtype=torch.float32, device=self.device)
        self.state_dx = torch.zeros((self.n, self.d), dtype=torch.float32, device=self.device)
        self.age = torch.zeros((self.n,), dtype=torch.int32, device=self.device)
        self._lib = _lib.load()

    def step(self, x: torch.Tensor, flags: Optional[torch.Tensor] = None, dt: float = 1.0 / 30.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One sample for every row: `x` float32 `[n,d]` on the device with a unit column stride (any row stride >= d), `flags`
        int32 `[n]` or None, `dt` the seconds since the last sample. `out`: where to write (`x` itself for in place), or None for a
        new tensor. -> `out`."""
        if not torch.is_tensor(x) or x.dtype != torch.float32 or x.device != self.device or tuple(x.shape) != (self.n, self.d):
            raise ValueError(f"x: expected float32 [{self.n},{self.d}] on {self.device}")
        if out is None:
            out = torch.empty((self.n, self.d), dtype=torch.float32, device=self.device)
        elif not torch.is_tensor(out) or out.dtype != torch.float32 or out.device != self.device or tuple(out.shape) != (self.n, self.d):
            raise ValueError(f"out: expected float32 [{self.n},{self.d}] on {self.device}")
        for name, t in (("x", x), ("out", out)):
            if self.n and (t.stride(1) != 1 or (self.n > 1 and t.stride(0) < self.d)):
                raise ValueError(f"{name}: expected a unit column stride and a row stride >= {self.d}, got {t.stride()}")
        if flags is not None and (not torch.is_tensor(flags) or flags.dtype != torch.int32 or flags.device != self.device
                                  or tuple(flags.shape) != (self.n,) or not flags.is_contiguous()):
            raise ValueError(f"flags: expected contiguous int32 [{self.n}] on {self.device}")
        rate, two_pi_dt, alpha_d = one_euro_scalars(dt, self.d_cutoff)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._lib.dad3d_one_euro_rows(x.data_ptr(), max(x.stride(0), self.d), out.data_ptr(), max(out.stride(0), self.d), self.n, self.d,
                                                 None if flags is None else flags.data_ptr(), self.min_cutoff.data_ptr(), self.beta.data_ptr(),
                                                 float(rate), float(two_pi_dt), float(alpha_d), self.state_x.data_ptr(),
                                                 self.state_dx.data_ptr(), self.age.data_ptr(), self.device.index, stream))
        return out

    def reset(self, rows: Any = None, mask: Optional[torch.Tensor] = None) -> None:
        """The tracks of `rows` (device or host indices; None: all) restart at their next sample. Device rows are never read on the
        host: one outside 0 .. n - 1 moves nothing. `mask` instead of `rows`: a tensor `[n]` on the device, the rows where it is
        not 0 (the `spawned` of `dad3d_track_assign_detections`): one masked fill, no index list. Nothing waits."""
        if mask is not None:
            if rows is not None:
                raise ValueError("reset: rows or mask, not both")
            if not torch.is_tensor(mask) or mask.device != self.device or tuple(mask.shape) != (self.n,) or mask.is_floating_point():
                raise ValueError(f"mask: expected an integer or bool tensor [{self.n}] on {self.device}")
            self.age.masked_fill_(mask != 0, 0)
            return
        if rows is None:
            self.age.zero_()
            return
        ids = rows if torch.is_tensor(rows) else torch.from_numpy(np.asarray(rows).reshape(-1).astype(np.int64))
        ids = ids.to(self.device, torch.int64).reshape(-1)
        if ids.numel() == 0:
            return
        spare = torch.where((ids >= 0) & (ids < self.n), ids, torch.full_like(ids, self.n))
        self.age.copy_(torch.cat([self.age, self.age.new_zeros(1)]).index_fill_(0, spare, 0)[: self.n])


class SteadyConfig:
    """What `HeadTracker(steady=...)` filters a 3DMM row with: `rate` (frames a second; a step's default `dt` is `1/rate`),
    `d_cutoff` (Hz, the derivative's cutoff) and `groups`, `{group name: (min_cutoff, beta)}` over the groups of `FLAME_CONSTS`;
    a group that is not named keeps its default (`DEFAULT_GROUPS`, `DEFAULT_OTHER` -- untuned design choices)."""

    def __init__(self, rate: float = 30.0, d_cutoff: float = 1.0, groups: Optional[Dict[str, Tuple[float, float]]] = None):
        self.rate, self.d_cutoff = float(rate), float(d_cutoff)
        if not (self.rate > 0.0 and math.isfinite(self.rate)):
            raise ValueError(f"rate {rate} must be finite and positive")
        one_euro_scalars(1.0 / self.rate, self.d_cutoff)
        self.groups = dict(DEFAULT_GROUPS)
        for name, pair in (groups or {}).items():
            if name not in FLAME_CONSTS:
                raise ValueError(f"groups: {name!r} is no group of a 3DMM row ({', '.join(_SLICE_ORDER)})")
            mc, be = (float(v) for v in pair)
            if not (mc > 0.0 and math.isfinite(mc) and be >= 0.0 and math.isfinite(be)):
                raise ValueError(f"groups[{name!r}]: min_cutoff {mc} must be > 0 and beta {be} >= 0, both finite")
            self.groups[name] = (mc, be)

    @property
    def dt(self) -> float:
        return 1.0 / self.rate

    def expand(self, consts: Optional[Dict[str, int]] = None) -> Tuple[np.ndarray, np.ndarray]:
        """(min_cutoff, beta) as float32 `[413]`: every group's pair over its entries, in the order of a 3DMM row."""
        consts = FLAME_CONSTS if consts is None else consts
        pairs = [self.groups.get(key, DEFAULT_OTHER) for key in _SLICE_ORDER for _ in range(int(consts[key]))]
        both = np.asarray(pairs, dtype=np.float32).reshape(-1, 2)
        return np.ascontiguousarray(both[:, 0]), np.ascontiguousarray(both[:, 1])
