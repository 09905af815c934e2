"""ctypes front of csrc/cnn_glue.hip and csrc/net_tail.hip: the fused streaming kernels InferenceNet puts between the framework's
convolutions, and the forward's tail (the fusion layer's input and output, the regression heads).
Device tensors only (there is no CPU fallback in this package: callers keep the framework's own ops for CPU tensors and for
shapes the kernels do not take -- `supported()` says which)."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch
from torch import Tensor

from . import _lib

_DTYPE = {torch.float32: (0, 4), torch.float16: (1, 8), torch.bfloat16: (2, 8)}


def _nhwc(t: Tensor) -> bool:
    return t.ndim == 4 and t.is_contiguous(memory_format=torch.channels_last)


def supported(y: Tensor, *others: Optional[Tensor]) -> bool:
    """A channels-last CUDA tensor of a dtype the kernels take, channel count a multiple of 16 bytes' worth; `others` (the
    residual, further inputs) the same dtype, device and layout."""
    if not (y.is_cuda and y.dtype in _DTYPE and _nhwc(y) and y.shape[1] % _DTYPE[y.dtype][1] == 0 and y.data_ptr() % 16 == 0):
        return False
    for o in others:
        if o is not None and not (o.is_cuda and o.dtype == y.dtype and o.device == y.device and _nhwc(o) and o.shape[1] == y.shape[1]
                                  and o.data_ptr() % 16 == 0):
            return False
    return True


def bias_act_(y: Tensor, bias: Tensor, z: Optional[Tensor] = None, relu: bool = True) -> Tensor:
    """In place: y = act(y + bias[c] (+ z)). `supported(y, z)` must hold, bias is [C] of y's dtype, z has y's shape."""
    if z is not None and z.shape != y.shape:
        raise ValueError("bias_act_: the residual must have the output's shape")
    if bias.dtype != y.dtype or bias.numel() != y.shape[1] or not bias.is_contiguous():
        raise ValueError("bias_act_: bias must be a contiguous [C] tensor of the output's dtype")
    n, c, h, w = y.shape
    _lib.check(_lib.load().dad3d_nhwc_bias_act(y.data_ptr(), bias.data_ptr(), z.data_ptr() if z is not None else None, n * h * w, c,
                                               _DTYPE[y.dtype][0], int(relu), y.device.index or 0,
                                               torch.cuda.current_stream(y.device).cuda_stream))
    return y


def resize_sum(weights: Sequence[float], xs: Sequence[Tensor], size) -> Tensor:
    """sum_k weights[k] * F.interpolate(xs[k], size=size) (nearest) in one pass; up to three inputs, `supported(x)` for each."""
    k = len(xs)
    if not (1 <= k <= 3 and len(weights) == k):
        raise ValueError("resize_sum: one to three weighted inputs")
    x0 = xs[0]
    if not supported(x0, *xs[1:]) or any(x.dim() != 4 or x.shape[0] != x0.shape[0] for x in xs):
        raise ValueError("resize_sum: every input must be a channels-last CUDA tensor of one dtype, device, batch and channel count, "
                         "16-byte aligned (the kernel reads raw NHWC rows)")
    n, c = x0.shape[0], x0.shape[1]
    oh, ow = int(size[0]), int(size[1])
    out = torch.empty((n, c, oh, ow), dtype=x0.dtype, device=x0.device, memory_format=torch.channels_last)
    ptrs = (C.c_void_p * k)(*[x.data_ptr() for x in xs])
    hs, ws = (C.c_int * k)(*[x.shape[2] for x in xs]), (C.c_int * k)(*[x.shape[3] for x in xs])
    wt = (C.c_float * k)(*[float(v) for v in weights])
    _lib.check(_lib.load().dad3d_nhwc_resize_sum(out.data_ptr(), n, oh, ow, c, _DTYPE[x0.dtype][0], k, ptrs, hs, ws, wt,
                                                 x0.device.index or 0, torch.cuda.current_stream(x0.device).cuda_stream))
    return out


# ---- the forward's tail (csrc/net_tail.hip) ---------------------------------------------------------------------------------------

def _nhwc_cuda(t: Tensor, dtype, device) -> bool:
    return t.is_cuda and t.dtype == dtype and t.device == device and _nhwc(t) and t.data_ptr() % 16 == 0


def supported_fusion(x: Tensor, heatmap: Tensor, level: Tensor) -> bool:
    """Channels-last CUDA tensors of one dtype the kernels take, one device and one batch, 16-byte aligned; `x` and `level` of one
    extent; every segment's byte width a multiple of 8."""
    if not (x.dtype in _DTYPE and all(_nhwc_cuda(t, x.dtype, x.device) for t in (x, heatmap, level))):
        return False
    per_piece = _DTYPE[x.dtype][1] // 2
    return (x.shape[0] == heatmap.shape[0] == level.shape[0] and x.shape[2:] == level.shape[2:] and x.numel() > 0 and heatmap.numel() > 0
            and level.numel() > 0 and all(t.shape[1] % per_piece == 0 for t in (x, heatmap, level)))


def fusion_concat(x: Tensor, heatmap: Tensor, level: Tensor) -> Tensor:
    """cat([x, sigmoid(F.interpolate(heatmap, x's extent, bilinear, align_corners=True)), level], dim=1) in one pass: fp32, every
    operation rounded on its own, one rounding at the store. `supported_fusion(x, heatmap, level)` must hold."""
    if not supported_fusion(x, heatmap, level):
        raise ValueError("fusion_concat: channels-last CUDA tensors of one dtype, device and batch, 16-byte aligned, x and level of one "
                         "extent, every channel count a multiple of 8 bytes' worth")
    n, cx, oh, ow = x.shape
    ch, hh, hw = heatmap.shape[1:]
    cl = level.shape[1]
    out = torch.empty((n, cx + ch + cl, oh, ow), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    _lib.check(_lib.load().dad3d_nhwc_fusion_concat(out.data_ptr(), x.data_ptr(), heatmap.data_ptr(), level.data_ptr(), n, oh, ow, hh, hw,
                                                    cx, ch, cl, _DTYPE[x.dtype][0], x.device.index or 0,
                                                    torch.cuda.current_stream(x.device).cuda_stream))
    return out


def bias_mul_(y: Tensor, bias: Tensor, x: Tensor) -> Tensor:
    """In place: y = (y + bias[c]) * x. `supported(y, x)` must hold, bias is [C] of y's dtype, x has y's shape."""
    if x.shape != y.shape:
        raise ValueError("bias_mul_: the multiplier must have the output's shape")
    if bias.dtype != y.dtype or bias.numel() != y.shape[1] or not bias.is_contiguous():
        raise ValueError("bias_mul_: bias must be a contiguous [C] tensor of the output's dtype")
    n, c, h, w = y.shape
    _lib.check(_lib.load().dad3d_nhwc_bias_mul(y.data_ptr(), bias.data_ptr(), x.data_ptr(), n * h * w, c, _DTYPE[y.dtype][0],
                                               y.device.index or 0, torch.cuda.current_stream(y.device).cuda_stream))
    return y


def regression_heads(top: Tensor, heads, stages: bool = False):
    """The raw entry. `heads`: a sequence of (w1, b1, w2, b2, act, limit, dst, col_offset) with dst a float32 [B, ...] tensor whose
    dim-0 stride is the row stride. Allocates the workspace with torch.empty (a graph capture works). With `stages`, returns
    (pooled [B,C], hidden [B,sum hidden]) float32 as the launches wrote them."""
    b, c, h, w = top.shape
    hidden_total = sum(int(hd[0].shape[0]) for hd in heads)
    descs = (_lib.HeadDescC * len(heads))()
    for d, (w1, b1, w2, b2, act, limit, dst, col) in zip(descs, heads):
        d.w1, d.b1, d.w2, d.b2, d.dst = w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), dst.data_ptr()
        d.dst_row_stride, d.dst_col_offset = dst.stride(0), col
        d.hidden, d.out_dim, d.act, d.limit = w1.shape[0], w2.shape[0], act, limit
    work = torch.empty(b * (c + hidden_total), dtype=torch.float32, device=top.device)
    pooled = hidden = None
    if stages:
        pooled, hidden = work[:b * c].view(b, c), work[b * c:].view(b, hidden_total)
    _lib.check(_lib.load().dad3d_regression_heads(top.data_ptr(), b, c, h * w, _DTYPE[top.dtype][0], descs, len(heads), work.data_ptr(),
                                                  pooled.data_ptr() if stages else None, hidden.data_ptr() if stages else None,
                                                  top.device.index or 0, torch.cuda.current_stream(top.device).cuda_stream))
    return (pooled, hidden) if stages else None


class RegressionHeads:
    """The three `RegressionHead` modules (shape, pose, landmarks) of DAD3DNet behind one call: pooled once, three launches, float32
    out with nothing rounded to the serving dtype on the way. The weights' addresses are packed once per (device, dtype)."""

    def __init__(self, heads, limit_value: float):
        self.shape, self.pose, self.landmarks = heads
        self.limit_value = float(limit_value)
        self._packed = None

    def _weights(self, head):
        return head.mlp[0].weight, head.mlp[0].bias, head.mlp[3].weight, head.mlp[3].bias

    def supported(self, top: Tensor) -> bool:
        if not (top.is_cuda and top.dtype in _DTYPE and _nhwc(top) and top.data_ptr() % 16 == 0 and 0 < top.shape[0] <= 65535
                and top.shape[2] * top.shape[3] > 0):
            return False
        vec = _DTYPE[top.dtype][1]
        for head in (self.shape, self.pose, self.landmarks):
            w1, b1, w2, b2 = self._weights(head)
            if not (all(t.dtype == top.dtype and t.device == top.device and t.is_contiguous() for t in (w1, b1, w2, b2))
                    and w1.shape[1] == top.shape[1] and w1.shape[1] % vec == 0 and w1.shape[0] % vec == 0
                    and w1.data_ptr() % 16 == 0 and w2.data_ptr() % 16 == 0):
                return False
        return True

    def __call__(self, top: Tensor):
        """top [B,C,h,w] channels-last -> (params [B, shape + pose] float32, landmarks [B, n, 2] float32)."""
        if not self.supported(top):
            raise ValueError("RegressionHeads: a channels-last CUDA tensor of the weights' dtype and device, 16-byte aligned, channel and "
                             "hidden counts multiples of 16 bytes' worth")
        key = (top.device, top.dtype) + tuple(t.data_ptr() for head in (self.shape, self.pose, self.landmarks) for t in self._weights(head))
        if self._packed is None or self._packed[0] != key:
            s, p, l = (self._weights(head) for head in (self.shape, self.pose, self.landmarks))
            self._packed = (key, s, p, l, s[2].shape[0], p[2].shape[0], l[2].shape[0])
        _, s, p, l, n_shape, n_pose, n_lmk = self._packed
        b = top.shape[0]
        params = torch.empty((b, n_shape + n_pose), dtype=torch.float32, device=top.device)
        lmk = torch.empty((b, n_lmk // 2, 2), dtype=torch.float32, device=top.device)
        regression_heads(top, ((*s, _lib.HEAD_ACT_TANH, self.limit_value, params, 0), (*p, _lib.HEAD_ACT_NONE, 0.0, params, n_shape),
                               (*l, _lib.HEAD_ACT_RELU, 0.0, lmk, 0)))
        return params, lmk
