"""What the tests of csrc/net_tail.hip share: plain NumPy / torch statements, on the CPU, of the three entries, written from what they
replace (model_training/model/flame_regression.py:28-43, 45-59, 96-100) and from include/dad3d.h, not from the kernel source.

  * `bilinear_taps`, `interp_f32`, `fusion_concat_ref`   the fusion layer's input in NumPy float32, operation by operation (an array
                        operation of NumPy rounds once per element and fuses nothing), one rounding to the dtype at the end;
  * `bias_mul_ref`      (y + bias[c]) * x in fp32, two rounded operations, one rounding at the end;
  * `pool_ref`, `layer_ref`, `heads_ref`   float64 statements of the heads: per stage the exact value E and the magnitude sum M
                        that the accumulation bounds `pool_bound`, `layer_bound` are stated in;
  * `tanh_sweep_inputs`, `ulp_error`       the float32 sweep that measures the device library's tanhf.

tests/test_net_tail_host.py pins all of it to the framework's own CPU ops.
"""
import json
import os

import numpy as np
import torch

from cnn_glue_restatement import nhwc

U = 2.0 ** -23  # unit roundoff of CHOPPED fp32: covers a matrix unit's internal adds whatever their rounding mode
ACT_NONE, ACT_RELU, ACT_TANH = 0, 1, 2
BENCH_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "net_tail_bench.json")


# ---- 1. the fusion layer's input ------------------------------------------------------------------------------------------------------

def bilinear_taps(n_in, n_out):
    """(i0, i1 int32 [n_out], l0, l1 float32 [n_out]) of F.interpolate(mode="bilinear", align_corners=True), every step in float32."""
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0.0)
    src = scale * np.arange(n_out, dtype=np.float32)
    i0 = src.astype(np.int32)  # truncation
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(np.float32)
    l0 = np.float32(1.0) - l1
    assert src.dtype == l0.dtype == l1.dtype == np.float32
    return i0, i1.astype(np.int32), l0, l1


def interp_f32(heat, size):
    """heat float32 ndarray [N,C,H,W] -> v float32 [N,C,oh,ow] = lh0 * (lw0 * a + lw1 * b) + lh1 * (lw0 * c + lw1 * d)."""
    assert heat.dtype == np.float32
    y0, y1, lh0, lh1 = bilinear_taps(heat.shape[2], int(size[0]))
    x0, x1, lw0, lw1 = bilinear_taps(heat.shape[3], int(size[1]))
    lh0, lh1 = lh0[:, None], lh1[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        a, b = heat[:, :, y0][:, :, :, x0], heat[:, :, y0][:, :, :, x1]
        c, d = heat[:, :, y1][:, :, :, x0], heat[:, :, y1][:, :, :, x1]
        v = lh0 * (lw0 * a + lw1 * b) + lh1 * (lw0 * c + lw1 * d)
    assert v.dtype == np.float32
    return v


def sigmoid_f32(v, exp=np.exp):
    """1.0f / (1.0f + expf(-v)) in float32. `exp`: a float32 -> float32 exponential; NumPy's by default, and the GPU tests pass the
    device's own (through the framework's float32 sigmoid kernel, whose bits tests/test_gpu_heatmap_points.py sweeps against this
    library's `sigmoid_f32`), because two correctly working expf differ in the last bit of some arguments."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        e = exp(-v)
        assert e.dtype == np.float32
        return np.float32(1.0) / (np.float32(1.0) + e)


def fusion_concat_ref(x, heat, level, sigmoid=sigmoid_f32):
    """[N,cx+ch+cl,oh,ow] channels-last of x's dtype: [ x | round(sigmoid(interp(heat))) | level ]. `sigmoid`: float32 ndarray -> float32 ndarray."""
    v = interp_f32(heat.float().numpy(), x.shape[2:])
    s = torch.from_numpy(np.ascontiguousarray(sigmoid(v))).to(x.dtype)  # the CPU cast rounds to nearest even
    return nhwc(torch.cat([x, s, level], dim=1))


# ---- 2. the fusion layer's output -----------------------------------------------------------------------------------------------------

def bias_mul_ref(y, bias, x):
    return nhwc(((y.float() + bias.float().view(1, -1, 1, 1)) * x.float()).to(y.dtype))


# ---- 3. the regression heads ----------------------------------------------------------------------------------------------------------

def pool_ref(top):
    """top [B,C,h,w] -> (E, M) float64 [B,C]: the mean over the positions and the mean of the magnitudes. (The magnitude sum of the
    issue, sum |x|, is the bound's unit for the SUM; the division by h*w scales the sum's error with it, so the bound on the pooled
    value is stated in sum |x| / (h*w) -- h*w times narrower than the unscaled one.)"""
    t = top.double().flatten(2)
    return t.mean(-1), t.abs().mean(-1)


def pool_bound(E, M, hw):
    """|got - E| <= (hw + 1) u M: hw - 1 additions and the division, each rounded, one spare unit for the second-order terms."""
    return (hw + 1) * U * M


def layer_ref(a, w, b):
    """a [B,K] (any float type, taken exactly), w [R,K], b [R] -> (E, M) float64 [B,R]: E = a . w^T + b, M = sum |a_i| |w_i| + |b|."""
    a, w, b = a.double(), w.double(), b.double()
    return a @ w.t() + b, a.abs() @ w.abs().t() + b.abs()


def layer_bound(M, k):
    """|got - E| <= (K + 2) u M in any order of accumulation: K multiply-adds (fused or not) and the bias. ReLU maps both sides
    through a contraction and is inside it."""
    return (k + 2) * U * M


def activation_ref(E, act, limit):
    if act == ACT_RELU:
        return torch.relu(E)  # NaN stays NaN
    if act == ACT_TANH:
        return float(np.float32(limit)) * torch.tanh(E)
    return E


def heads_ref(top, heads):
    """`heads`: (w1, b1, w2, b2, act, limit) per head, tensors of any float type. float64 throughout ->
    pooled [B,C], [hidden_k [B,H_k]], [out_k [B,O_k]]."""
    pooled, _ = pool_ref(top)
    hidden = [torch.relu(layer_ref(pooled, w1, b1)[0]) for w1, b1, *_ in heads]
    outs = [activation_ref(layer_ref(h, w2, b2)[0], act, limit) for h, (_, _, w2, b2, act, limit) in zip(hidden, heads)]
    return pooled, hidden, outs


def ulp32(x):
    """float64 tensor: the spacing of float32 at |x| (the smallest normal's spacing below it)."""
    return torch.from_numpy(np.spacing(np.maximum(np.abs(x.numpy()), 2.0 ** -126).astype(np.float32)).astype(np.float64))


def tanh_bound(E_pre, bound_pre, limit, tanh_ulps):
    """Tolerance of limit * tanhf(v) against limit * tanh(E_pre) when |v - E_pre| <= bound_pre: |tanh'| <= 1 carries the argument's
    error over, tanhf errs by `tanh_ulps` units in the last place of its result, the product by one more."""
    want = float(np.float32(limit)) * torch.tanh(E_pre)
    return abs(float(limit)) * bound_pre + (tanh_ulps + 1.0) * ulp32(want)


def recorded_tanh_ulps():
    """The largest ulp error of the device library's tanhf over the sweep below, as tests/perf/bench_net_tail.py measured and
    recorded it (the ROCm installation states no bound)."""
    with open(BENCH_JSON) as f:
        return float(json.load(f)["tanhf_sweep"]["max_ulp_error"])


def tanh_sweep_inputs():
    """Every float32 in [-9.1, 9.1] whose bit pattern is a multiple of 4099 steps from zero's, both signs: float32 ndarray."""
    top = int(np.float32(9.1).view(np.uint32))
    pos = np.arange(0, top + 1, 4099, dtype=np.uint32)
    return np.concatenate([pos, pos | np.uint32(0x80000000)]).view(np.float32)


def ulp_error(got, want64):
    """max |got - want| in units of float32's spacing at |want| (float64 reference)."""
    spacing = np.spacing(np.maximum(np.abs(want64), 2.0 ** -126).astype(np.float32)).astype(np.float64)
    return float(np.max(np.abs(got.astype(np.float64) - want64) / spacing))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------

def exact_heads_case(batch, c, hidden, out_dims, h, w, dtype, seed=0):
    """(top, heads) whose every partial sum is exact in fp32 in any order: top holds integers in [-8, 8] and h*w is a power of two;
    weights are in {0, +-0.5, +-1, +-2}; biases small integers. Head k's W2 row j carries (k, j) in two columns a head, row or
    column mix-up cannot cancel: column 0 holds +-(0.5, 1, 2)[k] and b2[j] = 16 (k + 1) + (j mod 13) (the hidden values are
    non-negative integers or halves, bounded by 8 C + 4, so the sums stay far below 2^24 halves)."""
    assert (h * w) & (h * w - 1) == 0
    g = torch.Generator().manual_seed(seed)
    values = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0])
    top = nhwc(torch.randint(-8, 9, (batch, c, h, w), generator=g).to(dtype))
    heads = []
    for k, (hid, out) in enumerate(zip(hidden, out_dims)):
        w1 = values[torch.randint(0, 7, (hid, c), generator=g)]
        w1 = w1 * (torch.rand(hid, c, generator=g) < min(1.0, 24.0 / c))  # sparse rows: the hidden values stay small
        b1 = torch.randint(-3, 4, (hid,), generator=g).float()
        w2 = values[torch.randint(0, 7, (out, hid), generator=g)] * (torch.rand(out, hid, generator=g) < min(1.0, 12.0 / hid))
        w2[:, 0] = (0.5, 1.0, 2.0, -1.0)[k] * (1 - 2 * (torch.arange(out) % 2))
        b2 = (16.0 * (k + 1) + (torch.arange(out) % 13)).float()
        heads.append([t.to(dtype) for t in (w1, b1, w2, b2)])
    return top, heads
