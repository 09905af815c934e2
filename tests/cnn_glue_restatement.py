"""What the CNN-glue tests share: a plain torch / NumPy statement, on the CPU, of the two streaming kernels of
csrc/cnn_glue.hip, written from what they replace (model_training/model/layers.py, bifpn.py:98-125) and not from the kernel source.

  * `bias_act_ref`    act((y + bias[c]) + z) in fp32, in that order, ONE rounding (to nearest even: the CPU cast) at the end;
  * `nearest_index`   the source index of F.interpolate(mode="nearest") as PyTorch evaluates it, in float32;
  * `resize_sum_ref`  sum_k w_k * nearest(x_k) in float64 from float32-rounded weights (the C ABI takes `float`): the exact sum E and
                      the magnitude M = sum_k |w_k * x_k| that the accumulation bound `resize_sum_bound` is stated in;
  * the comparison (`bit_mismatches`: bit equality, +-0 equal, NaN by NaN-ness) and the inputs of the exhaustive tests
    (`every_pattern`: each 2-byte pattern through each lane of a 16-byte vector).

tests/test_cnn_glue_host.py pins all of it to the framework's own CPU ops, so the GPU tests cannot be wrong about their reference.
"""
import numpy as np
import torch
import torch.nn.functional as F

VEC = {torch.float32: 4, torch.float16: 8, torch.bfloat16: 8}  # elements of a 16-byte vector
UNIT_ROUNDOFF = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
TINY = {torch.float32: 2.0 ** -149, torch.float16: 2.0 ** -24, torch.bfloat16: 2.0 ** -133}  # smallest subnormal
_BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}

# (in, out, dst) in 1..40 where float32 floor(dst * (in / out)) is NOT the exact dst * in // out
FLOAT_INDEX_EXCEPTIONS = {(26, 22, 11), (39, 33, 11), (39, 33, 22)}


def nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def bias_act_ref(y, bias, z=None, relu=True):
    """[N,C,H,W] of any layout -> the same shape and dtype, channels-last."""
    v = y.float() + bias.float().view(1, -1, 1, 1)
    if z is not None:
        v = v + z.float()
    if relu:
        v = F.relu(v)  # NaN stays NaN
    return nhwc(v.to(y.dtype))


def nearest_index(n_in, n_out):
    """int64 [n_out]: min(floor(float32(d) * (float32(in) / float32(out))), in - 1), every step in float32."""
    scale = np.float32(n_in) / np.float32(n_out)
    src = np.floor(np.arange(n_out, dtype=np.float32) * scale)
    assert src.dtype == np.float32 and scale.dtype == np.float32
    return np.minimum(src.astype(np.int64), n_in - 1)


def gather_nearest(x, size):
    iy = torch.from_numpy(nearest_index(x.shape[2], int(size[0])))
    ix = torch.from_numpy(nearest_index(x.shape[3], int(size[1])))
    return x[:, :, iy[:, None], ix[None, :]]


def resize_sum_ref(weights, xs, size):
    """(E, M) float64 [N,C,oh,ow]: E = sum_k w_k * x_k[nearest], M = sum_k |w_k * x_k[nearest]|, w_k rounded to float32 first.
    A float32 weight times a <= 24-bit value is exact in float64; the (at most two) float64 additions err by 2^-53 relative,
    2^29 times below the smallest term of the bound."""
    E = M = None
    for w, x in zip(weights, xs):
        t = gather_nearest(x, size).double() * float(np.float32(w))
        E = t if E is None else E + t
        M = t.abs() if M is None else M + t.abs()
    return E, M


def resize_sum_bound(dtype, E, M):
    """|got - E| <= u |E| + 4 * 2^-24 * M + tiny. The kernel accumulates in fp32 from zero: at most three multiply-adds, each either
    fused (one rounding of 2^-24 relative to a partial sum <= M (1 + 2^-22)) or a product and a sum rounded apiece (the products err
    by 2^-24 of their own term, together 2^-24 M; the first sum, onto zero, is exact) -- 3 * 2^-24 * M to first order either way,
    the fourth unit covers the second-order terms and u times that error in the last step. Then ONE rounding to the output type:
    u |acc| for a normal result, half a subnormal step (< tiny) below that."""
    return UNIT_ROUNDOFF[dtype] * E.abs() + 4.0 * 2.0 ** -24 * M + TINY[dtype]


def bit_mismatches(got, want):
    """Boolean tensor, true where `got` is NOT `want` to the bit; +0 and -0 are one value and every NaN is one value (the payload
    and sign of a produced NaN are not specified)."""
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    g, w = got.cpu().contiguous(), want.cpu().contiguous()
    same = (g.view(_BITS[g.dtype]) == w.view(_BITS[w.dtype])) | (g.isnan() & w.isnan()) | ((g == 0) & (w == 0))
    return ~same


def describe_mismatches(got, want, inputs=(), limit=4):
    """'' when bit-equal, else the count and the first few (index, got, want, inputs...) with their bit patterns."""
    bad = bit_mismatches(got, want)
    n = int(bad.sum())
    if n == 0:
        return ""
    lines = [f"{n} of {bad.numel()} elements differ"]
    for idx in bad.nonzero()[:limit].tolist():
        i = tuple(idx)
        bits = lambda t: int(t.cpu()[i].view(_BITS[t.dtype])) & (0xFFFFFFFF if t.dtype == torch.float32 else 0xFFFF)
        lines.append(f"  at {i}: got {float(got.cpu()[i])!r} (0x{bits(got):x}) want {float(want.cpu()[i])!r} (0x{bits(want):x})"
                     + "".join(f" in{k} {float(t.cpu()[i])!r}" for k, t in enumerate(inputs) if t is not None and t.shape == got.shape))
    return "\n".join(lines)


# ---- inputs of the exhaustive store / load tests -------------------------------------------------------------------------------

def every_pattern(dtype, seed=0):
    """(y, z) channels-last [1, 8, 256, 256]: y[pixel p][channel c] is value number (p + c) mod 2^16 of a list of 2^16 values, so
    every value passes through every lane of the 16-byte vector (both of its vectors for fp32). For the 2-byte types the list is
    ALL bit patterns; for fp32 it is the special values followed by uniformly drawn bit patterns (every exponent equally likely).
    z pairs each y with another list entry: a fixed odd multiplier permutes the 2-byte patterns; for fp32 half the partners are
    drawn within two binades of y (sums that cancel and round), half anywhere."""
    rng = np.random.default_rng(seed)
    p = np.arange(65536, dtype=np.int64)[:, None]
    c = np.arange(8, dtype=np.int64)[None, :]
    if dtype == torch.float32:
        specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 2.0 ** -149, -2.0 ** -149, 2.0 ** -126, -2.0 ** -126,
                             np.finfo(np.float32).max, -np.finfo(np.float32).max, 1.0, -1.0, 1.0 + 2.0 ** -23, 2.0 ** -24, 0.5],
                            dtype=np.float32).view(np.uint32)
        values = rng.integers(0, 2 ** 32, 65536, dtype=np.uint64).astype(np.uint32)
        values[:specials.size] = specials
        yb = values[(p + c) % 65536]
        zb = rng.integers(0, 2 ** 32, yb.shape, dtype=np.uint64).astype(np.uint32)
        near = rng.random(yb.shape) < 0.5
        exp = np.clip(((yb >> 23) & 0xFF).astype(np.int64) + rng.integers(-2, 3, yb.shape), 0, 255).astype(np.uint32)
        zb = np.where(near, (zb & np.uint32(0x807FFFFF)) | (exp << 23), zb)
        as_t = lambda b: torch.from_numpy(b.view(np.int32).copy()).view(torch.float32)
    else:
        yb = ((p + c) % 65536).astype(np.uint16)
        zb = (((p + c) * 40503 + 7919 * c + 12345) % 65536).astype(np.uint16)
        as_t = lambda b: torch.from_numpy(b.view(np.int16).copy()).view(dtype)
    shape = lambda t: nhwc(t.view(1, 256, 256, 8).permute(0, 3, 1, 2))
    return shape(as_t(yb)), shape(as_t(zb))


def edge_bias(dtype):
    """Eight distinct biases: -0, the smallest subnormal, the largest finite value, then what makes the store's rounding visible:
    +-u (half a unit in the last place of [1, 2): y + bias is an exact TIE for every y there, with even and odd neighbours),
    1.5 u (past the tie), 1 and -0.75."""
    u = UNIT_ROUNDOFF[dtype]
    b = torch.tensor([-0.0, TINY[dtype], torch.finfo(dtype).max, u, -u, 1.5 * u, 1.0, -0.75], dtype=torch.float64).to(dtype)
    assert len(set(b.view(_BITS[dtype]).tolist())) == 8
    return b


NONFINITE_VALUES = (float("nan"), float("inf"), float("-inf"), -2.0, -1.0, -0.0, 0.0, 0.5, 1.0, 3.0)


def nonfinite_case(dtype):
    """(y, z, bias): every ordered pair of NONFINITE_VALUES as (y, z), in every lane; the finite values and the biases are small
    dyadic numbers, so each finite sum is exact in all three types and in any order of evaluation."""
    c, k = VEC[dtype], len(NONFINITE_VALUES)
    v = torch.tensor(NONFINITE_VALUES, dtype=torch.float32)
    y = nhwc(v.view(1, 1, k, 1).expand(1, c, k, k).to(dtype))
    z = nhwc(v.view(1, 1, 1, k).expand(1, c, k, k).to(dtype))
    bias = torch.tensor([0.0, 1.0, -1.0, 2.0, -0.5, 0.25, -3.0, 4.0][:c], dtype=torch.float32).to(dtype)
    return y, z, bias


def plain_conv_bias_act(bias, relu):
    """A ConvBiasAct whose convolution is the identity: its forward is the bias / residual / ReLU step alone."""
    from dad_3dheads_amd.network import ConvBiasAct

    m = ConvBiasAct(torch.nn.Conv2d(bias.numel(), bias.numel(), 1, bias=True), relu)
    m.conv = torch.nn.Identity()
    m.bias = torch.nn.Parameter(bias.clone(), requires_grad=False)
    return m


def indexed_input(n, c, h, w, dtype, seed):
    """[n,c,h,w] channels-last whose channel vector names its source pixel: channel 0 = row, 1 = column, 2 = image (small integers,
    exact in every type), the rest seeded noise -- a wrong source index cannot produce the right vector."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, h, w, generator=g) * 4.0
    x[:, 0] = torch.arange(h, dtype=torch.float32).view(1, h, 1)
    x[:, 1] = torch.arange(w, dtype=torch.float32).view(1, 1, w)
    x[:, 2] = torch.arange(n, dtype=torch.float32).view(n, 1, 1) + 1.0
    return nhwc(x.to(dtype))
