"""CPU: the statements of tests/net_tail_restatement.py against the framework's own CPU ops, the derived accumulation bounds against
emulated fp32 sums, and InferenceNet's `tail` keyword where no kernel can run."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import net_tail_restatement as T
from dad_3dheads_amd import _lib
from dad_3dheads_amd.network import DAD3DNet, InferenceNet, RegressionHead


def test_head_statement_is_three_regression_head_modules_in_double():
    """tanh * limit, ReLU, and the [shape | pose] column order of DAD3DNet.forward."""
    torch.manual_seed(3)
    c, limit = 40, 3.0
    mods = [RegressionHead(c, 11, hidden=24).double().eval(), RegressionHead(c, 5, hidden=8).double().eval(),
            RegressionHead(c, 6, hidden=16).double().eval()]
    top = torch.randn(3, c, 7, 5, dtype=torch.float64)
    acts = ((T.ACT_TANH, limit), (T.ACT_NONE, 0.0), (T.ACT_RELU, 0.0))
    heads = [(m.mlp[0].weight, m.mlp[0].bias, m.mlp[3].weight, m.mlp[3].bias, act, lim) for m, (act, lim) in zip(mods, acts)]
    with torch.no_grad():
        pooled, hidden, outs = T.heads_ref(top, heads)
        want_params = torch.cat([torch.tanh(mods[0](top)) * limit, mods[1](top)], dim=1)
        want_lmk = F.relu(mods[2](top)).reshape(3, -1, 2)
        want_hidden = [m.mlp[1](m.mlp[0](top.mean(dim=(2, 3)))) for m in mods]
    torch.testing.assert_close(pooled, top.mean(dim=(2, 3)), rtol=1e-12, atol=0)
    for got, want in zip(hidden, want_hidden):
        torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-15)
    torch.testing.assert_close(torch.cat(outs[:2], dim=1), want_params, rtol=1e-12, atol=1e-15)
    torch.testing.assert_close(outs[2].reshape(3, -1, 2), want_lmk, rtol=1e-12, atol=1e-15)


def test_fusion_statement_agrees_with_the_framework_before_the_final_rounding():
    """|heat| <= 1: the interpolation is four levels of rounded operations (product, inner sum, outer product, outer sum: six operations)
    on terms whose magnitudes sum to at most 1, so |dv| <= 4 * 2^-24 to first order; d ln(sigmoid) / dv = 1 - sigmoid <= 1 carries that
    over as a relative error, and expf (below one unit in the last place, 2 * 2^-24), the add and the division bring 4 * 2^-24 more:
    8 * 2^-24 relative. That holds where the float32 scale (n_in - 1) / (n_out - 1) is exact, as in the first five extents below.
    Where it is not (63 / 15, 4 / 3, 4 / 10: the last three, shapes of the GPU tests), the float64 framework works from another
    source coordinate: the statement's is off by up to 2^-23 of itself (the scale's rounding and the product's), which moves v by at
    most that times the difference of two neighbours (<= 2) on each axis: 4 * 2^-24 * ((hh - 1) + (hw - 1)) more. Measured on 64 -> 16:
    149 x 2^-24 of a bound of 512 x 2^-24."""
    g = torch.Generator().manual_seed(5)
    u = 2.0 ** -24
    exact = (((65, 65), (17, 17)), ((7, 5), (3, 3)), ((9, 17), (17, 5)), ((4, 4), (4, 4)), ((3, 3), (1, 1)))
    inexact = (((64, 64), (16, 16)), ((7, 5), (3, 4)), ((5, 9), (11, 2)))
    for cases, is_exact in ((exact, True), (inexact, False)):
        for (hh, hw), size in cases:
            for n_in, n_out in ((hh, size[0]), (hw, size[1])):
                scale = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
                assert (float(np.float32(scale)) == scale) or not is_exact
            heat = (torch.randn(2, 68, hh, hw, generator=g) * 0.5).clamp(-1.0, 1.0)
            got = T.sigmoid_f32(T.interp_f32(heat.numpy(), size)).astype(np.float64)
            want = F.interpolate(heat.double(), size=size, mode="bilinear", align_corners=True).sigmoid().numpy()
            assert got.shape == want.shape
            worst = float(np.max(np.abs(got - want) / want))
            bound = 8 * u + (0.0 if is_exact else 4 * u * ((hh - 1) + (hw - 1)))
            print(f"fusion statement vs float64 framework, {hh}x{hw} -> {size}: worst relative error {worst / u:.2f} x 2^-24, bound {bound / u:.0f}")
            assert worst <= bound, ((hh, hw), size)


def test_fusion_statement_concatenates_like_the_framework_chain():
    """Against interpolate -> sigmoid -> cat in the dtype: the copied segments are the inputs, and in the 2-byte types the middle segment is within
    one unit in the last place (the chain rounds twice, the statement once)."""
    g = torch.Generator().manual_seed(6)
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        x, heat, level = (torch.randn(2, c, h, w, generator=g).to(dtype) for c, h, w in ((16, 3, 4), (68, 7, 5), (8, 3, 4)))
        got = T.fusion_concat_ref(x, heat, level)
        assert got.shape == (2, 92, 3, 4) and got.dtype == dtype and got.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(got[:, :16], x) and torch.equal(got[:, 84:], level)
        chain = F.interpolate(heat.float(), size=(3, 4), mode="bilinear", align_corners=True).to(dtype).float().sigmoid().to(dtype)
        if dtype != torch.float32:  # float32 against the framework: the test above
            ulp = chain.double().abs() * 2 * {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}[dtype]  # >= one unit in the last place
            assert bool(((got[:, 16:84].double() - chain.double()).abs() <= ulp).all())


def test_bilinear_taps_are_the_frameworks_on_integer_ramps_for_every_extent_to_40():
    """F.interpolate of the ramp 0, 1, .., n_in - 1 (float64: the framework's CPU kernel computes its lambdas in the tensor's type, and
    i0 + l1 is the source coordinate): the statement's float32 i0 + l1 is that coordinate to float32's rounding, its i0 is the
    coordinate's integer part wherever the coordinate is not within rounding of an integer, and i1 is the next row unless i0 is the
    last. n_out = 1 and n_in = n_out included, on both axes."""
    for n_in in range(1, 41):
        ramp = torch.arange(n_in, dtype=torch.float64)
        for n_out in range(1, 41):
            i0, i1, l0, l1 = T.bilinear_taps(n_in, n_out)
            assert i0.min() >= 0 and i1.max() <= n_in - 1 and np.array_equal(i1, np.minimum(i0 + 1, n_in - 1)), (n_in, n_out)
            assert np.all(l1 >= 0) and np.all(l1 < 1) and np.array_equal(l0, np.float32(1) - l1)
            along_h = F.interpolate(ramp.view(1, 1, n_in, 1).expand(1, 1, n_in, 2), size=(n_out, 2), mode="bilinear", align_corners=True)[0, 0, :, 0]
            along_w = F.interpolate(ramp.view(1, 1, 1, n_in).expand(1, 1, 2, n_in), size=(2, n_out), mode="bilinear", align_corners=True)[0, 0, 0]
            assert torch.equal(along_h, along_w)
            src = along_h.numpy()
            got = i0.astype(np.float64) + l1.astype(np.float64)
            assert np.all(np.abs(got - src) <= 2.0 ** -23 * np.maximum(src, 1.0)), (n_in, n_out)
            inside = np.abs(src - np.rint(src)) > 2.0 ** -17
            assert np.array_equal(i0[inside], np.floor(src[inside]).astype(np.int32)), (n_in, n_out)
            if n_out == 1:
                assert i0.tolist() == [0] and l1.tolist() == [0.0]
            if n_in == n_out:
                assert np.array_equal(i0, np.arange(n_in)) and not l1.any()


def test_bias_mul_statement_is_the_frameworks_ops_in_float32():
    g = torch.Generator().manual_seed(8)
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        y, x = (torch.randn(2, 16, 3, 5, generator=g).to(dtype) for _ in range(2))
        bias = torch.randn(16, generator=g).to(dtype)
        want = ((y.float() + bias.float()[None, :, None, None]) * x.float()).to(dtype)
        assert torch.equal(T.bias_mul_ref(y, bias, x), want)
    nan = T.bias_mul_ref(torch.tensor([[[[float("inf")]]]]), torch.zeros(1), torch.zeros(1, 1, 1, 1))
    assert bool(nan.isnan().all())


def _sequential(terms):
    acc = np.float32(0.0)
    for t in terms:
        acc = np.float32(acc + t)
    return acc


def _pairwise(terms):
    terms = list(terms)
    while len(terms) > 1:
        terms = [np.float32(terms[i] + terms[i + 1]) if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
    return terms[0]


@pytest.mark.parametrize("scale", (1e-3, 1.0, 1e2))
def test_plain_fp32_accumulation_stays_inside_each_bound(scale):
    """Sequential and pairwise float32 sums of float32 products (the loosest of what a kernel may do: fusing rounds less)."""
    rng = np.random.default_rng(11)
    worst_pool = worst_layer = 0.0
    for hw in (1, 35, 64):
        x = (rng.standard_normal((4, hw)) * scale).astype(np.float32)
        E, M = T.pool_ref(torch.from_numpy(x).view(4, 1, hw, 1))
        for order in (_sequential, _pairwise):
            got = np.array([np.float32(order(row) / np.float32(hw)) for row in x], dtype=np.float64)
            worst_pool = max(worst_pool, float(((torch.from_numpy(got).view(4, 1) - E).abs() / T.pool_bound(E, M, hw)).max()))
    for k in (8, 40, 512):
        a = (rng.standard_normal((3, k)) * scale).astype(np.float32)
        w = rng.standard_normal((5, k)).astype(np.float32)
        b = rng.standard_normal(5).astype(np.float32)
        E, M = T.layer_ref(torch.from_numpy(a), torch.from_numpy(w), torch.from_numpy(b))
        for order in (_sequential, _pairwise):
            got = np.array([[np.float32(order(a[i] * w[j]) + b[j]) for j in range(5)] for i in range(3)], dtype=np.float64)
            worst_layer = max(worst_layer, float(((torch.from_numpy(got) - E).abs() / T.layer_bound(M, k)).max()))
    print(f"scale {scale}: worst error / bound: pool {worst_pool:.3f}, layer {worst_layer:.3f}")
    assert 0.0 < worst_pool <= 1.0 and 0.0 < worst_layer <= 1.0


def test_exact_case_is_exact_in_float32_in_two_orders():
    top, heads = T.exact_heads_case(3, 40, (24, 8, 8), (5, 1, 2), 2, 4, torch.bfloat16)
    pooled, hidden, _ = T.heads_ref(top, [(*h, T.ACT_NONE, 0.0) for h in heads])
    assert torch.equal(pooled.float().double(), pooled)
    for (w1, b1, *_), hid in zip(heads, hidden):
        p, w = pooled.float().numpy(), w1.float().numpy()
        for order in (_sequential, _pairwise):
            got = np.array([[max(np.float32(order(p[i] * w[j]) + np.float32(float(b1[j]))), 0) for j in range(w.shape[0])] for i in range(3)])
            assert np.array_equal(got.astype(np.float64), hid.numpy())


def test_tail_keyword_on_cpu_is_the_framework_path():
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(1))
    plain = InferenceNet(DAD3DNet(seed=0), dtype=torch.float32)(x)
    for tail in ("framework", "hip"):
        got = InferenceNet(DAD3DNet(seed=0), dtype=torch.float32, tail=tail)(x)
        assert got.keys() == plain.keys()
        for k in plain:
            assert got[k].dtype == plain[k].dtype and torch.equal(got[k], plain[k]), (tail, k)
    net = DAD3DNet(seed=0)
    keys = set(net.state_dict())
    InferenceNet(net, dtype=torch.float32, fold_bn=False, tail="hip")
    assert set(net.state_dict()) == keys  # the flag adds no module, parameter or buffer
    with pytest.raises(ValueError, match="tail"):
        InferenceNet(DAD3DNet(seed=0), tail="triton")


def test_entries_are_bound_and_refuse_bad_arguments_before_any_device_work():
    lib = _lib.load()
    for name, n_args in (("dad3d_nhwc_fusion_concat", 15), ("dad3d_nhwc_bias_mul", 8), ("dad3d_regression_heads", 12)):
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == n_args
    a = 0x1000
    assert lib.dad3d_nhwc_fusion_concat(a, a, a, a, 1, 4, 4, 4, 4, 16, 66, 8, 2, 0, None) == _lib.E_INVALID  # 66 bf16 channels: 132 bytes
    assert b"multiples of 4 (8 bytes)" in lib.dad3d_last_error()
    assert lib.dad3d_nhwc_fusion_concat(a, a, a + 8, a, 1, 4, 4, 4, 4, 16, 68, 8, 2, 0, None) == _lib.E_INVALID
    assert b"16-byte aligned" in lib.dad3d_last_error()
    assert lib.dad3d_nhwc_fusion_concat(a, a, None, a, 1, 4, 4, 4, 4, 16, 68, 8, 2, 0, None) == _lib.E_INVALID
    assert lib.dad3d_nhwc_fusion_concat(None, None, None, None, 0, 4, 4, 4, 4, 16, 68, 8, 2, 0, None) == _lib.OK
    assert lib.dad3d_nhwc_bias_mul(a, a, a, 4, 12, 2, 0, None) == _lib.E_INVALID and b"multiple of 8 (16 bytes)" in lib.dad3d_last_error()
    assert lib.dad3d_nhwc_bias_mul(a, a, None, 4, 16, 2, 0, None) == _lib.E_INVALID and b"null tensor" in lib.dad3d_last_error()
    assert lib.dad3d_nhwc_bias_mul(a, a, a + 4, 4, 16, 2, 0, None) == _lib.E_INVALID and b"16-byte aligned" in lib.dad3d_last_error()
    assert lib.dad3d_nhwc_bias_mul(a, a, a, 4, 16, 3, 0, None) == _lib.E_INVALID
    assert lib.dad3d_nhwc_bias_mul(None, None, None, 0, 16, 2, 0, None) == _lib.OK

    def heads(**over):
        d = _lib.HeadDescC(w1=a, b1=a, w2=a, b2=a, dst=a, dst_row_stride=16, dst_col_offset=0, hidden=8, out_dim=10, act=0, limit=0.0)
        for k, v in over.items():
            setattr(d, k, v)
        return (_lib.HeadDescC * 1)(d)

    def call(descs=None, top=a, batch=2, channels=16, hw=4, dtype=2, n=1, work=a, pooled=None, hidden=None):
        return lib.dad3d_regression_heads(top, batch, channels, hw, dtype, descs if descs is not None else heads(), n, work, pooled, hidden, 0, None)

    for kwargs, message in ((dict(dtype=5), b"unknown dtype"), (dict(batch=0), b"bad size"), (dict(batch=65536), b"bad size"), (dict(n=5), b"bad size"),
                            (dict(channels=12), b"not a multiple of 8"), (dict(top=None), b"null argument"), (dict(work=None), b"null argument"),
                            (dict(pooled=a + 4), b"16-byte aligned"), (dict(descs=heads(hidden=12)), b"hidden 12"),
                            (dict(descs=heads(act=3)), b"unknown activation"), (dict(descs=heads(w2=None)), b"null tensor"),
                            (dict(descs=heads(w1=a + 8)), b"misaligned"), (dict(descs=heads(dst_col_offset=8)), b"does not hold columns")):
        assert call(**kwargs) == _lib.E_INVALID, kwargs
        assert message in lib.dad3d_last_error(), (kwargs, lib.dad3d_last_error())
