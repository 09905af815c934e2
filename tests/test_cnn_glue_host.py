"""The restatement of the CNN glue (tests/cnn_glue_restatement.py) pinned to the framework's own CPU ops, without a GPU: the GPU tests
of csrc/cnn_glue.hip hold the kernels to it to the bit, so it must not be wrong about what it restates."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cnn_glue_restatement as R

DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def test_nearest_index_is_the_frameworks_for_every_extent_to_40():
    for n_in in range(1, 41):
        ramp = torch.arange(n_in, dtype=torch.float32)
        for n_out in range(1, 41):
            want_h = F.interpolate(ramp.view(1, 1, n_in, 1), size=(n_out, 1), mode="nearest").flatten().long().numpy()
            want_w = F.interpolate(ramp.view(1, 1, 1, n_in), size=(1, n_out), mode="nearest").flatten().long().numpy()
            got = R.nearest_index(n_in, n_out)
            assert got.dtype == np.int64 and np.array_equal(got, want_h) and np.array_equal(got, want_w), (n_in, n_out)


def test_float_and_integer_source_index_differ_at_exactly_three_places():
    differ = {(n_in, n_out, d) for n_in in range(1, 41) for n_out in range(1, 41)
              for d in np.flatnonzero(R.nearest_index(n_in, n_out) != np.arange(n_out) * n_in // n_out).tolist()}
    assert differ == {(26, 22, 11), (39, 33, 11), (39, 33, 22)} == R.FLOAT_INDEX_EXCEPTIONS


def test_gather_nearest_equals_interpolate_on_both_axes_at_once():
    for (h, w), size in (((26, 39), (22, 33)), ((39, 26), (33, 22)), ((5, 7), (16, 3)), ((1, 40), (40, 1))):
        x = R.indexed_input(2, 4, h, w, torch.float32, seed=h)
        assert torch.equal(R.gather_nearest(x, size), F.interpolate(x, size=size, mode="nearest"))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_bias_act_ref_rounds_once_to_nearest_even_and_keeps_nan(dtype):
    u, c = R.UNIT_ROUNDOFF[dtype], R.VEC[dtype]
    one = lambda v: R.nhwc(torch.full((1, c, 1, 1), v, dtype=torch.float64).to(dtype))
    bias = lambda v: torch.full((c,), v, dtype=torch.float64).to(dtype)
    # 1 + u is a tie between 1 (even) and 1 + 2u (odd); 1 + 2u + u a tie between 1 + 2u (odd) and 1 + 4u (even)
    assert torch.equal(R.bias_act_ref(one(1.0), bias(u)), one(1.0))
    assert torch.equal(R.bias_act_ref(one(1.0 + 2 * u), bias(u)), one(1.0 + 4 * u))
    # one rounding, not two: (1 + u) + u/2 is past the tie; rounding y + bias to the type first would lose it
    if dtype != torch.float32:
        assert torch.equal(R.bias_act_ref(one(1.0), bias(u), one(u / 2)), one(1.0 + 2 * u))
    nan = R.bias_act_ref(one(float("nan")), bias(0.0), None, relu=True)
    assert bool(nan.isnan().all()) and bool(F.relu(torch.tensor(float("nan"))).isnan())
    assert torch.equal(R.bias_act_ref(one(float("-inf")), bias(0.0), None, relu=True), one(0.0))
    assert torch.equal(R.bias_act_ref(one(-3.0), bias(1.0), one(1.5), relu=False), one(-0.5))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_the_plain_branch_of_conv_bias_act_equals_the_restatement_on_non_finite_data(dtype):
    """ConvBiasAct's branch for CPU tensors and unsupported shapes (plain framework ops in the tensor's own type) on NaN, +-inf and
    exactly representable sums: the statement the GPU kernel is held to in tests/test_gpu_cnn_glue.py."""
    y, z, bias = R.nonfinite_case(dtype)
    for zz in (None, z):
        for relu in (False, True):
            got = R.plain_conv_bias_act(bias, relu)(y.clone(), zz)
            assert R.describe_mismatches(got, R.bias_act_ref(y, bias, zz, relu), (y, zz)) == "", (dtype, zz is not None, relu)
    want = R.bias_act_ref(y, bias, z, True)
    assert bool(want[0, 0, 0].isnan().all()) and bool(want[0, 0, :, 0].isnan().all())  # NaN in y or in z stays NaN through ReLU
    k = R.NONFINITE_VALUES.index
    assert float(want[0, 0, k(float("inf")), k(1.0)]) == float("inf") and float(want[0, 0, k(float("-inf")), k(1.0)]) == 0.0
    assert bool(want[0, 0, k(float("inf")), k(float("-inf"))].isnan())


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_every_pattern_inputs_put_each_value_in_each_lane(dtype):
    y, z = R.every_pattern(dtype)
    assert y.shape == z.shape == (1, 8, 256, 256) and y.is_contiguous(memory_format=torch.channels_last)
    rows = y.permute(0, 2, 3, 1).reshape(65536, 8).view(torch.int32 if dtype == torch.float32 else torch.int16).numpy()
    assert all(np.array_equal(np.roll(rows[:, 0], -c), rows[:, c]) for c in range(8))
    if dtype == torch.float32:
        lane0 = rows[:, 0].view(np.uint32)
        assert set(((lane0 >> 23) & 0xFF).tolist()) == set(range(256))  # every exponent, subnormals and inf / NaN among them
    else:
        assert np.array_equal(np.sort(rows[:, 0].view(np.uint16)), np.arange(65536))
        zr = z.permute(0, 2, 3, 1).reshape(65536, 8).view(torch.int16).numpy().view(np.uint16)
        assert all(np.array_equal(np.sort(zr[:, c]), np.arange(65536)) for c in range(8))
    assert R.edge_bias(dtype).dtype == dtype


def emulate_fp32_accumulation(weights, xs, dtype, fused):
    """The kernel's arithmetic restated in NumPy float32: acc = acc + w * x from zero, then one cast. `fused`: the product enters
    the sum unrounded (float64 holds a 24 x 24-bit product exactly; its sum is then rounded to float32)."""
    acc = np.zeros(xs[0].shape, dtype=np.float32)
    for w, x in zip(weights, xs):
        w32, x32 = np.float32(w), x.float().numpy()
        acc = (acc.astype(np.float64) + np.float64(w32) * x32.astype(np.float64)).astype(np.float32) if fused else acc + w32 * x32
        assert acc.dtype == np.float32
    return torch.from_numpy(acc).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_an_fp32_accumulation_stays_inside_the_stated_bound(dtype):
    g = torch.Generator().manual_seed(5)
    worst = 0.0
    for draw in range(20):
        k = 1 + draw % 3
        mags = 10.0 ** (torch.rand(k, generator=g) * 5.0 - 3.0)  # 1e-3 .. 1e2
        xs = [(torch.randn(1, 8, 32, 32, generator=g) * m).to(dtype) for m in mags.tolist()]
        weights = (torch.rand(k, generator=g) * 2.0 - 0.5).tolist()
        E, M = R.resize_sum_ref(weights, xs, (32, 32))
        bound = R.resize_sum_bound(dtype, E, M)
        for fused in (False, True):
            got = emulate_fp32_accumulation(weights, xs, dtype, fused)
            ratio = float(((got.double() - E).abs() / bound).max())
            assert ratio <= 1.0, (dtype, draw, fused, ratio)
            worst = max(worst, ratio)
    assert worst > 0.25, worst  # the bound is not vacuous: a plain accumulation uses a good part of it


def test_a_unit_weight_single_input_sum_is_a_plain_gather():
    x = R.indexed_input(2, 8, 5, 7, torch.bfloat16, seed=1)
    E, M = R.resize_sum_ref([1.0], [x], (9, 4))
    assert torch.equal(E, F.interpolate(x.double(), size=(9, 4))) and torch.equal(M, E.abs())
