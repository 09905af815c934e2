"""GPU: the three entries of csrc/net_tail.hip against their CPU statements (tests/net_tail_restatement.py, pinned to the framework
in tests/test_net_tail_host.py). `fusion_concat` and `bias_mul_` are held to the bit; the regression heads to the bit on inputs whose
sums are exact in any order, and to derived accumulation bounds, stage by stage, on real-valued inputs; then the whole tail inside
InferenceNet, eager and from a graph."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cnn_glue_restatement as R
import net_tail_restatement as T
from dad_3dheads_amd import _glue, _lib

pytestmark = pytest.mark.gpu

DTYPES = (torch.float32, torch.float16, torch.bfloat16)

# grid_for() in csrc/net_tail.hip caps a launch at 4096 blocks x 256 threads = 1,048,576 work items (8-byte pieces of fusion_concat's
# output, 16-byte vectors of bias_mul); the loop's later trips start there. Raise the shapes below with the cap.
GRID_ITEMS_PER_TRIP = 4096 * 256


def device_sigmoid(v):
    """float32 ndarray -> 1 / (1 + expf(-v)) with the DEVICE's expf: the framework's float32 sigmoid kernel, which
    tests/test_gpu_heatmap_points.py sweeps bit for bit against this library's sigmoid_f32."""
    return torch.sigmoid(torch.from_numpy(np.ascontiguousarray(v)).cuda()).cpu().numpy()


def as_bytes(t):
    return t.cpu().permute(0, 2, 3, 1).contiguous().view(torch.uint8)


# ---- fusion_concat --------------------------------------------------------------------------------------------------------------------

FUSION_SHAPES = (((64, 64), (16, 16)), ((7, 5), (3, 4)), ((5, 9), (11, 2)), ((4, 4), (4, 4)), ((3, 3), (1, 1)))


def fusion_inputs(n, cx, ch, cl, src, dst, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = R.nhwc(torch.randn(n, cx, *dst, generator=g).to(dtype))
    level = R.nhwc(torch.randn(n, cl, *dst, generator=g).to(dtype))
    heat = torch.randn(n, ch, *src, generator=g) * 6.0
    flat = heat.view(-1)
    flat[::7] = flat[::7] * 5.0  # logits beyond +-17: the sigmoid saturates in every type
    assert bool((heat.abs() > 17).any())
    if flat.numel() >= 40:
        flat[3], flat[17], flat[31] = float("nan"), float("inf"), float("-inf")
    return x, R.nhwc(heat.to(dtype)), level


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("channels", ((16, 68, 8), (1024, 68, 256)), ids=str)
@pytest.mark.parametrize("n", (1, 3))
def test_fusion_concat_is_the_statement_to_the_bit(dtype, channels, n):
    for k, (src, dst) in enumerate(FUSION_SHAPES):
        x, heat, level = fusion_inputs(n, *channels, src, dst, dtype, seed=k)
        want = T.fusion_concat_ref(x, heat, level, sigmoid=device_sigmoid)
        es = x.element_size()
        raw = torch.full((64 + want.numel() * es + 64,), 0x5A, dtype=torch.uint8, device="cuda")  # a guard band of 64 bytes on each side
        got = _glue.fusion_concat(x.cuda(), heat.cuda(), level.cuda())
        assert got.shape == want.shape and got.dtype == dtype and got.is_contiguous(memory_format=torch.channels_last)
        report = R.describe_mismatches(got.cpu(), want)
        assert report == "", f"{dtype} {channels} n={n} {src}->{dst}: {report}"
        cx, ch, _ = channels
        gb, wb = as_bytes(got), as_bytes(torch.cat([x, heat[:, :, :1, :1].expand(-1, -1, *dst), level], dim=1))
        assert torch.equal(gb[..., :cx * es], wb[..., :cx * es]) and torch.equal(gb[..., (cx + ch) * es:], wb[..., (cx + ch) * es:])
        # the same call through the C entry into the middle of the guarded buffer
        out = raw[64:64 + want.numel() * es].view(dtype).view(n, *dst, sum(channels)).permute(0, 3, 1, 2)
        assert out.data_ptr() % 16 == 0
        xs = [t.cuda() for t in (x, heat, level)]
        _lib.check(_lib.load().dad3d_nhwc_fusion_concat(out.data_ptr(), *(t.data_ptr() for t in xs), n, *dst, *src, *channels,
                                                        _glue._DTYPE[dtype][0], 0, torch.cuda.current_stream().cuda_stream))
        assert torch.equal(as_bytes(out), gb)
        assert bool((raw[:64] == 0x5A).all()) and bool((raw[-64:] == 0x5A).all())


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=str)
def test_fusion_concat_beyond_one_trip_of_the_grid(dtype):
    n, (cx, ch, cl), src, dst = 3, (1024, 68, 256), (64, 64), (33, 33)
    pieces = n * dst[0] * dst[1] * (cx + ch + cl) * torch.empty((), dtype=dtype).element_size() // 8
    assert pieces > GRID_ITEMS_PER_TRIP and pieces % GRID_ITEMS_PER_TRIP != 0
    x, heat, level = fusion_inputs(n, cx, ch, cl, src, dst, dtype, seed=9)
    got = _glue.fusion_concat(x.cuda(), heat.cuda(), level.cuda()).cpu()
    report = R.describe_mismatches(got, T.fusion_concat_ref(x, heat, level, sigmoid=device_sigmoid))
    assert report == "", f"{dtype}: {report}"


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_fusion_concat_against_the_frameworks_device_chain(dtype):
    """interpolate -> sigmoid -> cat on the device rounds twice (to the dtype after the interpolation, again after the sigmoid) where the
    kernel rounds once: every value within one unit in the last place of the dtype; how many differ is printed, not asserted.
    Logits inside (-2, 2), where that unit can be derived for the 2-byte types: the chain's first rounding moves v by at most half a
    step of [1, 2), 2^-8 resp. 2^-11, which moves the sigmoid by (1 - sigmoid) <= 0.88 of that relatively -- less than the smallest
    relative step of the type, 2^-8 resp. 2^-11 -- and two values less than one step apart round to neighbours at most.
    In float32 the chain does not round twice; its interpolation kernel fuses multiply-adds the statement rounds. Both evaluations
    of v are within 4 levels x 2^-24 x 1.9 of the exact value, so within 15.2 x 2^-24 of each other, which the sigmoid carries over
    as 0.88 x that relatively, under 14 steps of float32, and one more for the final roundings: 15. Measured: 4."""
    g = torch.Generator().manual_seed(21)
    x = R.nhwc(torch.randn(2, 16, 16, 16, generator=g).to(dtype)).cuda()
    level = R.nhwc(torch.randn(2, 8, 16, 16, generator=g).to(dtype)).cuda()
    heat = R.nhwc(torch.randn(2, 68, 64, 64, generator=g).clamp(-1.9, 1.9).to(dtype)).cuda()
    got = _glue.fusion_concat(x, heat, level)
    chain = torch.cat([x, F.interpolate(heat, size=(16, 16), mode="bilinear", align_corners=True).sigmoid(), level], dim=1)
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    steps = (got.contiguous().view(bits).int() - chain.contiguous().view(bits).int()).abs()  # sigmoids are positive: the patterns are ordered
    print(f"{dtype}: {int((steps != 0).sum())} of {steps.numel()} values differ from the framework's chain, the largest by {int(steps.max())} ulp")
    assert int(steps.max()) <= (15 if dtype == torch.float32 else 1)


def test_supported_fusion_says_which_tensors_the_kernel_takes():
    cl = lambda c, h, w, dtype=torch.bfloat16: torch.zeros(2, c, h, w, dtype=dtype, device="cuda").contiguous(memory_format=torch.channels_last)
    assert _glue.supported_fusion(cl(16, 4, 4), cl(68, 8, 8), cl(8, 4, 4))
    assert not _glue.supported_fusion(cl(16, 4, 4), cl(66, 8, 8), cl(8, 4, 4))  # 132 bytes: no multiple of 8
    assert _glue.supported_fusion(cl(16, 4, 4, torch.float32), cl(66, 8, 8, torch.float32), cl(8, 4, 4, torch.float32))
    assert not _glue.supported_fusion(cl(16, 4, 4), cl(68, 8, 8), cl(8, 4, 5))  # level at another extent
    assert not _glue.supported_fusion(cl(16, 4, 4), cl(68, 8, 8, torch.float16), cl(8, 4, 4))
    assert not _glue.supported_fusion(cl(16, 4, 4).cpu(), cl(68, 8, 8).cpu(), cl(8, 4, 4).cpu())
    assert not _glue.supported_fusion(torch.zeros(2, 16, 4, 4, dtype=torch.bfloat16, device="cuda"), cl(68, 8, 8), cl(8, 4, 4))  # NCHW
    with pytest.raises(ValueError, match="fusion_concat"):
        _glue.fusion_concat(cl(16, 4, 4), cl(66, 8, 8), cl(8, 4, 4))


# ---- bias_mul_ ------------------------------------------------------------------------------------------------------------------------

def run_bias_mul(y, bias, x):
    return _glue.bias_mul_(R.nhwc(y.cuda()), bias.cuda(), R.nhwc(x.cuda())).cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_bias_mul_is_bit_exact_on_every_pattern_in_every_lane(dtype):
    y, z = R.every_pattern(dtype)
    for bias in (torch.zeros(8, dtype=dtype), R.edge_bias(dtype)):
        report = R.describe_mismatches(run_bias_mul(y, bias, z), T.bias_mul_ref(y, bias, z), (y, z))
        assert report == "", f"{dtype}: {report}"


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_bias_mul_follows_ieee_on_non_finite_values(dtype):
    y, z, bias = R.nonfinite_case(dtype)
    want = T.bias_mul_ref(y, bias, z)
    assert int(want.isnan().sum()) > 0 and int(want.isinf().sum()) > 0
    report = R.describe_mismatches(run_bias_mul(y, bias, z), want, (y, z))
    assert report == "", f"{dtype}: {report}"


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_bias_mul_beyond_one_trip_of_the_grid(dtype):
    n, c, h, w = {torch.float32: (12, 24, 243, 241)}.get(dtype, (6, 24, 243, 241))
    cvec = c // R.VEC[dtype]
    assert n * h * w * cvec > GRID_ITEMS_PER_TRIP and cvec & (cvec - 1) != 0
    g = torch.Generator().manual_seed(33)
    y, x = (R.nhwc(torch.randn(n, c, h, w, generator=g).to(dtype)) for _ in range(2))
    bias = (torch.randn(c, generator=g) * 2.0).to(dtype)
    report = R.describe_mismatches(run_bias_mul(y, bias, x), T.bias_mul_ref(y, bias, x), (y, x))
    assert report == "", f"{dtype}: {report}"


# ---- regression_heads -----------------------------------------------------------------------------------------------------------------

ACTS = ((T.ACT_TANH, 3.0), (T.ACT_NONE, 0.0), (T.ACT_RELU, 0.0))
GUARD = -77.0


def run_heads(top, heads):
    """`heads`: (w1, b1, w2, b2) CPU tensors per head, ACTS in order. Heads 0 and 1 share one [B, out0 + out1 + 3] buffer (the params
    layout), head 2 writes at column 2 of its own; every row is wider than its columns. -> pooled, hidden, [out_k] on the CPU, after the
    guard columns have been checked."""
    b = top.shape[0]
    outs = [h[2].shape[0] for h in heads]
    params = torch.full((b, outs[0] + outs[1] + 3), GUARD, device="cuda")
    lmk = torch.full((b, outs[2] + 5), GUARD, device="cuda")
    dev = [[t.cuda() for t in h] for h in heads]
    where = ((params, 0), (params, outs[0]), (lmk, 2))
    pooled, hidden = _glue.regression_heads(top.cuda(), [(*d, act, lim, dst, col) for d, (act, lim), (dst, col) in zip(dev, ACTS, where)],
                                            stages=True)
    params, lmk = params.cpu(), lmk.cpu()
    assert bool((params[:, outs[0] + outs[1]:] == GUARD).all()) and bool((lmk[:, :2] == GUARD).all()) and bool((lmk[:, 2 + outs[2]:] == GUARD).all())
    return pooled.cpu(), hidden.cpu(), [params[:, :outs[0]], params[:, outs[0]:outs[0] + outs[1]], lmk[:, 2:2 + outs[2]]]


EXACT_SHAPES = (  # batch, C, hidden per head, out_dims, h, w
    (1, 8, (8, 8, 8), (5, 1, 2), 1, 1),
    (3, 40, (24, 8, 24), (5, 1, 2), 2, 4),
    (65, 40, (24, 24, 8), (403, 10, 136), 8, 8),
    (1, 2048, (512, 512, 512), (403, 10, 136), 8, 8),
    (3, 2048, (512, 24, 8), (5, 1, 2), 2, 4),
    (65, 2048, (512, 512, 512), (403, 10, 136), 1, 1),
    (65, 8, (8, 24, 512), (403, 10, 136), 2, 4),
    (9, 40, (24, 8, 512), (5, 10, 2), 8, 8),
)


@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_heads_are_bit_exact_where_every_partial_sum_is(shape, dtype):
    batch, c, hidden, out_dims, h, w = shape
    top, heads = T.exact_heads_case(batch, c, hidden, out_dims, h, w, dtype, seed=batch + c)
    want_pooled, want_hidden, want = T.heads_ref(top, [(*hd, act, lim) for hd, (act, lim) in zip(heads, ACTS)])
    pooled, hid, got = run_heads(top, heads)
    assert torch.equal(pooled.double(), want_pooled)
    assert torch.equal(hid.double(), torch.cat(want_hidden, dim=1))
    assert torch.equal(got[1].double(), want[1]) and torch.equal(got[2].double(), want[2])
    pre = T.layer_ref(want_hidden[0], heads[0][2], heads[0][3])[0]
    tol = T.tanh_bound(pre, torch.zeros_like(pre), 3.0, T.recorded_tanh_ulps())
    assert bool(((got[0].double() - want[0]).abs() <= tol).all())


@pytest.mark.parametrize("batch", (1, 20))
def test_heads_keep_a_nan_in_its_row_and_only_there(batch):
    top, heads = T.exact_heads_case(batch, 40, (24, 8, 24), (5, 1, 2), 2, 4, torch.bfloat16, seed=4)
    row = batch - 1
    top[row, 7, 1, 2] = float("nan")
    for hd in heads:
        hd[0][:, 7] = 1.0  # every hidden unit sees the channel
        hd[2][:, 1] = 0.5  # and every output sees a hidden unit
    _, _, got = run_heads(top, heads)
    for out in got:  # also through the ReLU head
        assert bool(out[row].isnan().all()) and not bool(out[:row].isnan().any())


@pytest.mark.parametrize("hw", ((7, 5), (8, 8)), ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_heads_stay_inside_the_derived_bounds_stage_by_stage(dtype, hw):
    """Each stage against the float64 statement of the kernel's OWN previous stage (pooled_out, hidden_out): pooling (hw + 1) u M,
    a layer (K + 2) u M, the tanh head with the recorded tanhf error on top."""
    g = torch.Generator().manual_seed(17)
    batch, c, hidden, outs = 19, 2048, (512, 24, 512), (403, 10, 136)
    scale = 10.0 ** torch.linspace(-3, 2, batch).view(batch, 1, 1, 1)  # magnitudes 1e-3 .. 1e2, one per image
    top = R.nhwc((torch.randn(batch, c, *hw, generator=g) * scale).to(dtype))
    heads = []
    for hid, out in zip(hidden, outs):
        heads.append([t.to(dtype) for t in (torch.randn(hid, c, generator=g) / c ** 0.5, torch.randn(hid, generator=g) * 0.1,
                                            torch.randn(out, hid, generator=g) / hid ** 0.5, torch.randn(out, generator=g) * 0.1)])
    pooled, hid_got, got = run_heads(top, heads)
    E, M = T.pool_ref(top)
    worst = {"pool": float(((pooled.double() - E).abs() / T.pool_bound(E, M, hw[0] * hw[1])).max())}
    column = 0
    for k, ((w1, b1, w2, b2), (act, lim)) in enumerate(zip(heads, ACTS)):
        E1, M1 = T.layer_ref(pooled, w1, b1)
        mine = hid_got[:, column:column + w1.shape[0]]
        column += w1.shape[0]
        worst[f"hidden{k}"] = float(((mine.double() - torch.relu(E1)).abs() / T.layer_bound(M1, c)).max())
        E2, M2 = T.layer_ref(mine, w2, b2)
        bound = T.layer_bound(M2, w1.shape[0])
        tol = T.tanh_bound(E2, bound, lim, T.recorded_tanh_ulps()) if act == T.ACT_TANH else bound
        worst[f"out{k}"] = float(((got[k].double() - T.activation_ref(E2, act, lim)).abs() / tol).max())
    print(f"{dtype} {hw}: worst error / bound per stage {worst}")
    assert max(worst.values()) <= 1.0, worst


def test_tanhf_sweep_stays_within_the_recorded_error():
    """Every float32 in [-9.1, 9.1] of stride 4099 bit patterns through the heads' own tanhf (a float32 head of zero weights whose biases
    are the arguments, limit 1): no worse than what profiles/net_tail_bench.json records."""
    worst = tanh_sweep()
    print(f"tanhf sweep: largest error {worst:.3f} ulp, recorded {T.recorded_tanh_ulps():.3f}")
    assert worst <= T.recorded_tanh_ulps()


def tanh_sweep():
    x = torch.from_numpy(T.tanh_sweep_inputs())
    n = x.numel()
    top = R.nhwc(torch.zeros(1, 4, 1, 1)).cuda()
    out = torch.empty(1, n, device="cuda")
    w1, b1, w2 = torch.zeros(4, 4, device="cuda"), torch.zeros(4, device="cuda"), torch.zeros(n, 4, device="cuda")
    _glue.regression_heads(top, [(w1, b1, w2, x.cuda(), T.ACT_TANH, 1.0, out, 0)])
    return T.ulp_error(out.cpu().numpy()[0], np.tanh(x.numpy().astype(np.float64)))


# ---- end to end -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def served():
    from dad_3dheads_amd.network import DAD3DNet, GraphedNet, InferenceNet

    x = torch.randn(2, 3, 128, 128, generator=torch.Generator().manual_seed(2)).cuda()
    hip = InferenceNet(DAD3DNet(seed=0), dtype=torch.bfloat16, tail="hip").cuda()
    plain = InferenceNet(DAD3DNet(seed=0), dtype=torch.bfloat16, tail="framework").cuda()
    captured = []
    handle = hip.net.encoder.stages[4].register_forward_hook(lambda m, i, o: captured.append(o.detach().clone()))
    out = hip(x)
    handle.remove()
    return x, hip, plain, out, captured[0], GraphedNet


def test_served_tail_is_the_statement_on_the_last_stages_map(served):
    from dad_3dheads_amd.network import HIP_TAIL_PIECES, OUTPUT_2D_LANDMARKS, OUTPUT_3DMM_PARAMS

    x, hip, plain, out, top, _ = served
    assert "heads" in HIP_TAIL_PIECES
    want_out = plain(x)
    assert out.keys() == want_out.keys()
    for k in out:
        assert out[k].shape == want_out[k].shape and out[k].dtype == want_out[k].dtype == torch.float32, k
    net, top = hip.net, top.cpu()
    assert top.shape == (2, 2048, 4, 4)
    E, M = T.pool_ref(top)
    pool_err = T.pool_bound(E, M, 16)
    worst = 0.0
    for name, (act, lim), got in (("shape", ACTS[0], out[OUTPUT_3DMM_PARAMS][:, :403]), ("pose", ACTS[1], out[OUTPUT_3DMM_PARAMS][:, 403:]),
                                  ("landmarks", ACTS[2], out[OUTPUT_2D_LANDMARKS].reshape(2, 136))):
        w1, b1, w2, b2 = (t.detach().cpu() for t in (getattr(net, name).mlp[0].weight, getattr(net, name).mlp[0].bias,
                                                     getattr(net, name).mlp[3].weight, getattr(net, name).mlp[3].bias))
        E1, M1 = T.layer_ref(E, w1, b1)
        err1 = T.layer_bound(M1, 2048) + pool_err @ w1.double().abs().t()  # the first layer's own rounding and the pooling's, carried through |w1|
        hid = torch.relu(E1)
        E2, M2 = T.layer_ref(hid, w2, b2)
        err2 = T.layer_bound(M2 + err1 @ w2.double().abs().t(), 512) + err1 @ w2.double().abs().t()
        tol = T.tanh_bound(E2, err2, lim, T.recorded_tanh_ulps()) if act == T.ACT_TANH else err2
        worst = max(worst, float(((got.cpu().double() - T.activation_ref(E2, act, lim)).abs() / tol).max()))
    print(f"served tail against the statement on the captured map: worst error / bound {worst:.3f}")
    assert worst <= 1.0


def test_tail_repeats_its_bits_eagerly_and_from_a_graph(served):
    """The three pieces on fixed inputs (the captured map; fusion inputs of the network's shapes): two eager calls and two replays of a
    captured graph give the same bits -- no atomics, a fixed order of every sum, workspaces from torch.empty inside the capture."""
    _, hip, _, _, top, _ = served
    g = torch.Generator().manual_seed(12)
    cl = lambda *shape: R.nhwc(torch.randn(*shape, generator=g).to(torch.bfloat16)).cuda()  # noqa: E731
    x, heat, level = cl(2, 1024, 8, 8), cl(2, 68, 32, 32), cl(2, 256, 8, 8)
    heads, bias = hip.net.__dict__["tail_heads"], hip.net.fusion.bias

    def tail():
        fused = _glue.fusion_concat(x, heat, level)
        return (fused, _glue.bias_mul_(x.clone(), bias, x), *heads(top))

    eager, again = tail(), tail()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        tail()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = tail()
    for _ in range(2):
        for t in static:
            t.fill_(7.0)
        graph.replay()
        for a, b, c in zip(eager, again, static):
            assert R.describe_mismatches(b, a) == "" and R.describe_mismatches(c, a) == ""


def test_graphed_net_captures_and_replays_the_hip_tail(served, monkeypatch):
    """GraphedNet over the served network: the keys, shapes and dtypes of the eager call, and after every replay the tail's outputs are,
    to the bit, what the eager entries give on the tensors that replay fed them. The comparison is on the tail's own inputs because
    the framework's convolutions in front of it do not repeat their bits on this runtime, neither from one eager call to the next
    nor from one replay to the next (the heat map, which no kernel of this library touches, differs; printed below). So the graph's
    static tensors are held on to: the inputs and the output of `fusion_concat`, and the last stage's map that feeds the heads."""
    from dad_3dheads_amd.network import OUTPUT_2D_LANDMARKS, OUTPUT_3DMM_PARAMS, OUTPUT_LANDMARKS_HEATMAP

    x, hip, _, out, _, GraphedNet = served
    fusion_calls, tops = [], []
    plain_fusion_concat = _glue.fusion_concat

    def recording_fusion_concat(a, heat, level):
        fused = plain_fusion_concat(a, heat, level)
        fusion_calls.append((a, heat, level, fused))
        return fused

    monkeypatch.setattr(_glue, "fusion_concat", recording_fusion_concat)
    handle = hip.net.encoder.stages[4].register_forward_hook(lambda m, i, o: tops.append(o))
    graphed = GraphedNet(hip)
    try:
        first = graphed(x)  # warm-up calls, then the capture: the last recorded tensors are the graph's own
    finally:
        handle.remove()
        monkeypatch.setattr(_glue, "fusion_concat", plain_fusion_concat)
    n_calls = len(tops)
    assert n_calls == len(fusion_calls) >= 1
    (a, heat, level, fused), top = fusion_calls[-1], tops[-1]
    heads = hip.net.__dict__["tail_heads"]
    assert first.keys() == out.keys()
    results = [first, graphed(x), graphed(x)]
    assert len(tops) == n_calls  # replays: no Python ran
    for k in out:
        assert all(r[k].shape == out[k].shape and r[k].dtype == torch.float32 and bool(torch.isfinite(r[k]).all()) for r in results), k
    # the static tensors hold the LAST replay's values: the tail's outputs of that replay against the eager entries on them
    last = results[-1]
    assert R.describe_mismatches(fused, plain_fusion_concat(a, heat, level)) == ""
    params, lmk = heads(top)
    assert torch.equal(last[OUTPUT_3DMM_PARAMS], params) and torch.equal(last[OUTPUT_2D_LANDMARKS], lmk)
    assert torch.equal(last[OUTPUT_LANDMARKS_HEATMAP], heat.float())
    for k in out:
        print(f"{k}: replay == replay to the bit: {torch.equal(results[1][k], results[2][k])}; replay == the eager call: "
              f"{torch.equal(last[k], out[k])}, largest difference {float((last[k] - out[k]).abs().max()):.3g}")


def test_predictor_with_the_hip_tail_predicts_finite_heads():
    from dad_3dheads_amd import synthetic
    from dad_3dheads_amd.predictor import FaceMeshPredictor

    static = synthetic.load_static()
    predictor = FaceMeshPredictor.random_init(tail="hip", flame_model=synthetic.synthetic_flame_model(0, static))
    rng = np.random.default_rng(0)
    images = [rng.integers(0, 256, (96, 80, 3), dtype=np.uint8), rng.integers(0, 256, (64, 120, 3), dtype=np.uint8)]
    results = predictor.predict_batch(images)
    assert len(results) == 2
    for r in results:
        assert {"points", "projected_vertices", "3d_vertices", "3dmm_params"} <= set(r.keys())
        assert bool(torch.isfinite(torch.as_tensor(r["3d_vertices"])).all())
