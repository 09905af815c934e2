"""GPU: the two streaming kernels of csrc/cnn_glue.hip (`nhwc_bias_act`, `nhwc_resize_sum`) against their CPU restatement
(tests/cnn_glue_restatement.py, pinned to the framework in tests/test_cnn_glue_host.py). `bias_act_` is held to the bit -- fp32
arithmetic in a fixed order, one rounding to nearest even at the store, NaN kept through the ReLU -- and `resize_sum` to PyTorch's
float source index and a derived accumulation bound; both beyond one sweep of the launch grid, next to guard bands, and at the
edges of their argument contract."""
import ctypes as C

import pytest
import torch

import cnn_glue_restatement as R
from dad_3dheads_amd import _glue, _lib

pytestmark = pytest.mark.gpu

DTYPES = (torch.float32, torch.float16, torch.bfloat16)
CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}  # DAD3D_DTYPE_*
FUSION_WEIGHTS = (0.43, 0.31, 0.27)

# More work items than the launch grid covers in ONE trip: grid_for() in csrc/cnn_glue.hip caps a launch at 4096 blocks x 256
# threads = 1,048,576 16-byte vectors, and the loop's later trips (the ones production batches run) start there. These shapes have
# 4,216,536 (fp32) and 1,054,134 (2-byte) vectors, and C / vector width = 6 resp. 3 is no power of two: 1,048,576 mod 6 = 4 and
# mod 3 = 1, so the bias phase shifts on every trip and the last trip is ragged. Raise them with the cap.
GRID_VECTORS_PER_TRIP = 4096 * 256
STRIDE_SHAPE = {torch.float32: (12, 24, 243, 241), torch.float16: (6, 24, 243, 241), torch.bfloat16: (6, 24, 243, 241)}
STRIDE_SOURCES = ((243, 241), (122, 121), (61, 60))


def dev(t):
    return None if t is None else R.nhwc(t.cuda())


def run_bias_act(y, bias, z, relu):
    got = _glue.bias_act_(dev(y), bias.cuda(), dev(z), relu)
    assert got.is_contiguous(memory_format=torch.channels_last)
    return got.cpu()


def assert_inside_bound(got, weights, xs, size, what):
    E, M = R.resize_sum_ref(weights, xs, size)
    assert got.shape == E.shape and got.dtype == xs[0].dtype and got.is_contiguous(memory_format=torch.channels_last), what
    err, bound = (got.cpu().double() - E).abs(), R.resize_sum_bound(got.dtype, E, M)
    worst = float((err / bound).max())
    assert worst <= 1.0, (what, "error / bound", worst, "at", tuple(int(i) for i in (err / bound).flatten().argmax().view(1)))


# ---- a. every 2-byte pattern in every lane; fp32 over the whole exponent range ----------------------------------------------------

@pytest.fixture(scope="module", params=DTYPES, ids=str)
def patterns(request):
    y, z = R.every_pattern(request.param)
    return request.param, y, z


@pytest.mark.parametrize("bias_kind", ("zero", "edge"))
def test_bias_act_is_bit_exact_on_every_pattern_in_every_lane(patterns, bias_kind):
    """Subnormal loads, overflow to inf at the store, ties and the direction of round-to-nearest-even, NaN and inf through the
    clamp: bit equality (+-0 equal, NaN by NaN-ness) with one fp32 evaluation rounded once."""
    dtype, y, z = patterns
    bias = torch.zeros(8, dtype=dtype) if bias_kind == "zero" else R.edge_bias(dtype)
    for zz in (None, z):
        for relu in (False, True):
            got = run_bias_act(y, bias, zz, relu)
            report = R.describe_mismatches(got, R.bias_act_ref(y, bias, zz, relu), (y, zz))
            assert report == "", f"{dtype} bias={bias_kind} z={zz is not None} relu={relu}: {report}"


# ---- b. non-finite values through the ReLU ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_relu_keeps_nan_and_clamps_infinities_like_the_framework(dtype):
    """NaN, +inf and -inf in y and in z with relu=True: the kernel, the restatement and ConvBiasAct's plain-ops branch (what CPU
    tensors and unsupported shapes get) agree -- a NaN activation must not leave the serving path as a clean zero."""
    y, z, bias = R.nonfinite_case(dtype)
    for zz in (None, z):
        want = R.bias_act_ref(y, bias, zz, True)
        module = R.plain_conv_bias_act(bias, True)
        plain = module(y.clone(), zz)  # CPU tensors: the plain branch
        assert R.describe_mismatches(plain, want, (y, zz)) == ""
        got = run_bias_act(y, bias, zz, True)
        assert R.describe_mismatches(got, want, (y, zz)) == "", f"{dtype} z={zz is not None}: {R.describe_mismatches(got, want, (y, zz))}"
        assert R.describe_mismatches(got, plain, (y, zz)) == ""
        served = module.cuda()(dev(y), dev(zz)).cpu()  # CUDA channels-last tensors: the same module goes through the kernel
        assert R.describe_mismatches(served, plain, (y, zz)) == "", f"{dtype} z={zz is not None}: ConvBiasAct on the GPU differs from its plain branch"
        assert bool(got[want.isnan()].isnan().all()) and int(want.isnan().sum()) > 0


# ---- c. the grid-stride loop and the channel phase --------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=DTYPES, ids=str)
def beyond_one_trip(request):
    dtype = request.param
    n, c, h, w = STRIDE_SHAPE[dtype]
    assert n * h * w * (c // R.VEC[dtype]) > GRID_VECTORS_PER_TRIP and (c // R.VEC[dtype]) & (c // R.VEC[dtype] - 1) != 0
    g = torch.Generator().manual_seed(31)
    y = R.nhwc(torch.randn(n, c, h, w, generator=g).to(dtype))
    z = R.nhwc(torch.randn(n, c, h, w, generator=g).to(dtype))
    bias = (torch.randn(c, generator=g) * 2.0).to(dtype)
    small = [R.nhwc(torch.randn(n, c, sh, sw, generator=g).to(dtype)) for sh, sw in STRIDE_SOURCES[1:]]
    return dtype, y, z, bias, small


def test_bias_act_beyond_one_trip_of_the_grid(beyond_one_trip):
    dtype, y, z, bias, _ = beyond_one_trip
    got = run_bias_act(y, bias, z, True)
    report = R.describe_mismatches(got, R.bias_act_ref(y, bias, z, True), (y, z))
    assert report == "", f"{dtype}: {report}"


def test_resize_sum_beyond_one_trip_of_the_grid(beyond_one_trip):
    dtype, y, _, _, small = beyond_one_trip
    xs = [y] + small
    got = _glue.resize_sum(FUSION_WEIGHTS, [dev(x) for x in xs], STRIDE_SOURCES[0])
    assert_inside_bound(got, FUSION_WEIGHTS, xs, STRIDE_SOURCES[0], dtype)


# ---- d. source indices and the accumulation bound ---------------------------------------------------------------------------------

def test_resize_gathers_the_frameworks_source_pixel_for_every_extent_to_40():
    """Every (in, out) in 1..40 along H, each with a DIFFERENT pair along W (the pair reversed and shifted, so an H / W mix-up
    shows), one input of weight 1.0: the output is the gathered input, bit for bit."""
    wrong = []
    for h_in in range(1, 41):
        for h_out in range(1, 41):
            w_in, w_out = h_out % 40 + 1, (h_in + 6) % 40 + 1
            x = R.indexed_input(2, 4, h_in, w_in, torch.float32, seed=h_in * 41 + h_out)
            got = _glue.resize_sum([1.0], [x.cuda()], (h_out, w_out)).cpu()
            if got.shape != (2, 4, h_out, w_out) or bool(R.bit_mismatches(got, R.gather_nearest(x, (h_out, w_out))).any()):
                wrong.append(((h_in, w_in), (h_out, w_out)))
    assert not wrong, f"{len(wrong)} of 1600 resizes gather another pixel than F.interpolate, first {wrong[:5]}"


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_resize_sum_where_float_and_integer_indices_part(dtype):
    """26 -> 22 (dst 11) and 39 -> 33 (dst 11 and 22): the only extents to 40 where PyTorch's floor(dst * (float) in / out) is not
    dst * in // out. Along H and along W, in every input slot, with 1, 2 and 3 inputs."""
    c = R.VEC[dtype]
    for size, special, others in (((22, 33), (26, 39), ((11, 66), (44, 17))), ((33, 22), (39, 26), ((66, 11), (17, 44)))):
        assert all((s, o, 11) in R.FLOAT_INDEX_EXCEPTIONS for s, o in zip(special, size))
        xs = [R.indexed_input(2, c, h, w, dtype, seed=h) for h, w in (special,) + others]
        for k in (1, 2, 3):
            for first in range(k):  # the special extents in slot (k - first) % k
                order = [xs[(j + first) % k] for j in range(k)]
                got = _glue.resize_sum(FUSION_WEIGHTS[:k], [x.cuda() for x in order], size)
                assert_inside_bound(got, FUSION_WEIGHTS[:k], order, size, (dtype, size, k, first))
        exact = _glue.resize_sum([1.0], [xs[0].cuda()], size).cpu()
        assert R.describe_mismatches(exact, R.gather_nearest(xs[0], size)) == "", (dtype, size)


# ---- e. guard bands, offset views, aliasing ---------------------------------------------------------------------------------------

def sentinel_buffer(n, c, h, w, dtype):
    """[n,c,h,w] channels-last on the GPU, every byte 0x5A (a finite value in all three types)."""
    raw = torch.full((n * h * w * c * torch.empty((), dtype=dtype).element_size(),), 0x5A, dtype=torch.uint8, device="cuda")
    return raw.view(dtype).view(n, h, w, c).permute(0, 3, 1, 2)


def as_bytes(t):
    """uint8 [N,H,W,C * element size] of a channels-last tensor, on the CPU."""
    return t.cpu().permute(0, 2, 3, 1).contiguous().view(torch.uint8)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_bias_act_in_place_on_a_view_leaves_its_neighbours_alone(dtype):
    n, c, h, w = 3, R.VEC[dtype] * 3, 3, 5
    assert (c * h * w * torch.empty((), dtype=dtype).element_size()) % 16 == 0
    g = torch.Generator().manual_seed(7)
    y, z = (R.nhwc(torch.randn(n, c, h, w, generator=g).to(dtype)) for _ in range(2))
    bias = torch.randn(c, generator=g).to(dtype)
    for zz in (None, z):
        buf = sentinel_buffer(n + 2, c, h, w, dtype)
        before = buf.cpu()
        view = buf[1:n + 1]
        view.copy_(y)
        assert view.data_ptr() != buf.data_ptr() and _glue.supported(view, dev(zz))
        out = _glue.bias_act_(view, bias.cuda(), dev(zz), True)
        assert out.data_ptr() == view.data_ptr()
        after = buf.cpu()
        assert R.describe_mismatches(after[1:n + 1], R.bias_act_ref(y, bias, zz, True), (y, zz)) == ""
        guard = as_bytes(torch.cat((after[:1], after[n + 1:])))
        assert torch.equal(guard, as_bytes(torch.cat((before[:1], before[n + 1:])))) and bool((guard == 0x5A).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_resize_sum_reads_views_into_larger_buffers(dtype):
    n, c = 2, R.VEC[dtype] * 3
    shapes, size = ((3, 5), (6, 9), (2, 3)), (5, 7)
    xs = [R.indexed_input(n, c, h, w, dtype, seed=10 + h) for h, w in shapes]
    bufs, views = [], []
    for x in xs:
        buf = sentinel_buffer(n + 2, *x.shape[1:], dtype)
        buf[1:n + 1].copy_(x)
        bufs.append(buf)
        views.append(buf[1:n + 1])
        assert views[-1].data_ptr() % 16 == 0 and views[-1].data_ptr() != buf.data_ptr()
    got = _glue.resize_sum(FUSION_WEIGHTS, views, size)
    assert_inside_bound(got, FUSION_WEIGHTS, xs, size, dtype)
    for buf in bufs:
        assert bool((as_bytes(torch.cat((buf[:1], buf[n + 1:]))) == 0x5A).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_bias_act_with_the_output_as_its_own_residual(dtype):
    """z is y: act(2 y + b). Each thread loads y and z before it stores y, and no other thread touches that vector."""
    g = torch.Generator().manual_seed(9)
    y = R.nhwc(torch.randn(2, R.VEC[dtype] * 5, 7, 3, generator=g).to(dtype))
    bias = torch.randn(y.shape[1], generator=g).to(dtype)
    y_dev = dev(y)
    got = _glue.bias_act_(y_dev, bias.cuda(), y_dev, True).cpu()
    assert R.describe_mismatches(got, R.bias_act_ref(y, bias, y, True), (y,)) == ""


# ---- f. the argument contract -----------------------------------------------------------------------------------------------------

def last_error():
    return _lib.load().dad3d_last_error().decode()


def raw_bias_act(y_ptr, bias_ptr, z_ptr, n_pixels, channels, code, relu=1):
    return _lib.load().dad3d_nhwc_bias_act(y_ptr, bias_ptr, z_ptr, n_pixels, channels, code, relu, 0,
                                           torch.cuda.current_stream().cuda_stream)


def raw_resize_sum(out_ptr, n, oh, ow, channels, code, k, ptrs, hs, ws, weights=(1.0, 1.0, 1.0, 1.0)):
    m = max(len(ptrs), 1)
    return _lib.load().dad3d_nhwc_resize_sum(out_ptr, n, oh, ow, channels, code, k, (C.c_void_p * m)(*ptrs), (C.c_int * m)(*hs),
                                             (C.c_int * m)(*ws), (C.c_float * m)(*weights[:m]), 0, torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_bias_act_refuses_bad_arguments_and_launches_nothing(dtype):
    vec = R.VEC[dtype]
    c = vec * 3
    y = torch.full((2, c, 2, 2), 1.0, dtype=dtype, device="cuda").contiguous(memory_format=torch.channels_last)
    bias = torch.ones(c + vec, dtype=dtype, device="cuda")
    before = y.clone()
    yp, bp = y.data_ptr(), bias.data_ptr()
    calls = (
        ((yp, bp, None, 8, c - vec // 2, CODE[dtype]), f"{c - vec // 2} channels are not a multiple of {vec} (16 bytes)"),
        ((yp + 4, bp, None, 4, c, CODE[dtype]), "tensors must be 16-byte aligned"),
        ((yp, bp + 4, None, 4, c, CODE[dtype]), "tensors must be 16-byte aligned"),
        ((yp, bp, yp + 4, 4, c, CODE[dtype]), "tensors must be 16-byte aligned"),
        ((yp, bp, None, 8, c, 3), "dad3d_nhwc_bias_act: bad argument"),
        ((yp, bp, None, 8, c, -1), "dad3d_nhwc_bias_act: bad argument"),
        ((yp, bp, None, -1, c, CODE[dtype]), "dad3d_nhwc_bias_act: bad argument"),
        ((yp, bp, None, 8, 0, CODE[dtype]), "dad3d_nhwc_bias_act: bad argument"),
        ((None, bp, None, 8, c, CODE[dtype]), "dad3d_nhwc_bias_act: null tensor"),
        ((yp, None, None, 8, c, CODE[dtype]), "dad3d_nhwc_bias_act: null tensor"),
    )
    for args, message in calls:
        assert raw_bias_act(*args) == _lib.E_INVALID, args
        assert message in last_error(), (args, last_error())
    assert raw_bias_act(None, None, None, 0, c, CODE[dtype]) == _lib.OK  # nothing to do: no pointer is looked at
    torch.cuda.synchronize()
    assert torch.equal(as_bytes(y), as_bytes(before))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_resize_sum_refuses_bad_arguments_and_launches_nothing(dtype):
    vec = R.VEC[dtype]
    c = vec * 2
    x = torch.ones((2, c, 4, 4), dtype=dtype, device="cuda").contiguous(memory_format=torch.channels_last)  # twice what n = 1 reads
    out = torch.full((2, c, 3, 3), 7.0, dtype=dtype, device="cuda").contiguous(memory_format=torch.channels_last)
    before = out.clone()
    xp, op, code = x.data_ptr(), out.data_ptr(), CODE[dtype]
    calls = (
        ((op, 1, 3, 3, c, code, 0, (xp,), (4,), (4,)), "dad3d_nhwc_resize_sum: bad argument"),
        ((op, 1, 3, 3, c, code, 4, (xp,) * 4, (4,) * 4, (4,) * 4), "dad3d_nhwc_resize_sum: bad argument"),
        ((op, 1, 3, 3, c, 3, 1, (xp,), (4,), (4,)), "dad3d_nhwc_resize_sum: bad argument"),
        ((op, 1, -1, 3, c, code, 1, (xp,), (4,), (4,)), "dad3d_nhwc_resize_sum: bad argument"),
        ((op, 1, 3, 3, c + vec // 2, code, 1, (xp,), (4,), (4,)), f"{c + vec // 2} channels are not a multiple of {vec} (16 bytes)"),
        ((op + 4, 1, 3, 3, c, code, 1, (xp,), (4,), (4,)), "tensors must be 16-byte aligned"),
        ((op, 1, 3, 3, c, code, 1, (xp,), (0,), (4,)), "input 0 is null, empty or not 16-byte aligned"),
        ((op, 1, 3, 3, c, code, 2, (xp, xp), (4, 4), (4, 0)), "input 1 is null, empty or not 16-byte aligned"),
        ((op, 1, 3, 3, c, code, 2, (xp, xp + 4), (4, 4), (4, 4)), "input 1 is null, empty or not 16-byte aligned"),
        ((op, 1, 3, 3, c, code, 2, (xp, None), (4, 4), (4, 4)), "input 1 is null, empty or not 16-byte aligned"),
        ((None, 1, 3, 3, c, code, 1, (xp,), (4,), (4,)), "dad3d_nhwc_resize_sum: null argument"),
    )
    for args, message in calls:
        assert raw_resize_sum(*args) == _lib.E_INVALID, args
        assert message in last_error(), (args, last_error())
    for n, oh, ow in ((0, 3, 3), (1, 0, 3), (1, 3, 0)):
        assert raw_resize_sum(op, n, oh, ow, c, code, 1, (xp,), (4,), (4,)) == _lib.OK
    torch.cuda.synchronize()
    assert torch.equal(as_bytes(out), as_bytes(before))


def test_supported_says_which_tensors_the_kernels_take():
    cl = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device="cuda").contiguous(memory_format=torch.channels_last)
    assert _glue.supported(cl(1, 64, 4, 4)) and _glue.supported(cl(1, 64, 4, 4, dtype=torch.bfloat16), cl(1, 64, 4, 4, dtype=torch.bfloat16))
    assert not _glue.supported(torch.zeros(1, 64, 4, 4, device="cuda"))  # NCHW
    assert not _glue.supported(cl(1, 68, 4, 4, dtype=torch.bfloat16))  # 68 channels: no multiple of 8
    assert _glue.supported(cl(1, 68, 4, 4))  # ... but of fp32's 4
    assert not _glue.supported(cl(1, 64, 4, 4, dtype=torch.bfloat16), cl(1, 64, 4, 4, dtype=torch.float16))  # another dtype
    assert not _glue.supported(cl(1, 64, 4, 4), torch.zeros(1, 64, 4, 4, device="cuda"))  # an NCHW residual
    assert not _glue.supported(cl(1, 64, 4, 4).cpu())
    assert not _glue.supported(cl(1, 64, 4, 4, dtype=torch.float64))
    flat = torch.zeros(1 * 4 * 4 * 64 + 4, device="cuda")
    off = flat[1:1 + 1024].view(1, 4, 4, 64).permute(0, 3, 1, 2)  # channels-last, 4 bytes past a 16-byte boundary
    assert off.is_contiguous(memory_format=torch.channels_last) and off.data_ptr() % 16 == 4
    assert not _glue.supported(off) and not _glue.supported(cl(1, 64, 4, 4), off)
    with pytest.raises(ValueError, match="16-byte aligned"):
        _glue.resize_sum([1.0], [off], (4, 4))


def test_bias_act_raises_on_a_bias_or_residual_that_does_not_fit():
    y = torch.ones(1, 16, 4, 4, device="cuda").contiguous(memory_format=torch.channels_last)
    before = y.clone()
    with pytest.raises(ValueError, match="bias must be a contiguous"):
        _glue.bias_act_(y, torch.ones(16, device="cuda", dtype=torch.float16))
    with pytest.raises(ValueError, match="bias must be a contiguous"):
        _glue.bias_act_(y, torch.ones(12, device="cuda"))
    with pytest.raises(ValueError, match="bias must be a contiguous"):
        _glue.bias_act_(y, torch.ones(32, device="cuda")[::2])
    with pytest.raises(ValueError, match="residual must have the output's shape"):
        _glue.bias_act_(y, torch.ones(16, device="cuda"), torch.ones(1, 16, 4, 2, device="cuda").contiguous(memory_format=torch.channels_last))
    with pytest.raises(ValueError, match="one to three weighted inputs"):
        _glue.resize_sum([], [], (4, 4))
    with pytest.raises(ValueError, match="one to three weighted inputs"):
        _glue.resize_sum([1.0] * 4, [y] * 4, (4, 4))
    torch.cuda.synchronize()
    assert torch.equal(y, before)
