// The tail of the DAD-3DNet forward for gfx950: what the framework ran as some thirty launches between the BiFPN and the params rows
// (model_training/model/flame_regression.py:28-43, 45-59, 96-100). The convolutions stay on PyTorch-ROCm.
//
//   nhwc_fusion_concat   out = [ x | sigmoid(bilinear_ac(heat)) | level ]      the fusion layer's input       flame_regression.py:36-41
//   nhwc_bias_mul        y = (y + bias[c]) * x, in place                        the fusion layer's output      flame_regression.py:42
//   regression_heads     avg-pool -> Linear -> ReLU -> Linear -> activation     the three RegressionHeads      flame_regression.py:45-59, 96-100
//
// Built with -ffp-contract=off: the interpolation, the add-then-multiply and the activations are stated operation by operation
// (include/dad3d.h); only the heads' dot products fuse, and they say fmaf().
//
// fusion_concat   a thread moves one 8-byte piece of an output pixel (the 68 heat-map channels leave the segment seams and the heat
//                 map's pixel stride 8-byte aligned, not 16). A piece of x or level is a byte copy; a piece of the middle segment
//                 reads the same piece of four heat-map pixels. bytes = read x + level + (<= 4x) heat, write out.
// bias_mul        the sibling of nhwc_bias_act_kernel (cnn_glue.hip): 16-byte vectors, grid-stride. bytes = read y + x, write y.
// heads           three launches, no atomics:
//   1. pool       a workgroup takes 32 16-byte channel vectors of one image; its 8 position slices meet in LDS in a fixed order.
//                 Every byte of `top` is read once. pooled = sum / (float)(h*w) in fp32.
//   2, 3. layer   one kernel for both Linear layers. A wave owns R rows of a head's weight matrix and streams them once in
//                 16-byte loads; the fp32 input rows (pooled, resp. hidden) of 16 images at a time are staged through LDS, shared by the
//                 workgroup's four waves, so a weight vector in registers meets 16 images. R = 1 up to 8 images -- W1's 1536 rows
//                 are then 384 workgroups, the whole chip, for the 6.3 MB stream that is all of the work at batch 1 -- and R = 4
//                 beyond, where the staged inputs are the larger traffic. Every further batch tile re-reads the wave's own rows
//                 (R x K x 2 bytes <= 16 KB), which the L2 still holds: HBM gives each weight byte once per call.
//                 A wave's 64 partial sums meet in a butterfly (collectives.hpp): a fixed order, so the bits repeat.
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include "collectives.hpp"
#include "common.hpp"

namespace dad3d {
namespace {

template <typename T>
struct Elem;  // raw element <-> fp32
template <>
struct Elem<float> {
    typedef unsigned raw;
    __device__ static float widen(unsigned r) { return __uint_as_float(r); }
    __device__ static unsigned narrow(float v) { return __float_as_uint(v); }
};
template <>
struct Elem<__hip_bfloat16> {
    typedef unsigned short raw;
    __device__ static float widen(unsigned short r) { return __uint_as_float((unsigned)r << 16); }
    __device__ static unsigned short narrow(float v) { return __builtin_bit_cast(unsigned short, __float2bfloat16(v)); }  // nearest even
};
template <>
struct Elem<__half> {
    typedef unsigned short raw;
    __device__ static float widen(unsigned short r) { return __half2float(__builtin_bit_cast(__half, r)); }
    __device__ static unsigned short narrow(float v) { return __builtin_bit_cast(unsigned short, __float2half(v)); }
};

// 8 bytes of T <-> fp32 lanes
template <typename T>
struct Vec8 {
    typedef typename Elem<T>::raw raw;
    static constexpr int N = 8 / sizeof(raw);
    __device__ static void load(const void* p, float (&v)[N]) {
        const uint2 q = *static_cast<const uint2*>(p);
        raw r[N];
        __builtin_memcpy(r, &q, 8);
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = Elem<T>::widen(r[i]);
    }
    __device__ static void store(void* p, const float (&v)[N]) {
        raw r[N];
#pragma unroll
        for (int i = 0; i < N; ++i) r[i] = Elem<T>::narrow(v[i]);
        uint2 q;
        __builtin_memcpy(&q, r, 8);
        *static_cast<uint2*>(p) = q;
    }
};

// 16 bytes of T -> fp32 lanes, and back
template <typename T>
struct Vec16 {
    typedef typename Elem<T>::raw raw;
    static constexpr int N = 16 / sizeof(raw);
    __device__ static void load(const void* p, float (&v)[N]) {
        const uint4 q = *static_cast<const uint4*>(p);
        raw r[N];
        __builtin_memcpy(r, &q, 16);
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = Elem<T>::widen(r[i]);
    }
    __device__ static void store(void* p, const float (&v)[N]) {
        raw r[N];
#pragma unroll
        for (int i = 0; i < N; ++i) r[i] = Elem<T>::narrow(v[i]);
        uint4 q;
        __builtin_memcpy(&q, r, 16);
        *static_cast<uint4*>(p) = q;
    }
};

__device__ __forceinline__ float sigmoid_f32(float x) { return 1.0f / (1.0f + expf(-x)); }  // as in heatmap_points.hip

inline int grid_for(size_t work_items, int threads) {
    const size_t blocks = (work_items + threads - 1) / threads;
    return (int)std::min<size_t>(std::max<size_t>(blocks, 1), 256 * 16);  // grid-stride beyond 16 blocks per CU
}

// ---- 1. the fusion layer's input ------------------------------------------------------------------------------------------------------

struct FusionConcatArgs {
    void* out;
    const void *x, *heat, *level;
    int n, oh, ow, hh, hw;
    int px, ph, pl;  // 8-byte pieces of a pixel of x, heat, level
    float sh, sw;    // (float)(in - 1) / (float)(out - 1), or 0 for one output row / column
};

// F.interpolate(mode="bilinear", align_corners=True) as the device evaluates it: src = scale * dst, i0 = (int)src, the neighbour
// one further unless i0 is the last, l1 = src - i0, l0 = 1 - l1
__device__ __forceinline__ void bilinear_taps(float scale, int dst, int n_in, int& i0, int& i1, float& l0, float& l1) {
    const float src = scale * (float)dst;
    i0 = min((int)src, n_in - 1);  // (int)src <= n_in - 1 for every scale the launcher derives; the min keeps any other in bounds
    i1 = i0 + (i0 < n_in - 1);
    l1 = src - (float)i0;
    l0 = 1.0f - l1;
}

template <typename T>
__global__ void nhwc_fusion_concat_kernel(FusionConcatArgs a) {
    constexpr int N = Vec8<T>::N;
    const int pieces = a.px + a.ph + a.pl;
    const size_t total = (size_t)a.n * a.oh * a.ow * pieces;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int piece = (int)(i % pieces);
        const size_t pixel = i / pieces;
        uint2* dst = static_cast<uint2*>(a.out) + i;
        if (piece < a.px) {
            *dst = static_cast<const uint2*>(a.x)[pixel * a.px + piece];
        } else if (piece >= a.px + a.ph) {
            *dst = static_cast<const uint2*>(a.level)[pixel * a.pl + (piece - a.px - a.ph)];
        } else {
            const int ox = (int)(pixel % a.ow);
            const size_t q = pixel / a.ow;
            const int oy = (int)(q % a.oh);
            const size_t img = q / a.oh;
            int y0, y1, x0, x1;
            float lh0, lh1, lw0, lw1;
            bilinear_taps(a.sh, oy, a.hh, y0, y1, lh0, lh1);
            bilinear_taps(a.sw, ox, a.hw, x0, x1, lw0, lw1);
            const uint2* h = static_cast<const uint2*>(a.heat) + (size_t)(piece - a.px);
            const size_t r0 = (img * a.hh + y0) * a.hw, r1 = (img * a.hh + y1) * a.hw;
            float ta[N], tb[N], tc[N], td[N], v[N];
            Vec8<T>::load(h + (r0 + x0) * a.ph, ta);
            Vec8<T>::load(h + (r0 + x1) * a.ph, tb);
            Vec8<T>::load(h + (r1 + x0) * a.ph, tc);
            Vec8<T>::load(h + (r1 + x1) * a.ph, td);
#pragma unroll
            for (int k = 0; k < N; ++k) v[k] = sigmoid_f32(lh0 * (lw0 * ta[k] + lw1 * tb[k]) + lh1 * (lw0 * tc[k] + lw1 * td[k]));
            Vec8<T>::store(dst, v);
        }
    }
}

template <typename T>
dad3d_status fusion_concat_t(const FusionConcatArgs& a, hipStream_t s) {
    const size_t total = (size_t)a.n * a.oh * a.ow * (a.px + a.ph + a.pl);
    const int threads = 256;
    hipLaunchKernelGGL((nhwc_fusion_concat_kernel<T>), dim3(grid_for(total, threads)), dim3(threads), 0, s, a);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

// ---- 2. the fusion layer's output -----------------------------------------------------------------------------------------------------

// y[p][c] = (y[p][c] + bias[c]) * x[p][c]: two rounded fp32 operations, one rounding at the store
template <typename T>
__global__ void nhwc_bias_mul_kernel(T* y, const T* bias, const T* x, size_t n_vec, int cvec) {
    constexpr int N = Vec16<T>::N;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_vec; i += (size_t)gridDim.x * blockDim.x) {
        float a[N], b[N], m[N];
        Vec16<T>::load(y + i * N, a);
        Vec16<T>::load(bias + (size_t)(i % (size_t)cvec) * N, b);
        Vec16<T>::load(x + i * N, m);
#pragma unroll
        for (int k = 0; k < N; ++k) a[k] = (a[k] + b[k]) * m[k];
        Vec16<T>::store(y + i * N, a);
    }
}

template <typename T>
dad3d_status bias_mul_t(void* y, const void* bias, const void* x, size_t n_pixels, int channels, hipStream_t s) {
    constexpr int N = Vec16<T>::N;
    const int cvec = channels / N, threads = 256;
    const size_t n_vec = n_pixels * (size_t)cvec;
    hipLaunchKernelGGL((nhwc_bias_mul_kernel<T>), dim3(grid_for(n_vec, threads)), dim3(threads), 0, s, static_cast<T*>(y),
                       static_cast<const T*>(bias), static_cast<const T*>(x), n_vec, cvec);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

// ---- 3. the regression heads ----------------------------------------------------------------------------------------------------------

constexpr int kPoolVecs = 32, kPoolSlices = 8;         // a pool workgroup: 32 channel vectors x 8 position slices
constexpr int kLayerWaves = 4, kLayerBatchTile = 16;  // a layer workgroup: 4 waves, 16 images per staged tile

// pooled[b][c] = (sum over the hw positions of top[b][p][c]) / (float)hw
template <typename T>
__global__ __launch_bounds__(kPoolVecs* kPoolSlices) void heads_pool_kernel(const T* top, float* pooled, int hw, int cvec) {
    constexpr int N = Vec16<T>::N;
    __shared__ float part[kPoolSlices][N][kPoolVecs];
    const int lane = threadIdx.x % kPoolVecs, slice = threadIdx.x / kPoolVecs;
    const int cv = blockIdx.x * kPoolVecs + lane, b = blockIdx.y;
    float acc[N];
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.0f;
    if (cv < cvec) {
        const T* src = top + ((size_t)b * hw * cvec + cv) * N;
        for (int p = slice; p < hw; p += kPoolSlices) {
            float v[N];
            Vec16<T>::load(src + (size_t)p * cvec * N, v);
#pragma unroll
            for (int k = 0; k < N; ++k) acc[k] += v[k];
        }
    }
#pragma unroll
    for (int k = 0; k < N; ++k) part[slice][k][lane] = acc[k];
    __syncthreads();
    if (slice == 0 && cv < cvec) {
        float out[N];
#pragma unroll
        for (int k = 0; k < N; ++k) {
            float sum = part[0][k][lane];
#pragma unroll
            for (int j = 1; j < kPoolSlices; ++j) sum += part[j][k][lane];
            out[k] = sum / (float)hw;
        }
        float* dst = pooled + ((size_t)b * cvec + cv) * N;
#pragma unroll
        for (int k = 0; k < N; k += 4) *reinterpret_cast<float4*>(dst + k) = make_float4(out[k], out[k + 1], out[k + 2], out[k + 3]);
    }
}

struct LayerHead {
    const void *w, *bias;  // [rows, k] row-major and [rows], the serving dtype
    const float* in;       // the head's first input column of image 0
    float* out;            // the head's first output column of image 0
    long long out_stride;  // floats between two images' output rows
    int rows, k, act;
    float limit;
    int first_block;       // this head's first workgroup
};
struct LayerArgs {
    LayerHead head[DAD3D_HEADS_MAX];
    int n_heads, batch;
    long long in_stride;  // floats between two images' input rows
};

__device__ __forceinline__ float activate(float v, int act, float limit) {
    if (act == DAD3D_HEAD_ACT_RELU) return __builtin_elementwise_maximum(v, 0.0f);  // IEEE maximum: a NaN stays a NaN, as in F.relu
    if (act == DAD3D_HEAD_ACT_TANH) return limit * tanhf(v);
    return v;
}

// out[b][j] = act(in[b][0:k] . w[j][0:k] + bias[j]) for the rows j of one head; wave = R rows, workgroup = 4 waves and one staged input tile
template <typename T, int R>
__global__ __launch_bounds__(kLayerWaves * 64) void heads_layer_kernel(LayerArgs a) {
    constexpr int N = Vec16<T>::N, Q = N / 4;  // a lane's elements of a chunk, as float4s
    constexpr int BT = kLayerBatchTile, CHUNK = 64 * N;
    __shared__ float4 tile[BT][Q][64];  // tile[b][q][lane] = input elements lane * N + 4 q .. + 3 of the chunk
    int hd = 0;
#pragma unroll
    for (int j = 1; j < DAD3D_HEADS_MAX; ++j)
        if (j < a.n_heads && (int)blockIdx.x >= a.head[j].first_block) hd = j;
    const LayerHead h = a.head[hd];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row0 = (((int)blockIdx.x - h.first_block) * kLayerWaves + wave) * R;
    const typename Elem<T>::raw* w = static_cast<const typename Elem<T>::raw*>(h.w);

    for (int b0 = 0; b0 < a.batch; b0 += BT) {
        float acc[R][BT];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int b = 0; b < BT; ++b) acc[r][b] = 0.0f;
        for (int k0 = 0; k0 < h.k; k0 += CHUNK) {
            const int k = k0 + lane * N;  // h.k is a multiple of N: a lane's vector is inside the row or beyond it
            float wv[R][N];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (row0 + r < h.rows && k < h.k) {
                    Vec16<T>::load(w + (size_t)(row0 + r) * h.k + k, wv[r]);
                } else {
#pragma unroll
                    for (int i = 0; i < N; ++i) wv[r][i] = 0.0f;
                }
            }
            __syncthreads();  // the previous tile has been read
            for (int i = threadIdx.x; i < BT * Q * 64; i += kLayerWaves * 64) {
                const int b = i / (Q * 64), f = i % (Q * 64);  // f: float4 number within the chunk; lane f / Q, quarter f % Q
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (b0 + b < a.batch && k0 + f * 4 < h.k) v = *reinterpret_cast<const float4*>(h.in + (size_t)(b0 + b) * a.in_stride + k0 + f * 4);
                tile[b][f % Q][f / Q] = v;
            }
            __syncthreads();
#pragma unroll
            for (int b = 0; b < BT; ++b) {
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    const float4 p = tile[b][q][lane];
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        acc[r][b] = fmaf(wv[r][4 * q], p.x, acc[r][b]);
                        acc[r][b] = fmaf(wv[r][4 * q + 1], p.y, acc[r][b]);
                        acc[r][b] = fmaf(wv[r][4 * q + 2], p.z, acc[r][b]);
                        acc[r][b] = fmaf(wv[r][4 * q + 3], p.w, acc[r][b]);
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int row = row0 + r;
            const float bias = row < h.rows ? Elem<T>::widen(static_cast<const typename Elem<T>::raw*>(h.bias)[row]) : 0.0f;
            float mine = 0.0f;  // lane b keeps image b0 + b's sum
#pragma unroll
            for (int b = 0; b < BT; ++b) {
                const float sum = wave_sum(acc[r][b]);
                mine = lane == b ? sum : mine;
            }
            if (lane < BT && row < h.rows && b0 + lane < a.batch) h.out[(size_t)(b0 + lane) * h.out_stride + row] = activate(mine + bias, h.act, h.limit);
        }
    }
}

template <typename T>
dad3d_status heads_t(const RegressionHeadsArgs& a, hipStream_t s) {
    constexpr int N = Vec16<T>::N;
    const int cvec = a.channels / N;
    hipLaunchKernelGGL((heads_pool_kernel<T>), dim3((cvec + kPoolVecs - 1) / kPoolVecs, a.batch), dim3(kPoolVecs * kPoolSlices), 0, s,
                       static_cast<const T*>(a.top), a.pooled, a.hw, cvec);
    DAD3D_HIP_TRY(hipGetLastError());
    const int rows_per_wave = a.batch <= 8 ? 1 : 4, rows_per_block = rows_per_wave * kLayerWaves;
    long long hidden_total = 0;
    for (int j = 0; j < a.n_heads; ++j) hidden_total += a.head[j].hidden;
    for (int layer = 0; layer < 2; ++layer) {
        LayerArgs l{};
        l.n_heads = a.n_heads, l.batch = a.batch, l.in_stride = layer == 0 ? a.channels : hidden_total;
        int blocks = 0;
        long long column = 0;
        for (int j = 0; j < a.n_heads; ++j) {
            const dad3d_head_desc& d = a.head[j];
            LayerHead& h = l.head[j];
            if (layer == 0) {
                h.w = d.w1, h.bias = d.b1, h.in = a.pooled, h.out = a.hidden + column, h.out_stride = hidden_total;
                h.rows = d.hidden, h.k = a.channels, h.act = DAD3D_HEAD_ACT_RELU, h.limit = 0.0f;
            } else {
                h.w = d.w2, h.bias = d.b2, h.in = a.hidden + column, h.out = d.dst + d.dst_col_offset, h.out_stride = d.dst_row_stride;
                h.rows = d.out_dim, h.k = d.hidden, h.act = d.act, h.limit = d.limit;
            }
            h.first_block = blocks;
            blocks += (h.rows + rows_per_block - 1) / rows_per_block;
            column += d.hidden;
        }
        if (rows_per_wave == 1) hipLaunchKernelGGL((heads_layer_kernel<T, 1>), dim3(blocks), dim3(kLayerWaves * 64), 0, s, l);
        else hipLaunchKernelGGL((heads_layer_kernel<T, 4>), dim3(blocks), dim3(kLayerWaves * 64), 0, s, l);
        DAD3D_HIP_TRY(hipGetLastError());
    }
    return DAD3D_OK;
}

}  // namespace

dad3d_status launch_nhwc_fusion_concat(void* out, const void* x, const void* heat, const void* level, int n, int oh, int ow, int hh, int hw,
                                       int cx, int ch, int cl, int dtype, hipStream_t s) {
    const int per_piece = dtype == DAD3D_DTYPE_F32 ? 2 : 4;
    FusionConcatArgs a{out, x, heat, level, n, oh, ow, hh, hw, cx / per_piece, ch / per_piece, cl / per_piece,
                       oh > 1 ? (float)(hh - 1) / (float)(oh - 1) : 0.0f, ow > 1 ? (float)(hw - 1) / (float)(ow - 1) : 0.0f};
    switch (dtype) {
        case DAD3D_DTYPE_F32: return fusion_concat_t<float>(a, s);
        case DAD3D_DTYPE_F16: return fusion_concat_t<__half>(a, s);
        case DAD3D_DTYPE_BF16: return fusion_concat_t<__hip_bfloat16>(a, s);
    }
    set_error("nhwc_fusion_concat: unknown dtype %d", dtype);
    return DAD3D_E_INVALID;
}

dad3d_status launch_nhwc_bias_mul(void* y, const void* bias, const void* x, size_t n_pixels, int channels, int dtype, hipStream_t s) {
    switch (dtype) {
        case DAD3D_DTYPE_F32: return bias_mul_t<float>(y, bias, x, n_pixels, channels, s);
        case DAD3D_DTYPE_F16: return bias_mul_t<__half>(y, bias, x, n_pixels, channels, s);
        case DAD3D_DTYPE_BF16: return bias_mul_t<__hip_bfloat16>(y, bias, x, n_pixels, channels, s);
    }
    set_error("nhwc_bias_mul: unknown dtype %d", dtype);
    return DAD3D_E_INVALID;
}

dad3d_status launch_regression_heads(const RegressionHeadsArgs& a, hipStream_t s) {
    switch (a.dtype) {
        case DAD3D_DTYPE_F32: return heads_t<float>(a, s);
        case DAD3D_DTYPE_F16: return heads_t<__half>(a, s);
        case DAD3D_DTYPE_BF16: return heads_t<__hip_bfloat16>(a, s);
    }
    set_error("regression_heads: unknown dtype %d", a.dtype);
    return DAD3D_E_INVALID;
}

}  // namespace dad3d
