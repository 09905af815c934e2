// From the network's 2-D outputs to landmark points, for gfx950: the peak of every heatmap plane and the readjustment of points to
// the input image, so that nothing between the CNN and the results waits for the host.
//
//   heatmap_argmax    yx[b][c] = (k // H, k % H), k = argmax over the H*W values of plane (b, c)        model/utils.py:44-52 (unravel_index)
//                     of sigmoid(heatmap) (predictor.py:108-112) or of the logits (flame_lightning_model.py:294-297)
//   points_readjust   clip, pad subtraction, division, truncation for a batch                          predictor.py:132-133,147-152
//
// The rule is torch.argmax / np.argmax: the first NaN if there is one, else the first position of the maximum; -0.0 == +0.0.
// Every value becomes a 32-bit key whose unsigned order is that order (NaN on top), and a (key, index) pair is one 64-bit word
// whose maximum is the answer (collectives.hpp, OpArgmax), so the result is independent of the order of combination.
// With `sigmoid` the values compared are torch.sigmoid's in the input's dtype: 1 / (1 + expf(-x)) in float32, rounded to nearest
// even to fp16 / bf16 for those inputs. The sigmoid merges logits (every float32 logit from 16.636066 up is exactly 1.0f), so the
// first saturated position wins, not the largest logit.
//
// Two layouts, each logit read once with the widest aligned load:
//   NCHW          one workgroup per (b, c) plane: a scalar head up to 16-byte alignment, 16-byte vectors, a scalar tail; a block reduction
//   channels-last a workgroup takes all channels of a run of pixels of one image. A load holds V adjacent channels of one pixel, V the
//                 largest power of two that divides C and keeps every pixel row aligned (68 channels: 4). A thread keeps one channel
//                 group and walks pixels, so its V running pairs stay in registers; the pixel slots of a channel meet in LDS and one
//                 wave reduces them. One workgroup per image left the chip idle (measured: DESIGN.md 4.22), so an image of 512 pixels
//                 or more is split over up to 1024 / B workgroups of at least 256 pixels each: yx_out, zeroed first, takes the packed
//                 pairs by a 64-bit atomic maximum (order-free, so still deterministic) and a second tiny pass unpacks them in place.
// NCHW has no atomics: a plane has one owner.
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include "collectives.hpp"
#include "common.hpp"
#include "points_math.hpp"

namespace dad3d {
namespace {

constexpr int kPlaneThreads = 256, kImageThreads = 512;

__device__ __forceinline__ float sigmoid_f32(float x) { return 1.0f / (1.0f + expf(-x)); }  // as in train_objective.hip

struct F32 {
    static constexpr int ES = 4;
    __device__ static float value(unsigned raw, bool sig) {
        const float x = __uint_as_float(raw);
        return sig ? sigmoid_f32(x) : x;
    }
};
struct F16 {
    static constexpr int ES = 2;
    __device__ static float value(unsigned raw, bool sig) {
        const float x = __half2float(__builtin_bit_cast(__half, (unsigned short)raw));
        return sig ? __half2float(__float2half(sigmoid_f32(x))) : x;  // round to nearest even, compared in fp16
    }
};
struct BF16 {
    static constexpr int ES = 2;
    __device__ static float value(unsigned raw, bool sig) {
        const float x = __uint_as_float(raw << 16);
        return sig ? __bfloat162float(__float2bfloat16(sigmoid_f32(x))) : x;
    }
};
struct U8 {
    static constexpr int ES = 1;
    __device__ static float value(unsigned raw, bool) { return (float)raw; }
};

// unsigned order of the keys == argmax's order of the values: -inf < .. < -0 == +0 < .. < +inf < NaN; every key is >= 1
__device__ __forceinline__ unsigned key_of(float x) {
    if (x != x) return 0xffffffffu;
    const unsigned b = x == 0.0f ? 0u : __float_as_uint(x);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}

// BYTES (1, 2, 4, 8 or 16) at an address aligned to BYTES
template <int BYTES>
__device__ __forceinline__ void load_words(const unsigned char* p, unsigned (&w)[4]) {
    w[0] = w[1] = w[2] = w[3] = 0;
    if (BYTES == 1) w[0] = *p;
    else if (BYTES == 2) w[0] = *reinterpret_cast<const unsigned short*>(p);
    else if (BYTES == 4) w[0] = *reinterpret_cast<const unsigned*>(p);
    else if (BYTES == 8) {
        const uint2 q = *reinterpret_cast<const uint2*>(p);
        w[0] = q.x, w[1] = q.y;
    } else {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        w[0] = q.x, w[1] = q.y, w[2] = q.z, w[3] = q.w;
    }
}

// element j (a constant after unrolling) of the loaded words
template <int ES>
__device__ __forceinline__ unsigned element(const unsigned (&w)[4], int j) {
    if (ES == 4) return w[j];
    if (ES == 2) return (w[j >> 1] >> (16 * (j & 1))) & 0xffffu;
    return (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
}

template <int ES>
__device__ __forceinline__ unsigned scalar_at(const unsigned char* base, size_t i) {
    unsigned w[4];
    load_words<ES>(base + i * ES, w);
    return w[0];
}

__device__ __forceinline__ void write_peak(const HeatmapArgmaxArgs& a, size_t plane, unsigned k, float value) {
    a.yx[2 * plane] = (int)(k / (unsigned)a.h);  // the reference's own unravel: // H and % H, also where H != W
    a.yx[2 * plane + 1] = (int)(k % (unsigned)a.h);
    if (a.peak) a.peak[plane] = value;
}

template <typename T>
__global__ __launch_bounds__(kPlaneThreads) void heatmap_argmax_nchw_kernel(HeatmapArgmaxArgs a) {
    constexpr int ES = T::ES, N = 16 / ES;
    __shared__ unsigned long long red[kPlaneThreads / 64];
    const int hw = a.h * a.w, t = threadIdx.x;
    const bool sig = a.sigmoid != 0;
    const size_t plane = blockIdx.x;
    const unsigned char* base = static_cast<const unsigned char*>(a.heatmap) + plane * (size_t)hw * ES;
    const int head = min(hw, (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(base) & 15u)) & 15u) / ES));
    const int nvec = (hw - head) / N, tail = head + nvec * N;
    // a thread meets its indices in ascending order, so `>` keeps the first position of its maximum
    unsigned best_key = 0, best_at = 0;
    if (t < head) best_key = key_of(T::value(scalar_at<ES>(base, t), sig)), best_at = t;
    for (int i = t; i < nvec; i += kPlaneThreads) {
        unsigned w[4];
        load_words<16>(base + ((size_t)head + (size_t)i * N) * ES, w);
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const unsigned key = key_of(T::value(element<ES>(w, j), sig));
            if (key > best_key) best_key = key, best_at = head + i * N + j;
        }
    }
    if (tail + t < hw) {
        const unsigned key = key_of(T::value(scalar_at<ES>(base, tail + t), sig));
        if (key > best_key) best_key = key, best_at = tail + t;
    }
    const unsigned long long top = block_reduce<OpArgmax, kPlaneThreads / 64>(argmax_pack(best_key, best_at), red);
    if (t == 0) {
        const unsigned k = argmax_index(top);
        write_peak(a, plane, k, T::value(scalar_at<ES>(base, k), sig));
    }
}

// the pixels [first, end) of image blockIdx.x for workgroup blockIdx.y of a.n_split
template <typename T, int V>
__global__ __launch_bounds__(kImageThreads) void heatmap_argmax_nhwc_kernel(HeatmapArgmaxArgs a) {
    constexpr int ES = T::ES, WAVES = kImageThreads / 64;
    __shared__ unsigned long long part[kImageThreads * V];  // [pixel slot][channel of this trip]
    const int hw = a.h * a.w, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const bool sig = a.sigmoid != 0;
    const int groups = a.channels / V;                                    // loads per pixel
    const int gt = min(groups, kImageThreads), slots = kImageThreads / gt;  // channel groups per trip, pixels in flight
    const int gl = t % gt, slot = t / gt;
    const unsigned char* img = static_cast<const unsigned char*>(a.heatmap) + (size_t)blockIdx.x * hw * a.channels * ES;
    const int run = (hw + a.n_split - 1) / a.n_split, first = min(hw, (int)blockIdx.y * run), end = min(hw, first + run);
    for (int g0 = 0; g0 < groups; g0 += gt) {  // one trip unless C / V > 512
        const int g = g0 + gl;
        unsigned best_key[V], best_at[V];
#pragma unroll
        for (int j = 0; j < V; ++j) best_key[j] = 0, best_at[j] = 0;
        if (slot < slots && g < groups) {
            const unsigned char* col = img + (size_t)g * (V * ES);
            const size_t row = (size_t)groups * (V * ES);  // bytes per pixel
            auto update = [&](const unsigned (&w)[4], int p) {
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const unsigned key = key_of(T::value(element<ES>(w, j), sig));
                    if (key > best_key[j]) best_key[j] = key, best_at[j] = p;  // p ascends: the first position stays
                }
            };
            int p = first + slot;
            for (; p + 3 * slots < end; p += 4 * slots) {  // four loads in flight
                unsigned w0[4], w1[4], w2[4], w3[4];
                load_words<V * ES>(col + (size_t)p * row, w0);
                load_words<V * ES>(col + (size_t)(p + slots) * row, w1);
                load_words<V * ES>(col + (size_t)(p + 2 * slots) * row, w2);
                load_words<V * ES>(col + (size_t)(p + 3 * slots) * row, w3);
                update(w0, p), update(w1, p + slots), update(w2, p + 2 * slots), update(w3, p + 3 * slots);
            }
            for (; p < end; p += slots) {
                unsigned w[4];
                load_words<V * ES>(col + (size_t)p * row, w);
                update(w, p);
            }
        }
#pragma unroll
        for (int j = 0; j < V; ++j) part[t * V + j] = argmax_pack(best_key[j], best_at[j]);  // t == slot * gt + gl
        __syncthreads();
        const int n_ch = min(gt, groups - g0) * V;
        for (int lc = wave; lc < n_ch; lc += WAVES) {  // a wave per channel: its lanes take the pixel slots
            unsigned long long top = 0;
            for (int s = lane; s < slots; s += 64) top = OpArgmax::of(top, part[(size_t)s * gt * V + lc]);
            top = wave_reduce<OpArgmax>(top);
            if (lane == 0) {
                const int ch = g0 * V + lc;
                const size_t plane = (size_t)blockIdx.x * a.channels + ch;
                if (a.n_split > 1) {  // a workgroup without pixels brings the pair (0, 0), below every value's
                    atomicMax(reinterpret_cast<unsigned long long*>(a.yx) + plane, top);
                } else {
                    const unsigned k = argmax_index(top);
                    write_peak(a, plane, k, T::value(scalar_at<ES>(img, (size_t)k * a.channels + ch), sig));
                }
            }
        }
        __syncthreads();  // the next trip writes `part` again
    }
}

// the second pass of a split channels-last launch: thread = one plane, its packed pair in yx unpacked in place
template <typename T>
__global__ __launch_bounds__(256) void heatmap_argmax_unpack_kernel(HeatmapArgmaxArgs a) {
    const size_t plane = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (plane >= (size_t)a.batch * a.channels) return;
    const unsigned k = argmax_index(reinterpret_cast<const unsigned long long*>(a.yx)[plane]);
    const size_t img = plane / a.channels, ch = plane % a.channels;
    const unsigned char* base = static_cast<const unsigned char*>(a.heatmap) + img * (size_t)(a.h * a.w) * a.channels * T::ES;
    write_peak(a, plane, k, T::value(scalar_at<T::ES>(base, (size_t)k * a.channels + ch), a.sigmoid != 0));
}

// predictor.py:132-133,147-152 for one coordinate: thread = one output int
__global__ __launch_bounds__(256) void points_readjust_kernel(PointsReadjustArgs a, int total) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int xy = i & 1, b = i / (2 * a.n_points);
    // (row, col) from the argmax is flipped to (x, y)
    const float s = a.src_kind == 0 ? static_cast<const float*>(a.src)[i] : (float)static_cast<const int32_t*>(a.src)[i ^ 1];
    double pad = xy == 0 ? a.pad_left : a.pad_top, scale = a.scale;  // the pads are integers held in float64
    if (a.geometry) pad = a.geometry[3 * b + xy], scale = a.geometry[3 * b + 2];
    a.points[i] = readjusted_coordinate(s, a.mul, a.limit, pad, scale);
}

template <typename T>
dad3d_status argmax_t(HeatmapArgmaxArgs a, hipStream_t s) {
    a.n_split = 1;
    if (a.layout == DAD3D_LAYOUT_NCHW) {
        hipLaunchKernelGGL(heatmap_argmax_nchw_kernel<T>, dim3((unsigned)((size_t)a.batch * a.channels)), dim3(kPlaneThreads), 0, s, a);
    } else {
        int v = 16 / T::ES;  // the widest load that divides C and keeps every pixel row aligned
        while (v > 1 && (a.channels % v != 0 || (reinterpret_cast<uintptr_t>(a.heatmap) % (size_t)(v * T::ES)) != 0)) v >>= 1;
        // enough workgroups for the chip (1024 of 512 threads), none with fewer than 256 pixels; the packed pairs need yx 8-byte aligned
        const size_t planes = (size_t)a.batch * a.channels;
        if (reinterpret_cast<uintptr_t>(a.yx) % 8 == 0) a.n_split = std::max(1, std::min((1024 + a.batch - 1) / a.batch, a.h * a.w / 256));
        if (a.n_split > 1) DAD3D_HIP_TRY(hipMemsetAsync(a.yx, 0, planes * 8, s));
        const dim3 grid(a.batch, a.n_split), block(kImageThreads);
        switch (v * T::ES) {  // bytes per load
            case 16: hipLaunchKernelGGL((heatmap_argmax_nhwc_kernel<T, 16 / T::ES>), grid, block, 0, s, a); break;
            case 8: hipLaunchKernelGGL((heatmap_argmax_nhwc_kernel<T, 8 / T::ES>), grid, block, 0, s, a); break;
            case 4: hipLaunchKernelGGL((heatmap_argmax_nhwc_kernel<T, 4 / T::ES>), grid, block, 0, s, a); break;
            case 2: hipLaunchKernelGGL((heatmap_argmax_nhwc_kernel<T, (T::ES <= 2 ? 2 / T::ES : 1)>), grid, block, 0, s, a); break;
            default: hipLaunchKernelGGL((heatmap_argmax_nhwc_kernel<T, 1>), grid, block, 0, s, a); break;
        }
        if (a.n_split > 1) {
            DAD3D_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(heatmap_argmax_unpack_kernel<T>, dim3((unsigned)((planes + 255) / 256)), dim3(256), 0, s, a);
        }
    }
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

}  // namespace

dad3d_status launch_heatmap_argmax(const HeatmapArgmaxArgs& a, hipStream_t s) {
    switch (a.dtype) {
        case DAD3D_DTYPE_F32: return argmax_t<F32>(a, s);
        case DAD3D_DTYPE_F16: return argmax_t<F16>(a, s);
        case DAD3D_DTYPE_BF16: return argmax_t<BF16>(a, s);
        case DAD3D_HEATMAP_DTYPE_U8: return argmax_t<U8>(a, s);
    }
    set_error("heatmap_argmax: unknown dtype %d", a.dtype);
    return DAD3D_E_INVALID;
}

dad3d_status launch_points_readjust(const PointsReadjustArgs& a, hipStream_t s) {
    const int total = a.batch * a.n_points * 2;
    hipLaunchKernelGGL(points_readjust_kernel, dim3((total + 255) / 256), dim3(256), 0, s, a, total);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

}  // namespace dad3d
