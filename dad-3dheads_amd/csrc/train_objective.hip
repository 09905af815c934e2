// The rest of the reference's training objective for gfx950 (MI355X): the heatmap target, the heatmap IoU loss, the
// landmark loss with visibility and the keypoint metrics of a training step.
//
//   heatmap_encode_kernel  HeatmapCoder.__call__ (model_training/data/coder.py:17-24, draw_gaussian data/utils.py:48-71) for a
//                          batch: every channel holds at most one stamp, so an element is table[dy][dx] inside the clipped
//                          window of its channel's centre and 0 elsewhere. The (2r+1)^2 table is built on the host with the
//                          reference's own expressions in the requested form (float32 / uint8(255 * h) / uint8 / 255), so the
//                          kernel only places bytes. One lane writes 16 bytes of the flat output.
//   iou_terms_kernel       IoULoss.iou_metric (losses/keypoint_losses.py:11-23) / soft_iou (metrics/iou.py:15-31): one 256-thread
//                          workgroup per channel; sum(t s), sum(t^2), sum(s^2) in float64 (fp32 products are exact there)
//   iou_finish_kernel      the mean over channels in index order (one workgroup): loss = 1 - mean, plus the metric's running sums
//   iou_grad_kernel        dL/dx = -g / (B C) (t D - N (2 s - t)) / D^2 s (1 - s) with the saved sums, g read from the device
//   visibility_loss_kernel LandmarksLossWVisibility (losses/landmarks_loss_w_visibility.py:17-26): criterion(pred * pp, target * tp),
//                          mean over B N 2, value and dL/dpred, one 1024-thread workgroup in a fixed order
//   keypoint_err_kernel    metrics/keypoints.py:19-53: per item mean_n |p_n - q_n|_2 and the norm sqrt(w h) | 2.0, float64
//   keypoint_finish_kernel NME = mean(err / norm) and count(err < thr norm) / B per threshold, in item order
// No float atomics anywhere: every sum runs in a fixed order, so two runs give the same bits. Built with -ffp-contract=off.
#include "common.hpp"

namespace dad3d {
namespace {

constexpr int kObjThreads = 256;
constexpr int kObjWaves = kObjThreads / 64;

// ---- heatmap encode -------------------------------------------------------------------------------------------------
// numpy's float32 floor_divide (npy_floor_dividef -> npy_divmodf): fmod first, then the quotient of the exact difference
__device__ __forceinline__ float npy_floor_divide_f32(float a, float b) {
    if (b == 0.0f) return a / b;
    float mod = fmodf(a, b);
    float div = (a - mod) / b;
    if (mod != 0.0f) {
        if ((b < 0.0f) != (mod < 0.0f)) div -= 1.0f;
    }
    float floordiv;
    if (div != 0.0f) {
        floordiv = floorf(div);
        if (div - floordiv > 0.5f) floordiv += 1.0f;
    } else {
        floordiv = copysignf(0.0f, a / b);
    }
    return floordiv;
}

struct Stamp {
    int cx, cy;  // int(point // stride) once the window is known to be non-empty
    bool on;
};

__device__ __forceinline__ Stamp channel_stamp(const HeatmapEncodeArgs& a, size_t ch, bool count) {
    Stamp st{0, 0, false};
    if (!a.presence[ch]) return st;
    const float fx = npy_floor_divide_f32(a.keypoints[2 * ch], a.stride);
    const float fy = npy_floor_divide_f32(a.keypoints[2 * ch + 1], a.stride);
    if (!isfinite(fx) || !isfinite(fy)) {  // int(nan) raises in the reference: left zero here, counted
        if (count && a.invalid) atomicAdd(a.invalid, 1);
        return st;
    }
    // compare in float before converting: a huge finite centre has no window (the reference's slices are empty)
    const float lo = -(float)a.radius, hi = (float)(a.size + a.radius);
    if (!(fx >= lo && fx < hi && fy >= lo && fy < hi)) return st;
    st.cx = (int)fx, st.cy = (int)fy, st.on = true;
    return st;
}

template <typename T>
__device__ __forceinline__ T stamp_value(const HeatmapEncodeArgs& a, const Stamp& st, int x, int y) {
    if (!st.on) return T(0);
    const int dx = x - st.cx + a.radius, dy = y - st.cy + a.radius, d = 2 * a.radius + 1;
    if (dx < 0 || dx >= d || dy < 0 || dy >= d) return T(0);
    return static_cast<const T*>(a.table)[dy * d + dx];
}

template <typename T>
__global__ __launch_bounds__(kObjThreads) void heatmap_encode_kernel(HeatmapEncodeArgs a) {
    constexpr int kPer = 16 / sizeof(T);
    const size_t plane = (size_t)a.size * a.size, total = a.channels * plane, chunks = (total + kPer - 1) / kPer;
    T* out = static_cast<T*>(a.out);
    for (size_t k = (size_t)blockIdx.x * kObjThreads + threadIdx.x; k < chunks; k += (size_t)gridDim.x * kObjThreads) {
        const size_t e0 = k * kPer;
        size_t ch = e0 / plane;
        int p = (int)(e0 - ch * plane);
        int y = p / a.size, x = p - y * a.size;
        Stamp st = channel_stamp(a, ch, p == 0);
        union {
            T v[kPer];
            uint4 q;
        } buf;
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            if (e0 + i < total) {
                if (p == (int)plane) {  // the chunk crosses into the next channel
                    ++ch, p = 0, x = 0, y = 0;
                    st = channel_stamp(a, ch, true);
                }
                buf.v[i] = stamp_value<T>(a, st, x, y);
                ++p;
                if (++x == a.size) x = 0, ++y;
            } else {
                buf.v[i] = T(0);
            }
        }
        if (e0 + kPer <= total) {
            *reinterpret_cast<uint4*>(out + e0) = buf.q;
        } else {
            for (int i = 0; e0 + i < total; ++i) out[e0 + i] = buf.v[i];
        }
    }
}

// ---- heatmap IoU ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float sigmoid_f32(float x) { return 1.0f / (1.0f + expf(-x)); }

template <typename TT>
__device__ __forceinline__ float target_value(TT t);
template <>
__device__ __forceinline__ float target_value<float>(float t) { return t; }
template <>
__device__ __forceinline__ float target_value<uint8_t>(uint8_t t) { return (float)t / 255.0f; }  // uint8_to_float32, fp32 division

template <typename TT, int N>
struct TargetVec;
template <>
struct TargetVec<float, 4> {
    using type = float4;
};
template <>
struct TargetVec<uint8_t, 4> {
    using type = uchar4;
};

// Not yet block_sum of collectives.hpp: the barrier comes first here and in block_min_f64. With the header's protocol the eager
// objective step measured slower, in runs whose host-bound scatter the record could not bound; moving over remains open
// (profiles/collectives_refactor_ab.md). The order of the additions is the header's.
template <int WAVES = kObjWaves>
__device__ __forceinline__ double block_sum_f64(double v, double* red, int tid) {  // every thread gets the sum; red: WAVES
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) s += red[w];
    return s;
}

template <bool SIGMOID, typename TT>
__device__ __forceinline__ void iou_accumulate(float x, TT traw, double& st, double& tt, double& ss) {
    const float s = SIGMOID ? sigmoid_f32(x) : x, t = target_value<TT>(traw);
    st += (double)t * (double)s, tt += (double)t * (double)t, ss += (double)s * (double)s;
}

template <bool SIGMOID, typename TT, bool VEC>
__global__ __launch_bounds__(kObjThreads) void iou_terms_kernel(IouArgs a) {
    __shared__ double red[kObjWaves];
    const size_t ch = blockIdx.x;
    const int tid = threadIdx.x;
    const float* x = a.pred + ch * a.hw;
    const TT* t = static_cast<const TT*>(a.target) + ch * a.hw;
    double st = 0.0, tt = 0.0, ss = 0.0;
    if (VEC) {
        using TV = typename TargetVec<TT, 4>::type;
        const float4* x4 = reinterpret_cast<const float4*>(x);
        const TV* t4 = reinterpret_cast<const TV*>(t);
        const int n4 = a.hw / 4;
#pragma unroll 4
        for (int i = tid; i < n4; i += kObjThreads) {
            const float4 xv = x4[i];
            const TV tv = t4[i];
            iou_accumulate<SIGMOID, TT>(xv.x, tv.x, st, tt, ss);
            iou_accumulate<SIGMOID, TT>(xv.y, tv.y, st, tt, ss);
            iou_accumulate<SIGMOID, TT>(xv.z, tv.z, st, tt, ss);
            iou_accumulate<SIGMOID, TT>(xv.w, tv.w, st, tt, ss);
        }
    } else {
        for (int i = tid; i < a.hw; i += kObjThreads) iou_accumulate<SIGMOID, TT>(x[i], t[i], st, tt, ss);
    }
    st = block_sum_f64(st, red, tid);
    tt = block_sum_f64(tt, red, tid);
    ss = block_sum_f64(ss, red, tid);
    if (tid == 0) {
        a.sums[3 * ch] = st, a.sums[3 * ch + 1] = tt, a.sums[3 * ch + 2] = ss;
        const double n = st + kIouEps, d = tt + ss - st + kIouEps;
        if (a.iou) a.iou[ch] = (float)(n / d);
    }
}

__global__ __launch_bounds__(kObjThreads) void iou_finish_kernel(IouArgs a) {
    __shared__ double red[kObjWaves];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (size_t c = tid; c < a.channels; c += kObjThreads) {
        const double st = a.sums[3 * c], tt = a.sums[3 * c + 1], ss = a.sums[3 * c + 2];
        acc += (st + kIouEps) / (tt + ss - st + kIouEps);
    }
    acc = block_sum_f64(acc, red, tid);
    if (tid == 0) {
        const double mean = acc / (double)a.channels;
        a.loss[0] = (float)(1.0 - mean), a.loss[1] = (float)mean;
        if (a.accum) a.accum[0] += (float)mean, a.accum[1] += 1.0f;
    }
}

template <typename TT>
__device__ __forceinline__ float iou_grad_value(float x, TT traw, double ca, double cb) {
    const float s = sigmoid_f32(x), t = target_value<TT>(traw);
    const double sd = s;
    return (float)((ca * (double)t + cb * sd) * (sd * (1.0 - sd)));
}

template <typename TT, bool VEC>
__global__ __launch_bounds__(kObjThreads) void iou_grad_kernel(IouArgs a) {
    const size_t ch = blockIdx.x;
    const int tid = threadIdx.x;
    const double st = a.sums[3 * ch], tt = a.sums[3 * ch + 1], ss = a.sums[3 * ch + 2];
    const double n = st + kIouEps, d = tt + ss - st + kIouEps;
    // dL/dx = k (t D - N (2 s - t)) s (1 - s) = (ca t + cb s) s (1 - s), k = -g / (B C D^2)
    const double k = -(double)a.grad_out[0] / ((double)a.channels * d * d), ca = k * (d + n), cb = -2.0 * k * n;
    const float* x = a.pred + ch * a.hw;
    const TT* t = static_cast<const TT*>(a.target) + ch * a.hw;
    float* g = a.grad + ch * a.hw;
    if (VEC) {
        using TV = typename TargetVec<TT, 4>::type;
        const float4* x4 = reinterpret_cast<const float4*>(x);
        const TV* t4 = reinterpret_cast<const TV*>(t);
        float4* g4 = reinterpret_cast<float4*>(g);
        const int n4 = a.hw / 4;
#pragma unroll 4
        for (int i = tid; i < n4; i += kObjThreads) {
            const float4 xv = x4[i];
            const TV tv = t4[i];
            g4[i] = make_float4(iou_grad_value<TT>(xv.x, tv.x, ca, cb), iou_grad_value<TT>(xv.y, tv.y, ca, cb),
                                iou_grad_value<TT>(xv.z, tv.z, ca, cb), iou_grad_value<TT>(xv.w, tv.w, ca, cb));
        }
    } else {
        for (int i = tid; i < a.hw; i += kObjThreads) g[i] = iou_grad_value<TT>(x[i], t[i], ca, cb);
    }
}

// ---- landmark loss with visibility ----------------------------------------------------------------------------------
// torch's L1Loss / MSELoss / SmoothL1Loss (beta 1) and their backward, NaN included: sign(NaN) = 0, 2 NaN = NaN, and
// SmoothL1's backward clamps with comparisons (NaN passes through)
__device__ __forceinline__ double vis_value(int crit, double d) {
    const double ad = fabs(d);
    if (crit == DAD3D_LOSS_L1) return ad;
    if (crit == DAD3D_LOSS_L2) return d * d;
    return ad < 1.0 ? 0.5 * d * d : ad - 0.5;
}
__device__ __forceinline__ double vis_slope(int crit, double d) {
    if (crit == DAD3D_LOSS_L1) return d > 0.0 ? 1.0 : d < 0.0 ? -1.0 : 0.0;
    if (crit == DAD3D_LOSS_L2) return 2.0 * d;
    return d < -1.0 ? -1.0 : d > 1.0 ? 1.0 : d;
}

constexpr int kVisThreads = 1024;  // one workgroup: the whole loss in a fixed order, 16 waves to overlap the loads

__global__ __launch_bounds__(kVisThreads) void visibility_loss_kernel(VisibilityLossArgs a) {
    __shared__ double red[kVisThreads / 64];
    const int tid = threadIdx.x;
    const size_t m = (size_t)a.batch * a.n_points * 2;
    const double inv = 1.0 / (double)m;
    double acc = 0.0;
    for (size_t i = tid; i < m; i += kVisThreads) {
        const size_t pt = i >> 1;
        const float pp = a.pred_presence[pt], tp = a.target_presence[pt];
        const float d = a.pred[i] * pp - a.target[i] * tp;  // the reference's fp32 products and difference
        acc += vis_value(a.criterion, d);
        if (a.grad_pred) a.grad_pred[i] = (float)(vis_slope(a.criterion, d) * inv * (double)pp);
    }
    acc = block_sum_f64<kVisThreads / 64>(acc, red, tid);
    if (tid == 0) a.loss[0] = (float)(acc * inv);
}

// ---- keypoint errors ----------------------------------------------------------------------------------------------------
template <int D>
struct KpPair {
    double p[D], q[D];
};

template <int D>
__device__ __forceinline__ KpPair<D> kp_point(const KeypointErrArgs& a, int b, int n) {
    const int vi = a.index ? a.index[n] : n;
    const bool ok = vi >= 0 && vi < a.n_verts;  // never read outside the arrays: an index out of range reads as NaN
    const int vp = ok ? vi : 0;
    const size_t at = ((size_t)b * a.n_verts + vp) * D;
    const double pres = a.presence ? (double)a.presence[(size_t)b * a.n_verts + vp] : 1.0;
    KpPair<D> r;
#pragma unroll
    for (int c = 0; c < D; ++c) {
        r.p[c] = ok ? (double)a.pred[at + c] * a.pred_scale * pres : NAN;
        r.q[c] = ok ? (double)a.target[at + c] * pres * a.target_scale : NAN;
    }
    return r;
}

__device__ __forceinline__ double block_min_f64(double v, double* red, int tid, bool want_max) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double w = __shfl_xor(v, o, 64);
        v = want_max ? fmax(v, w) : fmin(v, w);
    }
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < kObjWaves; ++w) s = want_max ? fmax(s, red[w]) : fmin(s, red[w]);
    return s;
}

template <int D>
__global__ __launch_bounds__(kObjThreads) void keypoint_err_kernel(KeypointErrArgs a) {
    __shared__ double red[kObjWaves];
    const int b = blockIdx.x, tid = threadIdx.x;
    // normalize_to_cube (model/utils.py:55-68) of both subsets: v1 = v - min v; v2 = v1 - 0.5 max v1; v2 / max_{n,c} v2
    double plo[D] = {}, phalf[D] = {}, qlo[D] = {}, qhalf[D] = {}, pscale = 1.0, qscale = 1.0;
    if (a.cube) {
        double pmin[D], pmax[D], qmin[D], qmax[D];
#pragma unroll
        for (int c = 0; c < D; ++c) pmin[c] = qmin[c] = INFINITY, pmax[c] = qmax[c] = -INFINITY;
        for (int n = tid; n < a.n_points; n += kObjThreads) {
            const KpPair<D> v = kp_point<D>(a, b, n);
#pragma unroll
            for (int c = 0; c < D; ++c) {
                pmin[c] = fmin(pmin[c], v.p[c]), pmax[c] = fmax(pmax[c], v.p[c]);
                qmin[c] = fmin(qmin[c], v.q[c]), qmax[c] = fmax(qmax[c], v.q[c]);
            }
        }
        pscale = qscale = -INFINITY;
#pragma unroll
        for (int c = 0; c < D; ++c) {
            pmin[c] = block_min_f64(pmin[c], red, tid, false), pmax[c] = block_min_f64(pmax[c], red, tid, true);
            qmin[c] = block_min_f64(qmin[c], red, tid, false), qmax[c] = block_min_f64(qmax[c], red, tid, true);
            plo[c] = pmin[c], phalf[c] = 0.5 * (pmax[c] - pmin[c]);
            qlo[c] = qmin[c], qhalf[c] = 0.5 * (qmax[c] - qmin[c]);
            pscale = fmax(pscale, (pmax[c] - pmin[c]) - phalf[c]);
            qscale = fmax(qscale, (qmax[c] - qmin[c]) - qhalf[c]);
        }
    }
    double acc = 0.0;
    for (int n = tid; n < a.n_points; n += kObjThreads) {
        KpPair<D> v = kp_point<D>(a, b, n);
        double d2 = 0.0;
#pragma unroll
        for (int c = 0; c < D; ++c) {
            if (a.cube) v.p[c] = ((v.p[c] - plo[c]) - phalf[c]) / pscale, v.q[c] = ((v.q[c] - qlo[c]) - qhalf[c]) / qscale;
            const double d = v.p[c] - v.q[c];
            d2 += d * d;
        }
        acc += sqrt(d2);
    }
    acc = block_sum_f64(acc, red, tid);
    if (tid == 0) {
        a.err[2 * b] = acc / (double)a.n_points;
        a.err[2 * b + 1] = a.bbox ? sqrt((double)a.bbox[4 * b + 2] * (double)a.bbox[4 * b + 3]) : 2.0;
    }
}

__global__ __launch_bounds__(kObjThreads) void keypoint_finish_kernel(KeypointErrArgs a) {
    __shared__ double red[kObjWaves];
    const int tid = threadIdx.x;
    double nme = 0.0, cnt[kMaxThresholds];
#pragma unroll
    for (int k = 0; k < kMaxThresholds; ++k) cnt[k] = 0.0;
    for (int b = tid; b < a.batch; b += kObjThreads) {
        const double e = a.err[2 * b], nrm = a.err[2 * b + 1];
        nme += e / nrm;
#pragma unroll
        for (int k = 0; k < kMaxThresholds; ++k) {
            const double lim = a.thresholds[k] * nrm;  // unused slots hold 0
            cnt[k] += (a.below ? e < lim : e > lim) ? 1.0 : 0.0;
        }
    }
    nme = block_sum_f64(nme, red, tid);
#pragma unroll
    for (int k = 0; k < kMaxThresholds; ++k) cnt[k] = block_sum_f64(cnt[k], red, tid);
    if (tid == 0) {
        const double inv = 1.0 / (double)a.batch;
        a.out[0] = (float)(nme * inv);
        if (a.accum) a.accum[0] += (float)(nme * inv), a.accum[1] += 1.0f;
#pragma unroll
        for (int k = 0; k < kMaxThresholds; ++k) {
            if (k >= a.n_thresholds) break;
            a.out[1 + k] = (float)(cnt[k] * inv);
            if (a.accum) a.accum[2 + 2 * k] += (float)(cnt[k] * inv), a.accum[3 + 2 * k] += 1.0f;
        }
    }
}

}  // namespace

dad3d_status launch_heatmap_encode(const HeatmapEncodeArgs& a, hipStream_t s) {
    const size_t per = a.form == DAD3D_HEATMAP_UINT8 ? 16 : 4;
    const size_t chunks = (a.channels * (size_t)a.size * a.size + per - 1) / per;
    const unsigned blocks = (unsigned)std::min<size_t>((chunks + kObjThreads - 1) / kObjThreads, 1u << 20);
    if (a.form == DAD3D_HEATMAP_UINT8)
        hipLaunchKernelGGL(heatmap_encode_kernel<uint8_t>, dim3(blocks), dim3(kObjThreads), 0, s, a);
    else
        hipLaunchKernelGGL(heatmap_encode_kernel<float>, dim3(blocks), dim3(kObjThreads), 0, s, a);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

template <bool SIGMOID, typename TT>
static void launch_terms(const IouArgs& a, bool vec, hipStream_t s) {
    if (vec)
        hipLaunchKernelGGL((iou_terms_kernel<SIGMOID, TT, true>), dim3(a.channels), dim3(kObjThreads), 0, s, a);
    else
        hipLaunchKernelGGL((iou_terms_kernel<SIGMOID, TT, false>), dim3(a.channels), dim3(kObjThreads), 0, s, a);
}

dad3d_status launch_heatmap_iou(const IouArgs& a, bool sigmoid, bool vec, hipStream_t s) {
    if (a.target_u8 && sigmoid)
        launch_terms<true, uint8_t>(a, vec, s);
    else if (a.target_u8)
        launch_terms<false, uint8_t>(a, vec, s);
    else if (sigmoid)
        launch_terms<true, float>(a, vec, s);
    else
        launch_terms<false, float>(a, vec, s);
    DAD3D_HIP_TRY(hipGetLastError());
    if (a.loss) {
        hipLaunchKernelGGL(iou_finish_kernel, dim3(1), dim3(kObjThreads), 0, s, a);
        DAD3D_HIP_TRY(hipGetLastError());
    }
    return DAD3D_OK;
}

template <typename TT>
static void launch_grad(const IouArgs& a, bool vec, hipStream_t s) {
    if (vec)
        hipLaunchKernelGGL((iou_grad_kernel<TT, true>), dim3(a.channels), dim3(kObjThreads), 0, s, a);
    else
        hipLaunchKernelGGL((iou_grad_kernel<TT, false>), dim3(a.channels), dim3(kObjThreads), 0, s, a);
}

dad3d_status launch_heatmap_iou_grad(const IouArgs& a, bool vec, hipStream_t s) {
    if (a.target_u8)
        launch_grad<uint8_t>(a, vec, s);
    else
        launch_grad<float>(a, vec, s);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

dad3d_status launch_visibility_loss(const VisibilityLossArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(visibility_loss_kernel, dim3(1), dim3(kVisThreads), 0, s, a);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

dad3d_status launch_keypoint_errors(const KeypointErrArgs& a, hipStream_t s) {
    if (a.dims == 2)
        hipLaunchKernelGGL(keypoint_err_kernel<2>, dim3(a.batch), dim3(kObjThreads), 0, s, a);
    else
        hipLaunchKernelGGL(keypoint_err_kernel<3>, dim3(a.batch), dim3(kObjThreads), 0, s, a);
    DAD3D_HIP_TRY(hipGetLastError());
    if (a.out) {
        hipLaunchKernelGGL(keypoint_finish_kernel, dim3(1), dim3(kObjThreads), 0, s, a);
        DAD3D_HIP_TRY(hipGetLastError());
    }
    return DAD3D_OK;
}

}  // namespace dad3d
