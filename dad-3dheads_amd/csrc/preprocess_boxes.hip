// The heads of a frame from bounding boxes, for gfx950 (MI355X): ONE launch from uint8 frames and a device table of boxes to the
// network's input, and the two small kernels that move a crop's results into its frame.
//
//   extend_bbox              grow (x, y, w, h) by the offset factors in float64, truncate to int32    model_training/data/utils.py:73-103
//   ensure_bbox_boundaries   clip the box to its frame, in integers                                   model_training/data/utils.py:106-115
//                            (the crop DAD-3DNet was trained on: model_training/data/flame_dataset.py:96-99)
//   _get_paddings            scale = S / float(max(h, w)); py3round(dim * scale); calculate_paddings  predictor.py:117-123
//   _transform               LongestMaxSize -> PadIfNeeded -> Normalize -> CHW of the crop            predictor.py:80-95,195-203
//   readjust_3dmm_to_the_input_image, then HeadMesh.adjust_3dmm_to_paddings(params, [y, _, x, _])     predictor.py:154-176, head_mesh.py:48-60
//   readjust_landmarks_to_the_input_image, then + (x, y)                                              predictor.py:147-152
//
// preprocess_boxes_kernel is preprocess.hip's kernel with the geometry moved in: one lane per output pixel, the crop read in place
// through the frame's row stride (its edges are the resize's borders: every tap is clamped to the crop), the box rule and the
// geometry recomputed per workgroup from a handful of uniform values, and the side outputs (crop, geometry, flags) written by one
// lane of the box's first workgroup. So boxes that a detector left on the device need no host wait in front of the first kernel.
// A streaming kernel, no LDS. Output either float32 planar (the bits of preprocess.hip on the copied crop) or fp16 / bf16
// channels-last, rounded to nearest even here, which is what InferenceNet.forward makes of the float32 tensor on every batch.
// Channels-last stores: a pixel is 6 bytes, so with an even row length two neighbouring lanes trade one value and write 8 + 4
// bytes, both dword-aligned and contiguous across the wave, instead of three 2-byte stores each.
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include "common.hpp"
#include "points_math.hpp"
#include "resize_taps.hpp"

namespace dad3d {
namespace {

constexpr double kBoxRange = 1073741824.0;  // 2^30: every integer sum of two values below it fits int32

__device__ __forceinline__ bool in_range(double v) { return fabs(v) < kBoxRange; }  // false for a NaN and for +-inf

struct BoxGeometry {
    int flags;
    int x, y, w, h;         // the crop used
    int nh, nw, top, left;  // the resized crop and where it lies in the padded square
    double scale;
    const unsigned char* src;  // the crop's first byte
    long long row_stride;
};

__device__ __forceinline__ double box_value(const void* boxes, int dtype, size_t i) {  // every dtype widens exactly
    switch (dtype) {
        case DAD3D_BOX_DTYPE_I32: return (double)static_cast<const int32_t*>(boxes)[i];
        case DAD3D_BOX_DTYPE_I64: return (double)static_cast<const long long*>(boxes)[i];
        case DAD3D_BOX_DTYPE_F32: return (double)static_cast<const float*>(boxes)[i];
        default: return static_cast<const double*>(boxes)[i];
    }
}

// uniform over the workgroup. A flagged box divides nothing and reads no pixel.
__device__ __forceinline__ BoxGeometry box_geometry(const PreprocessBoxesArgs& a, int b) {
#pragma clang fp contract(off)
    BoxGeometry g{0, 0, 0, 0, 0, 0, 0, 0, 0, 1.0, nullptr, 0};
    double v[4];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = box_value(a.boxes, a.box_dtype, (size_t)b * 4 + k), ok = ok && in_range(v[k]);
    const int image = a.image_index[b];
    long long frame_h = 0, frame_w = 0;
    const unsigned char* frame = nullptr;
    if (image >= 0 && image < a.n_images) {
        const long long* d = a.images + (size_t)image * 4;
        frame = reinterpret_cast<const unsigned char*>(d[0]);
        frame_h = d[1], frame_w = d[2], g.row_stride = d[3];
    }
    ok = ok && frame && frame_h > 0 && frame_w > 0 && frame_h < (long long)kBoxRange && frame_w < (long long)kBoxRange;
    if (ok && a.has_offset) {  // extend_bbox, float64, in the reference's order of operations
        const double ex = v[0] - v[2] * a.left, ey = v[1] - v[3] * a.top;
        const double ew = v[2] * ((1.0 + a.right) + a.left), eh = v[3] * ((1.0 + a.top) + a.bottom);
        v[0] = ex, v[1] = ey, v[2] = ew, v[3] = eh;
        ok = in_range(ex) && in_range(ey) && in_range(ew) && in_range(eh);
    }
    if (!ok) {
        g.flags = DAD3D_BOX_FLAG_RANGE;
        return g;
    }
    const int bx = (int)v[0], by = (int)v[1], bw = (int)v[2], bh = (int)v[3];  // astype("int32"): toward zero
    const int fw = (int)frame_w, fh = (int)frame_h;
    const int x1 = min(max(0, bx), fw), y1 = min(max(0, by), fh);  // ensure_bbox_boundaries
    const int x2 = min(max(0, x1 + bw), fw), y2 = min(max(0, y1 + bh), fh);
    g.x = x1, g.y = y1, g.w = x2 - x1, g.h = y2 - y1;
    if (g.w <= 0 || g.h <= 0) {
        g.flags = DAD3D_BOX_FLAG_EMPTY;
        return g;
    }
    const double scale = (double)a.out_size / (double)max(g.h, g.w);
    g.nh = (int)rint((double)g.h * scale), g.nw = (int)rint((double)g.w * scale);  // py3round: half to even
    if (g.nh == 0 || g.nw == 0) {
        g.flags = DAD3D_BOX_FLAG_COLLAPSED;
        g.nh = g.nw = 0;
        return g;
    }
    const int m = max(g.nh, g.nw);  // calculate_paddings
    g.top = (m - g.nh) / 2, g.left = (m - g.nw) / 2;
    g.scale = scale;
    g.src = frame + (long long)g.y * g.row_stride + 3LL * g.x;
    return g;
}

template <int FORMAT>
__device__ __forceinline__ unsigned half_bits(float v) {  // round to nearest even, as Tensor.to(dtype)
    if (FORMAT == DAD3D_PREPROCESS_OUT_BF16_NHWC) return __builtin_bit_cast(unsigned short, __float2bfloat16(v));
    return __builtin_bit_cast(unsigned short, __float2half(v));
}

struct __attribute__((packed, aligned(4))) Dwords2 {
    unsigned lo, hi;
};

template <int FORMAT>
__global__ __launch_bounds__(256) void preprocess_boxes_kernel(PreprocessBoxesArgs a) {
#pragma clang fp contract(off)
    const int b = blockIdx.z, s = a.out_size;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    const BoxGeometry g = box_geometry(a, b);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        int32_t* c = a.crops + (size_t)b * 4;
        c[0] = g.x, c[1] = g.y, c[2] = g.w, c[3] = g.h;
        double* q = a.geometry + (size_t)b * 5;
        q[0] = g.left, q[1] = g.top, q[2] = g.scale, q[3] = g.flags ? 0.0 : (double)g.x, q[4] = g.flags ? 0.0 : (double)g.y;
        a.flags[b] = g.flags;
    }
    float ch[3] = {0.0f, 0.0f, 0.0f};  // PadIfNeeded: constant 0 before the normalisation; a flagged box is all padding
    const int dy = y - g.top, dx = x - g.left;
    if (x < s && dy >= 0 && dy < g.nh && dx >= 0 && dx < g.nw) resized_pixel(g.src, g.row_stride, g.h, g.w, g.nh, g.nw, dx, dy, ch);
    const float o0 = (ch[0] - a.mean255.x) * a.inv_std255.x;
    const float o1 = (ch[1] - a.mean255.y) * a.inv_std255.y;
    const float o2 = (ch[2] - a.mean255.z) * a.inv_std255.z;
    if (FORMAT == DAD3D_PREPROCESS_OUT_F32_NCHW) {
        if (x >= s) return;
        const size_t plane = (size_t)s * s;
        float* o = static_cast<float*>(a.out) + (size_t)b * 3 * plane + (size_t)y * s + x;
        o[0] = o0, o[plane] = o1, o[2 * plane] = o2;
    } else {
        const unsigned q0 = half_bits<FORMAT>(o0), q1 = half_bits<FORMAT>(o1), q2 = half_bits<FORMAT>(o2);
        unsigned short* o = static_cast<unsigned short*>(a.out) + (((size_t)b * s + y) * s + x) * 3;
        if ((s & 1) == 0) {  // x and the pixel's index have one parity: pixels 2k and 2k + 1 are 12 bytes from a dword boundary
            const unsigned other = __shfl_xor((x & 1) ? q0 : q2, 1);  // the odd lane's first value goes to the even lane
            if (x >= s) return;
            if ((x & 1) == 0) *reinterpret_cast<Dwords2*>(o) = Dwords2{q0 | q1 << 16, q2 | other << 16};
            else *reinterpret_cast<unsigned*>(o + 1) = q1 | q2 << 16;
        } else {
            if (x >= s) return;
            o[0] = (unsigned short)q0, o[1] = (unsigned short)q1, o[2] = (unsigned short)q2;
        }
    }
}

// predictor.readjust_3dmm_to_the_input_image (predictor.py:154-176) as flame_decode.hip's readjust_kernel computes it, on the float32
// values of the float64 geometry, then HeadMesh.adjust_3dmm_to_paddings(params, [y, _, x, _]) (head_mesh.py:48-60):
// t + (float32([x, y, 0]) * 2) / img_size, every operation rounded once
__global__ void readjust_frame_kernel(float* params, int batch, ParamLayout lay, const double* geometry, float img_size) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    float* p = params + (size_t)b * lay.n_params;
    const double* g = geometry + (size_t)b * 5;
    const float pad_left = (float)g[0], pad_top = (float)g[1], scale = (float)g[2], ox = (float)g[3], oy = (float)g[4];
    const float s = p[lay.scale_off];
    const float t0 = p[lay.trans_off], t1 = p[lay.trans_off + 1], t2 = p[lay.trans_off + 2];
    p[lay.scale_off] = (s + 1.0f) / scale - 1.0f;
    const float u0 = (t0 + 1.0f - pad_left * 2.0f / img_size) / scale - 1.0f;
    const float u1 = (t1 + 1.0f - pad_top * 2.0f / img_size) / scale - 1.0f;
    const float u2 = (t2 + 1.0f - 0.0f * 2.0f / img_size) / scale - 1.0f;
    p[lay.trans_off] = u0 + ox * 2.0f / img_size;
    p[lay.trans_off + 1] = u1 + oy * 2.0f / img_size;
    p[lay.trans_off + 2] = u2 + 0.0f * 2.0f / img_size;
}

// heatmap_points.hip's points_readjust_kernel on the 5-column geometry: the crop's origin is added as an integer AFTER the
// reference's truncation (predictor.py:150-152), saturating
__global__ __launch_bounds__(256) void points_readjust_frame_kernel(PointsReadjustArgs a, int total) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int xy = i & 1, b = i / (2 * a.n_points);
    const float s = a.src_kind == 0 ? static_cast<const float*>(a.src)[i] : (float)static_cast<const int32_t*>(a.src)[i ^ 1];
    const double* g = a.geometry + (size_t)b * 5;
    const long long v = (long long)readjusted_coordinate(s, a.mul, a.limit, g[xy], g[2]) + (long long)g[3 + xy];
    a.points[i] = (int)min(max(v, (long long)INT32_MIN), (long long)INT32_MAX);
}

}  // namespace

dad3d_status launch_preprocess_boxes(PreprocessBoxesArgs a, const float mean[3], const float std[3], hipStream_t s) {
    normalize_constants(mean, std, a.mean255, a.inv_std255);
    const dim3 grid((a.out_size + 255) / 256, a.out_size, a.n_boxes), block(256);
    switch (a.out_format) {
        case DAD3D_PREPROCESS_OUT_F32_NCHW: hipLaunchKernelGGL(preprocess_boxes_kernel<DAD3D_PREPROCESS_OUT_F32_NCHW>, grid, block, 0, s, a); break;
        case DAD3D_PREPROCESS_OUT_F16_NHWC: hipLaunchKernelGGL(preprocess_boxes_kernel<DAD3D_PREPROCESS_OUT_F16_NHWC>, grid, block, 0, s, a); break;
        case DAD3D_PREPROCESS_OUT_BF16_NHWC: hipLaunchKernelGGL(preprocess_boxes_kernel<DAD3D_PREPROCESS_OUT_BF16_NHWC>, grid, block, 0, s, a); break;
        default: set_error("preprocess_boxes: unknown output format %d", a.out_format); return DAD3D_E_INVALID;
    }
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

dad3d_status launch_readjust_frame(float* params, int batch, ParamLayout lay, const double* geometry, float img_size, hipStream_t s) {
    hipLaunchKernelGGL(readjust_frame_kernel, dim3((batch + 63) / 64), dim3(64), 0, s, params, batch, lay, geometry, img_size);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

dad3d_status launch_points_readjust_frame(const PointsReadjustArgs& a, hipStream_t s) {
    const int total = a.batch * a.n_points * 2;
    hipLaunchKernelGGL(points_readjust_frame_kernel, dim3((total + 255) / 256), dim3(256), 0, s, a, total);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

}  // namespace dad3d
