// cv2.resize(INTER_LINEAR)'s coefficient set-up, shared by the kernels that resize a uint8 image through the 8-bit fixed-point
// path (preprocess.hip: whole images; preprocess_boxes.hip: crops read in place).
#pragma once
#include <hip/hip_runtime.h>

namespace dad3d {

constexpr int kCoefBits = 11;  // INTER_RESIZE_COEF_BITS

// cv2's coefficient set-up for one destination coordinate (resize.cpp, the `interpolation == INTER_LINEAR` branch of
// resize(): fx = (float)((dx + 0.5) * scale - 0.5); sx = cvFloor(fx); fx -= sx;
// ialpha = saturate_cast<short>(coef * INTER_RESIZE_COEF_SCALE) = round-half-even).
// HORIZONTAL only: at the borders resize() sets (fx, sx) = (0, 0) resp. (0, src - 1). For the rows it keeps the fractional
// part and clamps only the two row INDICES (`clip(sy + k, 0, ssize.height)` in the row loop): above the first and below the
// last source row both taps read the same row with weights that still sum to 2048 -- one LSB away from a zeroed fraction
// on some pixels of an up-scaled image's first and last rows.
template <bool HORIZONTAL>
__device__ __forceinline__ void linear_tap(int d, int src_n, int dst_n, int& s0, int& s1, int& c0, int& c1) {
    const double scale = 1.0 / ((double)dst_n / (double)src_n);
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (HORIZONTAL) {
        if (s < 0) f = 0.0f, s = 0;
        if (s >= src_n - 1) f = 0.0f, s = src_n - 1;
    }
    s0 = min(max(s, 0), src_n - 1);
    s1 = min(max(s + 1, 0), src_n - 1);
    c0 = __float2int_rn((1.0f - f) * (float)(1 << kCoefBits));
    c1 = __float2int_rn(f * (float)(1 << kCoefBits));
}

// The pixel (dx, dy) of the h x w uint8 RGB image at `src` (rows `row_stride` bytes apart) resized to nh x nw, as floats. Every tap
// lies inside [0, h) x [0, w).
__device__ __forceinline__ void resized_pixel(const unsigned char* src, long long row_stride, int h, int w, int nh, int nw, int dx, int dy,
                                              float (&ch)[3]) {
    if (nh == h && nw == w) {  // LongestMaxSize leaves an image of the right size alone
        const unsigned char* p = src + dy * row_stride + 3 * dx;
        ch[0] = p[0], ch[1] = p[1], ch[2] = p[2];
    } else {
        int sx, sx1, a0, a1, sy, sy1, b0, b1;
        linear_tap<true>(dx, w, nw, sx, sx1, a0, a1);
        linear_tap<false>(dy, h, nh, sy, sy1, b0, b1);
        const unsigned char* p00 = src + sy * row_stride + 3 * sx;
        const unsigned char* p01 = src + sy * row_stride + 3 * sx1;
        const unsigned char* p10 = src + sy1 * row_stride + 3 * sx;
        const unsigned char* p11 = src + sy1 * row_stride + 3 * sx1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int r0 = p00[c] * a0 + p01[c] * a1;  // HResizeLinear: 8-bit x 11-bit coefficients
            const int r1 = p10[c] * a0 + p11[c] * a1;
            // VResizeLinear<uchar,int,short>: (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2
            ch[c] = (float)((((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2);
        }
    }
}

// A.Normalize's constants as albumentations computes them: mean = float32(mean) * 255 ; denominator = reciprocal(float32(std) * 255),
// both in float32. Host.
inline void normalize_constants(const float mean[3], const float std[3], float3& mean255, float3& inv_std255) {
    volatile float m[3], sd[3];
    for (int c = 0; c < 3; ++c) m[c] = mean[c] * 255.0f, sd[c] = std[c] * 255.0f;
    mean255 = make_float3(m[0], m[1], m[2]);
    inv_std255 = make_float3(1.0f / sd[0], 1.0f / sd[1], 1.0f / sd[2]);
}

}  // namespace dad3d
