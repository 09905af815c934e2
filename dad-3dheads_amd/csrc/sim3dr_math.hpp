// The exact-arithmetic helpers of the Sim3DR raster kernels (sim3dr_kernels.hip, sim3dr_frames.hip), device only: the reference's
// conversions, std::min / std::max, the pixel-independent half of get_point_weight and the orderable depth.
//
// A UNIT THAT INCLUDES THIS IS COMPILED WITH -ffp-contract=off: the reference extension is an SSE2 build without FMA
// (Sim3DR/setup.py:12-18), so every multiply/add/subtract below must stay an individually rounded binary32 operation, in the
// reference's evaluation order, for the results to be bit-identical.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>

namespace dad3d {
namespace {

// (int) of a float as x86-64 cvttss2si (what `(int) ceil(..)` compiles to in the reference build).
__device__ __forceinline__ int f2i_x86(float f) {
    return (f >= -2147483648.0f && f < 2147483648.0f) ? (int)f : INT_MIN;
}
__device__ __forceinline__ float std_min(float a, float b) { return (b < a) ? b : a; }  // std::min
__device__ __forceinline__ float std_max(float a, float b) { return (a < b) ? b : a; }  // std::max

struct TriSetup {  // pixel-independent part of get_point_weight / is_point_in_tri
    float x0, y0, ax, ay, bx, by, d00, d01, d11, inv;
};

__device__ __forceinline__ TriSetup tri_setup(float x0, float y0, float x1, float y1, float x2, float y2) {
    TriSetup t;
    t.x0 = x0;
    t.y0 = y0;
    t.ax = x2 - x0;  // v0 = p2 - p0
    t.ay = y2 - y0;
    t.bx = x1 - x0;  // v1 = p1 - p0
    t.by = y1 - y0;
    t.d00 = t.ax * t.ax + t.ay * t.ay;
    t.d01 = t.ax * t.bx + t.ay * t.by;
    t.d11 = t.bx * t.bx + t.by * t.by;
    const float den = t.d00 * t.d11 - t.d01 * t.d01;
    t.inv = (den == 0.0f) ? 0.0f : 1.0f / den;
    return t;
}

// TriSetup from the corners and the stored inv: the expressions of tri_setup without its division, so the same bits
__device__ __forceinline__ TriSetup setup_from_corners(float x0, float y0, float x1, float y1, float x2, float y2, float inv) {
    TriSetup t;
    t.x0 = x0;
    t.y0 = y0;
    t.ax = x2 - x0;
    t.ay = y2 - y0;
    t.bx = x1 - x0;
    t.by = y1 - y0;
    t.d00 = t.ax * t.ax + t.ay * t.ay;
    t.d01 = t.ax * t.bx + t.ay * t.by;
    t.d11 = t.bx * t.bx + t.by * t.by;
    t.inv = inv;
    return t;
}

__device__ __forceinline__ void tri_uv(const TriSetup& t, float px, float py, float& u, float& v) {
    const float cx = px - t.x0, cy = py - t.y0;  // v2 = p - p0
    const float d02 = t.ax * cx + t.ay * cy;
    const float d12 = t.bx * cx + t.by * cy;
    u = (t.d11 * d02 - t.d01 * d12) * t.inv;
    v = (t.d00 * d12 - t.d01 * d02) * t.inv;
}

// orderable(z) for a z that is not NaN: one shift, one or, one xor
__device__ __forceinline__ unsigned depth_order_number(float z) {
    const int u = __float_as_int(z + 0.0f);  // -0 -> +0
    return (unsigned)u ^ ((unsigned)(u >> 31) | 0x80000000u);
}

}  // namespace
}  // namespace dad3d
