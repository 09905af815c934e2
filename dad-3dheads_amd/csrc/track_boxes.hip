// Tracking heads from frame to frame, for gfx950 (MI355X): ONE launch from the projected vertices of a call's heads to the boxes of
// the next call, so that a video loop predict -> boxes -> predict never brings a vertex to the host. 3DDFA_V2, the project Sim3DR
// comes from, tracks this way: detect once, then take each frame's box from the previous frame's fit.
//
// One workgroup of 256 lanes per head. A lane walks the selected vertices with the workgroup's stride and keeps (xmin, ymin, -xmax,
// -ymax) and a word of bits (a coordinate that is not finite, a subset index outside the vertices); ONE block_reduce of
// collectives.hpp over that five-word record -- minimum on the floats, or on the bits -- gives every lane the head's bounds, and
// lane 0 forms the box in integers and writes the head's five words. min and max do not round and the record's combination is
// commutative and associative, so the result does not depend on which lane met which vertex. A head that is decided before its
// vertices (the previous call flagged it, or its frame does not exist) reads none of them: its workgroup leaves before the loop.
// No atomics, no scratch; 5 words of LDS a wave for the reduction.
#include "collectives.hpp"
#include "common.hpp"

namespace dad3d {
namespace {

constexpr int kTrackThreads = 256, kTrackWaves = kTrackThreads / 64;
constexpr float kTrackRange = 1073741824.0f;  // 2^30, as the box rule of preprocess_boxes.hip: every difference of two integers below it fits int32
constexpr int kBitNonfinite = 1, kBitIndex = 2;

struct Bounds {
    float xmin, ymin, neg_xmax, neg_ymax;  // the maxima negated: one operation for all four
    int bits;
};
struct OpBounds {
    __device__ static __forceinline__ Bounds of(const Bounds& a, const Bounds& b) {
        return Bounds{fminf(a.xmin, b.xmin), fminf(a.ymin, b.ymin), fminf(a.neg_xmax, b.neg_xmax), fminf(a.neg_ymax, b.neg_ymax), a.bits | b.bits};
    }
};
// what wave_reduce of collectives.hpp calls for this record: five 32-bit shuffles
__device__ __forceinline__ Bounds lane_xor(const Bounds& v, int d) {
    return Bounds{__shfl_xor(v.xmin, d, 64), __shfl_xor(v.ymin, d, 64), __shfl_xor(v.neg_xmax, d, 64), __shfl_xor(v.neg_ymax, d, 64),
                  __shfl_xor(v.bits, d, 64)};
}

__device__ __forceinline__ void write_head(const TrackBoxesArgs& a, int i, int x, int y, int w, int h, int flags) {
    int32_t* b = a.boxes + (size_t)i * 4;
    const bool keep = flags == 0;  // any flag zeroes the box: the next preprocess launch flags it EMPTY and reads no pixel for it
    b[0] = keep ? x : 0, b[1] = keep ? y : 0, b[2] = keep ? w : 0, b[3] = keep ? h : 0;
    a.flags[i] = flags;
}

__global__ __launch_bounds__(kTrackThreads) void boxes_from_heads_kernel(TrackBoxesArgs a) {
#pragma clang fp contract(off)
    __shared__ Bounds red[kTrackWaves];
    const int i = blockIdx.x, t = threadIdx.x;
    // decided before the vertices; every condition is uniform over the workgroup
    int early = 0;
    long long frame_h = 0, frame_w = 0;
    if (a.prev_flags && a.prev_flags[i] != 0) {
        early = DAD3D_TRACK_FLAG_PREVIOUS;
    } else {
        const int image = a.image_index[i];
        bool ok = image >= 0 && image < a.n_frames;
        if (ok) {
            const long long* d = a.frames + (size_t)image * 4;
            frame_h = d[1], frame_w = d[2];
            ok = d[0] != 0 && frame_h > 0 && frame_w > 0 && frame_h < (long long)kTrackRange && frame_w < (long long)kTrackRange;
        }
        if (!ok) early = DAD3D_TRACK_FLAG_RANGE;
    }
    if (early) {
        if (t == 0) write_head(a, i, 0, 0, 0, 0, early);
        return;
    }
    const float inf = __builtin_inff();
    Bounds b{inf, inf, inf, inf, 0};
    const float* head = a.proj + (long long)i * a.head_stride;
    const int n = a.subset ? a.n_subset : a.n_verts;
    for (int k = t; k < n; k += kTrackThreads) {
        int v = k;
        if (a.subset) {
            v = a.subset[k];
            if (v < 0 || v >= a.n_verts) {  // flagged, and nothing is read through it
                b.bits |= kBitIndex;
                continue;
            }
        }
        const float* p = head + (long long)v * a.vertex_stride;
        const float x = p[0], y = p[1];
        if (!(fabsf(x) < inf) || !(fabsf(y) < inf)) b.bits |= kBitNonfinite;  // a NaN compares false
        b.xmin = fminf(b.xmin, x), b.ymin = fminf(b.ymin, y);
        b.neg_xmax = fminf(b.neg_xmax, -x), b.neg_ymax = fminf(b.neg_ymax, -y);
    }
    b = block_reduce<OpBounds, kTrackWaves>(b, red);
    if (t != 0) return;
    const float xmin = b.xmin, ymin = b.ymin, xmax = -b.neg_xmax, ymax = -b.neg_ymax;
    int flags = 0;
    if (b.bits & kBitIndex) flags = DAD3D_TRACK_FLAG_RANGE;
    else if (b.bits & kBitNonfinite) flags = DAD3D_TRACK_FLAG_NONFINITE;
    else if (!(fabsf(xmin) < kTrackRange && fabsf(xmax) < kTrackRange && fabsf(ymin) < kTrackRange && fabsf(ymax) < kTrackRange))
        flags = DAD3D_TRACK_FLAG_RANGE;
    if (flags) {
        write_head(a, i, 0, 0, 0, 0, flags);
        return;
    }
    const int x0 = (int)floorf(xmin), y0 = (int)floorf(ymin), x1 = (int)ceilf(xmax), y1 = (int)ceilf(ymax);  // exact below 2^30
    const int w = x1 - x0, h = y1 - y0;
    if (min(w, h) < a.min_side) flags |= DAD3D_TRACK_FLAG_SMALL;
    const long long area = (long long)w * h;
    if (area != 0) {  // the box against [0, W) x [0, H)
        const long long iw = max(0LL, min((long long)x1, frame_w) - max(x0, 0));
        const long long ih = max(0LL, min((long long)y1, frame_h) - max(y0, 0));
        if ((double)(iw * ih) < a.min_visible * (double)area) flags |= DAD3D_TRACK_FLAG_OUTSIDE;  // one product, no division
    }
    write_head(a, i, x0, y0, w, h, flags);
}

}  // namespace

dad3d_status launch_boxes_from_heads(const TrackBoxesArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(boxes_from_heads_kernel, dim3(a.n_heads), dim3(kTrackThreads), 0, s, a);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

}  // namespace dad3d
