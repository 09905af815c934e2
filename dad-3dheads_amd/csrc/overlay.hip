// The demo's overlays (demo_utils.py:22-94: cv2.circle dots, cv2.line(LINE_AA) mesh edges, cv2.arrowedLine pose axes) for gfx950
// (MI355X), drawn per pixel on uint8 [B,H,W,3] images. The stroke rules are this project's own, in exact integer arithmetic
// (DESIGN.md 4.17); tests/overlay_restatement.py states them once more on the CPU and the kernels are held to that to the bit.
//
//   overlay_segments_kernel  one workgroup per (image, tile of kTile x kTile pixels). It walks the segment list in index order in
//                            chunks of kThreads: a lane truncates one segment's ends, tests its grown bounding box against the
//                            tile, and block_exclusive_scan compacts the hits IN ORDER into LDS. Every lane then folds the chunk's
//                            list over its own kRows pixels, which stay in registers from the one load to the one store: the
//                            result is that of drawing the segments one after another. No atomics, no global scratch. A wave owns
//                            one kSub x kSub quarter of the tile and steps over a listed segment whose box misses that quarter
//                            (the same test in all its lanes), so the list is built once per tile and folded per quarter.
//   overlay_discs_kernel     the same walk over points; the discs of a call share a colour, so a pixel only remembers whether
//                            one covered it.
//
// Every rule is a closed form of (pixel, primitive). A primitive with a non-finite coordinate, one outside [-8192, 8192] after the
// truncation toward zero, or an index outside the point table is skipped whole. With |coordinate| <= 8192 and pixels in [0, 8192)
// every product below stays under 2^62; the anti-aliased quotient takes a 32-bit division where the segment is short enough for
// its numerator (the same for every lane: the branch is uniform).
#include "collectives.hpp"
#include "common.hpp"

namespace dad3d {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kTile = 32;            // pixels per tile side; the four waves own its quarters
constexpr int kSub = kTile / 2;      // a quarter's side
constexpr int kRowStep = 64 / kSub;  // a lane owns column lane % kSub of its quarter, rows lane / kSub + k * kRowStep
constexpr int kRows = kSub / kRowStep;
static_assert(kWaves == 4 && kRows * kRowStep == kSub, "one wave per quarter of the tile");
constexpr int kCoordMax = 8192;

struct Seg {
    int x0, y0, x1, y1;
    unsigned rgb;
};

// astype(int): toward zero. False for NaN, +-inf and anything that truncates outside [-kCoordMax, kCoordMax].
__device__ __forceinline__ bool truncate_coord(float v, int& out) {
    if (!(fabsf(v) < (float)(kCoordMax + 1))) return false;
    out = (int)v;
    return true;
}

template <typename T>
__device__ __forceinline__ T floor_div(T num, T den) {  // den > 0
    T q = num / den;
    if (num % den != 0 && num < 0) --q;
    return q;
}

// Step `major` of the anti-aliased segment: the row (column) `base` gets 256 - frac, base + 1 gets frac; `in` is false off its ends.
struct AaStep {
    int base, frac;
    bool in;
    __device__ __forceinline__ int weight(int minor) const { return !in ? 0 : minor == base ? 256 - frac : minor == base + 1 ? frac : 0; }
};
struct AaLine {
    int m0, minor0, n, sign, d_minor;
    template <typename T>
    __device__ __forceinline__ AaStep step(int major) const {
        const int i = (major - m0) * sign;
        const bool in = i >= 0 && i <= n;
        const T num = (T)2 * (T)(in ? i : 0) * (T)d_minor * (T)256 + (T)n;
        const int q = 256 * minor0 + (n ? (int)floor_div<T>(num, (T)2 * (T)n) : 0);
        return AaStep{q >> 8, q & 255, in};
    }
};

__device__ __forceinline__ int solid_weight(int x, int y, const Seg& s, long long t2) {
    const long long dx = s.x1 - s.x0, dy = s.y1 - s.y0, ux = x - s.x0, uy = y - s.y0, vx = x - s.x1, vy = y - s.y1;
    const long long l2 = dx * dx + dy * dy, dot = ux * dx + uy * dy, cr = ux * dy - uy * dx;
    const bool body = l2 > 0 && dot >= 0 && dot <= l2 && 4 * cr * cr <= t2 * l2;  // a zero-length segment: the end tests only
    return body || 4 * (ux * ux + uy * uy) <= t2 || 4 * (vx * vx + vy * vy) <= t2 ? 256 : 0;
}

__device__ __forceinline__ void blend(int (&px)[3], unsigned rgb, int a) {
#pragma unroll
    for (int c = 0; c < 3; ++c) px[c] = (px[c] * (256 - a) + (int)((rgb >> (8 * c)) & 255u) * a + 128) >> 8;
}

struct Pixels {
    int v[kRows][3];
    int x, y0;    // the lane's column and first row
    int qx, qy;   // the corner of the wave's quarter
    __device__ __forceinline__ void place(int tile_x, int tile_y) {
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        qx = tile_x + (wave & 1) * kSub, qy = tile_y + (wave >> 1) * kSub;
        x = qx + lane % kSub, y0 = qy + lane / kSub;
    }
    // does the box, grown by `grow`, touch the wave's quarter? The same in every lane of the wave.
    __device__ __forceinline__ bool touches(int xa, int xb, int ya, int yb, int grow) const {
        return min(xa, xb) - grow < qx + kSub && max(xa, xb) + grow >= qx && min(ya, yb) - grow < qy + kSub && max(ya, yb) + grow >= qy;
    }
    __device__ __forceinline__ void load(const uint8_t* img, int h, int w) {
#pragma unroll
        for (int k = 0; k < kRows; ++k) {
            const int y = y0 + k * kRowStep;
            v[k][0] = v[k][1] = v[k][2] = 0;
            if (x < w && y < h) {
                const uint8_t* p = img + ((size_t)y * w + x) * 3;
                v[k][0] = p[0], v[k][1] = p[1], v[k][2] = p[2];
            }
        }
    }
    __device__ __forceinline__ void store(uint8_t* img, int h, int w) const {
#pragma unroll
        for (int k = 0; k < kRows; ++k) {
            const int y = y0 + k * kRowStep;
            if (x < w && y < h) {
                uint8_t* p = img + ((size_t)y * w + x) * 3;
                p[0] = (uint8_t)v[k][0], p[1] = (uint8_t)v[k][1], p[2] = (uint8_t)v[k][2];
            }
        }
    }
};

__global__ __launch_bounds__(kThreads) void overlay_segments_kernel(OverlaySegmentsArgs a) {
    __shared__ Seg list[kThreads];
    __shared__ int red[kWaves];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int tiles_x = (a.w + kTile - 1) / kTile;
    const int tx0 = (int)(blockIdx.x % tiles_x) * kTile, ty0 = (int)(blockIdx.x / tiles_x) * kTile;
    const size_t image = (size_t)b * a.h * a.w * 3;
    Pixels px;
    px.place(tx0, ty0);
    px.load(a.src + image, a.h, a.w);

    const float* pts = a.points + (size_t)b * a.n_points * 2;
    const int grow = a.thickness ? (a.thickness + 1) / 2 : 1;
    const long long t2 = (long long)a.thickness * a.thickness;
    for (int first = 0; first < a.n_edges; first += kThreads) {
        const int e = first + tid;
        Seg s{0, 0, 0, 0, a.color};
        int hit = 0;
        if (e < a.n_edges) {
            const int i0 = a.edges[2 * e], i1 = a.edges[2 * e + 1];
            if (i0 >= 0 && i0 < a.n_points && i1 >= 0 && i1 < a.n_points) {
                const bool ok = truncate_coord(pts[2 * i0], s.x0) && truncate_coord(pts[2 * i0 + 1], s.y0) &&
                                truncate_coord(pts[2 * i1], s.x1) && truncate_coord(pts[2 * i1 + 1], s.y1);
                hit = ok && min(s.x0, s.x1) - grow < tx0 + kTile && max(s.x0, s.x1) + grow >= tx0 &&
                      min(s.y0, s.y1) - grow < ty0 + kTile && max(s.y0, s.y1) + grow >= ty0;
                if (hit && a.colors) {
                    const uint8_t* c = a.colors + (size_t)e * 3;
                    s.rgb = c[0] | (c[1] << 8) | (c[2] << 16);
                }
            }
        }
        int total;
        const int at = block_exclusive_scan<kWaves>(hit, red, total);
        if (total == 0) continue;  // the same in every lane
        if (hit) list[at] = s;
        __syncthreads();
        if (a.thickness == 0) {
            for (int j = 0; j < total; ++j) {
                const Seg g = list[j];
                if (!px.touches(g.x0, g.x1, g.y0, g.y1, grow)) continue;
                const int dx = g.x1 - g.x0, dy = g.y1 - g.y0;
                const bool x_major = abs(dx) >= abs(dy);
                const AaLine line{x_major ? g.x0 : g.y0, x_major ? g.y0 : g.x0, x_major ? abs(dx) : abs(dy),
                                  (x_major ? dx : dy) >= 0 ? 1 : -1, x_major ? dy : dx};
                // |numerator| <= 512 n |d_minor| + n < 2^31: a 32-bit division. Both tests are the same in every lane.
                const bool small = line.n * abs(line.d_minor) <= (1 << 21);
                if (x_major) {  // the lane's pixels share the column: one step
                    const AaStep st = small ? line.step<int>(px.x) : line.step<long long>(px.x);
#pragma unroll
                    for (int k = 0; k < kRows; ++k) blend(px.v[k], g.rgb, st.weight(px.y0 + k * kRowStep));
                } else {
#pragma unroll
                    for (int k = 0; k < kRows; ++k) {
                        const int y = px.y0 + k * kRowStep;
                        const AaStep st = small ? line.step<int>(y) : line.step<long long>(y);
                        blend(px.v[k], g.rgb, st.weight(px.x));
                    }
                }
            }
        } else {
            for (int j = 0; j < total; ++j) {
                const Seg g = list[j];
                if (!px.touches(g.x0, g.x1, g.y0, g.y1, grow)) continue;
#pragma unroll
                for (int k = 0; k < kRows; ++k) blend(px.v[k], g.rgb, solid_weight(px.x, px.y0 + k * kRowStep, g, t2));
            }
        }
        // no barrier here: the next chunk writes `list` behind the scan's barriers, which every lane reaches after this fold
    }
    px.store(a.dst + image, a.h, a.w);
}

__global__ __launch_bounds__(kThreads) void overlay_discs_kernel(OverlayDiscsArgs a) {
    __shared__ int2 list[kThreads];
    __shared__ int red[kWaves];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int tiles_x = (a.w + kTile - 1) / kTile;
    const int tx0 = (int)(blockIdx.x % tiles_x) * kTile, ty0 = (int)(blockIdx.x / tiles_x) * kTile;
    const size_t image = (size_t)b * a.h * a.w * 3;
    Pixels px;
    px.place(tx0, ty0);
    px.load(a.src + image, a.h, a.w);

    const float* pts = a.points + (size_t)b * a.n_points * 2;
    const int r = a.radius, r2 = r * r;  // (x - cx)^2 + (y - cy)^2 < 2^29
    bool covered[kRows] = {};
    for (int first = 0; first < a.n_discs; first += kThreads) {
        const int e = first + tid;
        int2 c = make_int2(0, 0);
        int hit = 0;
        if (e < a.n_discs) {
            const int i = a.index ? a.index[e] : e;
            if (i >= 0 && i < a.n_points) {
                const bool ok = truncate_coord(pts[2 * i], c.x) && truncate_coord(pts[2 * i + 1], c.y);
                hit = ok && c.x - r < tx0 + kTile && c.x + r >= tx0 && c.y - r < ty0 + kTile && c.y + r >= ty0;
            }
        }
        int total;
        const int at = block_exclusive_scan<kWaves>(hit, red, total);
        if (total == 0) continue;
        if (hit) list[at] = c;
        __syncthreads();
        for (int j = 0; j < total; ++j) {
            const int2 g = list[j];
            if (!px.touches(g.x, g.x, g.y, g.y, r)) continue;
            const int ex = px.x - g.x, ex2 = ex * ex;
#pragma unroll
            for (int k = 0; k < kRows; ++k) {
                const int ey = px.y0 + k * kRowStep - g.y;
                covered[k] |= ex2 + ey * ey <= r2;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kRows; ++k)
        if (covered[k]) blend(px.v[k], a.color, 256);
    px.store(a.dst + image, a.h, a.w);
}

dim3 overlay_grid(int batch, int h, int w) { return dim3(((w + kTile - 1) / kTile) * ((h + kTile - 1) / kTile), batch); }

}  // namespace

dad3d_status launch_overlay_segments(const OverlaySegmentsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(overlay_segments_kernel, overlay_grid(a.batch, a.h, a.w), dim3(kThreads), 0, s, a);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

dad3d_status launch_overlay_discs(const OverlayDiscsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(overlay_discs_kernel, overlay_grid(a.batch, a.h, a.w), dim3(kThreads), 0, s, a);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

}  // namespace dad3d
