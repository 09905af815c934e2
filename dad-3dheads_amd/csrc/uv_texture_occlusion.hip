// Self-occlusion for the UV-texture bake from frames: a depth map per head, and the bake of uv_texture_frames.hip with a depth test.
// The reference's rule (inference/uv_texture.py:38-46) has none: a texel that faces the camera behind the nose takes the nose's pixel.
//
// Coordinates are the bake's: frame pixel x, pixel y, z with the viewer at -z (n_dot_view = -n_z), so the nearer surface has the SMALLER z.
//
//   depth_window_kernel  one workgroup per head: min / max of x and y and "any x, y or z not finite" over its vertices -> flags[k] and
//                        window[k] = {x0, y0, ww, wh}, the head's box in the frame it names: x0 = max(floorf(min x), 0),
//                        x1 = min(ceilf(max x), w - 1) in float, likewise y. Outside the frame: ww = wh = 0, no flag. Wider or higher than
//                        D: DAD3D_BAKE_FLAG_DEPTH_WINDOW. A flagged head has the window {0, 0, 0, 0}.
//   depth_clear_kernel   the ww x wh window of every head := +inf ("uncovered"); nothing outside it is written.
//   depth_raster_kernel  a lane per (head, triangle): the box of rasterize_kernel.cpp:321-325 clipped to the frame (and to the window, which
//                        holds it), is_point_in_tri, get_point_weight's weights, z = w0 * z0 + w1 * z1 + w2 * z2 -- _rasterize_triangles on
//                        the head with z negated, negated back; negation is exact, so the reference's `-z > -1e8` is `z < 1e8` here. The
//                        minimum over the fragments of a pixel, by one 32-bit atomic on the float's own bits: a signed minimum for z >= 0
//                        and an unsigned maximum for z < 0 order floats of mixed signs against a value that started at +inf. -0 is stored
//                        as +0 and NaN never enters. A box of more than 64 pixels is walked by the whole wave.
//   bake_frames_occluded_kernel  bake_frames_kernel with a third test (uv_hidden, uv_texture.hpp) after uv_sample's two: a candidate
//                        behind the head's own depth at its rounded pixel is skipped like a back-facing one and the descending walk goes on.
//                        flags[k] = depth_flags[k] | INDEX; a head with any flag gives zeros (plain) or keeps its state (accumulate).
//
// Every store into a map is bounded by the head's own ww, wh <= D, read back from `window`: a device frame table that disagrees with the
// host's checked copy cannot reach outside the map. Compiled with -ffp-contract=off (sim3dr_math.hpp, uv_texture.hpp).
#include "common.hpp"
#include "collectives.hpp"
#include "sim3dr_math.hpp"
#include "uv_texture.hpp"

namespace dad3d {
namespace {

constexpr int kThreads = kUvBakeThreads;
constexpr int kWaves = kThreads / 64;
constexpr int kTexels = kUvBakeTexels;
constexpr int kLaneBoxPixels = 64;  // a larger box is taken by the whole wave
constexpr int kClearPerLane = 16;

struct OpMin {
    __device__ static __forceinline__ float of(float a, float b) { return fminf(a, b); }
};
struct OpMax {
    __device__ static __forceinline__ float of(float a, float b) { return fmaxf(a, b); }
};
struct OpOr {
    __device__ static __forceinline__ int of(int a, int b) { return a | b; }
};

// h and w of frame f as the bake reads them, or 0 x 0 for an entry the host's checks would have refused
__device__ __forceinline__ void frame_hw(const long long* frames, int f, int& h, int& w) {
    const long long fh = frames[4 * (size_t)f + 1], fw = frames[4 * (size_t)f + 2];
    const bool ok = fh >= 1 && fw >= 1 && fh <= INT_MAX && fw <= INT_MAX;
    h = ok ? (int)fh : 0, w = ok ? (int)fw : 0;
}

__device__ __forceinline__ int4 load_window(const int* window, int k) {  // workgroup-uniform; the table need not be 16-byte aligned
    const int* wp = window + 4 * (size_t)k;
    return make_int4(wp[0], wp[1], wp[2], wp[3]);
}

__global__ __launch_bounds__(kThreads) void depth_window_kernel(UvDepthFramesArgs a) {
    __shared__ float red[kWaves];
    __shared__ int red_i[kWaves];
    const int k = blockIdx.x;
    const float* vb = a.vertices + (size_t)k * a.n_verts * 3;
    float lo_x = INFINITY, lo_y = INFINITY, hi_x = -INFINITY, hi_y = -INFINITY;
    int bad = 0;
    for (int i = threadIdx.x; i < a.n_verts; i += kThreads) {
        const float x = vb[3 * i], y = vb[3 * i + 1], z = vb[3 * i + 2];
        bad |= !(fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY);  // NaN fails `<` too
        lo_x = fminf(lo_x, x), hi_x = fmaxf(hi_x, x), lo_y = fminf(lo_y, y), hi_y = fmaxf(hi_y, y);
    }
    bad = block_reduce<OpOr, kWaves>(bad, red_i);
    lo_x = block_reduce<OpMin, kWaves>(lo_x, red), hi_x = block_reduce<OpMax, kWaves>(hi_x, red);
    lo_y = block_reduce<OpMin, kWaves>(lo_y, red), hi_y = block_reduce<OpMax, kWaves>(hi_y, red);
    if (threadIdx.x != 0) return;
    const int f = a.image_index[k];
    const bool has_frame = f >= 0 && f < a.n_frames;
    int flag = (has_frame ? 0 : DAD3D_BAKE_FLAG_INDEX) | (bad ? DAD3D_BAKE_FLAG_NONFINITE : 0);
    int4 win = make_int4(0, 0, 0, 0);
    if (!flag) {
        int h, w;
        frame_hw(a.frames, f, h, w);
        const float fx0 = fmaxf(floorf(lo_x), 0.0f), fx1 = fminf(ceilf(hi_x), (float)(w - 1));
        const float fy0 = fmaxf(floorf(lo_y), 0.0f), fy1 = fminf(ceilf(hi_y), (float)(h - 1));
        if (fx0 <= fx1 && fy0 <= fy1) {  // else outside its frame (or a mesh without vertices): an ordinary outcome
            const float fw = fx1 - fx0 + 1.0f, fh = fy1 - fy0 + 1.0f;  // exact wherever they are <= D
            if (fw > (float)a.depth_side || fh > (float)a.depth_side) flag |= DAD3D_BAKE_FLAG_DEPTH_WINDOW;
            // the origin stays 4096 below INT_MAX (a float of a frame more than 2^31 - 64 pixels wide rounds up to 2^31): x0 + ww fits
            else win = make_int4((int)fminf(fx0, 2147479552.0f), (int)fminf(fy0, 2147479552.0f), (int)fw, (int)fh);
        }
    }
    a.flags[k] = flag;
    int* wp = a.window + 4 * (size_t)k;  // four dword stores: the table need not be 16-byte aligned
    wp[0] = win.x, wp[1] = win.y, wp[2] = win.z, wp[3] = win.w;
}

__global__ __launch_bounds__(kThreads) void depth_clear_kernel(UvDepthFramesArgs a) {
    const int k = blockIdx.y, D = a.depth_side;
    const int4 win = load_window(a.window, k);
    const int ww = min(win.z, D), wh = min(win.w, D);
    if (ww <= 0 || wh <= 0) return;
    float* map = a.depth + (size_t)k * D * D;
    const unsigned n = (unsigned)ww * (unsigned)wh;
    for (unsigned p = blockIdx.x * kThreads + threadIdx.x; p < n; p += gridDim.x * kThreads) {
        const unsigned j = p / (unsigned)ww, i = p - j * (unsigned)ww;
        map[(size_t)j * D + i] = INFINITY;
    }
}

__global__ __launch_bounds__(kThreads) void depth_raster_kernel(UvDepthFramesArgs a) {
    const int k = blockIdx.y, D = a.depth_side, lane = threadIdx.x & 63;
    const int4 win = load_window(a.window, k);
    const int ww = min(win.z, D), wh = min(win.w, D);
    const int f = a.image_index[k];
    if (ww <= 0 || wh <= 0 || win.x < 0 || win.y < 0 || f < 0 || f >= a.n_frames) return;  // workgroup-uniform
    int h, w;
    frame_hw(a.frames, f, h, w);
    // the pixels a store may reach, inclusive: the window inside the frame
    const int wx0 = win.x, wy0 = win.y, wx1 = min(wx0 + ww - 1, w - 1), wy1 = min(wy0 + wh - 1, h - 1);
    float* map = a.depth + (size_t)k * D * D;
    const float* vb = a.vertices + (size_t)k * a.n_verts * 3;

    // one pixel test: is_point_in_tri, get_point_weight's weights, the reference's `>` against -1e8 on the negated depth
    auto test_pixel = [&](const TriSetup& ts, float z0, float z1, float z2, int x, int y) {
        float u, v;
        tri_uv(ts, (float)x, (float)y, u, v);
        if (!(u >= 0.0f && v >= 0.0f && (u + v < 1.0f))) return;
        const float w0 = 1.0f - u - v;
        const float z = (w0 * z0 + v * z1 + u * z2) + 0.0f;  // -0 -> +0
        if (!(z < 1e8f)) return;                             // NaN never passes
        float* p = map + (size_t)(y - wy0) * D + (x - wx0);
        // no read in front of the atomic to spare it for a fragment behind what is there: the load's latency in every lane's serial walk
        // cost more than the atomics it saved (depth_frames 434 us against 231 us on the bench of DESIGN section 4.30)
        if (z >= 0.0f) (void)__hip_atomic_fetch_min(reinterpret_cast<int*>(p), __float_as_int(z), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else (void)__hip_atomic_fetch_max(reinterpret_cast<unsigned*>(p), __float_as_uint(z), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };

    const int t = blockIdx.x * kThreads + threadIdx.x;
    const bool have = t < a.n_tri;
    float x0 = 0.f, y0 = 0.f, z0 = 0.f, x1 = 0.f, y1 = 0.f, z1 = 0.f, x2 = 0.f, y2 = 0.f, z2 = 0.f;
    int bx0 = 1, bx1 = 0, by0 = 1, by1 = 0;
    if (have) {
        const int i0 = a.faces[3 * t], i1 = a.faces[3 * t + 1], i2 = a.faces[3 * t + 2];
        x0 = vb[3 * i0], y0 = vb[3 * i0 + 1], z0 = vb[3 * i0 + 2];
        x1 = vb[3 * i1], y1 = vb[3 * i1 + 1], z1 = vb[3 * i1 + 2];
        x2 = vb[3 * i2], y2 = vb[3 * i2 + 1], z2 = vb[3 * i2 + 2];
        // the box of rasterize_kernel.cpp:321-325, then clipped to what the window holds
        bx0 = max(max(f2i_x86(ceilf(std_min(x0, std_min(x1, x2)))), 0), wx0);
        bx1 = min(min(f2i_x86(floorf(std_max(x0, std_max(x1, x2)))), w - 1), wx1);
        by0 = max(max(f2i_x86(ceilf(std_min(y0, std_min(y1, y2)))), 0), wy0);
        by1 = min(min(f2i_x86(floorf(std_max(y0, std_max(y1, y2)))), h - 1), wy1);
    }
    const bool ok = have && bx0 <= bx1 && by0 <= by1;
    const int area = ok ? (bx1 - bx0 + 1) * (by1 - by0 + 1) : 0;  // at most D * D
    const bool big = area > kLaneBoxPixels;
    if (ok && !big) {
        const TriSetup ts = tri_setup(x0, y0, x1, y1, x2, y2);
        for (int y = by0; y <= by1; ++y)
            for (int x = bx0; x <= bx1; ++x) test_pixel(ts, z0, z1, z2, x, y);
    }
    unsigned long long todo = __ballot(big);
    while (todo) {  // wave-uniform: one large box at a time, all 64 lanes on its pixels
        const int j = __builtin_ctzll(todo);
        todo &= todo - 1;
        auto bf = [&](float v) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j)); };
        auto bi = [&](int v) { return __builtin_amdgcn_readlane(v, j); };
        const TriSetup ts = tri_setup(bf(x0), bf(y0), bf(x1), bf(y1), bf(x2), bf(y2));
        const float wz0 = bf(z0), wz1 = bf(z1), wz2 = bf(z2);
        const int ox = bi(bx0), oy = bi(by0);
        const unsigned bw = (unsigned)(bi(bx1) - ox + 1), warea = (unsigned)bi(area);
        for (unsigned p = lane; p < warea; p += 64) {
            const unsigned py = p / bw, px = p - py * bw;
            test_pixel(ts, wz0, wz1, wz2, ox + (int)px, oy + (int)py);
        }
    }
}

__global__ __launch_bounds__(kThreads) void bake_frames_occluded_kernel(UvBakeOccludedArgs o) {
    const UvBakeFramesArgs& a = o.bake;
    const int k = blockIdx.y;
    const int f = a.image_index[k];
    const bool has_frame = f >= 0 && f < a.n_frames;
    const int flag = o.depth_flags[k] | (has_frame ? 0 : DAD3D_BAKE_FLAG_INDEX);
    if (blockIdx.x == 0 && threadIdx.x == 0) a.flags[k] = flag;
    if (flag && a.score) return;  // accumulate: a flagged head changes no byte of its texture or score
    const int n_tex = a.size * a.size;
    const int t0 = (blockIdx.x * kThreads + threadIdx.x) * kTexels;
    if (t0 >= n_tex) return;
    const int nt = min(kTexels, n_tex - t0);
    // the frame entry, as bake_frames_kernel reads it
    const uint8_t* img = nullptr;
    long long stride = 0;
    int h = 0, w = 0;
    if (!flag) {
        const long long* fr = a.frames + 4 * (size_t)f;
        const long long fh = fr[1], fw = fr[2];
        if (fr[0] != 0 && fh >= 1 && fw >= 1 && fh <= INT_MAX && fw <= INT_MAX && fr[3] >= 3 * fw)
            img = reinterpret_cast<const uint8_t*>(fr[0]), h = (int)fh, w = (int)fw, stride = fr[3];
    }
    const int D = o.depth_side;
    const int4 win = load_window(o.window, k);
    const int ww = min(win.z, D), wh = min(win.w, D);  // no read outside the map, whatever the window says
    const float* map = o.depth + (size_t)k * D * D;
    const float* vb = a.vertices + (size_t)k * a.n_verts * 3;
    const double* nb = a.normals + (size_t)k * a.n_verts * 3;
    int ry = 0, rx = 0;  // the rounded pixel of the candidate uv_sample accepted
    auto pixel_at = [&](int y, int x) {
        ry = y, rx = x;
        return img + (long long)y * stride + 3ll * x;
    };
    unsigned rgb[kTexels];
    float s[kTexels];
    bool hit[kTexels];
#pragma unroll
    for (int i = 0; i < kTexels; ++i) {
        int px = -1;
        double ndv = 0.0;
        if (i < nt && w > 0) {
            const int end = a.texel_ptr[t0 + i + 1];
            for (int j = a.texel_ptr[t0 + i]; px < 0 && j < end; ++j) {
                const UvCand c = uv_load_cand(a.cand_verts, a.cand_bary, j);
                px = uv_sample(c, vb, nb, h, w, pixel_at, ndv);
                if (px < 0) continue;
                const long long dx = (long long)rx - win.x, dy = (long long)ry - win.y;
                const float d = (dx >= 0 && dx < ww && dy >= 0 && dy < wh) ? map[(size_t)dy * D + dx] : INFINITY;
                if (uv_hidden(c, vb, nb, ndv, d, o.depth_bias, o.slope_bias)) px = -1;  // skipped like a back-facing one: the walk goes on
            }
        }
        hit[i] = px >= 0;
        rgb[i] = hit[i] ? (unsigned)px : 0u;
        s[i] = (float)ndv;  // float64 -> float32, round to nearest even
    }
    uint8_t* out = a.texture + ((size_t)k * n_tex + t0) * 3;
    if (a.score) {
        float* sc = a.score + (size_t)k * n_tex + t0;
#pragma unroll
        for (int i = 0; i < kTexels; ++i)
            if (i < nt && hit[i] && s[i] > sc[i]) {  // strict: a tie keeps the older sample; NaN > x is false
                sc[i] = s[i];
                out[3 * i] = rgb[i] & 255, out[3 * i + 1] = (rgb[i] >> 8) & 255, out[3 * i + 2] = rgb[i] >> 16;
            }
        return;
    }
    if (nt == kTexels && (reinterpret_cast<uintptr_t>(out) & 3) == 0) {
        // 4 texels r g b r | g b r g | b r g b as three little-endian dwords
        const unsigned d0 = rgb[0] | (rgb[1] << 24);
        const unsigned d1 = (rgb[1] >> 8) | (rgb[2] << 16);
        const unsigned d2 = (rgb[2] >> 16) | (rgb[3] << 8);
        *reinterpret_cast<uint3*>(out) = make_uint3(d0, d1, d2);
    } else {
#pragma unroll
        for (int i = 0; i < kTexels; ++i)
            if (i < nt) out[3 * i] = rgb[i] & 255, out[3 * i + 1] = (rgb[i] >> 8) & 255, out[3 * i + 2] = rgb[i] >> 16;
    }
}

}  // namespace

dad3d_status launch_uv_depth_frames(const UvDepthFramesArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(depth_window_kernel, dim3(a.n_heads), dim3(kThreads), 0, s, a);
    DAD3D_HIP_TRY(hipGetLastError());
    const int side = a.depth_side;
    const int clear_blocks = max(1, (side * side + kThreads * kClearPerLane - 1) / (kThreads * kClearPerLane));
    hipLaunchKernelGGL(depth_clear_kernel, dim3(clear_blocks, a.n_heads), dim3(kThreads), 0, s, a);
    DAD3D_HIP_TRY(hipGetLastError());
    if (a.n_tri == 0) return DAD3D_OK;
    hipLaunchKernelGGL(depth_raster_kernel, dim3((a.n_tri + kThreads - 1) / kThreads, a.n_heads), dim3(kThreads), 0, s, a);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

dad3d_status launch_uv_bake_frames_occluded(const UvBakeOccludedArgs& a, hipStream_t s) {
    const int lanes = (a.bake.size * a.bake.size + kTexels - 1) / kTexels;
    const dim3 grid((lanes + kThreads - 1) / kThreads, a.bake.n_heads);
    hipLaunchKernelGGL(bake_frames_occluded_kernel, grid, dim3(kThreads), 0, s, a);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

}  // namespace dad3d
