// Textured heads into frames: the tile kernel of the frames chain (sim3dr_frames.hip) with the pixel test and the resolve of the
// textured render (sim3dr_kernels.hip `render_texture_kernel`, _render_texture_core, rasterize_kernel.cpp:358-463).
//
// Per frame, in ascending head order:  frame = (unsigned char) _render_texture_core(image = float(frame), vertices[k], ..,
// texture[k], a fresh depth buffer at -1e8). A later head paints over an earlier one wherever it covers a pixel; an uncovered pixel is
// not written.
//
// THIS FILE IS COMPILED WITH -ffp-contract=off (sim3dr_math.hpp).
//
// The first six launches are build_frame_lists, unchanged; the walk and the 64-bit key of this kernel are frames_tile_kernel's
//     head + 1 (16 bits) | orderable depth (32 bits) | 0xFFFE - triangle (16 bits)
// (a small box by its lane, a large one by the wave, 32 KiB of keys in LDS). What differs:
//   * coverage (:423): is_point_in_tri (u >= 0, v >= 0, u + v < 1) OR the pixel lies in the two-pixel border band of the FRAME
//     (x < 2 || x > w - 3 || y < 2 || y > h - 3), where every triangle whose box reaches the pixel competes with extrapolated weights.
//     Reference behaviour, kept on purpose; it only matters for a head whose triangle boxes reach the frame's outer two pixels.
//   * resolve (:430-453): tex_p = tex_p0 * w0 + tex_p1 * w1 + tex_p2 * w2, clamped with std::max(std::min(.)), nearest (roundf) or
//     bilinear (floor / ceil indices), every operation rounded on its own; the indices are clamped into the texture after conversion.
//     Three single-byte stores per pixel, (unsigned char) of the float; no byte outside [row, row + 3 w) of a row is touched.
#include "common.hpp"
#include "sim3dr_frames.hpp"
#include "sim3dr_math.hpp"

namespace dad3d {
namespace {

struct FrameTextureArgs {
    MeshDev m;
    FrameScratch sc;
    const long long* frames;
    int n_frames;
    const float* vertices;
    const float4* tex_tri;   // [ntri][2]  x0 y0 x1 y1 | x2 y2 - -  (dad3d_mesh_set_texcoords, either indexing mode)
    const void* texture;     // [N or 1][tex_h][tex_w][tex_c]  TEX
    size_t tex_head_stride;  // elements between two heads' textures; 0: one texture for all
    int tex_h, tex_w, tex_c, nearest;
};

__device__ __forceinline__ int texel_index(float t, int size) {  // (int) of an already rounded coordinate, kept inside the texture
    return min(max(f2i_x86(t), 0), size - 1);
}

template <class TEX>
__global__ __launch_bounds__(kFrameThreads) void frames_texture_tile_kernel(FrameTextureArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned long long keys[kFrameTile * kFrameTile];
    const int tid = threadIdx.x;
    const unsigned n_items = *a.sc.n_items;
    const size_t head_floats = (size_t)a.m.nver * 3;  // the resolve's
    for (unsigned item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int g = (int)a.sc.items[item];
        const FrameTile ft = frame_tile(a.sc, a.frames, a.n_frames, g);
        const FrameShape& fs = ft.fs;
        const int f = ft.f, px0 = ft.px0, py0 = ft.py0, px1 = ft.px1, py1 = ft.py1;
        for (int p = tid; p < kFrameTile * kFrameTile; p += kFrameThreads) keys[p] = 0ull;  // 0: no fragment (a head's keys start at 1 << 48)
        __syncthreads();

        // one pixel test: is_point_in_tri or the frame's border band, get_point_weight's weights, `>` against the head's own -1e8
        auto test_pixel = [&](const TriSetup& ts, float z0, float z1, float z2, unsigned long long key_hi, unsigned key_lo, int x, int y) {
            float u, v;
            tri_uv(ts, (float)x, (float)y, u, v);
            const bool band = x < 2 || x > fs.w - 3 || y < 2 || y > fs.h - 3;
            if (!(band || (u >= 0.0f && v >= 0.0f && (u + v < 1.0f)))) return;
            const float w0 = 1.0f - u - v;
            const float z = w0 * z0 + v * z1 + u * z2;
            if (!(z > -1e8f)) return;  // a fresh depth buffer per head; NaN never passes `>`
            const unsigned long long key = key_hi | ((unsigned long long)depth_order_number(z) << 16) | key_lo;
            (void)__hip_atomic_fetch_max(&keys[(y - py0) * kFrameTile + (x - px0)], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        };

        walk_frame_tile(a.m, a.sc, a.vertices, g, ft, test_pixel);
        __syncthreads();

        // resolve: every won pixel samples its head's texture once from its winner's weights and is written with three byte stores
        const long long addr = a.frames[4 * (size_t)f], stride = a.frames[4 * (size_t)f + 3];
        const int tw = px1 - px0 + 1, th = py1 - py0 + 1;
        const int tex_h = a.tex_h, tex_w = a.tex_w, tex_c = a.tex_c;
        const float xmax = (float)(tex_w - 1), ymax = (float)(tex_h - 1);
        for (int p = tid; p < kFrameTile * th; p += kFrameThreads) {
            const int ly = p >> kFrameTileShift, lx = p & (kFrameTile - 1);
            if (lx >= tw) continue;
            const unsigned long long key = keys[p];
            if (!key) continue;  // no head covers the pixel: its bytes are not touched
            const unsigned k = (unsigned)(key >> 48) - 1u, t = 0xFFFEu - (unsigned)(key & 0xffffu);
            const float* vb = a.vertices + k * head_floats;
            const TEX* tex = static_cast<const TEX*>(a.texture) + k * a.tex_head_stride;
            const int i0 = a.m.tri[3 * t], i1 = a.m.tri[3 * t + 1], i2 = a.m.tri[3 * t + 2];
            const float4 ta = a.tex_tri[2 * (size_t)t], tb = a.tex_tri[2 * (size_t)t + 1];
            const TriSetup ts = tri_setup(vb[3 * i0], vb[3 * i0 + 1], vb[3 * i1], vb[3 * i1 + 1], vb[3 * i2], vb[3 * i2 + 1]);
            const int gx = px0 + lx, gy = py0 + ly;
            float u, v;
            tri_uv(ts, (float)gx, (float)gy, u, v);
            const float w0 = 1.0f - u - v;
            float tx = ta.x * w0 + ta.z * v + tb.x * u;
            float ty = ta.y * w0 + ta.w * v + tb.y * u;
            tx = std_max(std_min(tx, xmax), 0.0f);
            ty = std_max(std_min(ty, ymax), 0.0f);
            uint8_t* out = reinterpret_cast<uint8_t*>(addr + (long long)gy * stride + 3ll * gx);
            auto texel = [&](int y, int x, int ch) { return (float)tex[((size_t)y * tex_w + x) * tex_c + ch]; };
            if (a.nearest) {
                const int y = texel_index(roundf(ty), tex_h), x = texel_index(roundf(tx), tex_w);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) out[ch] = (uint8_t)(f2i_x86(texel(y, x, ch)) & 0xff);  // (unsigned char) of the float
            } else {
                const float fy = floorf(ty), fx = floorf(tx);
                const float yd = ty - fy, xd = tx - fx;
                const int yf = texel_index(fy, tex_h), yc = texel_index(ceilf(ty), tex_h);
                const int xf = texel_index(fx, tex_w), xc = texel_index(ceilf(tx), tex_w);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const float ul = texel(yf, xf, ch), ur = texel(yf, xc, ch), dl = texel(yc, xf, ch), dr = texel(yc, xc, ch);
                    const float val = ul * (1.0f - xd) * (1.0f - yd) + ur * xd * (1.0f - yd) + dl * (1.0f - xd) * yd + dr * xd * yd;
                    out[ch] = (uint8_t)(f2i_x86(val) & 0xff);
                }
            }
        }
        __syncthreads();  // the keys are reused by the next item
    }
}

}  // namespace

dad3d_status launch_render_texture_frames(const MeshDev& m, void* scratch, const int64_t* frames, int n_frames, int total_tiles,
                                          const float* vertices, const float4* tex_tri, const void* texture, int texture_u8, size_t tex_head_stride,
                                          int tex_h, int tex_w, int tex_c, int nearest, const int32_t* image_index, int n_heads, int32_t* flags,
                                          hipStream_t s) {
    FrameScratch sc;
    int tile_blocks = 0;
    if (dad3d_status st = build_frame_lists(m, scratch, frames, n_frames, total_tiles, vertices, image_index, n_heads, flags, s, &sc, &tile_blocks)) return st;
    const FrameTextureArgs a{m, sc, reinterpret_cast<const long long*>(frames), n_frames, vertices, tex_tri, texture, tex_head_stride,
                             tex_h, tex_w, tex_c, nearest};
    if (texture_u8) hipLaunchKernelGGL(frames_texture_tile_kernel<uint8_t>, dim3(tile_blocks), dim3(kFrameThreads), 0, s, a);
    else hipLaunchKernelGGL(frames_texture_tile_kernel<float>, dim3(tile_blocks), dim3(kFrameThreads), 0, s, a);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

}  // namespace dad3d
