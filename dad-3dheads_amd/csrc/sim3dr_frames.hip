// Sim3DR into frames: the heads of a call, each with the frame it belongs to, drawn into frames of any sizes in one chain.
//
// Replaces a Python loop over the heads of `Sim3DR.rasterize(vertices, triangles, colors, bg=frame)` (Sim3DR/Sim3DR.py:14-29 around
// _rasterize, rasterize_kernel.cpp:219-292), and for dad3d_mesh_render_frames RenderPipeline.__call__ (lighting.py:37-71) per head.
// Every call of that loop starts from a z-buffer of -1e8 (Sim3DR.py:23), so head k paints over every head before it wherever it
// covers a pixel, whatever the depths; within a head the deepest fragment wins, and among equal depths the lowest triangle.
//
// THIS FILE IS COMPILED WITH -ffp-contract=off (sim3dr_math.hpp): the per-pixel arithmetic is that of sim3dr_kernels.hip.
//
// Painter's order without a sequence: the pixel of a frame belongs to the maximum of the 64-bit key
//     head + 1 (16 bits) | orderable depth (32 bits) | 0xFFFE - triangle (16 bits)
// over all fragments of all heads of that frame. A maximum does not depend on the order of its operands, so the lists below
// may be filled and walked in any order: no atomics on image bytes, and the same bytes whatever the scheduling.
//
// The chain, seven launches whatever N, M and the frame shapes:
//   frames_setup   zeroes the counters; block 0 turns the device frame table into frame_base[M + 1], the first 64 x 64 tile of
//                  every frame in one numbering of all tiles
//   frames_box     per (head, triangle): the screen box of rasterize_kernel.cpp:246-254 clipped to the head's frame, as a box of
//                  tiles; the head's number of (tile, triangle) entries
//   frames_plan    heads in ascending order take their entries from one pool of 4 * ntri * N; a head that does not fit any more
//                  is dropped whole (DAD3D_FRAME_FLAG_CAPACITY), a head without a frame gets DAD3D_FRAME_FLAG_INDEX
//   frames_bin<0>  the drawn heads' entries per tile, counted
//   frames_scan    list offsets (exclusive sums of the counts) and the list of non-empty tiles
//   frames_bin<1>  the lists: head << 16 | triangle
//   frames_tile    a workgroup per non-empty tile: keys in LDS, ds_max_u64 per fragment, then every won pixel is shaded once from
//                  its winning (head, triangle) and written with three byte stores -- no byte outside [row, row + 3 w) is touched
#include <algorithm>

#include "collectives.hpp"
#include "common.hpp"
#include "sim3dr_frames.hpp"
#include "sim3dr_math.hpp"

namespace dad3d {
namespace {

__global__ __launch_bounds__(kFrameThreads) void frames_setup_kernel(FrameScratch sc, const long long* frames, int n_frames, int n_heads) {
    __shared__ int red[kFrameWaves];
    const int tid = threadIdx.x;
    const size_t gid = (size_t)blockIdx.x * kFrameThreads + tid, gstride = (size_t)gridDim.x * kFrameThreads;
    for (size_t i = gid; i < (size_t)n_heads; i += gstride) sc.need[i] = 0;
    for (size_t i = gid; i < (size_t)sc.total_tiles; i += gstride) sc.tile_count[i] = 0;
    if (blockIdx.x != 0) return;
    if (tid == 0) *sc.n_items = 0;
    // a thread takes a run of frames: at most 65535 frames of at most 4096 tiles, the sums stay below 2^28
    const int per = (n_frames + kFrameThreads - 1) / kFrameThreads;
    const int f0 = min(tid * per, n_frames), f1 = min(f0 + per, n_frames);
    int sum = 0;
    for (int f = f0; f < f1; ++f) sum += frame_shape(frames, f).tiles;
    int total;
    int run = block_exclusive_scan<kFrameWaves>(sum, red, total);
    // clamped to the host's total: a device table that disagrees with the host's shapes cannot make a tile index leave the scratch
    // (frames_box draws into a frame only if frame_base[f + 1] - frame_base[f] is its tile count)
    for (int f = f0; f < f1; ++f) {
        sc.frame_base[f] = min(run, sc.total_tiles);
        run += frame_shape(frames, f).tiles;
    }
    if (tid == 0) sc.frame_base[n_frames] = min(total, sc.total_tiles);
}

__global__ __launch_bounds__(kFrameThreads) void frames_box_kernel(MeshDev m, FrameScratch sc, const long long* frames, int n_frames,
                                                                   const float* vertices, const int* image_index) {
    const int k = blockIdx.y, t = blockIdx.x * kFrameThreads + threadIdx.x;
    const int f = image_index[k];
    if (f < 0 || f >= n_frames) return;  // block-uniform; frames_plan flags the head
    const FrameShape fs = frame_shape(frames, f);
    const bool frame_ok = fs.tiles > 0 && sc.frame_base[f + 1] - sc.frame_base[f] == fs.tiles;
    unsigned cnt = 0;
    if (t < m.ntri) {
        uint2 box = make_uint2(1u, 1u);  // empty
        if (frame_ok) {
            const float* vb = vertices + (size_t)k * m.nver * 3;
            const int i0 = m.tri[3 * t], i1 = m.tri[3 * t + 1], i2 = m.tri[3 * t + 2];
            const float x0 = vb[3 * i0], y0 = vb[3 * i0 + 1];
            const float x1 = vb[3 * i1], y1 = vb[3 * i1 + 1];
            const float x2 = vb[3 * i2], y2 = vb[3 * i2 + 1];
            // bounding box exactly as rasterize_kernel.cpp:246-254
            const int bx0 = max(f2i_x86(ceilf(std_min(x0, std_min(x1, x2)))), 0);
            const int bx1 = min(f2i_x86(floorf(std_max(x0, std_max(x1, x2)))), fs.w - 1);
            const int by0 = max(f2i_x86(ceilf(std_min(y0, std_min(y1, y2)))), 0);
            const int by1 = min(f2i_x86(floorf(std_max(y0, std_max(y1, y2)))), fs.h - 1);
            if (bx0 <= bx1 && by0 <= by1) {  // else `continue` in the reference
                const unsigned tx0 = bx0 >> kFrameTileShift, tx1 = bx1 >> kFrameTileShift;
                const unsigned ty0 = by0 >> kFrameTileShift, ty1 = by1 >> kFrameTileShift;
                box = make_uint2(tx0 | (tx1 << 16), ty0 | (ty1 << 16));  // a frame has at most 4096 tiles: 12 bits each
                cnt = (tx1 - tx0 + 1) * (ty1 - ty0 + 1);
            }
        }
        sc.tri_box[(size_t)k * m.ntri + t] = box;
    }
    cnt = wave_sum(cnt);  // at most 4096 tiles x 65535 triangles a head: below 2^28
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&sc.need[k], cnt);
}

// One workgroup. If all heads fit the pool together nobody is dropped; otherwise the heads are admitted in ascending order by one
// thread (the rule is sequential: whether a head fits depends on which heads before it did).
__global__ __launch_bounds__(kPlanThreads) void frames_plan_kernel(FrameScratch sc, const int* image_index, int n_frames, int n_heads, int* flags) {
    __shared__ unsigned long long red[kPlanWaves];
    const int tid = threadIdx.x;
    unsigned long long sum = 0;
    for (int k = tid; k < n_heads; k += kPlanThreads) sum += sc.need[k];  // a head without a frame has none
    const unsigned long long total = block_sum<kPlanWaves>(sum, red);
    auto has_frame = [&](int k) {
        const int f = image_index[k];
        return f >= 0 && f < n_frames;
    };
    if (total <= sc.pool_entries) {
        for (int k = tid; k < n_heads; k += kPlanThreads) flags[k] = has_frame(k) ? 0 : DAD3D_FRAME_FLAG_INDEX;
        return;
    }
    if (tid != 0) return;
    unsigned used = 0;
    for (int k = 0; k < n_heads; ++k) {
        const unsigned need = sc.need[k];
        int flag = 0;
        if (!has_frame(k)) flag = DAD3D_FRAME_FLAG_INDEX;
        else if (need > sc.pool_entries - used) flag = DAD3D_FRAME_FLAG_CAPACITY;
        else used += need;
        flags[k] = flag;
    }
}

// FILL 0: count the entries of every tile. FILL 1: write them (tile_count is the cursor and ends where the count left it).
template <int FILL>
__global__ __launch_bounds__(kFrameThreads) void frames_bin_kernel(int ntri, FrameScratch sc, const long long* frames, const int* image_index,
                                                                   const int* flags) {
    const int k = blockIdx.y, t = blockIdx.x * kFrameThreads + threadIdx.x;
    if (flags[k] || t >= ntri) return;
    const uint2 box = sc.tri_box[(size_t)k * ntri + t];
    const unsigned tx0 = box.x & 0xffff, tx1 = box.x >> 16, ty0 = box.y & 0xffff, ty1 = box.y >> 16;
    if (tx0 > tx1) return;
    const int f = image_index[k];  // in range: the head has no flag
    const unsigned base = (unsigned)sc.frame_base[f], tiles_x = (unsigned)frame_shape(frames, f).tiles_x;
    for (unsigned ty = ty0; ty <= ty1; ++ty)
        for (unsigned tx = tx0; tx <= tx1; ++tx) {
            const unsigned g = base + ty * tiles_x + tx;
            const unsigned slot = atomicAdd(&sc.tile_count[g], 1u);
            if (FILL) {
                const unsigned at = sc.tile_off[g] + slot;
                if (at < sc.pool_entries) sc.pool[at] = ((unsigned)k << 16) | (unsigned)t;  // always: frames_plan admitted the head
            }
        }
}

// One workgroup: exclusive sums of the tile counts, the list of non-empty tiles, and the counts back to zero for the fill.
__global__ __launch_bounds__(kPlanThreads) void frames_scan_kernel(FrameScratch sc) {
    __shared__ int red[kPlanWaves];
    const int tid = threadIdx.x, T = sc.total_tiles;
    const int per = (T + kPlanThreads - 1) / kPlanThreads;
    const int g0 = min(tid * per, T), g1 = min(g0 + per, T);
    int sum = 0, filled = 0;
    for (int g = g0; g < g1; ++g) {
        const unsigned c = sc.tile_count[g];
        sum += (int)c, filled += c ? 1 : 0;  // the sum is at most the pool: 4 * 65535 * 65535 does not fit, the launcher caps the pool at 2^31 - 1
    }
    int total, n_filled;
    int run = block_exclusive_scan<kPlanWaves>(sum, red, total);
    int at = block_exclusive_scan<kPlanWaves>(filled, red, n_filled);
    for (int g = g0; g < g1; ++g) {
        const unsigned c = sc.tile_count[g];
        sc.tile_off[g] = (unsigned)run;
        run += (int)c;
        if (c) sc.items[at++] = (unsigned)g;
        sc.tile_count[g] = 0;
    }
    if (tid == 0) sc.tile_off[T] = (unsigned)total, *sc.n_items = (unsigned)n_filled;
}

struct FrameTileArgs {
    MeshDev m;
    FrameScratch sc;
    const long long* frames;
    int n_frames;
    const float* vertices;
    const float* colors;
    int reverse;
};

__global__ __launch_bounds__(kFrameThreads) void frames_tile_kernel(FrameTileArgs a) {
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

        // one pixel test: the arithmetic of _rasterize (get_point_weight, strict interior, `>` against the head's own -1e8)
        auto test_pixel = [&](const TriSetup& ts, float z0, float z1, float z2, unsigned long long key_hi, unsigned key_lo, int x, int y) {
            float u, v;
            tri_uv(ts, (float)x, (float)y, u, v);
            const float w0 = 1.0f - u - v;
            if (!(u > 0.0f && v > 0.0f && w0 > 0.0f)) return;
            const float z = w0 * z0 + v * z1 + u * z2;
            if (!(z > -1e8f)) return;  // Sim3DR.py:23: every head starts from -1e8; NaN never passes `>`
            const unsigned long long key = key_hi | ((unsigned long long)depth_order_number(z) << 16) | key_lo;
            (void)__hip_atomic_fetch_max(&keys[(y - py0) * kFrameTile + (x - px0)], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        };

        walk_frame_tile(a.m, a.sc, a.vertices, g, ft, test_pixel);
        __syncthreads();

        // resolve: every won pixel is shaded once from its winner and written with three byte stores
        const long long addr = a.frames[4 * (size_t)f], stride = a.frames[4 * (size_t)f + 3];
        const int tw = px1 - px0 + 1, th = py1 - py0 + 1;
        for (int p = tid; p < kFrameTile * th; p += kFrameThreads) {
            const int ly = p >> kFrameTileShift, lx = p & (kFrameTile - 1);
            if (lx >= tw) continue;
            const unsigned long long key = keys[p];
            if (!key) continue;  // no head covers the pixel: its bytes are not touched
            const unsigned k = (unsigned)(key >> 48) - 1u, t = 0xFFFEu - (unsigned)(key & 0xffffu);
            const float* vb = a.vertices + k * head_floats;
            const float* cb = a.colors + k * head_floats;
            const int i0 = a.m.tri[3 * t], i1 = a.m.tri[3 * t + 1], i2 = a.m.tri[3 * t + 2];
            const TriSetup ts = tri_setup(vb[3 * i0], vb[3 * i0 + 1], vb[3 * i1], vb[3 * i1 + 1], vb[3 * i2], vb[3 * i2 + 1]);
            const int gx = px0 + lx, gy = py0 + ly;
            float u, v;
            tri_uv(ts, (float)gx, (float)gy, u, v);
            const float w0 = 1.0f - u - v;
            const int row = a.reverse ? (fs.h - 1 - gy) : gy;
            uint8_t* px = reinterpret_cast<uint8_t*>(addr + (long long)row * stride + 3ll * gx);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float cv = w0 * cb[3 * i0 + ch] + v * cb[3 * i1 + ch] + u * cb[3 * i2 + ch];
                // (unsigned char)((1 - alpha) * old + alpha * 255 * col) with alpha == 1: the old value only contributes +0.0f
                px[ch] = (uint8_t)(f2i_x86(0.0f + 255.0f * cv) & 0xff);
            }
        }
        __syncthreads();  // the keys are reused by the next item
    }
}

}  // namespace

dad3d_status frames_check_shapes(const char* who, const int64_t* frames_host, int n_frames, int* total_tiles) {
    long long total = 0;
    for (int f = 0; f < n_frames; ++f) {
        const int64_t addr = frames_host[4 * (size_t)f], h = frames_host[4 * (size_t)f + 1], w = frames_host[4 * (size_t)f + 2],
                      stride = frames_host[4 * (size_t)f + 3];
        DAD3D_REQUIRE(addr != 0, "%s: frame %d has no address", who, f);
        DAD3D_REQUIRE(h >= 1 && w >= 1 && h <= (1 << 24) && w <= (1 << 24), "%s: frame %d is %lld x %lld pixels", who, f, (long long)h, (long long)w);
        DAD3D_REQUIRE(stride >= 3 * w, "%s: frame %d has a row stride of %lld bytes for %lld pixels of 3 bytes", who, f, (long long)stride,
                      (long long)w);
        const long long tiles = ((h + kFrameTile - 1) / kFrameTile) * ((w + kFrameTile - 1) / kFrameTile);
        DAD3D_REQUIRE(tiles <= DAD3D_FRAME_MAX_TILES, "%s: frame %d of %lld x %lld pixels has %lld tiles of %d x %d pixels, more than %d", who, f,
                      (long long)h, (long long)w, tiles, kFrameTile, kFrameTile, DAD3D_FRAME_MAX_TILES);
        total += tiles;
    }
    DAD3D_REQUIRE(total < (1ll << 24), "%s: %lld tiles in all frames, 2^24 or more", who, total);
    *total_tiles = (int)total;
    return DAD3D_OK;
}

size_t frames_scratch_bytes(int ntri, int n_frames, int n_heads, int total_tiles) {
    return FrameLayout(ntri, n_frames, n_heads, total_tiles).total;
}

dad3d_status build_frame_lists(const MeshDev& m, void* scratch, const int64_t* frames, int n_frames, int total_tiles, const float* vertices,
                               const int32_t* image_index, int n_heads, int32_t* flags, hipStream_t s, FrameScratch* lists, int* tile_blocks) {
    static int cus = 0;  // the same for every device of the node (one GPU model)
    if (!cus) {
        int dev = 0, n = 0;
        DAD3D_HIP_TRY(hipGetDevice(&dev));
        DAD3D_HIP_TRY(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
        cus = std::max(n, 1);
    }
    const FrameLayout lay(m.ntri, n_frames, n_heads, total_tiles);
    char* base = static_cast<char*>(scratch);
    const FrameScratch sc{reinterpret_cast<int*>(base + lay.frame_base),
                          reinterpret_cast<unsigned*>(base + lay.need),
                          reinterpret_cast<uint2*>(base + lay.tri_box),
                          reinterpret_cast<unsigned*>(base + lay.tile_count),
                          reinterpret_cast<unsigned*>(base + lay.tile_off),
                          reinterpret_cast<unsigned*>(base + lay.items),
                          reinterpret_cast<unsigned*>(base + lay.n_items),
                          reinterpret_cast<unsigned*>(base + lay.pool),
                          lay.pool_entries,
                          total_tiles};
    const long long* table = reinterpret_cast<const long long*>(frames);
    const int zero_blocks = std::max(1, std::min(4 * cus, (std::max(total_tiles, n_heads) + kFrameThreads - 1) / kFrameThreads));
    hipLaunchKernelGGL(frames_setup_kernel, dim3(zero_blocks), dim3(kFrameThreads), 0, s, sc, table, n_frames, n_heads);
    const dim3 tri_grid(std::max(1, (m.ntri + kFrameThreads - 1) / kFrameThreads), n_heads);  // no triangles: the flags are still written
    hipLaunchKernelGGL(frames_box_kernel, tri_grid, dim3(kFrameThreads), 0, s, m, sc, table, n_frames, vertices, image_index);
    hipLaunchKernelGGL(frames_plan_kernel, dim3(1), dim3(kPlanThreads), 0, s, sc, image_index, n_frames, n_heads, flags);
    hipLaunchKernelGGL(frames_bin_kernel<0>, tri_grid, dim3(kFrameThreads), 0, s, m.ntri, sc, table, image_index, flags);
    hipLaunchKernelGGL(frames_scan_kernel, dim3(1), dim3(kPlanThreads), 0, s, sc);
    hipLaunchKernelGGL(frames_bin_kernel<1>, tri_grid, dim3(kFrameThreads), 0, s, m.ntri, sc, table, image_index, flags);
    DAD3D_HIP_TRY(hipGetLastError());
    *lists = sc;
    *tile_blocks = std::min(total_tiles, 5 * cus);  // five workgroups of 32 KiB a CU; the grid is sized by the host's tile count
    return DAD3D_OK;
}

dad3d_status launch_rasterize_frames(const MeshDev& m, void* scratch, const int64_t* frames, int n_frames, int total_tiles, const float* vertices,
                                     const float* colors, const int32_t* image_index, int n_heads, int reverse, int32_t* flags, hipStream_t s) {
    FrameScratch sc;
    int tile_blocks = 0;
    if (dad3d_status st = build_frame_lists(m, scratch, frames, n_frames, total_tiles, vertices, image_index, n_heads, flags, s, &sc, &tile_blocks)) return st;
    // the items come from the device's list
    const FrameTileArgs a{m, sc, reinterpret_cast<const long long*>(frames), n_frames, vertices, colors, reverse};
    hipLaunchKernelGGL(frames_tile_kernel, dim3(tile_blocks), dim3(kFrameThreads), 0, s, a);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

}  // namespace dad3d
