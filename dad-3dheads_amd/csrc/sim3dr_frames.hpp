// What the two frames units (sim3dr_frames.hip, sim3dr_frames_texture.hip) share: the tile constants, the scratch of the chain as its
// kernels see it, a frame's shape from the device table, the scratch layout, and the first six launches -- the lists a tile kernel walks.
#pragma once

#include <algorithm>
#include <climits>

#include "common.hpp"
#include "sim3dr_math.hpp"

namespace dad3d {

constexpr int kFrameTileShift = 6;
constexpr int kFrameTile = 1 << kFrameTileShift;  // 64 x 64 u64 keys = 32 KiB of LDS
constexpr int kFrameThreads = 256;
constexpr int kFrameWaves = kFrameThreads / 64;
constexpr int kPlanThreads = 1024;
constexpr int kPlanWaves = kPlanThreads / 64;
constexpr int kWaveBoxPixels = 32;  // a box of more pixels inside the tile is walked by the whole wave, not by its own lane

struct FrameScratch {
    int* frame_base;       // [M + 1]   first tile of a frame; clamped to the host's tile total
    unsigned* need;        // [N]       (tile, triangle) entries of a head
    uint2* tri_box;        // [N][ntri] tile box of a triangle: tx0 | tx1 << 16, ty0 | ty1 << 16; tx0 > tx1: off screen
    unsigned* tile_count;  // [T]       entries of a tile (counted, then counted again as the write cursor)
    unsigned* tile_off;    // [T + 1]   first pool entry of a tile
    unsigned* items;       // [T]       the non-empty tiles
    unsigned* n_items;     // [1]
    unsigned* pool;        // [pool_entries]  head << 16 | triangle
    unsigned pool_entries;
    int total_tiles;       // T, from the host's copy of the shapes
};

struct FrameShape {
    int h, w, tiles_x, tiles;  // tiles == 0: not a frame the chain draws into
};
__device__ __forceinline__ FrameShape frame_shape(const long long* frames, int f) {
    const long long h = frames[4 * (size_t)f + 1], w = frames[4 * (size_t)f + 2];
    FrameShape s{0, 0, 0, 0};
    if (h < 1 || w < 1 || h > INT_MAX - kFrameTile || w > INT_MAX - kFrameTile) return s;
    const long long tx = (w + kFrameTile - 1) >> kFrameTileShift, ty = (h + kFrameTile - 1) >> kFrameTileShift;
    if (tx * ty > DAD3D_FRAME_MAX_TILES) return s;
    s.h = (int)h, s.w = (int)w, s.tiles_x = (int)tx, s.tiles = (int)(tx * ty);
    return s;
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct FrameLayout {
    size_t frame_base, need, tri_box, tile_count, tile_off, items, n_items, pool, total;
    unsigned pool_entries;
    FrameLayout(int ntri, int n_frames, int n_heads, int total_tiles) {
        // 4 * ntri * N entries: a triangle whose clipped box is at most 64 x 64 pixels touches at most 2 x 2 tiles
        pool_entries = (unsigned)std::min<unsigned long long>(4ull * (unsigned)ntri * (unsigned)n_heads, 0x7fffffffull);
        frame_base = 0;
        need = align256(frame_base + ((size_t)n_frames + 1) * sizeof(int));
        tri_box = align256(need + (size_t)n_heads * sizeof(unsigned));
        tile_count = align256(tri_box + (size_t)n_heads * ntri * sizeof(uint2));
        tile_off = align256(tile_count + (size_t)total_tiles * sizeof(unsigned));
        items = align256(tile_off + ((size_t)total_tiles + 1) * sizeof(unsigned));
        n_items = align256(items + (size_t)total_tiles * sizeof(unsigned));
        pool = align256(n_items + sizeof(unsigned));
        total = align256(pool + (size_t)pool_entries * sizeof(unsigned));
    }
};

// ---- device side of a tile kernel (a unit that uses it is compiled with -ffp-contract=off: sim3dr_math.hpp) ----------------------
namespace {

struct FrameTile {
    int f;                   // the frame the tile belongs to
    FrameShape fs;
    int px0, py0, px1, py1;  // its pixels inside the frame, inclusive
};

// tile g of the one numbering of all tiles -> its frame and pixel range
__device__ __forceinline__ FrameTile frame_tile(const FrameScratch& sc, const long long* frames, int n_frames, int g) {
    // the frame of tile g: the last f with frame_base[f] <= g (frames without tiles share a base with their successor)
    int lo = 0, hi = n_frames;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (sc.frame_base[mid] <= g) lo = mid;
        else hi = mid;
    }
    const int f = lo;
    const FrameShape fs = frame_shape(frames, f);
    const int tile = g - sc.frame_base[f];
    const int px0 = (tile % fs.tiles_x) * kFrameTile, py0 = (tile / fs.tiles_x) * kFrameTile;
    const int px1 = min(px0 + kFrameTile, fs.w) - 1, py1 = min(py0 + kFrameTile, fs.h) - 1;
    return FrameTile{f, fs, px0, py0, px1, py1};
}

// The list of tile g, walked by the workgroup (kFrameThreads threads): a wave reads 64 entries; a lane walks the box of its own entry, a box
// of more than kWaveBoxPixels pixels inside the tile is taken by the whole wave. test_pixel(TriSetup, z0, z1, z2, key_hi, key_lo, x, y)
// runs once per (entry, pixel of its box inside the tile) with key_hi = head + 1 << 48 and key_lo = 0xFFFE - triangle.
template <class TestPixel>
__device__ __forceinline__ void walk_frame_tile(const MeshDev& m, const FrameScratch& sc, const float* vertices, int g, const FrameTile& tile,
                                                TestPixel&& test_pixel) {
    const int tid = threadIdx.x, lane = tid & 63;
    const size_t head_floats = (size_t)m.nver * 3;
    const unsigned n_list = sc.tile_count[g], off = sc.tile_off[g];
    for (unsigned base = (unsigned)(tid & ~63); base < n_list; base += kFrameThreads) {
        const unsigned i = base + lane;
        const bool have = i < n_list;
        const unsigned e = have ? sc.pool[off + i] : 0u;
        const unsigned k = e >> 16, t = e & 0xffffu;
        float x0 = 0.f, y0 = 0.f, z0 = 0.f, x1 = 0.f, y1 = 0.f, z1 = 0.f, x2 = 0.f, y2 = 0.f, z2 = 0.f;
        int bx0 = 1, bx1 = 0, by0 = 1, by1 = 0;
        if (have) {
            const float* vb = vertices + k * head_floats;
            const int i0 = m.tri[3 * t], i1 = m.tri[3 * t + 1], i2 = m.tri[3 * t + 2];
            x0 = vb[3 * i0], y0 = vb[3 * i0 + 1], z0 = vb[3 * i0 + 2];
            x1 = vb[3 * i1], y1 = vb[3 * i1 + 1], z1 = vb[3 * i1 + 2];
            x2 = vb[3 * i2], y2 = vb[3 * i2 + 1], z2 = vb[3 * i2 + 2];
            // the box of rasterize_kernel.cpp:246-254 (as frames_box computed it), then clipped to this tile
            bx0 = max(max(f2i_x86(ceilf(std_min(x0, std_min(x1, x2)))), 0), tile.px0);
            bx1 = min(min(f2i_x86(floorf(std_max(x0, std_max(x1, x2)))), tile.fs.w - 1), tile.px1);
            by0 = max(max(f2i_x86(ceilf(std_min(y0, std_min(y1, y2)))), 0), tile.py0);
            by1 = min(min(f2i_x86(floorf(std_max(y0, std_max(y1, y2)))), tile.fs.h - 1), tile.py1);
        }
        const bool ok = have && bx0 <= bx1 && by0 <= by1;
        const int area = ok ? (bx1 - bx0 + 1) * (by1 - by0 + 1) : 0;
        const bool big = area > kWaveBoxPixels;
        const unsigned long long key_hi = (unsigned long long)(k + 1) << 48;
        const unsigned key_lo = 0xFFFEu - t;
        if (ok && !big) {
            const TriSetup ts = tri_setup(x0, y0, x1, y1, x2, y2);
            for (int y = by0; y <= by1; ++y)
                for (int x = bx0; x <= bx1; ++x) test_pixel(ts, z0, z1, z2, key_hi, key_lo, x, y);
        }
        unsigned long long todo = __ballot(big);
        while (todo) {  // wave-uniform: one large box at a time, all 64 lanes on its pixels
            const int j = __builtin_ctzll(todo);
            todo &= todo - 1;
            auto bf = [&](float v) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j)); };
            auto bi = [&](int v) { return __builtin_amdgcn_readlane(v, j); };
            const TriSetup ts = tri_setup(bf(x0), bf(y0), bf(x1), bf(y1), bf(x2), bf(y2));
            const float wz0 = bf(z0), wz1 = bf(z1), wz2 = bf(z2);
            const unsigned we = (unsigned)bi((int)e);
            const unsigned long long wkey_hi = (unsigned long long)((we >> 16) + 1) << 48;
            const unsigned wkey_lo = 0xFFFEu - (we & 0xffffu);
            const int wx0 = bi(bx0), wy0 = bi(by0), bw = bi(bx1) - wx0 + 1, warea = bi(area);
            const float rcp_bw = __builtin_amdgcn_rcpf((float)bw);
            for (int p = lane; p < warea; p += 64) {
                // exact p / bw for p < 4096, bw <= 64: (p + 0.5) / bw is at least 1 / 128 away from an integer, the product's error < 1e-3
                const int py = (int)(((float)p + 0.5f) * rcp_bw), px = p - py * bw;
                test_pixel(ts, wz0, wz1, wz2, wkey_hi, wkey_lo, wx0 + px, wy0 + py);
            }
        }
    }
}

}  // namespace

// setup, box, plan, bin<0>, scan, bin<1> (sim3dr_frames.hip): the flags of the heads and, per non-empty tile, the list of (head, triangle)
// entries a tile kernel walks. *lists: the scratch as the kernels see it; *tile_blocks: the grid of a tile kernel (workgroups of 32 KiB).
dad3d_status build_frame_lists(const MeshDev& m, void* scratch, const int64_t* frames, int n_frames, int total_tiles, const float* vertices,
                               const int32_t* image_index, int n_heads, int32_t* flags, hipStream_t s, FrameScratch* lists, int* tile_blocks);

}  // namespace dad3d
