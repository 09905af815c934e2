// The reference's single-image Sim3DR API (Sim3DR/lib/rasterize.h:84-100), both halves: the exact-signature host entry points in C linkage
// and their C++-linkage doubles. Everything here goes through the public dad3d_mesh_* ABI: the mesh handle stays private to capi_render.cpp.
// The reference API carries no vertex count for three of the five calls; it is derived from the
// triangle list (max index + 1), which is all the GPU needs to stage.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "common.hpp"

using namespace dad3d;

namespace {

struct HostMeshCache {
    std::mutex mu;
    dad3d_mesh* mesh = nullptr;
    int device = 0;  // the device `mesh` lives on
    uint64_t hash = 0;
    int ntri = -1, nver = -1;
    ~HostMeshCache() { /* process teardown: the HIP runtime may already be gone; leak on purpose */ }
};
HostMeshCache g_cache;

int compat_device() {
    const char* e = std::getenv("DAD3D_DEVICE");
    return e ? std::atoi(e) : 0;
}

// Content hash of the triangle list (the reference API re-passes it on every call): 8 bytes per step, four
// independent lanes -- a byte-wise FNV over 120 KB cost more than the kernels it guards.
uint64_t fnv1a(const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    uint64_t h[4] = {1469598103934665603ull, 0x9E3779B97F4A7C15ull, 0xC2B2AE3D27D4EB4Full, 0x165667B19E3779F9ull};
    size_t i = 0;
    for (; i + 32 <= n; i += 32)
        for (int k = 0; k < 4; ++k) {
            uint64_t w;
            std::memcpy(&w, b + i + 8 * k, 8);
            h[k] = (h[k] ^ w) * 1099511628211ull;
            h[k] ^= h[k] >> 29;
        }
    uint64_t t = n;
    for (; i < n; ++i) t = (t ^ b[i]) * 1099511628211ull;
    return ((h[0] * 31 + h[1]) * 31 + h[2]) * 31 + h[3] + t * 0x9E3779B97F4A7C15ull;
}

int max_index_plus_one(const int* tri, int ntri) {
    int mx = -1;
    for (int i = 0; i < 3 * ntri; ++i) mx = std::max(mx, tri[i]);
    return mx + 1;
}

// topology is static across calls in practice (one mesh, many frames): rebuild only when it changes
dad3d_mesh* cached_mesh(const int* tri, int ntri, int nver) {
    const uint64_t hsh = fnv1a(tri, sizeof(int) * 3 * (size_t)ntri);
    if (g_cache.mesh && g_cache.hash == hsh && g_cache.ntri == ntri && g_cache.nver == nver) return g_cache.mesh;
    if (g_cache.mesh) dad3d_mesh_destroy(g_cache.mesh);
    g_cache.mesh = nullptr;
    g_cache.device = compat_device();
    if (dad3d_mesh_create(tri, ntri, nver, g_cache.device, &g_cache.mesh) != DAD3D_OK) return nullptr;
    g_cache.hash = hsh;
    g_cache.ntri = ntri;
    g_cache.nver = nver;
    return g_cache.mesh;
}

// Staging buffers of the single-image host entry points: a few grow-only device buffers kept for the life of the process
// (a hipMalloc + hipFree per call cost more than the kernels; calls are serialised by g_cache.mu). A DevBuf takes the next
// free slot of the arena; the arena is rewound when the call returns. Not DeviceScratch (device_memory.hpp): a slot is replaced without
// waiting for the device -- every call here ends synchronised -- and is never freed, and DeviceScratch would do both.
struct StagingArena {
    static constexpr int kSlots = 4;
    void* buf[kSlots] = {};
    size_t cap[kSlots] = {};
    int next = 0;
    ~StagingArena() { /* process teardown: leak on purpose, see HostMeshCache */ }
};
StagingArena g_arena;

struct DevBuf {
    void* p = nullptr;
    bool alloc(size_t bytes) {
        if (g_arena.next >= StagingArena::kSlots) return false;
        const int s = g_arena.next++;
        bytes = std::max<size_t>(bytes, 4);
        if (g_arena.cap[s] < bytes) {
            if (g_arena.buf[s]) (void)hipFree(g_arena.buf[s]);
            g_arena.buf[s] = nullptr, g_arena.cap[s] = 0;
            if (hipMalloc(&g_arena.buf[s], bytes) != hipSuccess) return false;
            g_arena.cap[s] = bytes;
        }
        p = g_arena.buf[s];
        return true;
    }
};
struct ArenaScope {  // declared after the lock in every entry point
    ArenaScope() { g_arena.next = 0; }
    ~ArenaScope() { g_arena.next = 0; }
};

bool h2d(void* d, const void* h, size_t n) { return n == 0 || hipMemcpy(d, h, n, hipMemcpyHostToDevice) == hipSuccess; }
bool d2h(void* h, const void* d, size_t n) { return n == 0 || hipMemcpy(h, d, n, hipMemcpyDeviceToHost) == hipSuccess; }

}  // namespace

extern "C" {

void dad3d_sim3dr_get_tri_normal(float* tri_normal, float* vertices, int* triangles, int ntri, int norm_flg) {
    if (ntri <= 0) return;
    std::lock_guard<std::mutex> lock(g_cache.mu);
    ArenaScope arena_scope;
    const int nver = max_index_plus_one(triangles, ntri);
    dad3d_mesh* m = cached_mesh(triangles, ntri, nver);
    if (!m) return;
    DeviceGuard guard(g_cache.device);
    DevBuf dv, dn;
    const size_t vb = sizeof(float) * 3 * (size_t)nver, nb = sizeof(float) * 3 * (size_t)ntri;
    if (!dv.alloc(vb) || !dn.alloc(nb) || !h2d(dv.p, vertices, vb)) return set_error("sim3dr compat: staging failed");
    if (dad3d_mesh_get_tri_normal(m, (float*)dn.p, (const float*)dv.p, 1, norm_flg, nullptr)) return;
    if (hipDeviceSynchronize() != hipSuccess || !d2h(tri_normal, dn.p, nb)) set_error("sim3dr compat: readback failed");
}

void dad3d_sim3dr_get_ver_normal(float* ver_normal, float* tri_normal, int* triangles, int nver, int ntri) {
    if (nver <= 0) return;
    std::lock_guard<std::mutex> lock(g_cache.mu);
    ArenaScope arena_scope;
    dad3d_mesh* m = cached_mesh(triangles, std::max(ntri, 0), nver);
    if (!m) return;
    DeviceGuard guard(g_cache.device);
    DevBuf dt, dn;
    const size_t tb = sizeof(float) * 3 * (size_t)std::max(ntri, 0), nb = sizeof(float) * 3 * (size_t)nver;
    if (!dt.alloc(tb) || !dn.alloc(nb) || !h2d(dt.p, tri_normal, tb) || !h2d(dn.p, ver_normal, nb))
        return set_error("sim3dr compat: staging failed");
    if (dad3d_mesh_get_ver_normal(m, (float*)dn.p, (const float*)dt.p, 1, DAD3D_NORMAL_ACCUMULATE, nullptr)) return;
    if (hipDeviceSynchronize() != hipSuccess || !d2h(ver_normal, dn.p, nb)) set_error("sim3dr compat: readback failed");
}

void dad3d_sim3dr_get_normal(float* ver_normal, float* vertices, int* triangles, int nver, int ntri) {
    if (nver <= 0) return;
    std::lock_guard<std::mutex> lock(g_cache.mu);
    ArenaScope arena_scope;
    dad3d_mesh* m = cached_mesh(triangles, std::max(ntri, 0), nver);
    if (!m) return;
    DeviceGuard guard(g_cache.device);
    DevBuf dv, dn;
    const size_t nb = sizeof(float) * 3 * (size_t)nver;
    if (!dv.alloc(nb) || !dn.alloc(nb) || !h2d(dv.p, vertices, nb) || !h2d(dn.p, ver_normal, nb))
        return set_error("sim3dr compat: staging failed");
    if (dad3d_mesh_get_normal(m, (float*)dn.p, (const float*)dv.p, 1, DAD3D_NORMAL_ACCUMULATE, nullptr)) return;
    if (hipDeviceSynchronize() != hipSuccess || !d2h(ver_normal, dn.p, nb)) set_error("sim3dr compat: readback failed");
}

void dad3d_sim3dr_rasterize_triangles(float* vertices, int* triangles, float* depth_buffer, int* triangle_buffer,
                                      float* barycentric_weight, int ntri, int h, int w) {
    if (ntri <= 0 || h <= 0 || w <= 0) return;
    std::lock_guard<std::mutex> lock(g_cache.mu);
    ArenaScope arena_scope;
    const int nver = max_index_plus_one(triangles, ntri);
    dad3d_mesh* m = cached_mesh(triangles, ntri, nver);
    if (!m) return;
    DeviceGuard guard(g_cache.device);
    DevBuf dv, dd, dt, db;
    const size_t vb = sizeof(float) * 3 * (size_t)nver, pb = (size_t)h * w;
    if (!dv.alloc(vb) || !dd.alloc(pb * 4) || !dt.alloc(pb * 4) || !db.alloc(pb * 12) || !h2d(dv.p, vertices, vb) ||
        !h2d(dd.p, depth_buffer, pb * 4) || !h2d(dt.p, triangle_buffer, pb * 4) || !h2d(db.p, barycentric_weight, pb * 12))
        return set_error("sim3dr compat: staging failed");
    if (dad3d_mesh_rasterize_triangles(m, (const float*)dv.p, (float*)dd.p, (int32_t*)dt.p, (float*)db.p, 1, h, w, nullptr))
        return;
    if (hipDeviceSynchronize() != hipSuccess || !d2h(depth_buffer, dd.p, pb * 4) || !d2h(triangle_buffer, dt.p, pb * 4) ||
        !d2h(barycentric_weight, db.p, pb * 12))
        set_error("sim3dr compat: readback failed");
}

void dad3d_sim3dr_rasterize(unsigned char* image, float* vertices, int* triangles, float* colors, float* depth_buffer,
                            int ntri, int h, int w, int c, float alpha, int reverse) {
    if (ntri <= 0 || h <= 0 || w <= 0) return;
    std::lock_guard<std::mutex> lock(g_cache.mu);
    ArenaScope arena_scope;
    const int nver = max_index_plus_one(triangles, ntri);
    dad3d_mesh* m = cached_mesh(triangles, ntri, nver);
    if (!m) return;
    DeviceGuard guard(g_cache.device);
    DevBuf dv, dc, dd, di;
    const size_t vb = sizeof(float) * 3 * (size_t)nver, cb = sizeof(float) * (size_t)c * nver, pb = (size_t)h * w;
    if (!dv.alloc(vb) || !dc.alloc(cb) || !dd.alloc(pb * 4) || !di.alloc(pb * c) || !h2d(dv.p, vertices, vb) ||
        !h2d(dc.p, colors, cb) || !h2d(dd.p, depth_buffer, pb * 4) || !h2d(di.p, image, pb * c))
        return set_error("sim3dr compat: staging failed");
    if (dad3d_mesh_rasterize(m, (uint8_t*)di.p, (const float*)dv.p, (const float*)dc.p, (float*)dd.p, 1, h, w, c, alpha,
                             reverse, nullptr))
        return;
    if (hipDeviceSynchronize() != hipSuccess || !d2h(image, di.p, pb * c) || !d2h(depth_buffer, dd.p, pb * 4))
        set_error("sim3dr compat: readback failed");
}

}  // extern "C"

// C++-linkage doubles of the reference's Sim3DR entry points, prototype for prototype
// (Sim3DR/lib/rasterize.h:88-100), forwarding to the C ABI. With these exported, the reference's Cython
// binding (Sim3DR/lib/rasterize.pyx, `cdef extern from "rasterize.h"`) links against libdad3d_hip.so
// instead of rasterize_kernel.cpp without a source change -- see INTEGRATION.md.

DAD3D_EXPORT void _get_tri_normal(float* tri_normal, float* vertices, int* triangles, int ntri, bool norm_flg) {
    dad3d_sim3dr_get_tri_normal(tri_normal, vertices, triangles, ntri, norm_flg ? 1 : 0);
}

DAD3D_EXPORT void _get_ver_normal(float* ver_normal, float* tri_normal, int* triangles, int nver, int ntri) {
    dad3d_sim3dr_get_ver_normal(ver_normal, tri_normal, triangles, nver, ntri);
}

DAD3D_EXPORT void _get_normal(float* ver_normal, float* vertices, int* triangles, int nver, int ntri) {
    dad3d_sim3dr_get_normal(ver_normal, vertices, triangles, nver, ntri);
}

DAD3D_EXPORT void _rasterize_triangles(float* vertices, int* triangles, float* depth_buffer, int* triangle_buffer,
                                       float* barycentric_weight, int ntri, int h, int w) {
    dad3d_sim3dr_rasterize_triangles(vertices, triangles, depth_buffer, triangle_buffer, barycentric_weight, ntri, h, w);
}

DAD3D_EXPORT void _rasterize(unsigned char* image, float* vertices, int* triangles, float* colors, float* depth_buffer,
                             int ntri, int h, int w, int c, float alpha, bool reverse) {
    dad3d_sim3dr_rasterize(image, vertices, triangles, colors, depth_buffer, ntri, h, w, c, alpha, reverse ? 1 : 0);
}
