// C ABI, render side: the Sim3DR mesh handle, the UV-map handle and the overlays (sim3dr_*.hip, uv_texture*.hip, overlay.hip).
#include <algorithm>
#include <cmath>
#include <memory>

#include "capi_checks.hpp"
#include "mesh_plan.hpp"

using namespace dad3d;

struct dad3d_mesh {
    int device = 0;
    int ntri = 0, nver = 0;
    DeviceArray<int> d_tri, d_adj_ptr, d_adj_face;
    DeviceArray<int4> d_adj_tri;
    std::vector<int> h_tri;  // the triangle list on the host (dad3d_mesh_set_texcoords reads it)
    DeviceArray<uint2> d_nc_faces[kNormalChunkings];  // chunk face lists of the normals kernels (NormalChunksDev)
    DeviceArray<unsigned short> d_nc_slot[kNormalChunkings];
    DeviceArray<uint4> d_nc_row8[kNormalChunkings];
    NormalChunksDev nc[kNormalChunkings] = {};
    unsigned long long* d_trace = nullptr;  // diagnostics (dad3d_mesh_debug_trace): the caller's buffer, borrowed
    DeviceArray<float4> d_tex_tri[2];  // texel coordinates per triangle corner, [ntri][2] (dad3d_mesh_set_texcoords): corner / reference indexing
    DeviceScratch d_raster;  // per-image triangle boxes + corner planes, grown on demand (one stream at a time)
    int raster_batch = 0, raster_h = 0, raster_w = 0;
    // The scratch layout depends on (batch, h, w): a change of shape re-zeroes the tile counters in stream order.
    dad3d_status raster_scratch(int batch, int h, int w, hipStream_t s) {
        if (batch == raster_batch && h == raster_h && w == raster_w) return DAD3D_OK;
        const size_t had = d_raster.capacity();
        const dad3d_status grown = d_raster.grow(raster_scratch_bytes(dev(), batch, h, w));
        if (d_raster.capacity() != had) raster_batch = 0;  // a new buffer holds no shape
        if (grown) return grown;
        if (dad3d_status st = raster_scratch_init(dev(), d_raster.get(), batch, h, w, s)) return st;
        raster_batch = batch, raster_h = h, raster_w = w;
        return DAD3D_OK;
    }
    DeviceScratch d_frames;  // scratch of the frames chain (sim3dr_frames.hip), grown on demand like d_raster; needs no initialisation
    dad3d_status frames_scratch(int n_frames, int n_heads, int total_tiles) {
        return d_frames.grow(frames_scratch_bytes(ntri, n_frames, n_heads, total_tiles));
    }
    MeshDev dev() const { return MeshDev{d_tri.get(), d_adj_ptr.get(), d_adj_face.get(), d_adj_tri.get(), ntri, nver}; }
};

// the checks the two frames entries share, all on the host; *total_tiles = 0: nothing to do
static dad3d_status frames_arguments(const char* who, dad3d_mesh* m, const int64_t* frames, const int64_t* frames_host, int n_frames,
                                     const float* vertices, const float* colors, const int32_t* image_index, int n_heads, int32_t* flags,
                                     int* total_tiles) {
    *total_tiles = 0;
    DAD3D_REQUIRE(m && n_frames >= 0 && n_heads >= 0, "%s: bad argument", who);
    DAD3D_REQUIRE(n_frames <= DAD3D_FRAME_MAX_COUNT && n_heads <= DAD3D_FRAME_MAX_COUNT, "%s: %d frames and %d heads, at most %d each", who,
                  n_frames, n_heads, DAD3D_FRAME_MAX_COUNT);
    if (n_heads == 0) return DAD3D_OK;
    DAD3D_REQUIRE(image_index && flags, "%s: null buffer", who);
    if (n_frames == 0) return DAD3D_OK;
    DAD3D_REQUIRE(frames && frames_host && (m->ntri == 0 || (vertices && colors)), "%s: null buffer", who);
    DAD3D_REQUIRE(m->ntri <= 65535 && 4ll * m->ntri * n_heads < (1ll << 31), "%s: %d triangles and %d heads exceed 65535 triangles or 2^31 list entries",
                  who, m->ntri, n_heads);
    return frames_check_shapes(who, frames_host, n_frames, total_tiles);
}

struct dad3d_uvmap {
    int device = 0;
    int nver = 0, size = 0, n_cand = 0;
    DeviceArray<int> d_adj_ptr;  // vertex -> faces (UvNormalArgs)
    DeviceArray<int4> d_adj;
    DeviceArray<int> d_texel_ptr;  // texel -> candidates, descending (UvBakeArgs)
    DeviceArray<int> d_cand_verts;
    DeviceArray<double> d_cand_bary;
    DeviceArray<int> d_faces;  // [ntri,3]: the depth maps' triangles (UvDepthFramesArgs)
    int ntri = 0;
};

extern "C" {

dad3d_status dad3d_mesh_create(const int32_t* tri, int ntri, int nver, int device, dad3d_mesh** out) {
    DAD3D_REQUIRE(out && ntri >= 0 && nver >= 0 && (tri || ntri == 0), "dad3d_mesh_create: bad argument");
    *out = nullptr;
    for (int i = 0; i < 3 * ntri; ++i)
        DAD3D_REQUIRE(tri[i] >= 0 && tri[i] < nver, "triangle index %d out of range [0,%d)", tri[i], nver);
    DAD3D_SELECT_DEVICE(device);
    const plan::MeshAdjacency adj = plan::mesh_adjacency(tri, ntri, nver);
    std::unique_ptr<dad3d_mesh> m(new dad3d_mesh);
    m->device = device;
    m->ntri = ntri;
    m->nver = nver;
    m->h_tri.assign(tri, tri + 3 * (size_t)ntri);
    dad3d_status st;
    if ((st = m->d_tri.upload(m->h_tri)) || (st = m->d_adj_ptr.upload(adj.ptr)) || (st = m->d_adj_face.upload(adj.face)) ||
        (st = m->d_adj_tri.upload(adj.adj_tri)))
        return st;
    // chunk face lists for 1, 2, 4 and 8 vertex chunks per image (only where table + staged vertices fit the LDS)
    for (int k = 0; k < kNormalChunkings; ++k) {
        const plan::NormalChunkPlan p = plan::plan_normal_chunks(tri, ntri, nver, adj, 1 << k, normal_table_lds_bytes);
        if (!p.built) continue;
        if ((st = m->d_nc_faces[k].upload(p.faces)) || (st = m->d_nc_slot[k].upload(p.slot)) || (st = m->d_nc_row8[k].upload(p.row8))) return st;
        m->nc[k] = NormalChunksDev{m->d_nc_faces[k].get(), {}, m->d_nc_slot[k].get(), m->d_nc_row8[k].get(), p.chunks, p.vpb, p.max_faces};
        std::copy(p.face_ptr.begin(), p.face_ptr.end(), m->nc[k].face_ptr);
    }
    *out = m.release();
    return DAD3D_OK;
}

void dad3d_mesh_destroy(dad3d_mesh* m) { delete m; }

dad3d_status dad3d_mesh_get_normal(dad3d_mesh* m, float* ver_normal, const float* vertices, int batch, unsigned flags,
                                   void* stream) {
    DAD3D_REQUIRE(m && batch >= 0, "dad3d_mesh_get_normal: bad argument");
    if (batch == 0 || m->nver == 0) return DAD3D_OK;
    DAD3D_REQUIRE(ver_normal && vertices, "dad3d_mesh_get_normal: null buffer");
    DeviceGuard guard(m->device);
    return launch_get_normal(m->dev(), m->nc, ver_normal, vertices, batch, flags, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_mesh_get_tri_normal(dad3d_mesh* m, float* tri_normal, const float* vertices, int batch,
                                       int norm_flg, void* stream) {
    DAD3D_REQUIRE(m && batch >= 0, "dad3d_mesh_get_tri_normal: bad argument");
    if (batch == 0 || m->ntri == 0) return DAD3D_OK;
    DAD3D_REQUIRE(tri_normal && vertices, "dad3d_mesh_get_tri_normal: null buffer");
    DeviceGuard guard(m->device);
    return launch_tri_normal(m->dev(), tri_normal, vertices, batch, norm_flg, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_mesh_get_ver_normal(dad3d_mesh* m, float* ver_normal, const float* tri_normal, int batch,
                                       unsigned flags, void* stream) {
    DAD3D_REQUIRE(m && batch >= 0, "dad3d_mesh_get_ver_normal: bad argument");
    if (batch == 0 || m->nver == 0) return DAD3D_OK;
    DAD3D_REQUIRE(ver_normal && (tri_normal || m->ntri == 0), "dad3d_mesh_get_ver_normal: null buffer");
    DeviceGuard guard(m->device);
    return launch_ver_normal(m->dev(), ver_normal, tri_normal, batch, flags, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_mesh_rasterize(dad3d_mesh* m, uint8_t* image, const float* vertices, const float* colors,
                                  float* depth, int batch, int h, int w, int c, float alpha, int reverse,
                                  void* stream) {
    DAD3D_REQUIRE(m && batch >= 0 && h >= 0 && w >= 0 && c >= 0, "dad3d_mesh_rasterize: bad argument");
    DAD3D_REQUIRE(alpha == alpha, "dad3d_mesh_rasterize: alpha is NaN");
    if (batch == 0 || h == 0 || w == 0) return DAD3D_OK;
    DAD3D_REQUIRE(image && (vertices || m->ntri == 0) && (colors || m->ntri == 0 || c == 0),
                  "dad3d_mesh_rasterize: null buffer");
    DeviceGuard guard(m->device);
    if (dad3d_status st = m->raster_scratch(batch, h, w, static_cast<hipStream_t>(stream))) return st;
    // alpha != 1: the blends of rasterize_kernel.cpp:268-284 replayed in triangle order (mode 2)
    return launch_rasterize(m->dev(), m->nc, m->d_raster.get(), m->d_trace, image, vertices, colors, depth, nullptr, nullptr, batch, h, w, c, reverse,
                            alpha == 1.0f ? 0 : 2, nullptr, static_cast<hipStream_t>(stream), alpha);
}

dad3d_status dad3d_mesh_render(dad3d_mesh* m, uint8_t* image, const float* vertices, float* light, float* depth, int batch,
                               int h, int w, const dad3d_light* cfg, int flags, void* stream) {
    DAD3D_REQUIRE(m && cfg && batch >= 0 && h >= 0 && w >= 0, "dad3d_mesh_render: bad argument");
    if (batch == 0 || h == 0 || w == 0) return DAD3D_OK;
    DAD3D_REQUIRE(image, "dad3d_mesh_render: null buffer");
    DeviceGuard guard(m->device);
    if (m->ntri == 0) {  // nothing to draw: only the background
        if (flags & DAD3D_RENDER_CLEAR) DAD3D_HIP_TRY(hipMemsetAsync(image, 0, (size_t)batch * h * w * 3, static_cast<hipStream_t>(stream)));
        return DAD3D_OK;
    }
    DAD3D_REQUIRE(vertices && light, "dad3d_mesh_render: null buffer");
    if (dad3d_status st = m->raster_scratch(batch, h, w, static_cast<hipStream_t>(stream))) return st;
    return launch_rasterize(m->dev(), m->nc, m->d_raster.get(), m->d_trace, image, vertices, light, depth, nullptr, nullptr, batch, h, w, 3,
                            flags, 0, cfg, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_mesh_rasterize_frames(dad3d_mesh* m, const int64_t* frames, const int64_t* frames_host, int n_frames, const float* vertices,
                                         const float* colors, const int32_t* image_index, int n_heads, int reverse, int32_t* flags, void* stream) {
    int total_tiles = 0;
    if (dad3d_status st = frames_arguments("dad3d_mesh_rasterize_frames", m, frames, frames_host, n_frames, vertices, colors, image_index, n_heads,
                                           flags, &total_tiles))
        return st;
    if (total_tiles == 0) return DAD3D_OK;  // no frames or no heads
    DeviceGuard guard(m->device);
    if (dad3d_status st = m->frames_scratch(n_frames, n_heads, total_tiles)) return st;
    return launch_rasterize_frames(m->dev(), m->d_frames.get(), frames, n_frames, total_tiles, vertices, colors, image_index, n_heads, reverse ? 1 : 0,
                                   flags, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_mesh_render_frames(dad3d_mesh* m, const int64_t* frames, const int64_t* frames_host, int n_frames, const float* vertices,
                                      float* light, const int32_t* image_index, int n_heads, const dad3d_light* cfg, int render_flags,
                                      int32_t* flags, void* stream) {
    DAD3D_REQUIRE(cfg, "dad3d_mesh_render_frames: bad argument");
    DAD3D_REQUIRE(!(render_flags & ~DAD3D_RENDER_REVERSE),
                  "dad3d_mesh_render_frames: render flags %d: only DAD3D_RENDER_REVERSE (a frame is the caller's picture: no DAD3D_RENDER_CLEAR)", render_flags);
    int total_tiles = 0;
    if (dad3d_status st = frames_arguments("dad3d_mesh_render_frames", m, frames, frames_host, n_frames, vertices, light, image_index, n_heads, flags,
                                           &total_tiles))
        return st;
    if (total_tiles == 0) return DAD3D_OK;
    DeviceGuard guard(m->device);
    if (dad3d_status st = m->frames_scratch(n_frames, n_heads, total_tiles)) return st;
    // the light of every head, flagged or not, as dad3d_mesh_normal_phong_light computes it; then it is the colours
    if (dad3d_status st = launch_phong(m->dev(), m->nc, light, vertices, nullptr, nullptr, n_heads, *cfg, static_cast<hipStream_t>(stream))) return st;
    return launch_rasterize_frames(m->dev(), m->d_frames.get(), frames, n_frames, total_tiles, vertices, light, image_index, n_heads,
                                   render_flags & DAD3D_RENDER_REVERSE, flags, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_mesh_render_texture_frames(dad3d_mesh* m, const int64_t* frames, const int64_t* frames_host, int n_frames, const float* vertices,
                                              const void* texture, int texture_dtype, int texture_batched, int tex_h, int tex_w, int tex_c,
                                              int mapping_type, int indexing, const int32_t* image_index, int n_heads, int32_t* flags, void* stream) {
    const char* who = "dad3d_mesh_render_texture_frames";
    // the scalar arguments and the host table first: a bad one is refused before the handle is looked at or any device work starts
    DAD3D_REQUIRE(texture_dtype == DAD3D_DTYPE_F32 || texture_dtype == DAD3D_DTYPE_U8, "%s: the texture is float32 (DAD3D_DTYPE_F32) or uint8 (DAD3D_DTYPE_U8)", who);
    DAD3D_REQUIRE(tex_h >= 1 && tex_w >= 1 && tex_c >= 1 && (size_t)tex_h * tex_w * tex_c < (1ull << 31), "%s: texture of %d x %d x %d", who, tex_h, tex_w, tex_c);
    DAD3D_REQUIRE(tex_c >= 3, "%s: a frame has three channels, tex_c = %d", who, tex_c);
    DAD3D_REQUIRE(indexing == DAD3D_TEX_INDEX_CORNER || indexing == DAD3D_TEX_INDEX_REFERENCE, "%s: unknown indexing mode %d", who, indexing);
    DAD3D_REQUIRE(n_frames >= 0 && n_heads >= 0, "%s: bad argument", who);
    DAD3D_REQUIRE(n_frames <= DAD3D_FRAME_MAX_COUNT && n_heads <= DAD3D_FRAME_MAX_COUNT, "%s: %d frames and %d heads, at most %d each", who,
                  n_frames, n_heads, DAD3D_FRAME_MAX_COUNT);
    int total_tiles = 0;
    if (n_frames > 0 && n_heads > 0 && frames_host)
        if (dad3d_status st = frames_check_shapes(who, frames_host, n_frames, &total_tiles)) return st;
    DAD3D_REQUIRE(m, "%s: null handle", who);
    if (dad3d_status st = frames_arguments(who, m, frames, frames_host, n_frames, vertices, vertices, image_index, n_heads, flags, &total_tiles)) return st;
    if (total_tiles == 0) return DAD3D_OK;  // no frames or no heads
    if (m->ntri > 0) {
        DAD3D_REQUIRE(texture, "%s: null buffer", who);
        DAD3D_REQUIRE(m->d_tex_tri[DAD3D_TEX_INDEX_CORNER], "%s: no texture coordinates attached (dad3d_mesh_set_texcoords)", who);
        DAD3D_REQUIRE(m->d_tex_tri[indexing], "%s: reference indexing needs tex_coords rows of 3 floats, one for every vertex a triangle names", who);
    }
    DeviceGuard guard(m->device);
    if (dad3d_status st = m->frames_scratch(n_frames, n_heads, total_tiles)) return st;
    return launch_render_texture_frames(m->dev(), m->d_frames.get(), frames, n_frames, total_tiles, vertices, m->d_tex_tri[indexing].get(), texture,
                                        texture_dtype == DAD3D_DTYPE_U8, texture_batched ? (size_t)tex_h * tex_w * tex_c : 0, tex_h, tex_w, tex_c,
                                        mapping_type == 0, image_index, n_heads, flags, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_mesh_frames_scratch_bytes(dad3d_mesh* m, size_t* bytes) {
    DAD3D_REQUIRE(m && bytes, "dad3d_mesh_frames_scratch_bytes: bad argument");
    *bytes = m->d_frames.capacity();
    return DAD3D_OK;
}

dad3d_status dad3d_mesh_rasterize_triangles(dad3d_mesh* m, const float* vertices, float* depth, int32_t* tri_buf,
                                            float* bary, int batch, int h, int w, void* stream) {
    DAD3D_REQUIRE(m && batch >= 0 && h >= 0 && w >= 0, "dad3d_mesh_rasterize_triangles: bad argument");
    if (batch == 0 || h == 0 || w == 0) return DAD3D_OK;
    DAD3D_REQUIRE(depth && tri_buf && bary && (vertices || m->ntri == 0), "dad3d_mesh_rasterize_triangles: null buffer");
    DeviceGuard guard(m->device);
    if (dad3d_status st = m->raster_scratch(batch, h, w, static_cast<hipStream_t>(stream))) return st;
    return launch_rasterize(m->dev(), m->nc, m->d_raster.get(), m->d_trace, nullptr, vertices, nullptr, depth, tri_buf, bary, batch, h, w, 3, 0, 1,
                            nullptr, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_mesh_set_texcoords(dad3d_mesh* m, const float* tex_coords, int n_tex, int stride, const int32_t* tex_triangles) {
    DAD3D_REQUIRE(m, "dad3d_mesh_set_texcoords: null handle");
    DAD3D_REQUIRE(stride == 2 || stride == 3, "dad3d_mesh_set_texcoords: tex_coords rows of 2 or 3 floats, got %d", stride);
    DAD3D_REQUIRE(n_tex >= 0 && (tex_coords || n_tex == 0) && (tex_triangles || m->ntri == 0), "dad3d_mesh_set_texcoords: bad argument");
    const size_t nt = (size_t)m->ntri;
    for (size_t i = 0; i < 3 * nt; ++i)
        DAD3D_REQUIRE(tex_triangles[i] >= 0 && tex_triangles[i] < n_tex, "texture triangle index %d out of range [0,%d)", tex_triangles[i], n_tex);
    const plan::TexcoordTables T = plan::plan_texcoords(m->h_tri, tex_coords, n_tex, stride, tex_triangles);
    DeviceGuard guard(m->device);
    DAD3D_HIP_TRY(hipDeviceSynchronize());  // a launch in flight may still read the tables being replaced
    for (DeviceArray<float4>& t : m->d_tex_tri) t.reset();
    if (nt == 0) return DAD3D_OK;
    if (dad3d_status st = m->d_tex_tri[DAD3D_TEX_INDEX_CORNER].upload(T.corner)) return st;
    return T.ref_ok ? m->d_tex_tri[DAD3D_TEX_INDEX_REFERENCE].upload(T.ref) : DAD3D_OK;
}

dad3d_status dad3d_mesh_render_texture(dad3d_mesh* m, void* image, int image_dtype, const float* vertices, const void* texture,
                                       int texture_dtype, int texture_batched, float* depth, int batch, int h, int w, int c, int tex_h,
                                       int tex_w, int tex_c, int mapping_type, int indexing, void* stream) {
    // the scalar arguments first: a bad one is refused before the handle is looked at or any device work starts
    DAD3D_REQUIRE(batch >= 0 && h >= 0 && w >= 0, "dad3d_mesh_render_texture: negative batch or image size");
    DAD3D_REQUIRE((image_dtype == DAD3D_DTYPE_F32 || image_dtype == DAD3D_DTYPE_U8) && (texture_dtype == DAD3D_DTYPE_F32 || texture_dtype == DAD3D_DTYPE_U8),
                  "dad3d_mesh_render_texture: image and texture are float32 (DAD3D_DTYPE_F32) or uint8 (DAD3D_DTYPE_U8)");
    DAD3D_REQUIRE(tex_h >= 1 && tex_w >= 1 && tex_c >= 1 && (size_t)tex_h * tex_w * tex_c < (1ull << 31), "dad3d_mesh_render_texture: texture of %d x %d x %d", tex_h, tex_w, tex_c);
    DAD3D_REQUIRE(c >= 1 && c <= 4 && c <= tex_c, "dad3d_mesh_render_texture: c = %d channels, need 1..4 and at most tex_c = %d", c, tex_c);
    DAD3D_REQUIRE(indexing == DAD3D_TEX_INDEX_CORNER || indexing == DAD3D_TEX_INDEX_REFERENCE, "dad3d_mesh_render_texture: unknown indexing mode %d", indexing);
    DAD3D_REQUIRE(m, "dad3d_mesh_render_texture: null handle");
    if (batch == 0 || h == 0 || w == 0 || m->ntri == 0) return DAD3D_OK;
    DAD3D_REQUIRE(image && vertices && texture, "dad3d_mesh_render_texture: null buffer");
    DAD3D_REQUIRE(m->d_tex_tri[DAD3D_TEX_INDEX_CORNER], "dad3d_mesh_render_texture: no texture coordinates attached (dad3d_mesh_set_texcoords)");
    DAD3D_REQUIRE(m->d_tex_tri[indexing], "dad3d_mesh_render_texture: reference indexing needs tex_coords rows of 3 floats, one for every vertex a triangle names");
    DeviceGuard guard(m->device);
    if (dad3d_status st = m->raster_scratch(batch, h, w, static_cast<hipStream_t>(stream))) return st;
    return launch_render_texture(m->dev(), m->d_raster.get(), image, image_dtype == DAD3D_DTYPE_U8, vertices, m->d_tex_tri[indexing].get(), texture,
                                 texture_dtype == DAD3D_DTYPE_U8, texture_batched ? (size_t)tex_h * tex_w * tex_c : 0, depth, batch, h, w, c, tex_h,
                                 tex_w, tex_c, mapping_type == 0, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_mesh_debug_trace(dad3d_mesh* m, unsigned long long* device_buffer) {
    DAD3D_REQUIRE(m, "null handle");
    m->d_trace = device_buffer;
    return DAD3D_OK;
}

dad3d_status dad3d_mesh_normal_plan(dad3d_mesh* m, int entry, int batch, int h, int w, int* form, int* chunks, int* built_mask) {
    DAD3D_REQUIRE(m && form && chunks && built_mask, "dad3d_mesh_normal_plan: null argument");
    DAD3D_REQUIRE(entry == DAD3D_PLAN_GET_NORMAL || entry == DAD3D_PLAN_PHONG || entry == DAD3D_PLAN_RENDER,
                  "dad3d_mesh_normal_plan: unknown entry %d", entry);
    DAD3D_REQUIRE(entry == DAD3D_PLAN_RENDER ? (h >= 1 && w >= 1) : batch >= 1, "dad3d_mesh_normal_plan: batch or image size below 1");
    DAD3D_REQUIRE(m->nver > 0 && (entry != DAD3D_PLAN_RENDER || m->ntri > 0), "dad3d_mesh_normal_plan: an empty mesh launches nothing");
    DeviceGuard guard(m->device);
    const NormalPlan p = entry == DAD3D_PLAN_GET_NORMAL ? plan_get_normal(m->dev(), m->nc, batch)
                         : entry == DAD3D_PLAN_PHONG    ? plan_phong(m->dev(), m->nc, false, batch)
                                                        : plan_render_light(m->dev(), m->nc, h, w);
    *form = p.form;
    *chunks = p.form == DAD3D_FORM_REFUSED ? 0 : p.chunks;
    *built_mask = 0;
    for (int k = 0; k < kNormalChunkings; ++k)
        if (m->nc[k].chunks) *built_mask |= 1 << k;
    return DAD3D_OK;
}

dad3d_status dad3d_mesh_phong_light(dad3d_mesh* m, float* light, const float* vertices, const float* normals,
                                    int batch, const dad3d_light* cfg, void* stream) {
    DAD3D_REQUIRE(m && cfg && batch >= 0, "dad3d_mesh_phong_light: bad argument");
    if (batch == 0 || m->nver == 0) return DAD3D_OK;
    DAD3D_REQUIRE(light && vertices && normals, "dad3d_mesh_phong_light: null buffer");
    DeviceGuard guard(m->device);
    return launch_phong(m->dev(), m->nc, light, vertices, normals, nullptr, batch, *cfg, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_mesh_normal_phong_light(dad3d_mesh* m, float* light, float* ver_normal, const float* vertices,
                                           int batch, const dad3d_light* cfg, void* stream) {
    DAD3D_REQUIRE(m && cfg && batch >= 0, "dad3d_mesh_normal_phong_light: bad argument");
    if (batch == 0 || m->nver == 0) return DAD3D_OK;
    DAD3D_REQUIRE(light && vertices, "dad3d_mesh_normal_phong_light: null buffer");
    DeviceGuard guard(m->device);
    return launch_phong(m->dev(), m->nc, light, vertices, nullptr, ver_normal, batch, *cfg, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_uvmap_create(const int32_t* faces, int ntri, int nver, const int32_t* cand_texel, const int32_t* cand_verts,
                                const double* cand_bary, int n, int img_size, int device, dad3d_uvmap** out) {
    DAD3D_REQUIRE(out, "dad3d_uvmap_create: null output handle");
    *out = nullptr;
    DAD3D_REQUIRE(ntri >= 0 && nver >= 0 && n >= 0, "dad3d_uvmap_create: negative size (ntri %d, nver %d, n %d)", ntri, nver, n);
    DAD3D_REQUIRE(img_size > 0 && img_size <= 46340, "dad3d_uvmap_create: texture size %d outside 1..46340", img_size);
    DAD3D_REQUIRE((faces || ntri == 0) && ((cand_texel && cand_verts && cand_bary) || n == 0), "dad3d_uvmap_create: null argument");
    for (size_t i = 0; i < 3 * (size_t)ntri; ++i)
        DAD3D_REQUIRE(faces[i] >= 0 && faces[i] < nver, "dad3d_uvmap_create: face %zu names vertex %d outside [0,%d)", i / 3,
                      faces[i], nver);
    const int n_tex = img_size * img_size;
    for (int i = 0; i < n; ++i) {
        DAD3D_REQUIRE(cand_texel[i] >= 0 && cand_texel[i] < n_tex, "dad3d_uvmap_create: candidate %d on texel %d outside [0,%d)", i,
                      cand_texel[i], n_tex);
        for (int c = 0; c < 3; ++c)
            DAD3D_REQUIRE(cand_verts[3 * (size_t)i + c] >= 0 && cand_verts[3 * (size_t)i + c] < nver,
                          "dad3d_uvmap_create: candidate %d names vertex %d outside [0,%d)", i, cand_verts[3 * (size_t)i + c], nver);
    }
    DAD3D_SELECT_DEVICE(device);
    const plan::UvAdjacency adj = plan::uv_adjacency(faces, ntri, nver);
    const plan::UvTexelTables tex = plan::uv_texel_tables(cand_texel, cand_verts, cand_bary, n, n_tex);
    std::unique_ptr<dad3d_uvmap> m(new dad3d_uvmap);
    m->device = device, m->nver = nver, m->size = img_size, m->n_cand = n, m->ntri = ntri;
    dad3d_status st;
    if ((st = m->d_faces.upload(std::vector<int>(faces, faces + 3 * (size_t)ntri))) || (st = m->d_adj_ptr.upload(adj.ptr)) ||
        (st = m->d_adj.upload(adj.adj)) || (st = m->d_texel_ptr.upload(tex.tptr)) || (st = m->d_cand_verts.upload(tex.verts)) ||
        (st = m->d_cand_bary.upload(tex.bary)))
        return st;
    *out = m.release();
    return DAD3D_OK;
}

void dad3d_uvmap_destroy(dad3d_uvmap* m) { delete m; }

int dad3d_uvmap_size(const dad3d_uvmap* m) { return m ? m->size : 0; }

dad3d_status dad3d_uvmap_vertex_normals(dad3d_uvmap* m, double* normals, const float* vertices, int batch, void* stream) {
    DAD3D_REQUIRE(m && batch >= 0, "dad3d_uvmap_vertex_normals: bad argument");
    DAD3D_REQUIRE(batch <= 65535, "dad3d_uvmap_vertex_normals: batch beyond the launch grid");
    if (batch == 0 || m->nver == 0) return DAD3D_OK;
    DAD3D_REQUIRE(normals && vertices, "dad3d_uvmap_vertex_normals: null argument");
    DAD3D_SELECT_DEVICE(m->device);
    UvNormalArgs a{m->d_adj_ptr.get(), m->d_adj.get(), vertices, normals, batch, m->nver};
    return launch_uv_vertex_normals(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_uvmap_bake(dad3d_uvmap* m, uint8_t* texture, const float* vertices, const double* normals, const uint8_t* images,
                              const int32_t* hw, int batch, int h, int w, void* stream) {
    DAD3D_REQUIRE(m && batch >= 0 && h > 0 && w > 0, "dad3d_uvmap_bake: bad argument (batch %d, h %d, w %d)", batch, h, w);
    DAD3D_REQUIRE(uv_bake_grid_y(batch, kUvBakeChunk) <= 65535, "dad3d_uvmap_bake: batch beyond the launch grid");
    if (batch == 0) return DAD3D_OK;
    DAD3D_REQUIRE(texture && images && ((vertices && normals) || m->n_cand == 0), "dad3d_uvmap_bake: null argument");
    DAD3D_SELECT_DEVICE(m->device);
    UvBakeArgs a{m->d_texel_ptr.get(), m->d_cand_verts.get(), m->d_cand_bary.get(), vertices, normals, images, hw, texture,
                 batch, m->nver, m->size, h, w, kUvBakeChunk};
    return launch_uv_bake(a, static_cast<hipStream_t>(stream));
}

// the scalars and the host frame table of the bakes from frames: a bad one is refused before the handle is looked at or any device work starts
static dad3d_status uv_frames_checked(const char* who, const int64_t* frames_host, int n_frames, int n_heads) {
    DAD3D_REQUIRE(n_frames >= 0 && n_heads >= 0, "%s: negative count (%d frames, %d heads)", who, n_frames, n_heads);
    DAD3D_REQUIRE(n_heads <= 65535, "%s: %d heads, beyond the launch grid of 65535", who, n_heads);
    DAD3D_REQUIRE(n_frames == 0 || frames_host, "%s: null host frame table", who);
    // the shapes as frames_check_shapes reads them, without the raster chain's tile limits: nothing here works in tiles
    for (int f = 0; f < n_frames; ++f) {
        const int64_t addr = frames_host[4 * (size_t)f], h = frames_host[4 * (size_t)f + 1], w = frames_host[4 * (size_t)f + 2],
                      stride = frames_host[4 * (size_t)f + 3];
        DAD3D_REQUIRE(addr != 0, "%s: frame %d has no address", who, f);
        DAD3D_REQUIRE(h >= 1 && w >= 1 && h <= INT32_MAX && w <= INT32_MAX, "%s: frame %d is %lld x %lld pixels", who, f, (long long)h, (long long)w);
        DAD3D_REQUIRE(stride >= 3 * w, "%s: frame %d has a row stride of %lld bytes for %lld pixels of 3 bytes", who, f, (long long)stride,
                      (long long)w);
    }
    return DAD3D_OK;
}

dad3d_status dad3d_uvmap_bake_frames(dad3d_uvmap* m, uint8_t* texture, float* score, const float* vertices, const double* normals,
                                     const int64_t* frames, const int64_t* frames_host, int n_frames, const int32_t* image_index, int n_heads,
                                     int32_t* flags, void* stream) {
    const char* who = "dad3d_uvmap_bake_frames";
    if (dad3d_status st = uv_frames_checked(who, frames_host, n_frames, n_heads)) return st;
    DAD3D_REQUIRE(m, "%s: null handle", who);
    if (n_heads == 0) return DAD3D_OK;
    DAD3D_REQUIRE(texture && image_index && flags && ((vertices && normals) || m->n_cand == 0), "%s: null buffer", who);
    DAD3D_REQUIRE(n_frames == 0 || frames, "%s: null device frame table", who);
    DAD3D_SELECT_DEVICE(m->device);
    UvBakeFramesArgs a{m->d_texel_ptr.get(), m->d_cand_verts.get(), m->d_cand_bary.get(), vertices, normals, reinterpret_cast<const long long*>(frames), image_index,
                       texture, score, flags, n_heads, n_frames, m->nver, m->size};
    return launch_uv_bake_frames(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_uvmap_depth_frames(dad3d_uvmap* m, float* depth, int32_t* window, const float* vertices, const int64_t* frames,
                                      const int64_t* frames_host, int n_frames, const int32_t* image_index, int n_heads, int depth_side,
                                      int32_t* flags, void* stream) {
    const char* who = "dad3d_uvmap_depth_frames";
    if (dad3d_status st = uv_frames_checked(who, frames_host, n_frames, n_heads)) return st;
    DAD3D_REQUIRE(depth_side >= 1 && depth_side <= DAD3D_BAKE_MAX_DEPTH_SIDE, "%s: depth_side %d outside 1..%d", who, depth_side,
                  DAD3D_BAKE_MAX_DEPTH_SIDE);
    DAD3D_REQUIRE(n_heads == 0 || (depth && window && image_index && flags), "%s: null buffer", who);
    DAD3D_REQUIRE(n_heads == 0 || n_frames == 0 || frames, "%s: null device frame table", who);
    DAD3D_REQUIRE(m, "%s: null handle", who);
    if (n_heads == 0) return DAD3D_OK;
    DAD3D_REQUIRE(vertices || m->nver == 0, "%s: null vertices", who);
    DAD3D_SELECT_DEVICE(m->device);
    UvDepthFramesArgs a{m->d_faces.get(), vertices, reinterpret_cast<const long long*>(frames), image_index, depth, window, flags,
                        n_heads, n_frames, m->nver, m->ntri, depth_side};
    return launch_uv_depth_frames(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_uvmap_bake_frames_occluded(dad3d_uvmap* m, uint8_t* texture, float* score, const float* vertices, const double* normals,
                                              const int64_t* frames, const int64_t* frames_host, int n_frames, const int32_t* image_index,
                                              int n_heads, const float* depth, const int32_t* window, const int32_t* depth_flags, int depth_side,
                                              double depth_bias, double slope_bias, int32_t* flags, void* stream) {
    const char* who = "dad3d_uvmap_bake_frames_occluded";
    if (dad3d_status st = uv_frames_checked(who, frames_host, n_frames, n_heads)) return st;
    DAD3D_REQUIRE(depth_side >= 1 && depth_side <= DAD3D_BAKE_MAX_DEPTH_SIDE, "%s: depth_side %d outside 1..%d", who, depth_side,
                  DAD3D_BAKE_MAX_DEPTH_SIDE);
    DAD3D_REQUIRE(std::isfinite(depth_bias) && depth_bias >= 0.0 && std::isfinite(slope_bias) && slope_bias >= 0.0,
                  "%s: depth_bias %g and slope_bias %g must be finite and not negative", who, depth_bias, slope_bias);
    DAD3D_REQUIRE(n_heads == 0 || (texture && image_index && flags && depth && window && depth_flags), "%s: null buffer", who);
    DAD3D_REQUIRE(n_heads == 0 || n_frames == 0 || frames, "%s: null device frame table", who);
    DAD3D_REQUIRE(m, "%s: null handle", who);
    if (n_heads == 0) return DAD3D_OK;
    DAD3D_REQUIRE((vertices && normals) || m->n_cand == 0, "%s: null vertices or normals", who);
    DAD3D_SELECT_DEVICE(m->device);
    UvBakeOccludedArgs a{{m->d_texel_ptr.get(), m->d_cand_verts.get(), m->d_cand_bary.get(), vertices, normals, reinterpret_cast<const long long*>(frames),
                          image_index, texture, score, flags, n_heads, n_frames, m->nver, m->size},
                         depth, window, depth_flags, depth_side, depth_bias, slope_bias};
    return launch_uv_bake_frames_occluded(a, static_cast<hipStream_t>(stream));
}

static dad3d_status overlay_checked(const char* who, const uint8_t* src, uint8_t* dst, int batch, int h, int w, const float* points,
                                    int n_points, int n_prims) {
    DAD3D_REQUIRE(batch >= 0 && batch <= 65535, "%s: batch %d outside 0 .. 65535", who, batch);
    DAD3D_REQUIRE(h >= 1 && w >= 1 && h <= DAD3D_OVERLAY_MAX_COORD && w <= DAD3D_OVERLAY_MAX_COORD, "%s: an image of %d x %d (1 .. %d)", who, h,
                  w, DAD3D_OVERLAY_MAX_COORD);
    DAD3D_REQUIRE(n_points >= 0 && n_prims >= 0 && n_points <= 0x3fffffff && n_prims <= 0x3fffffff, "%s: %d points, %d primitives", who,
                  n_points, n_prims);
    if (batch == 0) return DAD3D_OK;
    DAD3D_REQUIRE(src && dst, "%s: null image", who);
    DAD3D_REQUIRE(n_prims == 0 || n_points == 0 || points, "%s: null point table", who);
    return DAD3D_OK;
}

dad3d_status dad3d_overlay_segments(const uint8_t* src, uint8_t* dst, int batch, int h, int w, const float* points, int n_points,
                                    const int32_t* edges, int n_edges, const uint8_t* colors, uint32_t color, int thickness, int device,
                                    void* stream) {
    DAD3D_REQUIRE(thickness >= 0 && thickness <= 255, "dad3d_overlay_segments: thickness %d outside 0 (anti-aliased) .. 255", thickness);
    const dad3d_status st = overlay_checked("dad3d_overlay_segments", src, dst, batch, h, w, points, n_points, n_edges);
    if (st != DAD3D_OK || batch == 0) return st;
    DAD3D_REQUIRE(n_edges == 0 || edges, "dad3d_overlay_segments: null edge list");
    DAD3D_REQUIRE(n_edges == 0 || aligned(edges, 4), "dad3d_overlay_segments: misaligned edge list");
    DAD3D_SELECT_DEVICE(device);
    OverlaySegmentsArgs a{src, dst, points, edges, colors, color & 0xffffffu, batch, h, w, n_points, n_edges, thickness};
    return launch_overlay_segments(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_overlay_discs(const uint8_t* src, uint8_t* dst, int batch, int h, int w, const float* points, int n_points,
                                 const int32_t* index, int n_discs, int radius, uint32_t color, int device, void* stream) {
    DAD3D_REQUIRE(radius >= 1 && radius <= DAD3D_OVERLAY_MAX_COORD, "dad3d_overlay_discs: radius %d outside 1 .. %d", radius,
                  DAD3D_OVERLAY_MAX_COORD);
    const dad3d_status st = overlay_checked("dad3d_overlay_discs", src, dst, batch, h, w, points, n_points, n_discs);
    if (st != DAD3D_OK || batch == 0) return st;
    DAD3D_REQUIRE(index || n_discs <= n_points, "dad3d_overlay_discs: %d discs from %d points without an index list", n_discs, n_points);
    DAD3D_SELECT_DEVICE(device);
    OverlayDiscsArgs a{src, dst, points, index, color & 0xffffffu, batch, h, w, n_points, n_discs, radius};
    return launch_overlay_discs(a, static_cast<hipStream_t>(stream));
}

}  // extern "C"
