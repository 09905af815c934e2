// The UV-texture bake of the reference demo (inference/uv_texture.py `UVTextureCreator._compute_texture_map`) for gfx950
// (MI355X), in float64 like the reference's NumPy:
//
//   vertex_normals_kernel  psbody-mesh's `Mesh.estimate_vertex_normals` (unpinned here: restated from psbody-mesh's
//                          published source): the unnormalised face normal cross(v1 - v0, v2 - v0), summed over the faces of
//                          a vertex in ascending face order as the scipy CSR product `faces_by_vertex * face_normals` does
//                          (y = 0; y += m * n_f, m = how often the face names the vertex), then n / sqrt((x*x + y*y) + z*z)
//                          with a zero norm replaced by 1. One lane per (image, vertex).
//   bake_kernel            the per-candidate loop. Each texel owns the list of its candidates in DESCENDING candidate order,
//                          so the first one that passes both tests is the reference's last writer: no atomics, no ordering
//                          hazard, every output byte written once. A lane owns four consecutive texels (12 output bytes) and
//                          walks a chunk of kBakeChunk images; the first candidate of each texel (three vertex ids and three
//                          float64 barycentrics) stays in registers for the whole chunk, so the table is read once per chunk.
//                          Per image it gathers vertex x and y, normal z and the source pixel.
//
// Compiled with -ffp-contract=off: every product and sum rounds on its own, as NumPy's does. The f64 division and sqrt lower
// to the correctly rounded sequences (v_div_scale/v_div_fmas/v_div_fixup; v_rsq_f64 with the Newton-Raphson refinement and
// fix-up), so the normals are bit-equal to the float64 restatement.
#include "common.hpp"
#include "uv_texture.hpp"

namespace dad3d {
namespace {

constexpr int kNormThreads = 256;
constexpr int kBakeThreads = kUvBakeThreads;
constexpr int kBakeTexels = kUvBakeTexels;

__global__ __launch_bounds__(kNormThreads) void vertex_normals_kernel(UvNormalArgs a) {
    const int v = blockIdx.x * kNormThreads + threadIdx.x;
    const int b = blockIdx.y;
    if (v >= a.n_verts) return;
    const float* vb = a.vertices + (size_t)b * a.n_verts * 3;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    const int e1 = a.adj_ptr[v + 1];
    for (int e = a.adj_ptr[v]; e < e1; ++e) {
        const int4 t = a.adj[e];  // the face's corners and how often it names v
        const double x0 = vb[t.x * 3], y0 = vb[t.x * 3 + 1], z0 = vb[t.x * 3 + 2];
        const double ax = (double)vb[t.y * 3] - x0, ay = (double)vb[t.y * 3 + 1] - y0, az = (double)vb[t.y * 3 + 2] - z0;
        const double bx = (double)vb[t.z * 3] - x0, by = (double)vb[t.z * 3 + 1] - y0, bz = (double)vb[t.z * 3 + 2] - z0;
        const double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
        const double m = (double)t.w;
        sx = sx + m * nx, sy = sy + m * ny, sz = sz + m * nz;
    }
    double norm = sqrt((sx * sx + sy * sy) + sz * sz);
    if (norm == 0.0) norm = 1.0;
    double* o = a.normals + ((size_t)b * a.n_verts + v) * 3;
    o[0] = sx / norm, o[1] = sy / norm, o[2] = sz / norm;
}

__global__ __launch_bounds__(kBakeThreads) void bake_kernel(UvBakeArgs a) {
    const int n_tex = a.size * a.size;
    const int t0 = (blockIdx.x * kBakeThreads + threadIdx.x) * kBakeTexels;
    if (t0 >= n_tex) return;
    const int nt = min(kBakeTexels, n_tex - t0);
    int beg[kBakeTexels], end[kBakeTexels];
    UvCand first[kBakeTexels];
#pragma unroll
    for (int k = 0; k < kBakeTexels; ++k) {
        beg[k] = end[k] = 0;
        first[k] = UvCand{0, 0, 0, 0.0, 0.0, 0.0};
        if (k < nt) {
            beg[k] = a.texel_ptr[t0 + k], end[k] = a.texel_ptr[t0 + k + 1];
            if (beg[k] < end[k]) first[k] = uv_load_cand(a.cand_verts, a.cand_bary, beg[k]);
        }
    }
    const int b1 = min(a.batch, (int)(blockIdx.y + 1) * a.chunk);
    for (int b = blockIdx.y * a.chunk; b < b1; ++b) {
        int h = a.h, w = a.w;
        if (a.hw) h = min(max(a.hw[b * 2], 0), a.h), w = min(max(a.hw[b * 2 + 1], 0), a.w);  // never past the padded image
        const float* vb = a.vertices + (size_t)b * a.n_verts * 3;
        const double* nb = a.normals + (size_t)b * a.n_verts * 3;
        const uint8_t* img = a.images + (size_t)b * a.h * a.w * 3;
        auto pixel_at = [&](int y, int x) { return img + ((size_t)y * a.w + x) * 3; };
        double ndv;
        unsigned rgb[kBakeTexels];
#pragma unroll
        for (int k = 0; k < kBakeTexels; ++k) {
            int px = -1;
            if (beg[k] < end[k]) {
                px = uv_sample(first[k], vb, nb, h, w, pixel_at, ndv);
                for (int j = beg[k] + 1; px < 0 && j < end[k]; ++j) px = uv_sample(uv_load_cand(a.cand_verts, a.cand_bary, j), vb, nb, h, w, pixel_at, ndv);
            }
            rgb[k] = px < 0 ? 0u : (unsigned)px;
        }
        const size_t o = ((size_t)b * n_tex + t0) * 3;
        uint8_t* out = a.texture + o;
        if (nt == kBakeTexels && (reinterpret_cast<uintptr_t>(out) & 3) == 0) {
            // 4 texels r g b r | g b r g | b r g b as three little-endian dwords
            const unsigned d0 = rgb[0] | (rgb[1] << 24);
            const unsigned d1 = (rgb[1] >> 8) | (rgb[2] << 16);
            const unsigned d2 = (rgb[2] >> 16) | (rgb[3] << 8);
            *reinterpret_cast<uint3*>(out) = make_uint3(d0, d1, d2);
        } else {
#pragma unroll
            for (int k = 0; k < kBakeTexels; ++k)
                if (k < nt) out[3 * k] = rgb[k] & 255, out[3 * k + 1] = (rgb[k] >> 8) & 255, out[3 * k + 2] = rgb[k] >> 16;
        }
    }
}

}  // namespace

dad3d_status launch_uv_vertex_normals(const UvNormalArgs& a, hipStream_t s) {
    const dim3 grid((a.n_verts + kNormThreads - 1) / kNormThreads, a.batch);
    hipLaunchKernelGGL(vertex_normals_kernel, grid, dim3(kNormThreads), 0, s, a);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

int uv_bake_grid_y(int batch, int chunk) { return (batch + chunk - 1) / chunk; }

dad3d_status launch_uv_bake(const UvBakeArgs& a, hipStream_t s) {
    const int lanes = (a.size * a.size + kBakeTexels - 1) / kBakeTexels;
    const dim3 grid((lanes + kBakeThreads - 1) / kBakeThreads, uv_bake_grid_y(a.batch, a.chunk));
    hipLaunchKernelGGL(bake_kernel, grid, dim3(kBakeThreads), 0, s, a);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

}  // namespace dad3d
