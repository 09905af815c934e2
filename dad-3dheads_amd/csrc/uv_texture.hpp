// What the two UV-texture units (uv_texture.hip, uv_texture_frames.hip) share: the argument structs of their kernels, the launchers'
// declarations and the per-candidate routine of the bake -- the source pixel of a candidate, or -1 where the reference skips it.
//
// A UNIT THAT CALLS uv_sample IS COMPILED WITH -ffp-contract=off: every product and sum rounds on its own, as NumPy's does.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/dad3d.h"

namespace dad3d {

// the reference demo's UV-texture bake, float64 like its NumPy
struct UvNormalArgs {
    const int* adj_ptr;   // [V+1] CSR rows: the faces of a vertex, ascending face index, each face once
    const int4* adj;      // [adj_ptr[V]] {corner 0, corner 1, corner 2, how often the face names the vertex}
    const float* vertices;  // [B,V,3]
    double* normals;        // [B,V,3]
    int batch, n_verts;
};
struct UvBakeArgs {
    const int* texel_ptr;     // [S*S+1] CSR rows: the candidates of a texel, DESCENDING candidate index
    const int* cand_verts;    // [n,3] in texel-list order
    const double* cand_bary;  // [n,3] in texel-list order
    const float* vertices;    // [B,V,3]
    const double* normals;    // [B,V,3]
    const uint8_t* images;    // [B,h,w,3]
    const int* hw;            // [B,2] per-item (height, width) inside the padded h x w, or null
    uint8_t* texture;         // [B,S,S,3], every byte written
    int batch, n_verts, size, h, w, chunk;
};
// the bake from frames (uv_texture_frames.hip): head k reads the frame image_index[k] names and owns texture k
struct UvBakeFramesArgs {
    const int* texel_ptr;        // the table of UvBakeArgs
    const int* cand_verts;
    const double* cand_bary;
    const float* vertices;       // [N,V,3]
    const double* normals;       // [N,V,3]
    const long long* frames;     // [M][4] {address, h, w, row stride in bytes}
    const int* image_index;      // [N]
    uint8_t* texture;            // [N,S,S,3]
    float* score;                // [N,S,S] n_dot_view of the sample a texel holds, or null: plain bake, every byte written
    int* flags;                  // [N]
    int n_heads, n_frames, n_verts, size;
};
constexpr int kUvBakeChunk = 8;  // images per bake workgroup: the table is read once per chunk
constexpr int kUvBakeThreads = 256;
constexpr int kUvBakeTexels = 4;  // texels per lane: 12 output bytes, three dword stores
int uv_bake_grid_y(int batch, int chunk);
dad3d_status launch_uv_vertex_normals(const UvNormalArgs& a, hipStream_t s);
dad3d_status launch_uv_bake(const UvBakeArgs& a, hipStream_t s);
dad3d_status launch_uv_bake_frames(const UvBakeFramesArgs& a, hipStream_t s);

namespace {

struct UvCand {
    int v0, v1, v2;
    double w0, w1, w2;
};

__device__ __forceinline__ UvCand uv_load_cand(const int* cand_verts, const double* cand_bary, int j) {
    const int* v = cand_verts + (size_t)j * 3;
    const double* w = cand_bary + (size_t)j * 3;
    return UvCand{v[0], v[1], v[2], w[0], w[1], w[2]};
}

// The source pixel of candidate c (r | g << 8 | b << 16), or -1 where it is skipped (back-facing or outside the strict bounds).
// vb, nb: the head's vertices and normals; its picture has h x w pixels and pixel_at(y, x) is the address of the three bytes of pixel
// (y, x) -- the caller's layout, a dense batch or a frame with a row stride in bytes; ndv: n_dot_view of the candidate (meaningful where
// a pixel is returned).
template <class PixelAt>
__device__ __forceinline__ int uv_sample(const UvCand& c, const float* vb, const double* nb, int h, int w, PixelAt&& pixel_at, double& ndv) {
    const double nz = (nb[c.v0 * 3 + 2] * c.w0 + nb[c.v1 * 3 + 2] * c.w1) + nb[c.v2 * 3 + 2] * c.w2;
    ndv = -nz;
    if (ndv < 0.0) return -1;  // -0.0 and NaN pass, as in the reference
    const double px = ((double)vb[c.v0 * 3] * c.w0 + (double)vb[c.v1 * 3] * c.w1) + (double)vb[c.v2 * 3] * c.w2;
    const double py = ((double)vb[c.v0 * 3 + 1] * c.w0 + (double)vb[c.v1 * 3 + 1] * c.w1) + (double)vb[c.v2 * 3 + 1] * c.w2;
    const double rx = rint(px), ry = rint(py);  // np.round: half to even
    // compared as doubles: NaN and +-inf fail here, where NumPy's astype(int) turns them into INT64_MIN
    if (!(rx > 0.0 && rx < (double)w && ry > 0.0 && ry < (double)h)) return -1;
    const uint8_t* p = pixel_at((int)ry, (int)rx);
    return p[0] | (p[1] << 8) | (p[2] << 16);
}

}  // namespace
}  // namespace dad3d
