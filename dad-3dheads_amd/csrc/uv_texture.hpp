// What the UV-texture units (uv_texture.hip, uv_texture_frames.hip, uv_texture_occlusion.hip) share: the argument structs of their
// kernels, the launchers' declarations and the per-candidate routines of the bake -- the source pixel of a candidate, or -1 where the
// reference skips it, and the depth test of the occluded bake.
//
// A UNIT THAT CALLS uv_sample OR uv_hidden IS COMPILED WITH -ffp-contract=off: every product and sum rounds on its own, as NumPy's does.
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
// the depth maps of heads in frames (uv_texture_occlusion.hip): head k's nearest z per pixel of its window in the frame it names
struct UvDepthFramesArgs {
    const int* faces;         // [n_tri,3]
    const float* vertices;    // [N,V,3] frame pixel x, pixel y, z with the viewer at -z
    const long long* frames;  // [M][4]: only h and w are read
    const int* image_index;   // [N]
    float* depth;             // [N,D,D]
    int* window;              // [N,4] {x0, y0, ww, wh}
    int* flags;               // [N]
    int n_heads, n_frames, n_verts, n_tri, depth_side;
};
// the bake from frames with the depth test (uv_texture_occlusion.hip)
struct UvBakeOccludedArgs {
    UvBakeFramesArgs bake;
    const float* depth;      // [N,D,D] of UvDepthFramesArgs, read only
    const int* window;       // [N,4]
    const int* depth_flags;  // [N]
    int depth_side;
    double depth_bias, slope_bias;
};
constexpr int kUvBakeChunk = 8;  // images per bake workgroup: the table is read once per chunk
constexpr int kUvBakeThreads = 256;
constexpr int kUvBakeTexels = 4;  // texels per lane: 12 output bytes, three dword stores
int uv_bake_grid_y(int batch, int chunk);
dad3d_status launch_uv_vertex_normals(const UvNormalArgs& a, hipStream_t s);
dad3d_status launch_uv_bake(const UvBakeArgs& a, hipStream_t s);
dad3d_status launch_uv_bake_frames(const UvBakeFramesArgs& a, hipStream_t s);
dad3d_status launch_uv_depth_frames(const UvDepthFramesArgs& a, hipStream_t s);
dad3d_status launch_uv_bake_frames_occluded(const UvBakeOccludedArgs& a, hipStream_t s);

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

// The third test of the occluded bake, for a candidate that passed uv_sample's two with n_dot_view ndv: is its point behind the head's
// own surface at its pixel? d: the head's depth there (+inf where the map has none). The candidate's z and the normal's x and y are
// float64 sums of products in uv_sample's order; the comparison is false on NaN, so an uncovered pixel, ndv == +0 (a slope of inf, or
// NaN where slope_bias == 0 or nx == ny == 0) and a NaN anywhere leave the candidate visible.
__device__ __forceinline__ bool uv_hidden(const UvCand& c, const float* vb, const double* nb, double ndv, float d, double depth_bias,
                                          double slope_bias) {
    const double pz = ((double)vb[c.v0 * 3 + 2] * c.w0 + (double)vb[c.v1 * 3 + 2] * c.w1) + (double)vb[c.v2 * 3 + 2] * c.w2;
    const double nx = (nb[c.v0 * 3] * c.w0 + nb[c.v1 * 3] * c.w1) + nb[c.v2 * 3] * c.w2;
    const double ny = (nb[c.v0 * 3 + 1] * c.w0 + nb[c.v1 * 3 + 1] * c.w1) + nb[c.v2 * 3 + 1] * c.w2;
    return pz > (double)d + (depth_bias + slope_bias * ((fabs(nx) + fabs(ny)) / ndv));
}

}  // namespace
}  // namespace dad3d
