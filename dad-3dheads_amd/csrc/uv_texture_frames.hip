// The UV-texture bake (uv_texture.hip `bake_kernel`, inference/uv_texture.py `_compute_texture_map`) for heads that name their frames:
// head k reads the frame `image_index[k]` of the frame table of dad3d_preprocess_boxes {address, h, w, row stride} -- frames of any
// sizes and row strides, nothing gathered into a batch -- and owns texture k.
//
//   bake_frames_kernel   the work split of bake_kernel: a lane owns four consecutive texels of one head (grid y), each texel's
//                        candidates are walked in DESCENDING order and the first that passes both tests (uv_sample, against the
//                        frame's own h and w) is the reference's last writer. The head's frame entry is uniform for the workgroup
//                        and read once. No atomics: a lane owns its texels and head k owns texture k.
//     score == null      plain bake: every byte of texture k is written, the pixel where there is a candidate, zeros elsewhere (and
//                        everywhere for a head whose index names no frame).
//     score != null      "best view wins": s = (float)n_dot_view of the chosen candidate replaces the texel's bytes and score iff
//                        s > score (a NaN never does, a tie keeps the older sample); a texel without a candidate and a head without
//                        a frame keep their state.
//
// Compiled with -ffp-contract=off (uv_texture.hpp): the candidate's point and normal are NumPy's float64 sums of products.
#include "common.hpp"
#include "uv_texture.hpp"

namespace dad3d {
namespace {

constexpr int kThreads = kUvBakeThreads;
constexpr int kTexels = kUvBakeTexels;

__global__ __launch_bounds__(kThreads) void bake_frames_kernel(UvBakeFramesArgs a) {
    const int k = blockIdx.y;
    const int f = a.image_index[k];
    const bool has_frame = f >= 0 && f < a.n_frames;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.flags[k] = has_frame ? 0 : DAD3D_BAKE_FLAG_INDEX;
    if (!has_frame && a.score) return;  // accumulate: a flagged head changes no byte of its texture or score
    const int n_tex = a.size * a.size;
    const int t0 = (blockIdx.x * kThreads + threadIdx.x) * kTexels;
    if (t0 >= n_tex) return;
    const int nt = min(kTexels, n_tex - t0);
    // the frame entry: workgroup-uniform scalar loads. A device table that disagrees with the host's checked copy can only shrink
    // the picture to nothing (no candidate passes 0 < x < 0).
    const uint8_t* img = nullptr;
    long long stride = 0;
    int h = 0, w = 0;
    if (has_frame) {
        const long long* fr = a.frames + 4 * (size_t)f;
        const long long fh = fr[1], fw = fr[2];
        if (fr[0] != 0 && fh >= 1 && fw >= 1 && fh <= INT_MAX && fw <= INT_MAX && fr[3] >= 3 * fw)
            img = reinterpret_cast<const uint8_t*>(fr[0]), h = (int)fh, w = (int)fw, stride = fr[3];
    }
    const float* vb = a.vertices + (size_t)k * a.n_verts * 3;
    const double* nb = a.normals + (size_t)k * a.n_verts * 3;
    auto pixel_at = [&](int y, int x) { return img + (long long)y * stride + 3ll * x; };  // rows `stride` bytes apart
    unsigned rgb[kTexels];
    float s[kTexels];
    bool hit[kTexels];
#pragma unroll
    for (int i = 0; i < kTexels; ++i) {
        int px = -1;
        double ndv = 0.0;
        if (i < nt && w > 0) {
            const int end = a.texel_ptr[t0 + i + 1];
            for (int j = a.texel_ptr[t0 + i]; px < 0 && j < end; ++j)
                px = uv_sample(uv_load_cand(a.cand_verts, a.cand_bary, j), vb, nb, h, w, pixel_at, ndv);
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

dad3d_status launch_uv_bake_frames(const UvBakeFramesArgs& a, hipStream_t s) {
    const int lanes = (a.size * a.size + kTexels - 1) / kTexels;
    const dim3 grid((lanes + kThreads - 1) / kThreads, a.n_heads);
    hipLaunchKernelGGL(bake_frames_kernel, grid, dim3(kThreads), 0, s, a);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

}  // namespace dad3d
