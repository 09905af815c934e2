// Ground-truth keypoints of a DAD-3DNet training batch for gfx950 (MI355X): the geometry of FlameDataset._parse_anno /
// _transform / _form_anno_dict (model_training/data/flame_dataset.py:100-199) for B items in ONE launch.
//
// For item b with full-image height H, crop (x, y, w, h) and output size S, and for the K subset points followed by the
// N mesh vertices:
//   1. world = MV . [v; 1]                                                      _load_mesh (:115-127)
//   2. subset: 68-landmark mode: the barycentric combination of the WORLD xyz of the three corners of each embedding face,
//      ((c0 w0 + c1 w1) + c2 w2) in fp32 products (get_68_landmarks, data/utils.py:120-132, on the world vertices), then w := 1
//      (:151-157); index mode: world[index], the full homogeneous row (:159). The combination comes BEFORE P: projecting a
//      barycentric combination is not the combination of projections.
//   3. clip = P . world; xy = clip.xy / clip.w; y := H - y; xy -= (x, y)       _project_vertices_onto_image (:130-141)
//   4. presence (subset only): 0 < x < w and 0 < y < h, in crop pixels before any resize (:167-170)
//   5. albumentations 1.0.0 keypoint geometry, in float64 and rounded to fp32 once (np.array(..., dtype=np.float32) at
//      :189-190): under the pinned numpy 1.22 an np.float32 keypoint times a Python float is a float64.
//        longest_max_size  (x s + pad_left, y s + pad_top), s = S / max(h, w)   LongestMaxSize.apply_to_keypoint + PadIfNeeded
//        resize            (x S/w, y S/h)                                        Resize.apply_to_keypoint
//   6. full [B,N,2] = the transformed vertices (TARGET_2D_FULL_LANDMARKS); subset_px [B,K,2] (the heatmap's input);
//      subset_norm [B,K,2] = subset_px / S as a correctly rounded fp32 division (TARGET_2D_LANDMARKS, :198); presence [B,K].
// Steps 1 and 3 are projection_math.hpp, shared with project_vertices_kernel. Numerics: sgemm sites 1 and 2 there (numpy may
// fuse or reorder the 4-term sums) are where agreement is fp32 rounding rather than bitwise; everything after the projection
// is exact restatement (the fp32 divide, flip and shift; the float64 scale and pad; one rounding to fp32). The unit is built
// with -ffp-contract=off, so the barycentric products and the float64 multiply-add stay unfused, as numpy and torch run them.
//
// One lane per (item, point); blockIdx.y is the item, so a workgroup never spans items and the matrices and the frame row
// are workgroup-uniform (scalar loads). A streaming kernel: 12 B read and 8 B written per vertex plus 128 B of matrices
// per item; no atomics, no allocation, no host sync. Non-finite inputs stay in their own item: NaN / inf coordinates fail
// every presence comparison.
#include "common.hpp"
#include "projection_math.hpp"

namespace dad3d {
namespace {

// A vertex id out of range reads nothing and gives a NaN point (its item's keypoint is then absent, never a stray read).
__device__ __forceinline__ float3 load_vertex(const float* verts, int id, int nver) {
    if ((unsigned)id >= (unsigned)nver) return make_float3(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""));
    const float* q = verts + (size_t)id * 3;
    return make_float3(q[0], q[1], q[2]);
}

__global__ __launch_bounds__(256) void gt_keypoints_kernel(GtKeypointsArgs a) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n_subset + a.nver) return;
    const float* mv = a.model_view + (size_t)b * 16;
    const float* pm = a.projection + (size_t)b * 16;
    const int* fr = a.frames + (size_t)b * 8;  // image height, crop x, y, w, h, pad_top, pad_left, 0
    const float* verts = a.vertices + (size_t)b * a.nver * 3;
    float w4[4];
    const bool subset = p < a.n_subset;
    if (subset && a.corners) {
        float c[3][4];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float3 q = load_vertex(verts, a.corners[p * 3 + k], a.nver);
            model_view_point(mv, q.x, q.y, q.z, c[k]);
        }
        const float* wt = a.weights + p * 3;
#pragma unroll
        for (int i = 0; i < 3; ++i) w4[i] = (c[0][i] * wt[0] + c[1][i] * wt[1]) + c[2][i] * wt[2];
        w4[3] = 1.0f;
    } else {
        const float3 q = load_vertex(verts, subset ? a.index[p] : p - a.n_subset, a.nver);
        model_view_point(mv, q.x, q.y, q.z, w4);
    }
    const float2 xy = project_onto_image(pm, w4, (float)fr[0], (float)fr[1], (float)fr[2]);
    const int w = fr[3], h = fr[4];
    double sx, sy, px = 0.0, py = 0.0;
    if (a.mode == DAD3D_RESIZE_LONGEST_MAX_SIZE) {
        sx = sy = (double)a.out_size / (double)max(w, h);
        px = (double)fr[6], py = (double)fr[5];
    } else {
        sx = (double)a.out_size / (double)w, sy = (double)a.out_size / (double)h;
    }
    double ox = (double)xy.x * sx, oy = (double)xy.y * sy;
    if (a.mode == DAD3D_RESIZE_LONGEST_MAX_SIZE) ox = ox + px, oy = oy + py;  // PadIfNeeded adds the int pads, even 0
    const float2 o = make_float2((float)ox, (float)oy);
    if (!subset) {
        reinterpret_cast<float2*>(a.full)[(size_t)b * a.nver + (p - a.n_subset)] = o;
        return;
    }
    const size_t s = (size_t)b * a.n_subset + p;
    const float size = (float)a.out_size;
    reinterpret_cast<float2*>(a.subset_px)[s] = o;
    reinterpret_cast<float2*>(a.subset_norm)[s] = make_float2(o.x / size, o.y / size);
    a.presence[s] = (0.0f < xy.x && xy.x < (float)w && 0.0f < xy.y && xy.y < (float)h) ? 1 : 0;
}

}  // namespace

dad3d_status launch_gt_keypoints(const GtKeypointsArgs& a, int batch, hipStream_t s) {
    const int points = a.n_subset + a.nver;
    if (batch == 0 || points == 0) return DAD3D_OK;
    hipLaunchKernelGGL(gt_keypoints_kernel, dim3((points + 255) / 256, batch), dim3(256), 0, s, a);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

}  // namespace dad3d
