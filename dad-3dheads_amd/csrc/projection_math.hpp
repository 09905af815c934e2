// The reference's GT projection arithmetic (model_training/data/flame_dataset.py:115-141, `_load_mesh` and
// `_project_vertices_onto_image`), ONE copy for every kernel that projects annotation meshes (projection.hip,
// train_batch.hip):
//     world = MV . [v; 1]          clip = P . world          xy = clip.xy / clip.w          xy = (x, H - y) - (crop_x, crop_y)
// Each product is summed k = 0..3 in order, without contraction (the pragma holds even in a unit built with contraction on).
// Where this differs from the reference: numpy's matmul hands both 4x4 products to sgemm, which may fuse the multiply-adds
// and pick its own k order; agreement is to fp32 rounding (1e-3 px at image scale), not bitwise. The divide, the flip and
// the crop shift are single correctly rounded fp32 operations, as in numpy (the int32 crop corner is exact in fp32 and in
// the float64 loop numpy's `-=` picks for it).
#pragma once

#include <hip/hip_runtime.h>

namespace dad3d {

// `_load_mesh` (flame_dataset.py:121-123): one point through the row-major model-view matrix mv[16]. sgemm site 1.
__device__ __forceinline__ void model_view_point(const float* mv, float x, float y, float z, float w4[4]) {
#pragma clang fp contract(off)
    const float in[4] = {x, y, z, 1.0f};
#pragma unroll
    for (int i = 0; i < 4; ++i) w4[i] = ((mv[4 * i] * in[0] + mv[4 * i + 1] * in[1]) + mv[4 * i + 2] * in[2]) + mv[4 * i + 3] * in[3];
}

// `_project_vertices_onto_image` (flame_dataset.py:137-141): a world-space homogeneous point through the row-major
// projection pm[16] (sgemm site 2), the perspective divide, the image-space flip and the crop shift.
__device__ __forceinline__ float2 project_onto_image(const float* pm, const float w4[4], float height, float crop_x, float crop_y) {
#pragma clang fp contract(off)
    float c4[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) c4[i] = ((pm[4 * i] * w4[0] + pm[4 * i + 1] * w4[1]) + pm[4 * i + 2] * w4[2]) + pm[4 * i + 3] * w4[3];
    return make_float2(c4[0] / c4[3] - crop_x, (height - c4[1] / c4[3]) - crop_y);
}

}  // namespace dad3d
