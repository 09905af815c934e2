// One coordinate of `readjust_landmarks_to_the_input_image` with the clip in front of it (predictor.py:132-133,147-152), shared by
// heatmap_points.hip (an image is its own frame) and preprocess_boxes.hip (a crop's points moved into its frame).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace dad3d {

// float32 v = s * mul; clip to [0, limit] in float32; widen; subtract the pad; divide by the float64 scale; truncate toward zero
__device__ __forceinline__ int readjusted_coordinate(float s, float mul, float limit, double pad, double scale) {
    float v = s * mul;
    v = v < 0.0f ? 0.0f : v;  // np.clip == minimum(maximum(v, 0), limit): a NaN passes through both
    v = v > limit ? limit : v;
    const double d = ((double)v - pad) / scale;
    if (d != d) return INT32_MIN;  // numpy's cast of a NaN is undefined: this project's choice
    if (d >= 2147483647.0) return INT32_MAX;
    if (d <= -2147483648.0) return INT32_MIN;
    return (int)d;  // toward zero
}

}  // namespace dad3d
