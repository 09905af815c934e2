// FaceMeshPredictor's image preprocessing for gfx950 (MI355X) in ONE launch for a batch of images of any sizes:
//
//   A.LongestMaxSize(S)  -> cv2.resize(INTER_LINEAR) of the uint8 image      (predictor.py:197; OpenCV resize.cpp: 8-bit path
//                           HResizeLinear<uchar,int,short> / VResizeLinear<uchar,int,short> with 11-bit coefficients)
//   A.PadIfNeeded(S, S)  -> centred, BORDER_CONSTANT 0                       (predictor.py:198)
//   A.Normalize(...)     -> (x - 255*mean) * (1 / (255*std)) in float32      (predictor.py:199; albumentations functional.normalize)
//   _array_to_batch      -> HWC -> CHW, batch dimension                      (predictor.py:80-84)
//
// One lane per output pixel (three channels), output rows contiguous per channel plane: a streaming kernel, 3 B read per
// tap (4 taps) and 12 B written per pixel; the batch of 64 x 256^2 is 50 MB of output, HBM-bound. Third-party cv2 and
// albumentations are absent from the image: the arithmetic is restated from their published sources; the test
// suite restates it once more in numpy and holds this kernel to it bit for bit (tests/test_preprocess.py).
#include "common.hpp"
#include "resize_taps.hpp"

namespace dad3d {
namespace {

__global__ __launch_bounds__(256) void preprocess_kernel(const long long* __restrict__ descs, int out_size, float3 mean255,
                                                         float3 inv_std255, float* __restrict__ out) {
#pragma clang fp contract(off)
    const int b = blockIdx.z;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= out_size) return;
    const long long* d = descs + (size_t)b * 8;
    const unsigned char* src = reinterpret_cast<const unsigned char*>(d[0]);
    const int h = (int)d[1], w = (int)d[2], nh = (int)d[3], nw = (int)d[4], top = (int)d[5], left = (int)d[6];
    const long long row_stride = d[7];
    float r = 0.0f, g = 0.0f, bl = 0.0f;  // PadIfNeeded: constant 0 before the normalisation
    const int dy = y - top, dx = x - left;
    if (dy >= 0 && dy < nh && dx >= 0 && dx < nw) {
        float ch[3];
        resized_pixel(src, row_stride, h, w, nh, nw, dx, dy, ch);
        r = ch[0], g = ch[1], bl = ch[2];
    }
    const size_t plane = (size_t)out_size * out_size;
    float* o = out + (size_t)b * 3 * plane + (size_t)y * out_size + x;
    o[0] = (r - mean255.x) * inv_std255.x;
    o[plane] = (g - mean255.y) * inv_std255.y;
    o[2 * plane] = (bl - mean255.z) * inv_std255.z;
}

}  // namespace

dad3d_status launch_preprocess(const long long* descs, int batch, int out_size, const float mean[3], const float std[3],
                               float* out, hipStream_t s) {
    float3 mean255, inv;
    normalize_constants(mean, std, mean255, inv);
    hipLaunchKernelGGL(preprocess_kernel, dim3((out_size + 255) / 256, out_size, batch), dim3(256), 0, s, descs, out_size, mean255,
                       inv, out);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

}  // namespace dad3d
