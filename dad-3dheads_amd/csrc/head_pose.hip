// Head pose and similarity alignment on the device, the routines of pose_math.hpp:
//   head_pose_kernel    one lane per params row: the float32 rotation matrix of rot_mat_from_6dof, (roll, pitch, yaw) in degrees as
//                       scipy's from_matrix / as_euler("xyz") give them, and the ten arrow points `draw_pose` hands to the segment
//                       kernel. A row reads 24 bytes and writes at most 148; everything between lives in registers.
//   procrustes_kernel   one wave per item: lanes stride over the points, first pass the two means, second pass the two centred norms
//                       and the 3x3 covariance, each reduced by the wave butterfly of collectives.hpp; lane 0 runs the 3x3 SVD.
//                       An item's bits do not depend on the batch: a wave sees its own item only and the order of additions is fixed
//                       by the point count.
// head_pose_host and procrustes_host run the same code on the CPU, the wave's order of additions included.
//
// Compiled with -ffp-contract=off (pose_math.hpp): the host and the device round the same operations.
#include <climits>

#include "collectives.hpp"
#include "common.hpp"
#include "pose_math.hpp"

namespace dad3d {
namespace {

constexpr int kWave = 64;

__host__ __device__ __forceinline__ void head_pose_row(const HeadPoseArgs& a, long long i) {
    const float* p = a.params + i * a.row_stride + a.rot_offset;
    const float rot6[6] = {p[0], p[1], p[2], p[3], p[4], p[5]};
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 6; ++k) finite = finite && (rot6[k] - rot6[k] == 0.0f);
    float R[9];
    pose_rot6_to_matrix(rot6, R);
    double rpy[3];
    int flags = rpy_from_rotation(R, rpy);
    if (!finite) {
        flags = DAD3D_POSE_FLAG_NONFINITE;
        rpy[0] = rpy[1] = rpy[2] = __builtin_nan("");
    }
    int h = a.h, w = a.w;
    bool has_frame = true;
    if (a.frames) {  // the frame table of dad3d_preprocess_boxes; only a frame's size is read, never a pixel
        const int f = a.image_index[i];
        has_frame = f >= 0 && f < a.n_frames;
        if (has_frame) {
            const long long fh = a.frames[4 * (size_t)f + 1], fw = a.frames[4 * (size_t)f + 2];
            has_frame = fh >= 1 && fw >= 1 && fh <= INT_MAX && fw <= INT_MAX;
            h = (int)fh, w = (int)fw;
        }
        if (!has_frame) flags |= DAD3D_POSE_FLAG_INDEX;
    }
    if (a.rotation) {
#pragma unroll
        for (int k = 0; k < 9; ++k) a.rotation[i * 9 + k] = R[k];
    }
    if (a.rpy) a.rpy[i * 3] = rpy[0], a.rpy[i * 3 + 1] = rpy[1], a.rpy[i * 3 + 2] = rpy[2];
    if (a.points) {
        float pts[2 * kPosePoints];
        if (has_frame) {
            pose_arrow_points(rpy, h, w, pts);
        } else {
#pragma unroll
            for (int k = 0; k < 2 * kPosePoints; ++k) pts[k] = 0.0f;
        }
#pragma unroll
        for (int k = 0; k < 2 * kPosePoints; ++k) a.points[i * (2 * kPosePoints) + k] = pts[k];
    }
    if (a.flags) a.flags[i] = flags;
}

__global__ __launch_bounds__(kWave) void head_pose_kernel(HeadPoseArgs a) {
    const long long i = (long long)blockIdx.x * kWave + threadIdx.x;
    if (i < a.n) head_pose_row(a, i);
}

// a lane's share of the two passes, over the points lane, lane + 64, .. in ascending order. Pass 1: sum x (3), sum y (3); pass 2:
// |X0|^2, |Y0|^2, then the covariance row by row
__host__ __device__ __forceinline__ void procrustes_pass1(const double* x, const double* y, int n, int lane, double s[6]) {
#pragma unroll
    for (int k = 0; k < 6; ++k) s[k] = 0.0;
    for (int p = lane; p < n; p += kWave) {
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] += x[3 * (size_t)p + k], s[3 + k] += y[3 * (size_t)p + k];
    }
}
__host__ __device__ __forceinline__ void procrustes_pass2(const double* x, const double* y, int n, int lane, const double mu[6], double s[11]) {
#pragma unroll
    for (int k = 0; k < 11; ++k) s[k] = 0.0;
    for (int p = lane; p < n; p += kWave) {
        double dx[3], dy[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) dx[k] = x[3 * (size_t)p + k] - mu[k], dy[k] = y[3 * (size_t)p + k] - mu[3 + k];
        s[0] += dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2];
        s[1] += dy[0] * dy[0] + dy[1] * dy[1] + dy[2] * dy[2];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) s[2 + 3 * i + j] += dx[i] * dy[j];
    }
}
__host__ __device__ __forceinline__ void procrustes_finish(const ProcrustesArgs& a, int item, const double mu[6], const double s[11]) {
    const double cov[3][3] = {{s[2], s[3], s[4]}, {s[5], s[6], s[7]}, {s[8], s[9], s[10]}};
    double b, t[3][3], c[3];
    const int flag = procrustes_fit(mu, mu + 3, sqrt(s[0]), sqrt(s[1]), cov, a.n_points, &b, t, c);
    a.b[item] = b;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        a.c[(size_t)item * 3 + i] = c[i];
#pragma unroll
        for (int j = 0; j < 3; ++j) a.t[(size_t)item * 9 + 3 * i + j] = t[i][j];
    }
    a.flags[item] = flag;
}

__global__ __launch_bounds__(kWave) void procrustes_kernel(ProcrustesArgs a) {
    const int item = blockIdx.x, lane = threadIdx.x;
    const double* x = a.x + (size_t)item * a.n_points * 3;
    const double* y = a.y + (size_t)item * a.n_points * 3;
    double mu[6], s[11];
    procrustes_pass1(x, y, a.n_points, lane, mu);
#pragma unroll
    for (int k = 0; k < 6; ++k) mu[k] = wave_sum(mu[k]) / a.n_points;
    procrustes_pass2(x, y, a.n_points, lane, mu, s);
#pragma unroll
    for (int k = 0; k < 11; ++k) s[k] = wave_sum(s[k]);
    if (lane == 0) procrustes_finish(a, item, mu, s);
}

// the xor butterfly of wave_sum on a host array: every step adds lane ^ d to lane, offsets 32 .. 1
double host_wave_sum(double v[kWave]) {
    for (int d = kWave / 2; d >= 1; d >>= 1) {
        double next[kWave];
        for (int l = 0; l < kWave; ++l) next[l] = v[l] + v[l ^ d];
        for (int l = 0; l < kWave; ++l) v[l] = next[l];
    }
    return v[0];
}

}  // namespace

dad3d_status launch_head_pose(const HeadPoseArgs& a, hipStream_t s) {
    const unsigned blocks = (unsigned)(((long long)a.n + kWave - 1) / kWave);
    hipLaunchKernelGGL(head_pose_kernel, dim3(blocks), dim3(kWave), 0, s, a);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

dad3d_status launch_procrustes(const ProcrustesArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(procrustes_kernel, dim3((unsigned)a.batch), dim3(kWave), 0, s, a);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

void head_pose_host(const HeadPoseArgs& a) {
    for (long long i = 0; i < a.n; ++i) head_pose_row(a, i);
}

void procrustes_host(const ProcrustesArgs& a) {
    for (int item = 0; item < a.batch; ++item) {
        const double* x = a.x + (size_t)item * a.n_points * 3;
        const double* y = a.y + (size_t)item * a.n_points * 3;
        double lanes1[6][kWave], lanes2[11][kWave], mu[6], s[11];
        for (int lane = 0; lane < kWave; ++lane) {
            double part[6];
            procrustes_pass1(x, y, a.n_points, lane, part);
            for (int k = 0; k < 6; ++k) lanes1[k][lane] = part[k];
        }
        for (int k = 0; k < 6; ++k) mu[k] = host_wave_sum(lanes1[k]) / a.n_points;
        for (int lane = 0; lane < kWave; ++lane) {
            double part[11];
            procrustes_pass2(x, y, a.n_points, lane, mu, part);
            for (int k = 0; k < 11; ++k) lanes2[k][lane] = part[k];
        }
        for (int k = 0; k < 11; ++k) s[k] = host_wave_sum(lanes2[k]);
        procrustes_finish(a, item, mu, s);
    }
}

}  // namespace dad3d
