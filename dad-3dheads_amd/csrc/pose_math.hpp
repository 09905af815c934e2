// Head pose and similarity alignment for one item. __host__ __device__, so the code the kernels of head_pose.hip
// run is the code dad3d_head_pose_host / dad3d_procrustes_host run on a CPU. float64 behind the float32 rotation matrix. No array
// is indexed by a run-time value and every loop has a fixed trip count: the kernels keep everything in registers (no scratch).
// Units that include this are built with -ffp-contract=off: a sum of products is rounded product by product, on both sides.
//
// roll, pitch, yaw follow scipy's `Rotation.from_matrix(M).as_euler("xyz", degrees=True)` (model_training/model/flame.py:254-264),
// which is not the textbook atan2 of matrix entries:
//   1. M is replaced by its orthogonal polar factor U V^T (a float32 rotation matrix is orthogonal only to ~1e-7)
//   2. a quaternion (x, y, z, w) from the largest of m00, m11, m22, trace; normalised
//   3. the angles from the quaternion by the half-angle formulas of Bernardes and Viollet (PLoS ONE 17(11), 2022), each wrapped
//      once into [-pi, pi]; within 1e-7 rad of the lock the third angle is 0
// The polar factor comes from a one-sided cyclic Jacobi SVD (Hestenes): the columns of A V are made orthogonal by plane
// rotations, their lengths are the singular values and their directions U. kPoseSweeps sweeps of the three column pairs, always
// all of them: the method converges quadratically, so a float32 rotation matrix (off by 1e-7) is done after two, and eight held
// 20000 covariances with singular values spread over six decades orthogonal to 2e-15.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/dad3d.h"

namespace dad3d {

constexpr int kPoseSweeps = 8;
constexpr double kPosePi = 3.14159265358979323846;
constexpr double kPoseLockEps = 1e-7;      // scipy's `eps` of _get_angles, radians
constexpr double kPoseMinSingular = 1e-6;  // below it the polar factor of a pose matrix counts as undefined
constexpr int kPosePoints = 10;

struct Vec3d {
    double x, y, z;
};
struct Mat3d {  // three columns
    Vec3d c0, c1, c2;
};
struct Svd3 {
    Mat3d u, v;         // A = U diag(s) V^T, columns; s0 >= s1 >= s2 >= 0
    double s0, s1, s2;
    double det_sign;    // the sign of det A (0 for a singular or non-finite A)
};

__host__ __device__ __forceinline__ double dot3(const Vec3d& a, const Vec3d& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__host__ __device__ __forceinline__ Vec3d cross3(const Vec3d& a, const Vec3d& b) {
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__host__ __device__ __forceinline__ Vec3d scale3(const Vec3d& a, double s) { return {a.x * s, a.y * s, a.z * s}; }
__host__ __device__ __forceinline__ Vec3d div3(const Vec3d& a, double s) { return {a.x / s, a.y / s, a.z / s}; }
__host__ __device__ __forceinline__ double det3(const Mat3d& m) { return dot3(m.c0, cross3(m.c1, m.c2)); }
__host__ __device__ __forceinline__ bool finite_d(double v) { return v - v == 0.0; }

// one plane rotation of the columns p and q of B = A V (and of V) that makes them orthogonal
__host__ __device__ __forceinline__ void jacobi_pair(Vec3d& bp, Vec3d& bq, Vec3d& vp, Vec3d& vq) {
    const double alpha = dot3(bp, bp), beta = dot3(bq, bq), gamma = dot3(bp, bq);
    double c = 1.0, s = 0.0;
    if (gamma != 0.0) {
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));  // an infinite zeta: t = 0
        c = 1.0 / sqrt(1.0 + t * t);
        s = c * t;
    }
    const Vec3d np = {c * bp.x - s * bq.x, c * bp.y - s * bq.y, c * bp.z - s * bq.z};
    const Vec3d nq = {s * bp.x + c * bq.x, s * bp.y + c * bq.y, s * bp.z + c * bq.z};
    const Vec3d wp = {c * vp.x - s * vq.x, c * vp.y - s * vq.y, c * vp.z - s * vq.z};
    const Vec3d wq = {s * vp.x + c * vq.x, s * vp.y + c * vq.y, s * vp.z + c * vq.z};
    bp = np, bq = nq, vp = wp, vq = wq;
}

__host__ __device__ __forceinline__ void swap_columns(bool doit, Vec3d& a, Vec3d& b) {
    // component by component: a select between two whole columns is a select between their addresses, which pins both to memory
    const Vec3d ta = {doit ? b.x : a.x, doit ? b.y : a.y, doit ? b.z : a.z};
    const Vec3d tb = {doit ? a.x : b.x, doit ? a.y : b.y, doit ? a.z : b.z};
    a = ta, b = tb;
}

// A (columns) = U diag(s) V^T. Where a singular value is below 1e-14 of the largest, its column of U is not defined by A: it is
// completed to an orthonormal basis, the last one so that det U = det V (the polar factor U V^T is then a proper rotation).
__host__ __device__ __forceinline__ Svd3 svd3(const Mat3d& a) {
    Svd3 r;
    const double det = det3(a);
    r.det_sign = det > 0.0 ? 1.0 : det < 0.0 ? -1.0 : 0.0;
    Vec3d b0 = a.c0, b1 = a.c1, b2 = a.c2;
    Vec3d v0 = {1.0, 0.0, 0.0}, v1 = {0.0, 1.0, 0.0}, v2 = {0.0, 0.0, 1.0};
#pragma unroll
    for (int sweep = 0; sweep < kPoseSweeps; ++sweep) {
        jacobi_pair(b0, b1, v0, v1);
        jacobi_pair(b0, b2, v0, v2);
        jacobi_pair(b1, b2, v1, v2);
    }
    double n0 = dot3(b0, b0), n1 = dot3(b1, b1), n2 = dot3(b2, b2);
    // descending by length: three compare-and-swaps of whole columns
    bool sw = n0 < n1;
    swap_columns(sw, b0, b1), swap_columns(sw, v0, v1);
    double t = sw ? n1 : n0;
    n1 = sw ? n0 : n1, n0 = t;
    sw = n0 < n2;
    swap_columns(sw, b0, b2), swap_columns(sw, v0, v2);
    t = sw ? n2 : n0;
    n2 = sw ? n0 : n2, n0 = t;
    sw = n1 < n2;
    swap_columns(sw, b1, b2), swap_columns(sw, v1, v2);
    t = sw ? n2 : n1;
    n2 = sw ? n1 : n2, n1 = t;
    r.s0 = sqrt(n0), r.s1 = sqrt(n1), r.s2 = sqrt(n2);
    r.v = {v0, v1, v2};
    const double tiny = 1e-14 * r.s0;
    Vec3d u0 = {1.0, 0.0, 0.0}, u1, u2;
    if (r.s0 > 0.0) u0 = div3(b0, r.s0);
    if (r.s1 > tiny) {
        u1 = div3(b1, r.s1);
    } else {  // any unit vector across u0: the axis u0 leans on least, made orthogonal to it
        const double ax = fabs(u0.x), ay = fabs(u0.y), az = fabs(u0.z);
        const Vec3d e = (ax <= ay && ax <= az) ? Vec3d{1.0, 0.0, 0.0} : (ay <= az) ? Vec3d{0.0, 1.0, 0.0} : Vec3d{0.0, 0.0, 1.0};
        const double k = dot3(e, u0);
        const Vec3d w = {e.x - k * u0.x, e.y - k * u0.y, e.z - k * u0.z};
        u1 = div3(w, sqrt(dot3(w, w)));
    }
    if (r.s2 > tiny) {
        u2 = div3(b2, r.s2);
    } else {
        const double dv = det3(r.v);
        u2 = scale3(cross3(u0, u1), dv < 0.0 ? -1.0 : 1.0);
    }
    r.u = {u0, u1, u2};
    return r;
}

// Q = U V^T as rows: q[i][j] = sum_k U[i][k] V[j][k], the sum from left to right
__host__ __device__ __forceinline__ void polar_from_svd(const Svd3& r, double q[3][3]) {
    const double u[3][3] = {{r.u.c0.x, r.u.c1.x, r.u.c2.x}, {r.u.c0.y, r.u.c1.y, r.u.c2.y}, {r.u.c0.z, r.u.c1.z, r.u.c2.z}};
    const double v[3][3] = {{r.v.c0.x, r.v.c1.x, r.v.c2.x}, {r.v.c0.y, r.v.c1.y, r.v.c2.y}, {r.v.c0.z, r.v.c1.z, r.v.c2.z}};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) q[i][j] = u[i][0] * v[j][0] + u[i][1] * v[j][1] + u[i][2] * v[j][2];
}

// The orthogonal polar factor of m (rows m[i][j]). Returns false where it is undefined for a pose: a singular value below
// kPoseMinSingular or det m <= 0, the matrices on which scipy raises.
__host__ __device__ __forceinline__ bool polar3(const double m[3][3], double q[3][3], double* smallest, double* det_sign) {
    const Mat3d a = {{m[0][0], m[1][0], m[2][0]}, {m[0][1], m[1][1], m[2][1]}, {m[0][2], m[1][2], m[2][2]}};
    const Svd3 r = svd3(a);
    polar_from_svd(r, q);
    *smallest = r.s2, *det_sign = r.det_sign;
    return r.s2 >= kPoseMinSingular && r.det_sign > 0.0;
}

// scipy's from_matrix: quaternion (x, y, z, w) by the largest of m00, m11, m22, trace (the first of equals), normalised
__host__ __device__ __forceinline__ void quat_from_matrix(const double m[3][3], double q[4]) {
    const double d0 = m[0][0], d1 = m[1][1], d2 = m[2][2], d3 = m[0][0] + m[1][1] + m[2][2];
    double x, y, z, w;
    if (d3 > d0 && d3 > d1 && d3 > d2) {
        x = m[2][1] - m[1][2], y = m[0][2] - m[2][0], z = m[1][0] - m[0][1], w = 1.0 + d3;
    } else if (d0 >= d1 && d0 >= d2) {
        x = 1.0 - d3 + 2.0 * d0, y = m[1][0] + m[0][1], z = m[2][0] + m[0][2], w = m[2][1] - m[1][2];
    } else if (d1 >= d2) {
        y = 1.0 - d3 + 2.0 * d1, z = m[2][1] + m[1][2], x = m[0][1] + m[1][0], w = m[0][2] - m[2][0];
    } else {
        z = 1.0 - d3 + 2.0 * d2, x = m[0][2] + m[2][0], y = m[1][2] + m[2][1], w = m[1][0] - m[0][1];
    }
    const double n = sqrt(x * x + y * y + z * z + w * w);
    q[0] = x / n, q[1] = y / n, q[2] = z / n, q[3] = w / n;
}

__host__ __device__ __forceinline__ double wrap_pi(double a) { return a < -kPosePi ? a + 2.0 * kPosePi : a > kPosePi ? a - 2.0 * kPosePi : a; }

// scipy's as_euler("xyz") in radians from the quaternion; returns true where the lock branch was taken
__host__ __device__ __forceinline__ bool euler_xyz_from_quat(const double q[4], double angles[3]) {
    const double a = q[3] - q[1], b = q[0] + q[2], c = q[1] + q[3], d = q[2] - q[0];
    double a1 = 2.0 * atan2(hypot(c, d), hypot(a, b));
    const int lock = fabs(a1) <= kPoseLockEps ? 1 : fabs(a1 - kPosePi) <= kPoseLockEps ? 2 : 0;
    const double half_sum = atan2(b, a), half_diff = atan2(d, c);
    double a0, a2;
    if (lock == 0) {
        a0 = half_sum - half_diff, a2 = half_sum + half_diff;
    } else {
        a2 = 0.0;
        a0 = lock == 1 ? 2.0 * half_sum : 2.0 * half_diff * -1.0;
    }
    a1 -= kPosePi / 2.0;
    angles[0] = wrap_pi(a0), angles[1] = wrap_pi(a1), angles[2] = wrap_pi(a2);
    return lock != 0;
}

// model_training/model/flame.py:239-251 in degrees: int() truncates toward zero, // floors, exactly +-180 stays
__host__ __device__ __forceinline__ long long floor_half(long long v) { return v >= 0 ? v / 2 : -((1 - v) / 2); }
__host__ __device__ __forceinline__ double limit_angle(double angle) {
    const double pi = 180.0;
    if (angle < -pi) {
        const long long k = -2 * floor_half((long long)(angle / pi));
        angle = angle + (double)k * pi;
    }
    if (angle > pi) {
        const long long k = 2 * floor_half((long long)(angle / pi) + 1);
        angle = angle - (double)k * pi;
    }
    return angle;
}

// rot_mat_from_6dof (model_training/model/utils.py:92-101) in float32, the rule of flame_math.hpp's rot6_to_matrix operation for
// operation: sqrt of the left-to-right sum of squares, the clamp at 1e-12, three divisions, the two crosses. Row-major, columns b1 b2 b3.
__host__ __device__ __forceinline__ void pose_normalize3(float v[3]) {
    const float n = fmaxf(sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), 1e-12f);
    v[0] /= n, v[1] /= n, v[2] /= n;
}
__host__ __device__ __forceinline__ void pose_rot6_to_matrix(const float rot6[6], float R[9]) {
    float b1[3] = {rot6[0], rot6[1], rot6[2]};
    const float vy[3] = {rot6[3], rot6[4], rot6[5]};
    pose_normalize3(b1);
    float b3[3] = {b1[1] * vy[2] - b1[2] * vy[1], b1[2] * vy[0] - b1[0] * vy[2], b1[0] * vy[1] - b1[1] * vy[0]};
    pose_normalize3(b3);
    const float b2[3] = {-(b1[1] * b3[2] - b1[2] * b3[1]), -(b1[2] * b3[0] - b1[0] * b3[2]), -(b1[0] * b3[1] - b1[1] * b3[0])};
    R[0] = b1[0], R[1] = b2[0], R[2] = b3[0];
    R[3] = b1[1], R[4] = b2[1], R[5] = b3[1];
    R[6] = b1[2], R[7] = b2[2], R[8] = b3[2];
}

// (roll, pitch, yaw) in degrees from the float32 matrix of pose_rot6_to_matrix: R transposed, the three steps, degrees, then
// limit_angle of (a[2], a[0] - 180, a[1]). Returns DAD3D_POSE_FLAG_*; NaN angles with NONFINITE or DEGENERATE.
__host__ __device__ __forceinline__ int rpy_from_rotation(const float R[9], double rpy[3]) {
    double m[3][3], q[3][3], quat[4], ang[3], smallest, det_sign;
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            m[i][j] = (double)R[j * 3 + i];
            finite = finite && finite_d(m[i][j]);
        }
    const double nan = __builtin_nan("");
    rpy[0] = rpy[1] = rpy[2] = nan;
    if (!finite) return DAD3D_POSE_FLAG_NONFINITE;
    if (!polar3(m, q, &smallest, &det_sign)) return DAD3D_POSE_FLAG_DEGENERATE;
    quat_from_matrix(q, quat);
    const bool lock = euler_xyz_from_quat(quat, ang);
    const double k = 180.0 / kPosePi;
    rpy[0] = limit_angle(ang[2] * k);
    rpy[1] = limit_angle(ang[0] * k - 180.0);
    rpy[2] = limit_angle(ang[1] * k);
    return lock ? DAD3D_POSE_FLAG_GIMBAL : 0;
}

// The ten points of the three arrows of a frame of h x w (demo_utils.py:73-92 with cv2.arrowedLine's tips), as float32 (x, y):
// the centre, the three ends by int() truncation, then per arrow the two tip ends at 0.1 of its length and +- pi / 4, rounded
// half to even. Non-finite angles: all ten at the centre.
__host__ __device__ __forceinline__ void pose_arrow_points(const double rpy[3], int h, int w, float pts[2 * kPosePoints]) {
    const int tdx = w / 2, tdy = h / 2, size = h / 10;
    if (!(finite_d(rpy[0]) && finite_d(rpy[1]) && finite_d(rpy[2]))) {
#pragma unroll
        for (int i = 0; i < kPosePoints; ++i) pts[2 * i] = (float)tdx, pts[2 * i + 1] = (float)tdy;
        return;
    }
    const double roll = rpy[0] * kPosePi / 180.0, pitch = rpy[1] * kPosePi / 180.0, yaw = -(rpy[2] * kPosePi / 180.0);
    const double cr = cos(roll), sr = sin(roll), cp = cos(pitch), sp = sin(pitch), cy = cos(yaw), sy = sin(yaw);
    const double ex[3] = {size * (cy * cr) + tdx, size * (-cy * sr) + tdx, size * sy + tdx};
    const double ey[3] = {size * (cp * sr + cr * sp * sy) + tdy, size * (cp * cr - sp * sy * sr) + tdy, size * (-cy * sp) + tdy};
    pts[0] = (float)tdx, pts[1] = (float)tdy;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int x = (int)ex[k], y = (int)ey[k];  // |value| <= h / 10 + max(h, w) / 2: inside int
        pts[2 + 2 * k] = (float)x, pts[3 + 2 * k] = (float)y;
        const double tip = 0.1 * hypot((double)(tdx - x), (double)(tdy - y));
        const double angle = atan2((double)(tdy - y), (double)(tdx - x));
        pts[8 + 4 * k] = (float)rint(x + tip * cos(angle + kPosePi / 4.0));
        pts[9 + 4 * k] = (float)rint(y + tip * sin(angle + kPosePi / 4.0));
        pts[10 + 4 * k] = (float)rint(x + tip * cos(angle + -kPosePi / 4.0));
        pts[11 + 4 * k] = (float)rint(y + tip * sin(angle + -kPosePi / 4.0));
    }
}

// evaluation.procrustes (utils.py:183-272, scaling, reflection="best") for one item from its reduced sums: the two means, the two
// centred Frobenius norms and cov[i][j] = sum_p X0[p][i] Y0[p][j] of the CENTRED, not yet normalised points. With
// X0^T Y0 / (|X0| |Y0|) = U S V^T: T = V U^T (no determinant fix: T may be a reflection), b = sum(S) |X0| / |Y0|,
// c = mu_x - b mu_y T. Returns DAD3D_POSE_FLAG_DEGENERATE, with NaN results, where a norm is 0 or not finite. "0" is 0 as far as
// float64 can tell: the mean of n equal values v is off by up to n eps |v|, which leaves a centred norm of up to n sqrt(n) eps |v|
// where the exact one is 0, so a norm within that of 0 counts as 0 (a set that narrow against its offset has no correct digit left).
__host__ __device__ __forceinline__ double procrustes_norm_floor(const double mu[3], int n) {
    return (double)n * sqrt((double)n) * 2.220446049250313e-16 * fmax(fmax(fabs(mu[0]), fabs(mu[1])), fabs(mu[2]));
}
__host__ __device__ __forceinline__ int procrustes_fit(const double mu_x[3], const double mu_y[3], double norm_x, double norm_y, const double cov[3][3],
                                                       int n_points, double* b, double t[3][3], double c[3]) {
    if (!(norm_x > procrustes_norm_floor(mu_x, n_points) && norm_y > procrustes_norm_floor(mu_y, n_points) && finite_d(norm_x) &&
          finite_d(norm_y))) {
        const double nan = __builtin_nan("");
        *b = nan;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            c[i] = nan;
#pragma unroll
            for (int j = 0; j < 3; ++j) t[i][j] = nan;
        }
        return DAD3D_POSE_FLAG_DEGENERATE;
    }
    const double d = norm_x * norm_y;
    const Mat3d a = {{cov[0][0] / d, cov[1][0] / d, cov[2][0] / d}, {cov[0][1] / d, cov[1][1] / d, cov[2][1] / d},
                     {cov[0][2] / d, cov[1][2] / d, cov[2][2] / d}};
    const Svd3 r = svd3(a);
    double q[3][3];  // U V^T
    polar_from_svd(r, q);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) t[i][j] = q[j][i];
    *b = (r.s0 + r.s1 + r.s2) * norm_x / norm_y;
#pragma unroll
    for (int j = 0; j < 3; ++j) c[j] = mu_x[j] - *b * (mu_y[0] * t[0][j] + mu_y[1] * t[1][j] + mu_y[2] * t[2][j]);
    return 0;
}

}  // namespace dad3d
