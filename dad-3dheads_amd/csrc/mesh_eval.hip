// The two dense point-set steps of the DAD-3DHeads benchmark scorer (dad_3dheads_benchmark/benchmark.py `DADEvaluator`,
// utils.py `calc_ch_dist`) for gfx950 (MI355X):
//
//   nearest_kernel   one-sided nearest neighbours, query [B,Q,3] against points [B,Nmax,3] with a ragged count per item.
//                    The per-item similarity p' = s * p . R + t (row vector times R: utils.py:160-168 `align_pred_to_gt`) is
//                    applied while the points are staged into LDS, so the alignment costs nothing extra. One lane owns one
//                    query and keeps a running top-K (K <= 8, a template argument) in registers; every lane of the wave
//                    reads the SAME float4 of the tile (a broadcast: no bank conflicts). The Chamfer term of the scorer is
//                    K = 1: mean over the 2094 GT face vertices of the min squared distance (kaolin's one-sided
//                    `chamfer_distance(gt, pred, 1.0, 0.0)`).
//   z5_rank_kernel   one workgroup per (item, anchor): the K <= 4096 head-subset distances to the anchor, sorted as
//                    (distance bits << 32 | index) keys by a bitonic sort in LDS (ties to the lower index), then the
//                    z-order comparisons of benchmark.py:126-147 `calc_zn` at every rank: vertex i against the i-th
//                    nearest vertex of the anchor (the script's `argsort(cdist(g, g), dim=0)[:, 1:6]` indexing).
//
// Distances are the direct-difference form (qx-px)^2 + (qy-py)^2 + (qz-pz)^2 in fp32, never |q|^2 + |p|^2 - 2 q.p: the
// expansion cancels at world-scale coordinates (the reference's own `cdist` noise). Neither kernel allocates; both are
// stream-ordered and can be captured into a graph.
#include "collectives.hpp"
#include "common.hpp"

namespace dad3d {
namespace {

constexpr int kNnThreads = 256;
constexpr int kNnTile = 1024;  // points per LDS tile: 16 KB of float4

__device__ __forceinline__ float dist2(float qx, float qy, float qz, float4 p) {
    const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
    return dx * dx + dy * dy + dz * dz;
}

template <int K>
__global__ __launch_bounds__(kNnThreads) void nearest_kernel(EvalNearestArgs a) {
    __shared__ float4 tile[kNnTile];
    const int b = blockIdx.y;
    const int q = blockIdx.x * kNnThreads + threadIdx.x;
    const bool live = q < a.n_query;
    float qx = 0.0f, qy = 0.0f, qz = 0.0f;
    if (live) {
        const float* qp = a.query + ((size_t)b * a.n_query + q) * 3;
        qx = qp[0], qy = qp[1], qz = qp[2];
    }
    int n = a.n_points;
    if (a.counts) n = min(max(a.counts[b], 0), a.n_points);  // rows past the count are never read
    float s = 1.0f, R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
    if (a.similarity) {
        const float* m = a.similarity + (size_t)b * 13;
        s = m[0];
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = m[1 + i];
#pragma unroll
        for (int i = 0; i < 3; ++i) t[i] = m[10 + i];
    }
    float bd[K];
    int bi[K];
#pragma unroll
    for (int i = 0; i < K; ++i) bd[i] = INFINITY, bi[i] = -1;
    const float* pts = a.points + (size_t)b * a.n_points * 3;
    for (int base = 0; base < n; base += kNnTile) {
        const int cnt = min(kNnTile, n - base);
        __syncthreads();  // the previous tile is no longer read
        for (int j = threadIdx.x; j < cnt; j += kNnThreads) {
            const float* p = pts + (size_t)(base + j) * 3;
            const float x = p[0], y = p[1], z = p[2];
            tile[j] = make_float4(s * (x * R[0] + y * R[3] + z * R[6]) + t[0], s * (x * R[1] + y * R[4] + z * R[7]) + t[1],
                                  s * (x * R[2] + y * R[5] + z * R[8]) + t[2], 0.0f);
        }
        __syncthreads();
        if (!live) continue;
        const int skip = a.self_exclude ? q - base : -1;  // the tile position of the query itself
        for (int j = 0; j < cnt; ++j) {
            float d = dist2(qx, qy, qz, tile[j]);
            if (j == skip) d = INFINITY;
            if (K == 1) {
                // points arrive in ascending index: strict < keeps the lower index of a tie
                if (d < bd[0]) bd[0] = d, bi[0] = base + j;
            } else if (d < bd[K - 1]) {
                // insertion into the sorted list, top slot first; equal distances stay behind (lower index first)
#pragma unroll
                for (int i = K - 1; i > 0; --i) {
                    const bool shift = d < bd[i - 1];
                    const bool place = !shift && d < bd[i];
                    bd[i] = shift ? bd[i - 1] : place ? d : bd[i];
                    bi[i] = shift ? bi[i - 1] : place ? base + j : bi[i];
                }
                if (d < bd[0]) bd[0] = d, bi[0] = base + j;
            }
        }
    }
    if (!live) return;
    const size_t o = (size_t)b * a.n_query + q;
    a.min_dist2[o] = bd[0];
#pragma unroll
    for (int i = 0; i < K; ++i) {  // K == a.k: the launcher picks the instantiation
        if (a.knn_index) a.knn_index[o * K + i] = bi[i];
        if (a.knn_dist2) a.knn_dist2[o * K + i] = bd[i];
    }
}

constexpr int kZ5Threads = 1024;

__global__ __launch_bounds__(kZ5Threads) void z5_rank_kernel(EvalZ5Args a) {
    __shared__ unsigned long long keys[kEvalMaxHead];  // 32 KB
    __shared__ int red[kZ5Threads / 64];
    const int ai = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int K = a.n_head, P = a.sort_len;  // P: the power of two >= K (host), <= kEvalMaxHead
    const float* g = a.gt_head + (size_t)b * K * 3;
    const float* w = a.pred_head + (size_t)b * K * 3;
    const int anchor = a.anchors[ai];
    const float ax = g[anchor * 3], ay = g[anchor * 3 + 1], az = g[anchor * 3 + 2];
    for (int i = tid; i < P; i += kZ5Threads) {
        unsigned long long key = ~0ull;  // padding sorts behind every real key (even a NaN distance)
        if (i < K) {
            const float dx = g[i * 3] - ax, dy = g[i * 3 + 1] - ay, dz = g[i * 3 + 2] - az;
            const float d = dx * dx + dy * dy + dz * dz;  // >= 0: its bit pattern orders as an unsigned integer
            key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)i;
        }
        keys[i] = key;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += kZ5Threads) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));  // lower element of the t-th pair at stride j
                const int l = i + j;
                const unsigned long long x = keys[i], y = keys[l];
                const bool ascending = (i & k) == 0;
                if ((x > y) == ascending) keys[i] = y, keys[l] = x;
            }
            __syncthreads();
        }
    }
    int c = 0;
    const size_t ob = ((size_t)b * a.n_anchors + ai) * K;
    for (int i = tid; i < K; i += kZ5Threads) {
        const int o = (int)(unsigned)(keys[i] & 0xffffffffull);  // < K: the K real keys sort in front of the padding
        c += (g[i * 3 + 2] >= g[o * 3 + 2]) == (w[i * 3 + 2] >= w[o * 3 + 2]);
        if (a.order) a.order[ob + i] = o;
    }
    // Not block_sum of collectives.hpp: only lane 0 needs the sum and `red` is not used again, and the 16 waves' second barrier
    // costs this kernel 0.3 % (profiles/collectives_refactor_ab.md).
    c = wave_sum(c);
    if ((tid & 63) == 0) red[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        int sum = 0;
#pragma unroll
        for (int i = 0; i < kZ5Threads / 64; ++i) sum += red[i];
        a.counts[(size_t)b * a.n_anchors + ai] = sum;
    }
}

}  // namespace

dad3d_status launch_eval_nearest(const EvalNearestArgs& a, hipStream_t s) {
    const dim3 grid((a.n_query + kNnThreads - 1) / kNnThreads, a.batch), block(kNnThreads);
    switch (a.k) {
        case 1: hipLaunchKernelGGL(nearest_kernel<1>, grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL(nearest_kernel<2>, grid, block, 0, s, a); break;
        case 3: hipLaunchKernelGGL(nearest_kernel<3>, grid, block, 0, s, a); break;
        case 4: hipLaunchKernelGGL(nearest_kernel<4>, grid, block, 0, s, a); break;
        case 5: hipLaunchKernelGGL(nearest_kernel<5>, grid, block, 0, s, a); break;
        case 6: hipLaunchKernelGGL(nearest_kernel<6>, grid, block, 0, s, a); break;
        case 7: hipLaunchKernelGGL(nearest_kernel<7>, grid, block, 0, s, a); break;
        case 8: hipLaunchKernelGGL(nearest_kernel<8>, grid, block, 0, s, a); break;
        default: set_error("launch_eval_nearest: k = %d outside 1..%d", a.k, kEvalMaxK); return DAD3D_E_INVALID;
    }
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

dad3d_status launch_eval_z5(const EvalZ5Args& a, hipStream_t s) {
    hipLaunchKernelGGL(z5_rank_kernel, dim3(a.n_anchors, a.batch), dim3(kZ5Threads), 0, s, a);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

}  // namespace dad3d
