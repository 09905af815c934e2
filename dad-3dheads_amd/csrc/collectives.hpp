// The collectives of the kernels, device only: a reduction over the 64 lanes of a wave, a reduction over a workgroup and an
// exclusive scan over a workgroup. One definition, one barrier protocol, one order of combination.
//
// The contract, which the bit-reproducible float caller (flame_backward.hip) relies on, and which the private sums of
// mesh_losses.hip and train_objective.hip (barrier first; kept for their measured speed) follow in their order of additions:
//   wave    the xor butterfly with the offsets 32, 16, 8, 4, 2, 1, in that order; a step is v = op(v, v of lane ^ offset), so every
//           lane ends with the same bits
//   block   the wave reduction; lane 0 of wave w writes red[w]; barrier; every lane combines ((red[0] op red[1]) op red[2]) ..
//           in ascending order; barrier. Every lane gets the result, and `red` (WAVES elements of LDS) is free on return: calls may
//           follow each other on the same `red` with nothing in between.
//   scan    the same protocol; a wave's inclusive prefix by __shfl_up with the offsets 1, 2, .., 32
// The trailing barrier orders nothing in front of the call: a caller whose `red` another routine may still be reading puts its
// own barrier in front. Every lane of the workgroup must make the call, and the workgroup is WAVES full waves in x.
#pragma once

#include <hip/hip_runtime.h>

namespace dad3d {
namespace {

struct OpSum {
    template <typename T>
    __device__ static __forceinline__ T of(T a, T b) { return a + b; }
};
struct OpXor {
    template <typename T>
    __device__ static __forceinline__ T of(T a, T b) { return a ^ b; }
};

// argmax over (key, index) pairs packed into one 64-bit word by argmax_pack: the larger key wins, and among equal keys the
// smaller index, so the result does not depend on the order of combination. 0 is below every packed pair of a key >= 1.
struct OpArgmax {
    __device__ static __forceinline__ unsigned long long of(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
};
__device__ __forceinline__ unsigned long long argmax_pack(unsigned key, unsigned index) {
    return (unsigned long long)key << 32 | (0xffffffffu - index);
}
__device__ __forceinline__ unsigned argmax_index(unsigned long long packed) { return 0xffffffffu - (unsigned)packed; }

template <typename T>
__device__ __forceinline__ T lane_xor(T v, int d) { return __shfl_xor(v, d, 64); }
__device__ __forceinline__ unsigned long long lane_xor(unsigned long long v, int d) {  // two 32-bit shuffles
    const unsigned lo = __shfl_xor((unsigned)v, d, 64), hi = __shfl_xor((unsigned)(v >> 32), d, 64);
    return (unsigned long long)hi << 32 | lo;
}

template <typename Op, typename T>
__device__ __forceinline__ T wave_reduce(T v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = Op::of(v, lane_xor(v, d));
    return v;
}

template <typename Op, int WAVES, typename T>
__device__ __forceinline__ T block_reduce(T v, T* red) {
    v = wave_reduce<Op>(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = red[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) v = Op::of(v, red[w]);
    __syncthreads();
    return v;
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) { return wave_reduce<OpSum>(v); }
template <typename T>
__device__ __forceinline__ T wave_xor(T v) { return wave_reduce<OpXor>(v); }

template <int WAVES, typename T>
__device__ __forceinline__ T block_sum(T v, T* red) { return block_reduce<OpSum, WAVES>(v, red); }
template <int WAVES, typename T>
__device__ __forceinline__ T block_xor(T v, T* red) { return block_reduce<OpXor, WAVES>(v, red); }

// the sum of v over the lanes in front of this one; total = the sum over the workgroup
template <int WAVES>
__device__ __forceinline__ int block_exclusive_scan(int v, int* red, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) red[wave] = incl;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += red[w];
    total = red[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) total += red[w];
    __syncthreads();
    return base + incl - v;
}

}  // namespace
}  // namespace dad3d
