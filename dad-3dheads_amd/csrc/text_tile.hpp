// What the two text formatters (obj_text.hip, json_text.hip) share: workgroups of 256 lanes that sum lengths and copy an LDS image
// of their tile's bytes out in aligned 16-byte stores.
#pragma once

#include <hip/hip_runtime.h>

namespace dad3d {
namespace {

constexpr int kTextTile = 256;  // lanes per workgroup

__device__ inline int wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// sum over the 256 lanes of the workgroup; red: 4 ints of LDS, reusable after the call
__device__ inline int block_sum(int v, int* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return v;
}

// image bytes [lead, end) of `stage` -> out[lead .. end), `out` 16-byte aligned: whole units as one 16-byte store, a unit shared
// with the neighbouring tile byte by byte (only this tile's bytes)
__device__ inline void copy_tile_out(const uint4* stage, unsigned char* out, int lead, int end) {
    const unsigned char* s = reinterpret_cast<const unsigned char*>(stage);
    for (int c = threadIdx.x; c * 16 < end; c += kTextTile) {
        const int lo = c * 16, hi = lo + 16;
        if (lo >= lead && hi <= end) {
            reinterpret_cast<uint4*>(out)[c] = stage[c];
        } else {
            for (int i = max(lo, lead); i < min(hi, end); ++i) out[i] = s[i];
        }
    }
}

}  // namespace
}  // namespace dad3d
