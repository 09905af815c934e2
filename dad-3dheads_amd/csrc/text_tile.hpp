// What the text kernels share: workgroups of 256 lanes (kTextTile, kTextWaves) whose sums and scans are the ones of collectives.hpp,
// and, for obj_text.hip, json_text.hip and png_encode.hip, the copy of an LDS image of the tile's bytes out in aligned 16-byte
// stores. json_parse.hip and annotation_parse.hip read text instead: a lane holds kTextLaneBytes consecutive bytes in four registers and
// picks them apart with selects (is_ws, byte_of, put_byte, load_chunk).
#pragma once

#include <hip/hip_runtime.h>

#include "collectives.hpp"

namespace dad3d {
namespace {

constexpr int kTextTile = 256;              // lanes per workgroup
constexpr int kTextWaves = kTextTile / 64;  // the `red` of a sum or a scan: this many words of LDS
constexpr int kTextLaneBytes = 16;          // a reading lane's chunk

__device__ inline bool is_ws(unsigned char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }

__device__ inline unsigned byte_of(const uint4& v, int k) {  // selects, no indexing into memory: k may be a loop variable
    const unsigned w = (k >> 2) == 0 ? v.x : (k >> 2) == 1 ? v.y : (k >> 2) == 2 ? v.z : v.w;
    return (w >> (8 * (k & 3))) & 0xffu;
}

__device__ inline void put_byte(uint4& v, int k, unsigned b) {
    const unsigned s = b << (8 * (k & 3));
    if ((k >> 2) == 0) v.x |= s;
    else if ((k >> 2) == 1) v.y |= s;
    else if ((k >> 2) == 2) v.z |= s;
    else v.w |= s;
}

// this lane's 16 bytes of `src` (16-byte aligned) from `base`; the bytes at and behind n read as 0
__device__ inline uint4 load_chunk(const unsigned char* __restrict__ src, long long base, long long n, int& valid) {
    valid = (int)min((long long)kTextLaneBytes, max(n - base, 0ll));
    uint4 v = make_uint4(0, 0, 0, 0);
    if (valid == kTextLaneBytes) {
        v = *reinterpret_cast<const uint4*>(src + base);
    } else {
#pragma unroll
        for (int k = 0; k < kTextLaneBytes; ++k)
            if (k < valid) put_byte(v, k, src[base + k]);
    }
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
