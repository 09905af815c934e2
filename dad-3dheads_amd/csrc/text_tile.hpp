// What the text kernels share: workgroups of 256 lanes (kTextTile, kTextWaves) whose sums and scans are the ones of collectives.hpp,
// and, for obj_text.hip, json_text.hip and png_encode.hip, the copy of an LDS image of the tile's bytes out in aligned 16-byte
// stores. json_parse.hip takes only the two constants and the collectives from here.
#pragma once

#include <hip/hip_runtime.h>

#include "collectives.hpp"

namespace dad3d {
namespace {

constexpr int kTextTile = 256;              // lanes per workgroup
constexpr int kTextWaves = kTextTile / 64;  // the `red` of a sum or a scan: this many words of LDS

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
