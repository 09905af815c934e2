// The details of PNG and zlib that the encoder (png_encode.hip) and the decoder (png_decode.hip, inflate.hpp) must agree on.
#pragma once

namespace dad3d {

constexpr unsigned kAdlerMod = 65521u;  // Adler-32: both sums are taken modulo the largest prime below 2^16

// the Paeth predictor of filter type 4: of left, above and above left, the one nearest to left + above - above left
__device__ inline int png_paeth(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

}  // namespace dad3d
