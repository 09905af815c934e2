// CRC-32 of PNG chunks (reflected, polynomial EDB88320) in pieces: a lane takes the CRC of its bytes bit by bit, and the CRCs of A and B
// give the CRC of A || B by a multiplication in GF(2)[x] / P. Shared by csrc/png_encode.hip and csrc/png_decode.hip.
#pragma once

namespace dad3d {

constexpr unsigned kCrcPoly = 0xEDB88320u;

// ---- CRC-32 (reflected, polynomial EDB88320): bit 31 of a word is the coefficient of x^0 ----
__host__ __device__ constexpr unsigned gf_mul(unsigned a, unsigned b) {
    unsigned p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? kCrcPoly : 0u);
    }
    return p;
}
// x^(8 k) mod P by square and multiply from the top bit; k < 2^16
__device__ inline unsigned gf_x_pow_bytes(unsigned k) {
    unsigned p = 0x80000000u;
    for (int bit = 15; bit >= 0; --bit) {
        p = gf_mul(p, p);
        if ((k >> bit) & 1u) p = gf_mul(p, 0x00800000u);  // x^8
    }
    return p;
}
__device__ inline unsigned crc_bitwise(unsigned crc, unsigned byte) {
    crc ^= byte;
#pragma unroll
    for (int k = 0; k < 8; ++k) crc = (crc >> 1) ^ ((crc & 1u) ? kCrcPoly : 0u);
    return crc;
}
// the CRC of A || B from the CRCs of A and B
__device__ inline unsigned crc_append(unsigned crc_a, unsigned crc_b, unsigned bytes_b) { return gf_mul(gf_x_pow_bytes(bytes_b), crc_a) ^ crc_b; }
// the same for any k < 2^32
__device__ inline unsigned gf_x_pow_bytes_wide(unsigned k) {
    unsigned p = 0x80000000u;
#pragma unroll 1
    for (int bit = k ? 31 - __clz((int)k) : -1; bit >= 0; --bit) {  // from the top set bit: most chunks are short
        p = gf_mul(p, p);
        if ((k >> bit) & 1u) p = gf_mul(p, 0x00800000u);
    }
    return p;
}

}  // namespace dad3d
