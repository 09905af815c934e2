// The text json.dump writes for a float32 widened to double: float.__repr__(d), the shortest decimal string that reads back to d
// (DESIGN.md 4.13). __host__ __device__ and integers only, so the code the kernels of json_text.hip run is the code
// dad3d_json_number_host runs on a CPU.
//
// Digits (Schubfach, R. Giulietti, "The Schubfach way to render doubles", 2020): d = c 2^q with 2^52 <= c < 2^53. The rounding
// interval runs to the DOUBLE neighbours, [c - 1/2, c + 1/2] 2^q, both ends included because c = m24 << 29 is even, and its lower
// half is half as wide when c = 2^52 (x a power of two; float32 denormals are normal doubles, so that includes 2^-149). With
// k = floor(log10(2^q)) (floor(log10(3/4 2^q)) for c = 2^52) the interval holds at most one multiple of 10^(k+1) and at least one
// of 10^k. The three numbers 4 (c -+ 1/2) 2^q / 10^k and 4 c 2^q / 10^k are floored with a sticky last bit from one 64 x 128-bit
// product each against g(-k) of json_pow10_table.hpp; a multiple of 10^(k+1) inside the interval wins, else the multiple of 10^k
// next to d that is inside, else of the two the nearer, a tie to the even one. Trailing zeros are dropped.
//
// Layout (Python's format_float_short for 'r'): value = 0.D 10^decpt; -4 < decpt <= 16 positional, zero-padded, ".0" when no
// fraction digit is left; else d[.ddd]e+-XX. A float32's decimal exponent is -45 .. 38: always two exponent digits.
//
// Longest text, DAD3D_JSON_MAX_NUMBER_BYTES = 23: D has at most 17 digits.
//   decpt in -3 .. 0    "-" "0." -decpt zeros D              <= 1 + 2 + 3 + 17 = 23   (-0.00010000000474974513 is one)
//   0 < decpt < |D|     "-" D with a "." inside              <= 1 + 17 + 1     = 19
//   |D| <= decpt <= 16  "-" D zeros ".0"                     <= 1 + 16 + 2     = 19
//   exponent form       "-" d "." 16 digits "e" sign XX      <= 1 + 1 + 1 + 16 + 1 + 1 + 2 = 23   (-1.1754942106924411e-38)
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dad3d.h"
#include "json_pow10_table.hpp"

namespace dad3d {

struct JsonPow10 {
    unsigned long long hi, lo;
};
// namespace-scope constexpr: the device compilation emits it as constant memory, the host one as read-only data
static constexpr JsonPow10 kJsonPow10[DAD3D_JSON_POW10_MAX - DAD3D_JSON_POW10_MIN + 1] = {DAD3D_JSON_POW10_TABLE};

struct JsonNumber {
    unsigned long long digits;  // D as an integer, no trailing zeros (0 for +-0.0)
    int ndigits;                // 1 .. 17
    int decpt;                  // value = 0.D x 10^decpt
    int neg;
};

__host__ __device__ inline unsigned long long json_mulhi(unsigned long long a, unsigned long long b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (unsigned long long)(((unsigned __int128)a * b) >> 64);
#endif
}

// floor(cp g / 2^128) with the bits below it ORed into bit 0
__host__ __device__ inline unsigned long long json_round_to_odd(const JsonPow10& g, unsigned long long cp) {
    const unsigned long long x_hi = json_mulhi(cp, g.lo);
    const unsigned long long y_lo = cp * g.hi + x_hi;
    const unsigned long long y_hi = json_mulhi(cp, g.hi) + (y_lo < x_hi);
    return y_hi | (unsigned long long)(y_lo > 1ull);
}

__host__ __device__ inline int json_decimal_digits(unsigned long long v) {  // v < 10^17
    int n = 1;
    unsigned long long p = 10ull;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        n += v >= p;
        p *= 10ull;
    }
    return n;
}

// false: NaN or +-inf (the caller flags the item)
__host__ __device__ inline bool json_number(unsigned bits, JsonNumber& n) {
    const unsigned be = (bits >> 23) & 0xffu, fr = bits & 0x7fffffu;
    n.neg = (int)(bits >> 31);
    if (be == 255u) return false;
    if (be == 0u && fr == 0u) {
        n.digits = 0, n.ndigits = 1, n.decpt = 1;
        return true;
    }
    unsigned m24;  // the significand with its top bit at 2^23
    int q;         // d = (m24 << 29) 2^q
    if (be) {
        m24 = fr | 0x800000u, q = (int)be - 179;
    } else {
#if defined(__HIP_DEVICE_COMPILE__)
        const int lz = __clz((int)fr) - 8;
#else
        const int lz = __builtin_clz(fr) - 8;
#endif
        m24 = fr << lz, q = -178 - lz;
    }
    const unsigned long long c = (unsigned long long)m24 << 29;
    const int closer = m24 == 0x800000u;  // the lower neighbour is half as far
    const int k = (q * 1262611 - (closer ? 524031 : 0)) >> 22;        // floor(log10(2^q)) / floor(log10(3/4 2^q))
    const int h = q + ((-k * 1741647) >> 19) + 1;                     // 1 .. 4: 2^q 10^-k = g 2^(h - 128)
    const JsonPow10 g = kJsonPow10[-k - DAD3D_JSON_POW10_MIN];
    const unsigned long long vbl = json_round_to_odd(g, (4ull * c - 2ull + closer) << h);
    const unsigned long long vb = json_round_to_odd(g, (4ull * c) << h);
    const unsigned long long vbr = json_round_to_odd(g, (4ull * c + 2ull) << h);
    const unsigned long long s = vb >> 2;  // floor(d / 10^k); the interval is [vbl, vbr] / 4, ends included (c is even)
    unsigned long long digits;
    int exp10 = k;
    const unsigned long long sp = s / 10ull;
    const bool up_inside = vbl <= 40ull * sp, wp_inside = 40ull * sp + 40ull <= vbr;
    if (s >= 10ull && up_inside != wp_inside) {
        digits = sp + wp_inside, exp10 = k + 1;
    } else {
        const bool u_inside = vbl <= 4ull * s, w_inside = 4ull * s + 4ull <= vbr;
        if (u_inside != w_inside) {
            digits = s + w_inside;
        } else {
            const unsigned long long mid = 4ull * s + 2ull;
            digits = s + (vb > mid || (vb == mid && (s & 1ull)));
        }
    }
    for (int i = 0; i < 17; ++i) {  // at most 16 trailing zeros
        const unsigned long long t = digits / 10ull;
        if (t * 10ull != digits) break;
        digits = t, ++exp10;
    }
    n.digits = digits;
    n.ndigits = json_decimal_digits(digits);
    n.decpt = n.ndigits + exp10;
    return true;
}

__host__ __device__ inline bool json_exponent_form(const JsonNumber& n) { return n.decpt <= -4 || n.decpt > 16; }

__host__ __device__ inline int json_number_length(const JsonNumber& n) {
    if (json_exponent_form(n)) return n.neg + n.ndigits + (n.ndigits > 1) + 4;
    if (n.decpt <= 0) return n.neg + 2 - n.decpt + n.ndigits;
    return n.neg + (n.decpt >= n.ndigits ? n.decpt + 2 : n.ndigits + 1);
}

// the characters of the number at s (host memory, or the LDS image of a tile); returns the byte after them
__host__ __device__ inline unsigned char* json_put_number(unsigned char* s, const JsonNumber& n) {
    if (n.neg) *s++ = '-';
    const bool expo = json_exponent_form(n);
    int before_dot;  // digits of D in front of the '.'; ndigits: no '.' inside D
    if (expo) {
        before_dot = n.ndigits > 1 ? 1 : n.ndigits;
    } else if (n.decpt <= 0) {
        *s++ = '0', *s++ = '.';
        for (int i = 0; i < -n.decpt; ++i) *s++ = '0';
        before_dot = n.ndigits;
    } else {
        before_dot = n.decpt < n.ndigits ? n.decpt : n.ndigits;
    }
    const int dot = before_dot < n.ndigits;
    unsigned lo = (unsigned)(n.digits % 1000000000ull), hi = (unsigned)(n.digits / 1000000000ull);
    int j = n.ndigits - 1;
    for (int i = 0; i < 9 && j >= 0; ++i, --j) {
        s[j + (j >= before_dot)] = (unsigned char)('0' + lo % 10u);
        lo /= 10u;
    }
    for (; j >= 0; --j) {
        s[j + (j >= before_dot)] = (unsigned char)('0' + hi % 10u);
        hi /= 10u;
    }
    if (dot) s[before_dot] = '.';
    s += n.ndigits + dot;
    if (expo) {
        int e = n.decpt - 1;
        *s++ = 'e', *s++ = e < 0 ? '-' : '+';
        e = e < 0 ? -e : e;
        *s++ = (unsigned char)('0' + e / 10), *s++ = (unsigned char)('0' + e % 10);
    } else if (n.decpt >= n.ndigits) {
        for (int i = n.ndigits; i < n.decpt; ++i) *s++ = '0';
        *s++ = '.', *s++ = '0';
    }
    return s;
}

}  // namespace dad3d
