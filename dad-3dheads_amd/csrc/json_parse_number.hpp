// The double json.loads makes of a JSON number token: float(text), correctly rounded. __host__ __device__ and integers
// only, so the code the kernels of json_parse.hip run is the code dad3d_json_parse_number_host runs on a CPU.
//
// Grammar: -?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][+-]?[0-9]+)?  over the whole byte range. The digits, leading zeros dropped, give a decimal
// significand w < 10^19 and an exponent q: value = w 10^q.
//
// Rounding (Eisel-Lemire: D. Lemire, "Number parsing at a gigabyte per second", 2021): w is shifted until its top bit is set and
// multiplied by the 128-bit truncated power of five t(q) of json_pow5_table.hpp. The high 64 bits of w * t.hi hold the 53 bits of the
// double, a rounding bit and 9 more; only when those 9 are all ones can the truncated low half of t(q) change them, and then the second
// partial product w * t.lo is added. A result exactly between two doubles is possible only for q in -4 .. 23 (5^q must divide or be
// divided inside 64 bits); there the tie goes to the even significand, everywhere else the half rounds up.
//
// The routine never guesses: a token gets a DAD3D_JSON_PARSE_FLAG_* bit and no value when it has more than 19 significant digits, is an
// integer beyond 2^53 (json.loads keeps those as exact ints), lands in the subnormal range or below, overflows, or leaves the product
// ambiguous (low word all ones with q outside -27 .. 55). The caller hands such a token's array to the host parser.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dad3d.h"
#include "json_pow5_table.hpp"

namespace dad3d {

struct JsonPow5 {
    unsigned long long hi, lo;
};
// namespace-scope constexpr: the device compilation emits it as constant memory, the host one as read-only data
static constexpr JsonPow5 kJsonPow5[DAD3D_JSON_POW5_MAX - DAD3D_JSON_POW5_MIN + 1] = {DAD3D_JSON_POW5_TABLE};

__host__ __device__ inline unsigned long long json_parse_mulhi(unsigned long long a, unsigned long long b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (unsigned long long)(((unsigned __int128)a * b) >> 64);
#endif
}

__host__ __device__ inline int json_parse_clz(unsigned long long v) {  // v != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)v);
#else
    return __builtin_clzll(v);
#endif
}

__host__ __device__ inline bool json_is_digit(unsigned char c) { return c >= '0' && c <= '9'; }
// the bytes a number token is made of: a token is a maximal run of them outside strings
__host__ __device__ inline bool json_is_number_byte(unsigned char c) {
    return json_is_digit(c) || c == '+' || c == '-' || c == '.' || c == 'e' || c == 'E';
}

// w 10^q, w != 0, q in DAD3D_JSON_POW5_MIN .. DAD3D_JSON_POW5_MAX -> the bits of the nearest double (no sign); returns flag bits
__host__ __device__ inline unsigned json_decimal_to_double(unsigned long long w, int q, unsigned long long& bits) {
    int lz = json_parse_clz(w);
    w <<= lz;
    const JsonPow5 t = kJsonPow5[q - DAD3D_JSON_POW5_MIN];
    unsigned long long lo = w * t.hi, hi = json_parse_mulhi(w, t.hi);
    if ((hi & 0x1ffull) == 0x1ffull) {  // the truncated half of t(q) can still carry into the bits that decide
        const unsigned long long second_hi = json_parse_mulhi(w, t.lo);
        lo += second_hi;
        if (second_hi > lo) ++hi;
    }
    if (lo == 0xffffffffffffffffull && (q < -27 || q > 55)) return DAD3D_JSON_PARSE_FLAG_AMBIGUOUS;
    const int upper = (int)(hi >> 63);
    const int shift = upper + 64 - 52 - 3;
    unsigned long long m = hi >> shift;  // 54 bits: the significand and one rounding bit
    int e2 =(((152170 + 65536) * q) >> 16) + 63 + upper - lz + 1023;  // the biased exponent
    if (e2 <= 0) return DAD3D_JSON_PARSE_FLAG_SUBNORMAL;
    // exactly half way: only then is the product exact (lo <= 1 and nothing shifted out); to even
    if (lo <= 1 && q >= -4 && q <= 23 && (m & 3) == 1 && (m << shift) == hi) m &= ~1ull;
    m += m & 1;
    m >>= 1;
    if (m >= (2ull << 52)) {
        m = 1ull << 52;
        ++e2;
    }
    m &= ~(1ull << 52);
    if (e2 >= 0x7ff) return DAD3D_JSON_PARSE_FLAG_OVERFLOW;
    bits = ((unsigned long long)e2 << 52) | m;
    return 0;
}

// the token text[start, end): returns 0 and the double's bits + is_int (no fraction and no exponent part: json.loads makes a Python int),
// or DAD3D_JSON_PARSE_FLAG_* bits and bits = 0
__host__ __device__ inline unsigned json_parse_number(const unsigned char* text, long long start, long long end, unsigned long long& bits,
                                                      int& is_int) {
    bits = 0, is_int = 0;
    long long i = start;
    const unsigned long long neg = (i < end && text[i] == '-') ? 1ull : 0ull;
    i += (long long)neg;
    if (i >= end) return DAD3D_JSON_PARSE_FLAG_GRAMMAR;
    unsigned long long w = 0;
    int nd = 0;  // significant digits taken into w
    bool too_many = false;
    long long frac = 0, e10 = 0;
    bool has_frac = false, has_exp = false;
    if (text[i] == '0') {
        ++i;
        if (i < end && json_is_digit(text[i])) return DAD3D_JSON_PARSE_FLAG_GRAMMAR;  // a leading zero
    } else if (json_is_digit(text[i])) {
        for (; i < end && json_is_digit(text[i]); ++i) {
            if (nd < 19) w = w * 10ull + (unsigned long long)(text[i] - '0'), ++nd;
            else too_many = true;
        }
    } else {
        return DAD3D_JSON_PARSE_FLAG_GRAMMAR;
    }
    if (i < end && text[i] == '.') {
        has_frac = true;
        ++i;
        if (i >= end || !json_is_digit(text[i])) return DAD3D_JSON_PARSE_FLAG_GRAMMAR;
        for (; i < end && json_is_digit(text[i]); ++i, ++frac) {
            const unsigned d = text[i] - '0';
            if (nd == 0 && d == 0) continue;  // a zero in front of the first significant digit
            if (nd < 19) w = w * 10ull + d, ++nd;
            else too_many = true;
        }
    }
    if (i < end && (text[i] == 'e' || text[i] == 'E')) {
        has_exp = true;
        ++i;
        bool eneg = false;
        if (i < end && (text[i] == '+' || text[i] == '-')) eneg = text[i] == '-', ++i;
        if (i >= end || !json_is_digit(text[i])) return DAD3D_JSON_PARSE_FLAG_GRAMMAR;
        for (; i < end && json_is_digit(text[i]); ++i)
            if (e10 < 1000000) e10 = e10 * 10 + (text[i] - '0');  // past any double either way; no wrap
        if (eneg) e10 = -e10;
    }
    if (i != end) return DAD3D_JSON_PARSE_FLAG_GRAMMAR;
    is_int = !has_frac && !has_exp;
    if (too_many) return DAD3D_JSON_PARSE_FLAG_DIGITS;
    if (w == 0) {  // 0, -0, 0.0, 0e5: exact
        bits = neg << 63;
        return 0;
    }
    if (is_int && w > (1ull << 53)) return DAD3D_JSON_PARSE_FLAG_BIG_INT;
    const long long q = e10 - frac;
    if (q < DAD3D_JSON_POW5_MIN) return DAD3D_JSON_PARSE_FLAG_SUBNORMAL;  // w < 10^19: below 10^-323
    if (q > DAD3D_JSON_POW5_MAX) return DAD3D_JSON_PARSE_FLAG_OVERFLOW;
    unsigned long long mag = 0;
    const unsigned why = json_decimal_to_double(w, (int)q, mag);
    if (why) return why;
    bits = mag | (neg << 63);
    return 0;
}

}  // namespace dad3d
