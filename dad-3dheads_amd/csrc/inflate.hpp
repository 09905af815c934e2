// Inflate of a zlib stream (RFC 1950, 1951), one routine for the host and the device. The stream arrives through an
// input policy (a list of byte ranges: the IDAT payloads of a file, or one range) and leaves through an output policy (literals, copies
// and stored bytes); csrc/png_decode.hip gives it 64-lane policies in LDS, dad3d_inflate_host serial ones, so tests/test_png_decode_host.py
// fuzzes on a CPU the code the kernels run. Every lane of a wave runs the routine with the same values: the policies alone use the lane.
//
// What is accepted is what zlib's inflate accepts: a header with CM = 8, CINFO <= 7, a valid FCHECK and no FDICT; stored, fixed and
// dynamic blocks; a code-length code that is complete; literal/length and distance codes that are complete, or hold a single code of
// one bit, or (distances) no code at all; bytes behind the Adler-32 are ignored. Everything else sets kInflateMalformed: truncation,
// block type 3, oversubscribed or incomplete code lengths, a repeat with nothing in front of it or running past HLIT + HDIST, no end
// of block code, symbols 286 / 287, distance codes 30 / 31, a distance in front of the output, LEN != ~NLEN, an Adler mismatch. Output
// past the capacity sets kInflateOverflow. The routine reads nothing outside the ranges and writes nothing outside the capacity.
//
// kInflateSegment is the mode of the segmented PNG path: no header and no trailer, blocks until the input ends, which it must do with
// no bit left behind a block; a final block is refused. The output's Adler sums start at (0, 0), so they are the sum of x and the sum
// of (n - i) x[i]. An output policy may hold `lead()` bytes of history in front of its first byte (the segmented path: the last bytes
// of the segment before); a distance may reach that far and no further.
#pragma once

#include "png_common.hpp"

#ifndef DAD3D_HD
#define DAD3D_HD __host__ __device__ inline
#endif

namespace dad3d {

constexpr int kInflateMalformed = 0x1, kInflateOverflow = 0x4;  // DAD3D_PNG_DECODE_FLAG_MALFORMED / _OVERFLOW
constexpr int kInflateZlib = 0, kInflateSegment = 1;

// canonical codes as counts per length and symbols in code order; `lengths` and `offs` are the table builder's work space
struct InflateWork {
    unsigned short lcount[16], lsym[288], dcount[16], dsym[32], lengths[320], offs[16];
};

// On the device every lane holds the same value of everything in this file. Saying so where a value comes out of a table keeps the
// decoder's state and its branches in scalar registers; the host reads the value as it is. The loops stay rolled (`unroll 1`):
// unrolled, the table reads of a whole loop are live in scalar registers at once and spill.
DAD3D_HD int inflate_same(int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_readfirstlane(v);
#else
    return v;
#endif
}

// > 0: incomplete, < 0: oversubscribed, 0: complete (or no code at all)
DAD3D_HD int inflate_construct(unsigned short* count, unsigned short* symbol, unsigned short* offs, const unsigned short* lengths, int n) {
    #pragma unroll 1
    for (int len = 0; len < 16; ++len) count[len] = 0;
    #pragma unroll 1
    for (int s = 0; s < n; ++s) {
        const int len = inflate_same(lengths[s]);
        count[len] = (unsigned short)(inflate_same(count[len]) + 1);
    }
    if (inflate_same(count[0]) == n) return 0;
    int left = 1;
    #pragma unroll 1
    for (int len = 1; len < 16; ++len) {
        left = (left << 1) - inflate_same(count[len]);
        if (left < 0) return left;
    }
    int at = 0;
    #pragma unroll 1
    for (int len = 1; len < 16; ++len) {
        offs[len] = (unsigned short)at;
        at += inflate_same(count[len]);
    }
    #pragma unroll 1
    for (int s = 0; s < n; ++s) {
        const int len = inflate_same(lengths[s]);
        if (len) {
            const int to = inflate_same(offs[len]);
            symbol[to] = (unsigned short)s;
            offs[len] = (unsigned short)(to + 1);
        }
    }
    return left;
}

template <class In, class Out>
struct Inflater {
    In& in;
    Out& out;
    InflateWork& w;
    unsigned long long buf = 0;
    int cnt = 0, flag = 0;

    DAD3D_HD Inflater(In& i, Out& o, InflateWork& work) : in(i), out(o), w(work) {}

    DAD3D_HD void fill(int want) {
        #pragma unroll 1
        while (cnt < want) {
            const int b = in.byte();
            if (b < 0) return;
            buf |= (unsigned long long)(unsigned)b << cnt;
            cnt += 8;
        }
    }
    DAD3D_HD unsigned bits(int n) {  // n <= 32
        if (n == 0 || flag) return 0;
        fill(n);
        if (cnt < n) {
            flag |= kInflateMalformed;
            return 0;
        }
        const unsigned v = (unsigned)(buf & ((1ull << n) - 1ull));
        buf >>= n, cnt -= n;
        return v;
    }
    DAD3D_HD int decode(const unsigned short* count, const unsigned short* symbol) {
        fill(15);
        int code = 0, first = 0, index = 0;
        #pragma unroll 1
        for (int len = 1; len <= 15; ++len) {
            if (len > cnt) return -1;  // the stream ends inside a code
            code |= (int)((buf >> (len - 1)) & 1ull);
            const int c = inflate_same(count[len]);
            if (code - c < first) {
                buf >>= len, cnt -= len;
                return inflate_same(symbol[index + (code - first)]);
            }
            index += c, first += c;
            first <<= 1, code <<= 1;
        }
        return -1;  // a code the table does not hold
    }

    DAD3D_HD void stored() {
        const int drop = cnt & 7;
        buf >>= drop, cnt -= drop;
        unsigned len = bits(16);
        const unsigned nlen = bits(16);
        if (flag) return;
        if (len != (~nlen & 0xffffu)) {
            flag |= kInflateMalformed;
            return;
        }
        if (!out.room((int)len)) {
            flag |= kInflateOverflow;
            return;
        }
        #pragma unroll 1
        while (len && cnt >= 8) {
            out.lit((int)(buf & 255ull));
            buf >>= 8, cnt -= 8, --len;
        }
        #pragma unroll 1
        while (len) {
            const int k = in.chunk((int)len);
            if (k <= 0) {
                flag |= kInflateMalformed;
                return;
            }
            out.bytes(in.ptr(), k);
            in.skip(k);
            len -= (unsigned)k;
        }
    }

    DAD3D_HD void codes() {
        #pragma unroll 1
        while (!flag) {
            int sym = decode(w.lcount, w.lsym);
            if (sym < 0) break;
            if (sym < 256) {
                if (!out.room(1)) {
                    flag |= kInflateOverflow;
                    return;
                }
                out.lit(sym);
                continue;
            }
            if (sym == 256) return;
            sym -= 257;
            if (sym >= 29) break;  // 286, 287
            int len = sym + 3, extra = 0;
            if (sym == 28) {
                len = 258;
            } else if (sym >= 8) {
                extra = (sym - 4) >> 2;
                len = 3 + ((4 + (sym & 3)) << extra);
            }
            len += (int)bits(extra);
            const int ds = decode(w.dcount, w.dsym);
            if (flag || ds < 0 || ds >= 30) break;
            int dist = ds + 1;
            extra = 0;
            if (ds >= 4) {
                extra = (ds >> 1) - 1;
                dist = 1 + ((2 + (ds & 1)) << extra);
            }
            dist += (int)bits(extra);
            if (flag || (long long)dist > out.produced() + out.lead()) break;
            if (!out.room(len)) {
                flag |= kInflateOverflow;
                return;
            }
            out.copy(dist, len);
        }
        flag |= kInflateMalformed;
    }

    DAD3D_HD void fixed() {
        #pragma unroll 1
        for (int s = 0; s < 288; ++s) w.lengths[s] = (unsigned short)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
        inflate_construct(w.lcount, w.lsym, w.offs, w.lengths, 288);
        #pragma unroll 1
        for (int s = 0; s < 30; ++s) w.lengths[s] = 5;
        inflate_construct(w.dcount, w.dsym, w.offs, w.lengths, 30);
        codes();
    }

    DAD3D_HD void dynamic() {
        const int nlen = (int)bits(5) + 257, ndist = (int)bits(5) + 1, ncode = (int)bits(4) + 4;
        if (flag) return;
        if (nlen > 286 || ndist > 30) {
            flag |= kInflateMalformed;
            return;
        }
        #pragma unroll 1
        for (int i = 0; i < 19; ++i) w.lengths[i] = 0;
        #pragma unroll 1
        for (int i = 0; i < ncode; ++i) {
            // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
            const int at = i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 8 - ((i - 3) >> 1) : 8 + ((i - 4) >> 1);
            w.lengths[at] = (unsigned short)bits(3);
        }
        if (flag) return;
        if (inflate_construct(w.lcount, w.lsym, w.offs, w.lengths, 19) != 0) {
            flag |= kInflateMalformed;
            return;
        }
        int index = 0;
        #pragma unroll 1
        while (index < nlen + ndist) {
            const int sym = decode(w.lcount, w.lsym);
            if (sym < 0) {
                flag |= kInflateMalformed;
                return;
            }
            if (sym < 16) {
                w.lengths[index++] = (unsigned short)sym;
                continue;
            }
            int val = 0, rep;
            if (sym == 16) {
                if (index == 0) {
                    flag |= kInflateMalformed;
                    return;
                }
                val = inflate_same(w.lengths[index - 1]);
                rep = 3 + (int)bits(2);
            } else if (sym == 17) {
                rep = 3 + (int)bits(3);
            } else {
                rep = 11 + (int)bits(7);
            }
            if (flag) return;
            if (index + rep > nlen + ndist) {
                flag |= kInflateMalformed;
                return;
            }
            #pragma unroll 1
            while (rep--) w.lengths[index++] = (unsigned short)val;
        }
        if (inflate_same(w.lengths[256]) == 0) {
            flag |= kInflateMalformed;
            return;
        }
        int err = inflate_construct(w.lcount, w.lsym, w.offs, w.lengths, nlen);
        if (err && (err < 0 || nlen != inflate_same(w.lcount[0]) + inflate_same(w.lcount[1]))) {
            flag |= kInflateMalformed;
            return;
        }
        err = inflate_construct(w.dcount, w.dsym, w.offs, w.lengths + nlen, ndist);
        if (err && (err < 0 || ndist != inflate_same(w.dcount[0]) + inflate_same(w.dcount[1]))) {
            flag |= kInflateMalformed;
            return;
        }
        codes();
    }

    DAD3D_HD int run(int mode) {
        if (mode == kInflateZlib) {
            const unsigned cmf = bits(8), flg = bits(8);
            if (flag) return flag;
            if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 0x20u)) return flag |= kInflateMalformed;
        }
        for (;;) {
            if (mode == kInflateSegment && cnt == 0 && in.at_end()) break;
            const unsigned last = bits(1), type = bits(2);
            if (flag) return flag;
            if (type == 3 || (mode == kInflateSegment && last)) return flag |= kInflateMalformed;
            if (type == 0)
                stored();
            else if (type == 1)
                fixed();
            else
                dynamic();
            if (flag) return flag;
            if (last) break;
        }
        const unsigned got = out.finish();
        if (mode == kInflateZlib) {
            const int drop = cnt & 7;
            buf >>= drop, cnt -= drop;
            unsigned want = 0;
            #pragma unroll 1
            for (int i = 0; i < 4; ++i) want = want << 8 | bits(8);
            if (flag) return flag;
            if (want != got) return flag |= kInflateMalformed;
        }
        return flag;
    }
};

// ---- the serial policies of the host ----
struct HostInflateIn {
    const unsigned char* const* ptrs;
    const long long* lens;
    int n, r = 0;
    long long at = 0;
    HostInflateIn(const unsigned char* const* p, const long long* l, int count) : ptrs(p), lens(l), n(count) {}
    bool settle() {
        while (r < n && at >= lens[r]) ++r, at = 0;
        return r < n;
    }
    int byte() { return settle() ? ptrs[r][at++] : -1; }
    int chunk(int want) {
        if (!settle()) return 0;
        const long long left = lens[r] - at;
        return left < want ? (int)left : want;
    }
    const unsigned char* ptr() const { return ptrs[r] + at; }
    void skip(int k) { at += k; }
    bool at_end() { return !settle(); }
};

struct HostInflateOut {
    unsigned char* out;
    long long cap, n = 0;
    unsigned a, b = 0;
    HostInflateOut(unsigned char* o, long long capacity, unsigned a0) : out(o), cap(capacity), a(a0) {}
    long long produced() const { return n; }
    long long lead() const { return 0; }
    bool room(int k) const { return n + k <= cap; }
    void lit(int x) {
        out[n++] = (unsigned char)x;
        a += (unsigned)x;
        if (a >= kAdlerMod) a -= kAdlerMod;
        b += a;
        if (b >= kAdlerMod) b -= kAdlerMod;
    }
    void copy(int dist, int len) {
        for (int i = 0; i < len; ++i) lit(out[n - dist]);
    }
    void bytes(const unsigned char* p, int k) {
        for (int i = 0; i < k; ++i) lit(p[i]);
    }
    unsigned finish() const { return b << 16 | a; }
};

}  // namespace dad3d
