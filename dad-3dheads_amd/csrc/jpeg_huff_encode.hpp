// Baseline JPEG written, the entropy half (ITU-T T.81, jchuff.c): the standard Huffman tables of Annex K.3 as (code, length) per
// symbol, the bits of one block -- the DC difference, run/size pairs with ZRL and EOB -- and the header SOI .. SOS in libjpeg's order.
// Shared by csrc/jpeg_encode.hip and dad3d_jpeg_encode_host. A code and the value bits behind it leave in one call of
// the caller's `put(bits, count)`, count <= 27, most significant bit first.
#pragma once

#include "jpeg_fdct.hpp"

namespace dad3d {

// the worst block: a DC code of 11 bits + 11 value bits, and 63 AC codes of 16 bits + 10 value bits
constexpr int kJpegEncMaxBlockBits = 22 + 63 * 26;
constexpr int kJpegEncPoison = 0xffff;  // the AC bit count of a block with a coefficient outside baseline's categories

struct JpegHuffSpec {  // a DHT payload: the number of codes of each length 1 .. 16, the symbols in code order
    unsigned char counts[16];
    unsigned char symbols[162];
    int n;
};
struct JpegHuffCodes {
    unsigned short code[256];
    unsigned char len[256];  // 0: the table has no such symbol
};

// Annex K.3; `which` = 0 DC luma, 1 AC luma, 2 DC chroma, 3 AC chroma
constexpr JpegHuffSpec jpeg_std_spec(int which) {
    constexpr unsigned char counts[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                             {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
                                             {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
                                             {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
    constexpr unsigned char ac[2][162] = {
        {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
         0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
         0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
         0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
         0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
         0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
         0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
         0xfa},
        {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
         0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
         0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
         0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
         0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
         0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
         0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
         0xfa}};
    JpegHuffSpec s{};
    for (int i = 0; i < 16; ++i) s.counts[i] = counts[which][i];
    s.n = which & 1 ? 162 : 12;
    for (int i = 0; i < s.n; ++i) s.symbols[i] = which & 1 ? ac[which >> 1][i] : (unsigned char)i;
    return s;
}
constexpr JpegHuffCodes jpeg_canonical_codes(const JpegHuffSpec& s) {
    JpegHuffCodes t{};
    int code = 0, k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < s.counts[len - 1]; ++i, ++k, ++code) t.code[s.symbols[k]] = (unsigned short)code, t.len[s.symbols[k]] = (unsigned char)len;
        code <<= 1;
    }
    return t;
}
DAD3D_HD const JpegHuffSpec& jpeg_huff_spec(int which) {
    static constexpr JpegHuffSpec t[4] = {jpeg_std_spec(0), jpeg_std_spec(1), jpeg_std_spec(2), jpeg_std_spec(3)};
    return t[which];
}
DAD3D_HD const JpegHuffCodes& jpeg_huff_codes(int which) {
    static constexpr JpegHuffCodes t[4] = {jpeg_canonical_codes(jpeg_std_spec(0)), jpeg_canonical_codes(jpeg_std_spec(1)),
                                           jpeg_canonical_codes(jpeg_std_spec(2)), jpeg_canonical_codes(jpeg_std_spec(3))};
    return t[which];
}

// an AC table as one word per symbol, code << 8 | length: what the packing kernel copies into LDS, where a lookup costs no trip to memory
constexpr int kJpegAcLutWords = 256;
struct JpegAcLut {
    unsigned word[kJpegAcLutWords];
};
constexpr JpegAcLut jpeg_pack_codes(const JpegHuffCodes& t) {
    JpegAcLut l{};
    for (int i = 0; i < 256; ++i) l.word[i] = (unsigned)t.code[i] << 8 | t.len[i];
    return l;
}
DAD3D_HD const unsigned* jpeg_ac_lut(int chroma) {
    static constexpr JpegAcLut t[2] = {jpeg_pack_codes(jpeg_canonical_codes(jpeg_std_spec(1))), jpeg_pack_codes(jpeg_canonical_codes(jpeg_std_spec(3)))};
    return t[chroma].word;
}

DAD3D_HD int jpeg_enc_category(int v) {  // the bits of |v|
    const unsigned m = (unsigned)(v < 0 ? -v : v);
    return m ? 32 - __builtin_clz(m) : 0;
}

// The AC half of a block's cost, which no neighbour changes: its bits and the zigzag position of its last non-zero coefficient
// (0: none). kJpegEncPoison for a coefficient beyond category 10, which baseline's tables cannot code.
DAD3D_HD void jpeg_enc_ac_stats(const short* zz, int chroma, int& bits, int& last) {
    const JpegHuffCodes& ac = jpeg_huff_codes(2 * chroma + 1);
    int run = 0;
    bool bad = false;
    bits = 0, last = 0;
#pragma unroll
    for (int k = 1; k < 64; ++k) {
        const int v = zz[k];
        if (v == 0) {
            ++run;
            continue;
        }
        const int n = jpeg_enc_category(v);
        bad = bad || n > 10;
        bits += (run >> 4) * ac.len[0xf0] + ac.len[(run & 15) << 4 | (n & 15)] + n;
        run = 0, last = k;
    }
    if (last < 63) bits += ac.len[0];
    if (bad) bits = kJpegEncPoison;
}

// the DC half: the bits of the difference against the component's previous block; -1 beyond category 11
DAD3D_HD int jpeg_enc_dc_bits(int diff, int chroma) {
    const int n = jpeg_enc_category(diff);
    return n > 11 ? -1 : jpeg_huff_codes(2 * chroma).len[n] + n;
}

// the value bits of v in n bits: v itself, or v - 1 for a negative one
DAD3D_HD unsigned jpeg_enc_value_bits(int v, int n) { return (unsigned)(v < 0 ? v - 1 : v) & ((1u << n) - 1u); }

// the bits of one block through put(bits, count); `last` from jpeg_enc_ac_stats bounds the walk. The coefficients are read eight at a
// time, so `zz` is 16-byte aligned: a lane that walked them one by one would wait for a load per coefficient.
// `ac` is jpeg_ac_lut(chroma) or a copy of it.
template <typename Put>
DAD3D_HD void jpeg_enc_block_emit(const short* zz, int last, int pred, int chroma, const unsigned* ac, Put& put) {
    const JpegHuffCodes& dc = jpeg_huff_codes(2 * chroma);
    int run = 0;
    for (int k0 = 0; k0 <= last; k0 += 8) {
        short c[8];
        __builtin_memcpy(c, __builtin_assume_aligned(zz + k0, 16), 16);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = k0 + j, v = c[j];
            if (k == 0) {
                const int diff = v - pred, n = jpeg_enc_category(diff) & 15;
                put((unsigned)dc.code[n] << n | jpeg_enc_value_bits(diff, n), dc.len[n] + n);
                continue;
            }
            if (k > last) continue;
            if (v == 0) {
                ++run;
                continue;
            }
            for (; run > 15; run -= 16) put(ac[0xf0] >> 8, ac[0xf0] & 255);
            const int n = jpeg_enc_category(v) & 15;
            const unsigned sym = ac[run << 4 | n];
            put((sym >> 8) << n | jpeg_enc_value_bits(v, n), (sym & 255) + n);
            run = 0;
        }
    }
    if (last < 63) put(ac[0] >> 8, ac[0] & 255);
}

// SOI, JFIF APP0 (units 0, density 1 x 1), a DQT per table, SOF0, a DHT per table (DC then AC), DRI when there is an interval, SOS
DAD3D_HD int jpeg_enc_header_bytes(int c, int interval) {
    const int tables = c == 1 ? 1 : 2;
    return 2 + 18 + tables * 69 + (10 + 3 * c) + tables * (33 + 183) + (interval ? 6 : 0) + (8 + 2 * c) + 0;
}
// Lane `lane` of `lanes` writes its share (the host: lane 0 of 1); every lane returns the length.
DAD3D_HD int jpeg_enc_write_header(const JpegEncGeom& g, unsigned char* out, int lane = 0, int lanes = 1) {
    unsigned char* p = out;
    const int tables = g.c == 1 ? 1 : 2;
    const bool first = lane == 0;
    auto byte = [&p, first](int v) {
        if (first) *p = (unsigned char)v;
        ++p;
    };
    auto marker = [&byte](int m, int length) { byte(0xff), byte(m), byte(length >> 8), byte(length); };
    byte(0xff), byte(0xd8);
    marker(0xe0, 16);
    static constexpr unsigned char jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    for (int i = lane; i < 14; i += lanes) p[i] = jfif[i];
    p += 14;
    for (int t = 0; t < tables; ++t) {
        marker(0xdb, 67);
        byte(t);
        for (int k = lane; k < 64; k += lanes) p[k] = (unsigned char)jpeg_enc_quant(t, jpeg_natural(k), g.scale);
        p += 64;
    }
    marker(0xc0, 8 + 3 * g.c);
    byte(8), byte(g.h >> 8), byte(g.h), byte(g.w >> 8), byte(g.w), byte(g.c);
    for (int i = 0; i < g.c; ++i) byte(i + 1), byte(i ? 0x11 : g.hs << 4 | g.vs), byte(i ? 1 : 0);
    for (int t = 0; t < 2 * tables; ++t) {
        const JpegHuffSpec& s = jpeg_huff_spec(t);
        marker(0xc4, 19 + s.n);
        byte((t & 1) << 4 | t >> 1);
        for (int i = lane; i < 16; i += lanes) p[i] = s.counts[i];
        p += 16;
        for (int i = lane; i < s.n; i += lanes) p[i] = s.symbols[i];
        p += s.n;
    }
    if (g.interval) {
        marker(0xdd, 4);
        byte(g.interval >> 8), byte(g.interval);
    }
    marker(0xda, 6 + 2 * g.c);
    byte(g.c);
    for (int i = 0; i < g.c; ++i) byte(i + 1), byte(i ? 0x11 : 0);
    byte(0), byte(63), byte(0);
    return (int)(p - out);
}

// The proven bound on a file: the header; every block at kJpegEncMaxBlockBits, rounded up to bytes per block so that the sum also
// covers the padding of every interval; every entropy byte doubled by stuffing; a two-byte marker behind every interval (EOI behind
// the last), counted twice because the device checks a chunk against the row as if every byte of it, markers included, were
// stuffed; 16 bytes for that check's own slack.
DAD3D_HD long long jpeg_enc_intervals(const JpegEncGeom& g) {
    const long long mcus = (long long)g.mcus_x * g.mcus_y;
    return g.interval ? (mcus + g.interval - 1) / g.interval : 1;
}
DAD3D_HD long long jpeg_enc_max_bytes(int h, int w, int c, int subsampling) {
    const JpegEncGeom g = jpeg_enc_geometry(h, w, c, 50, subsampling, 1);  // an interval of one MCU: the most markers, and the DRI segment
    return jpeg_enc_header_bytes(c, 1) + 2 * ((kJpegEncMaxBlockBits + 7) / 8) * jpeg_enc_blocks(g) + 4 * jpeg_enc_intervals(g) + 16;
}

}  // namespace dad3d
