// Baseline JPEG written, the arithmetic half, byte-equal to libjpeg-turbo as PIL drives it: the geometry of the scan,
// RGB -> YCbCr in 16-bit fixed point (jccolor.c), edge replication and the h2v1 / h2v2 box filters with their alternating bias
// (jcprepct.c, jcsample.c), the level shift, the IJG "islow" forward DCT (jfdctint.c) and the quantiser that divides by 8 Q and rounds
// half away from zero (jcdctmgr.c). Shared by csrc/jpeg_encode.hip and dad3d_jpeg_encode_host. Every index is clamped into the
// image before it is used, so a routine reads nothing outside [img, img + h * w * c).
#pragma once

#include "jpeg_entropy.hpp"  // DAD3D_HD, and jpeg_natural: the zigzag order is the decoder's

namespace dad3d {

constexpr int kJpegEncMaxBlocks = 1 << 22;  // per image, dummy blocks included: every block index and every chunk count stays inside an int

// The scan of one image. A colour scan is interleaved: an MCU is hs x vs luma blocks, then Cb, then Cr. A grey scan has one component,
// so it is not interleaved: an MCU is one block and nothing is padded to sampling factors.
struct JpegEncGeom {
    int h, w, c;
    int hs, vs;            // sampling of the luma; the chroma is 1 x 1
    int mcus_x, mcus_y;
    int per_mcu;           // blocks of an MCU
    int real_x, real_y;    // luma blocks that hold samples; the MCU grid may ask for more (dummy blocks)
    int scale;             // jpeg_quality_scaling(quality)
    int interval;          // MCUs per restart interval, 0: none
};

DAD3D_HD JpegEncGeom jpeg_enc_geometry(int h, int w, int c, int quality, int subsampling, int interval) {
    JpegEncGeom g;
    g.h = h, g.w = w, g.c = c;
    g.hs = c == 3 && subsampling >= 1 ? 2 : 1, g.vs = c == 3 && subsampling == 2 ? 2 : 1;
    g.real_x = (w + 7) / 8, g.real_y = (h + 7) / 8;
    g.mcus_x = (g.real_x + g.hs - 1) / g.hs, g.mcus_y = (g.real_y + g.vs - 1) / g.vs;
    g.per_mcu = c == 1 ? 1 : g.hs * g.vs + 2;
    g.scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    g.interval = interval;
    return g;
}
DAD3D_HD long long jpeg_enc_blocks(const JpegEncGeom& g) { return (long long)g.mcus_x * g.mcus_y * g.per_mcu; }

// Annex K.1 scaled by jpeg_set_quality(quality, force_baseline): entry `natural` (row-major) of table `which` (0 luma, 1 chroma)
DAD3D_HD int jpeg_enc_quant(int which, int natural, int scale) {
    static constexpr unsigned char luma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                                               69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
                                               81, 104, 113, 92, 49, 64,  78,  87,  103, 121, 120, 101, 72, 92,  95,  98,  112, 100, 103, 99};
    static constexpr unsigned char chroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                                 99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                                 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
    const int q = ((which ? chroma[natural] : luma[natural]) * scale + 50) / 100;
    return q < 1 ? 1 : q > 255 ? 255 : q;
}

// Block `index` of the scan: its component and the block of that component whose samples it is made from. A dummy block keeps the
// DC of its source and no AC (jccoefct.c): on the right the source is the block in front of it, which ends at the last real block of
// the row; in a dummy row at the bottom it is, for every block of the row, the LAST block of the MCU's row above.
struct JpegEncBlock {
    int comp, bx, by;
    bool dummy;
};
DAD3D_HD JpegEncBlock jpeg_enc_locate(const JpegEncGeom& g, int index) {
    const int mcu = index / g.per_mcu, j = index - mcu * g.per_mcu, my = mcu / g.mcus_x, mx = mcu - my * g.mcus_x;
    JpegEncBlock b;
    b.dummy = false;
    if (g.c == 1 || j >= g.hs * g.vs) {
        b.comp = g.c == 1 ? 0 : j - g.hs * g.vs + 1, b.bx = mx, b.by = my;
        return b;
    }
    const int v = j / g.hs, u = j - v * g.hs, by = my * g.vs + v, bx = mx * g.hs + u;
    const int src_x = by < g.real_y ? bx : mx * g.hs + g.hs - 1;
    b.comp = 0, b.dummy = by >= g.real_y || bx >= g.real_x;
    b.bx = src_x < g.real_x ? src_x : g.real_x - 1, b.by = by < g.real_y ? by : g.real_y - 1;
    return b;
}

// component `comp` (0 Y, 1 Cb, 2 Cr) of one RGB pixel
DAD3D_HD int jpeg_enc_ycc(const unsigned char* px, int comp) {
    const int r = px[0], g = px[1], b = px[2];
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// The 64 level-shifted samples of block (bx, by) of a component. Columns past the image repeat its last column BEFORE the box filter;
// rows repeat the last row up to a multiple of vs before the filter, and the last filtered row behind it.
DAD3D_HD void jpeg_enc_samples(const unsigned char* img, const JpegEncGeom& g, const JpegEncBlock& b, int* d) {
    const int hs = b.comp ? g.hs : 1, vs = b.comp ? g.vs : 1, rows = (g.h + vs - 1) / vs;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        int j = b.by * 8 + r;
        j = j < rows ? j : rows - 1;
        const int y0 = j * vs < g.h ? j * vs : g.h - 1, y1 = j * vs + vs - 1 < g.h ? j * vs + vs - 1 : g.h - 1;
        const unsigned char *row0 = img + (size_t)y0 * g.w * g.c, *row1 = img + (size_t)y1 * g.w * g.c;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int i = b.bx * 8 + k;
            const int x0 = i * hs < g.w ? i * hs : g.w - 1, x1 = i * hs + hs - 1 < g.w ? i * hs + hs - 1 : g.w - 1;
            int s;
            if (g.c == 1) {
                s = row0[x0];
            } else if (hs == 1) {
                s = jpeg_enc_ycc(row0 + 3 * x0, b.comp);
            } else if (vs == 1) {
                s = (jpeg_enc_ycc(row0 + 3 * x0, b.comp) + jpeg_enc_ycc(row0 + 3 * x1, b.comp) + (k & 1)) >> 1;
            } else {
                s = (jpeg_enc_ycc(row0 + 3 * x0, b.comp) + jpeg_enc_ycc(row0 + 3 * x1, b.comp) + jpeg_enc_ycc(row1 + 3 * x0, b.comp) +
                     jpeg_enc_ycc(row1 + 3 * x1, b.comp) + 1 + (k & 1)) >> 2;
            }
            d[r * 8 + k] = s - 128;
        }
    }
}

// one pass of jfdctint.c over eight values at `stride`, in place; the first pass scales up by PASS1_BITS, the second takes it off
DAD3D_HD int jpeg_enc_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
DAD3D_HD void jpeg_fdct_1d(int* d, int stride, bool first) {
    const int t0 = d[0] + d[7 * stride], t7 = d[0] - d[7 * stride], t1 = d[stride] + d[6 * stride], t6 = d[stride] - d[6 * stride];
    const int t2 = d[2 * stride] + d[5 * stride], t5 = d[2 * stride] - d[5 * stride], t3 = d[3 * stride] + d[4 * stride],
              t4 = d[3 * stride] - d[4 * stride];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2, n = first ? 11 : 15;
    d[0] = first ? (t10 + t11) * 4 : jpeg_enc_descale(t10 + t11, 2);
    d[4 * stride] = first ? (t10 - t11) * 4 : jpeg_enc_descale(t10 - t11, 2);
    int z1 = (t12 + t13) * 4433;
    d[2 * stride] = jpeg_enc_descale(z1 + t13 * 6270, n);
    d[6 * stride] = jpeg_enc_descale(z1 - t12 * 15137, n);
    z1 = t4 + t7;
    const int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7, z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    const int b1 = z1 * -7373, b2 = z2 * -20995, b3 = z3 * -16069 + z5, b4 = z4 * -3196 + z5;
    d[7 * stride] = jpeg_enc_descale(a4 + b1 + b3, n);
    d[5 * stride] = jpeg_enc_descale(a5 + b2 + b4, n);
    d[3 * stride] = jpeg_enc_descale(a6 + b2 + b3, n);
    d[stride] = jpeg_enc_descale(a7 + b1 + b4, n);
}

// x / div for 0 <= x < 2^24 and 1 <= div < 2^12, exactly, without an integer division: the float quotient is within one of the
// true one (x and div are exact in float, the reciprocal and the product each err by a relative 2^-23 or less, and x / div < 2^24),
// and the remainder says which way.
DAD3D_HD int jpeg_enc_divide(int x, int div) {
#ifdef __HIP_DEVICE_COMPILE__
    const float r = __builtin_amdgcn_rcpf((float)div);
#else
    const float r = 1.0f / (float)div;
#endif
    int q = (int)((float)x * r);
    const int rest = x - q * div;
    q += rest >= div ? 1 : 0;
    q -= rest < 0 ? 1 : 0;
    return q;
}

// Samples (level-shifted, natural order, destroyed) -> quantised coefficients in zigzag order. |sample| <= 128 keeps every
// intermediate inside 32 bits: pass 1 leaves at most 2^12, pass 2's products stay below 2^30.
DAD3D_HD void jpeg_fdct_quantise(int* d, int which, int scale, bool dummy, short* zz) {
#pragma unroll
    for (int r = 0; r < 8; ++r) jpeg_fdct_1d(d + 8 * r, 1, true);
#pragma unroll
    for (int k = 0; k < 8; ++k) jpeg_fdct_1d(d + k, 8, false);
#pragma unroll
    for (int k = 0; k < 64; ++k) {
        const int n = jpeg_natural(k), div = 8 * jpeg_enc_quant(which, n, scale), v = d[n];
        const int mag = jpeg_enc_divide((v < 0 ? -v : v) + (div >> 1), div);
        zz[k] = dummy && k ? (short)0 : (short)(v < 0 ? -mag : mag);
    }
}

}  // namespace dad3d
