// Baseline JPEG, the arithmetic half, bit-equal to libjpeg-turbo as PIL drives it: the IJG "islow" integer IDCT,
// the "fancy" chroma upsampling and the YCbCr -> RGB conversion. Shared by csrc/jpeg_decode.hip and dad3d_jpeg_decode_host.
// The sums are taken in unsigned words, so that a damaged file's coefficients wrap instead of overflowing; a file whose values leave
// the ranges libjpeg-turbo's vector code keeps (16 bits in front of and behind the first pass, -512 .. 511 behind the second, where
// its range table wraps) is flagged before any such value is used.
#pragma once

#include "jpeg_entropy.hpp"

namespace dad3d {

// the eight outputs of one pass, before the descale
DAD3D_HD void jpeg_idct_1d(const int* in, int stride, int* o) {
    typedef unsigned U;
    const U i0 = (U)in[0], i1 = (U)in[stride], i2 = (U)in[2 * stride], i3 = (U)in[3 * stride], i4 = (U)in[4 * stride], i5 = (U)in[5 * stride],
            i6 = (U)in[6 * stride], i7 = (U)in[7 * stride];
    U z1 = (i2 + i6) * 4433u;
    U t2 = z1 - i6 * 15137u, t3 = z1 + i2 * 6270u;
    U t0 = (i0 + i4) << 13, t1 = (i0 - i4) << 13;
    const U a10 = t0 + t3, a13 = t0 - t3, a11 = t1 + t2, a12 = t1 - t2;
    t0 = i7, t1 = i5, t2 = i3, t3 = i1;
    z1 = t0 + t3;
    U z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const U z5 = (z3 + z4) * 9633u;
    t0 *= 2446u, t1 *= 16819u, t2 *= 25172u, t3 *= 12299u;
    z1 *= (U)-7373, z2 *= (U)-20995, z3 *= (U)-16069, z4 *= (U)-3196;
    z3 += z5, z4 += z5;
    t0 += z1 + z3, t1 += z2 + z4, t2 += z2 + z3, t3 += z1 + z4;
    o[0] = (int)(a10 + t3), o[7] = (int)(a10 - t3);
    o[1] = (int)(a11 + t2), o[6] = (int)(a11 - t2);
    o[2] = (int)(a12 + t1), o[5] = (int)(a12 - t1);
    o[3] = (int)(a13 + t0), o[4] = (int)(a13 - t0);
}

DAD3D_HD bool jpeg_fits_int16(int v) { return v >= -32768 && v <= 32767; }

// one block: dequantise, both passes, level shift and clamp; out[8 rows][pitch]. Returns the flag, and writes nothing when it is set.
DAD3D_HD int jpeg_idct_block(const short* coef, const unsigned short* quant, unsigned char* out, int pitch) {
    int ws[64];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        ws[i] = (int)coef[i] * (int)quant[i];
        ok = ok && jpeg_fits_int16(ws[i]);
    }
    if (!ok) return kJpegUnsupported;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        int o[8];
        jpeg_idct_1d(ws + c, 8, o);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            ws[r * 8 + c] = (o[r] + 1024) >> 11;
            ok = ok && jpeg_fits_int16(ws[r * 8 + c]);
        }
    }
    if (!ok) return kJpegUnsupported;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        int o[8];
        jpeg_idct_1d(ws + r * 8, 1, o);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            ws[r * 8 + c] = (o[c] + 131072) >> 18;
            ok = ok && ws[r * 8 + c] >= -512 && ws[r * 8 + c] <= 511;
        }
    }
    if (!ok) return kJpegUnsupported;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        unsigned lo = 0, hi = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int a = ws[r * 8 + c] + 128, b = ws[r * 8 + 4 + c] + 128;
            lo |= (unsigned)(a < 0 ? 0 : a > 255 ? 255 : a) << (8 * c);
            hi |= (unsigned)(b < 0 ? 0 : b > 255 ? 255 : b) << (8 * c);
        }
        unsigned* row = reinterpret_cast<unsigned*>(out + (size_t)r * pitch);  // the plane, its pitch and the block's column: multiples of 8
        row[0] = lo, row[1] = hi;
    }
    return 0;
}

// The chroma sample at (x, y) of the full-size image from a component kept at 1 / hs by 1 / vs, of dw x dh samples of its own (the
// block padding behind them is never read).
DAD3D_HD int jpeg_upsampled(const unsigned char* p, int pitch, int dw, int dh, int hs, int vs, int x, int y) {
    if (hs == 1) return p[(size_t)y * pitch + x];
    const int i = x >> 1;
    if (vs == 1) {
        const unsigned char* row = p + (size_t)y * pitch;
        if (dw <= 2) return row[i];
        if (x & 1) return i == dw - 1 ? row[i] : (3 * row[i] + row[i + 1] + 2) >> 2;
        return i == 0 ? row[0] : (3 * row[i] + row[i - 1] + 1) >> 2;
    }
    const int r = y >> 1;
    if (dw <= 2) return p[(size_t)r * pitch + i];
    const int other = (y & 1) ? (r + 1 < dh ? r + 1 : dh - 1) : (r > 0 ? r - 1 : 0);
    const unsigned char *near = p + (size_t)r * pitch, *far = p + (size_t)other * pitch;
    const int t = 3 * near[i] + far[i];
    if (x & 1) return i == dw - 1 ? (4 * t + 7) >> 4 : (3 * t + 3 * near[i + 1] + far[i + 1] + 7) >> 4;
    return i == 0 ? (4 * t + 8) >> 4 : (3 * t + 3 * near[i - 1] + far[i - 1] + 8) >> 4;
}

DAD3D_HD int jpeg_clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// one pixel of the output, `oc` bytes at px, from the planes of the file (component c at planes + 64 * jpeg_component_base(F, c))
DAD3D_HD void jpeg_pixel(const JpegFile& F, const unsigned char* planes, int x, int y, int oc, unsigned char* px) {
    const int lum = planes[(size_t)y * (jpeg_blocks_across(F, 0) * 8) + x];
    if (F.comps == 1) {
        px[0] = (unsigned char)lum;
        if (oc == 3) px[1] = px[2] = (unsigned char)lum;
        return;
    }
    const int dw = (F.w + F.hs - 1) / F.hs, dh = (F.h + F.vs - 1) / F.vs, pitch = F.mx * 8;
    const int cb = jpeg_upsampled(planes + (size_t)64 * jpeg_component_base(F, 1), pitch, dw, dh, F.hs, F.vs, x, y) - 128;
    const int cr = jpeg_upsampled(planes + (size_t)64 * jpeg_component_base(F, 2), pitch, dw, dh, F.hs, F.vs, x, y) - 128;
    const int r = jpeg_clamp255(lum + ((91881 * cr + 32768) >> 16));
    const int b = jpeg_clamp255(lum + ((116130 * cb + 32768) >> 16));
    const int g = jpeg_clamp255(lum + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
    if (oc == 3)
        px[0] = (unsigned char)r, px[1] = (unsigned char)g, px[2] = (unsigned char)b;
    else
        px[0] = (unsigned char)((19595u * (unsigned)r + 38470u * (unsigned)g + 7471u * (unsigned)b + 32768u) >> 16);
}

}  // namespace dad3d
