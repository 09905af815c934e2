// Baseline JPEG, the serial half (ITU-T T.81): the marker walk up to the scan, the tables, the bit reader and the Huffman decode of one
// entropy segment. Shared by the kernels of csrc/jpeg_decode.hip (one lane runs a routine) and by dad3d_jpeg_decode_host, so
// tests/test_jpeg_host.py holds to PIL, on a CPU, the code the kernels run. DESIGN.md 4.19 lists what is accepted; everything else
// is a flag, and a flagged file is decoded by PIL on the host. A routine reads nothing outside [file, file + len) and writes nothing
// outside the places it is handed; every loop is bounded by a byte count, a block count, 16 code lengths or 63 AC steps.
#pragma once

#include "../../include/dad3d.h"

#ifndef DAD3D_HD
#define DAD3D_HD __host__ __device__ inline
#endif

namespace dad3d {

constexpr int kJpegMalformed = DAD3D_JPEG_DECODE_FLAG_MALFORMED, kJpegUnsupported = DAD3D_JPEG_DECODE_FLAG_UNSUPPORTED;
constexpr int kJpegMaxBlocks = 1 << 22;  // per file, block padding included: every index below stays inside an int

// A Huffman table in canonical form: counts per length and the symbols in code order, as inflate.hpp holds its codes, and beside them
// what a 16-bit peek needs: a peek below limit[len] starts with a code of at most len bits, which is symbols[offset[len] + its
// first len bits]; and look[the peek's first eight bits] = length << 8 | symbol for a code of eight bits or fewer, else 0.
struct JpegHuff {
    unsigned limit[17];
    int offset[17];
    unsigned char counts[17];
    unsigned char pad[3];
    unsigned char symbols[256];
    unsigned short look[256];
};

struct JpegSegment {
    int start, end;  // the entropy bytes [start, end) from the start of the file
};

struct JpegFile {
    int flag, h, w, comps;
    int hs, vs;              // sampling of the first component; the others are 1 x 1
    int mx, my;              // the MCU grid
    int interval, nseg;      // restart interval in MCUs (0: none), entropy segments
    int scan_at, scan_end;   // the entropy data [scan_at, scan_end): scan_end is the place of EOI
    int id[3], tq[3], td[3], ta[3];
    unsigned short quant[4][64];  // natural order
    JpegHuff huff[8];             // class * 4 + id
};

DAD3D_HD int jpeg_natural(int k) {  // zigzag position -> natural (row-major) position
    static constexpr unsigned char order[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                                41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                                30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return order[k];
}

// the block capacity the host sizes scratch with from (h, w, components) alone: at least the blocks of any accepted sampling
DAD3D_HD long long jpeg_block_capacity(long long h, long long w, long long comps) { return comps * ((w + 7) / 8 + 1) * ((h + 7) / 8 + 1); }
// and the capacity of the segment table: a segment holds an MCU or more, and every one but the last ends in a two-byte marker
DAD3D_HD long long jpeg_segment_capacity(long long h, long long w, long long file_bytes) {
    const long long mcus = ((w + 7) / 8) * ((h + 7) / 8), by_bytes = file_bytes / 2 + 1;
    return mcus < by_bytes ? mcus : by_bytes;
}

// blocks across of component c, and where its blocks start among the file's
DAD3D_HD int jpeg_blocks_across(const JpegFile& F, int c) { return F.mx * (c == 0 ? F.hs : 1); }
DAD3D_HD int jpeg_component_base(const JpegFile& F, int c) {
    const int luma = F.mx * F.hs * F.my * F.vs;
    return c == 0 ? 0 : luma + (c - 1) * F.mx * F.my;
}
DAD3D_HD int jpeg_total_blocks(const JpegFile& F) { return jpeg_component_base(F, F.comps); }

// DHT: one table from its 16 counts and its symbols; the validity libjpeg asks when it derives a table (no code reaches the all-ones
// code of its length) and, for a DC table, symbols within 0 .. 15
DAD3D_HD int jpeg_build_huff(const unsigned char* d, int total, bool dc, JpegHuff& t) {
    unsigned code = 0;
    int k = 0;
    t.limit[0] = 0, t.offset[0] = 0, t.counts[0] = 0;
    for (int len = 1; len <= 16; ++len) {
        const unsigned c = d[len - 1];
        t.counts[len] = (unsigned char)c;
        t.offset[len] = k - (int)code;
        if (c && code + c >= (1u << len)) return kJpegMalformed;
        t.limit[len] = c ? (code + c) << (16 - len) : 0u;
        code = (code + c) << 1;
        k += (int)c;
    }
    for (int i = 0; i < 256; ++i) {
        const unsigned char s = i < total ? d[16 + i] : (unsigned char)0;
        if (dc && s > 15) return kJpegMalformed;
        t.symbols[i] = s;
        t.look[i] = 0;
    }
    code = 0, k = 0;
    for (int len = 1; len <= 8; ++len) {
        for (unsigned c = d[len - 1]; c; --c, ++code, ++k)  // the code is below 2^len: checked above
            for (unsigned fill = 0; fill < (1u << (8 - len)); ++fill) t.look[(code << (8 - len)) + fill] = (unsigned short)(len << 8 | d[16 + k]);
        code <<= 1;
    }
    return 0;
}

DAD3D_HD bool jpeg_tag(const unsigned char* d, char a, char b, char c, char e, char g) {
    return d[0] == (unsigned char)a && d[1] == (unsigned char)b && d[2] == (unsigned char)c && d[3] == (unsigned char)e && d[4] == (unsigned char)g;
}

// The marker walk from SOI to the first byte of the entropy data. Fills everything of F but nseg, scan_end and the flag; returns the flag.
DAD3D_HD int jpeg_parse_header(const unsigned char* f, long long len, JpegFile& F) {
    F.h = F.w = F.comps = 0, F.hs = F.vs = 1, F.mx = F.my = 0, F.interval = 0, F.nseg = 0, F.scan_at = F.scan_end = 0;
    if (len < 4 || len > 0x7fffffffll || f[0] != 0xff || f[1] != 0xd8) return kJpegMalformed;
    bool jfif = false, adobe = false, sof = false;
    unsigned quant_defined = 0, huff_defined = 0;
    long long pos = 2;
    for (;;) {  // every turn moves pos on by four bytes or more
        if (pos + 4 > len || f[pos] != 0xff) return kJpegMalformed;
        const int m = f[pos + 1], seg = f[pos + 2] << 8 | f[pos + 3];
        if (seg < 2 || pos + 2 + seg > len) return kJpegMalformed;
        const unsigned char* d = f + pos + 4;
        int n = seg - 2;
        if ((m >= 0xe0 && m <= 0xef) || m == 0xfe) {
            if (m == 0xe0 && n >= 14 && jpeg_tag(d, 'J', 'F', 'I', 'F', 0)) jfif = true;
            if (m == 0xee && n >= 5 && jpeg_tag(d, 'A', 'd', 'o', 'b', 'e')) adobe = true;
        } else if (m == 0xdb) {
            while (n > 0) {
                if (n < 65) return kJpegMalformed;
                const int pq = d[0] >> 4, tq = d[0] & 15;
                if (pq == 1) return kJpegUnsupported;  // 16-bit entries
                if (pq || tq > 3) return kJpegMalformed;
                for (int i = 0; i < 64; ++i) F.quant[tq][jpeg_natural(i)] = d[1 + i];
                quant_defined |= 1u << tq;
                d += 65, n -= 65;
            }
        } else if (m == 0xc4) {
            while (n > 0) {
                if (n < 17) return kJpegMalformed;
                const int tc = d[0] >> 4, th = d[0] & 15;
                int total = 0;
                for (int i = 1; i <= 16; ++i) total += d[i];
                if (tc > 1 || th > 3 || total > 256 || n < 17 + total) return kJpegMalformed;
                if (jpeg_build_huff(d + 1, total, tc == 0, F.huff[tc * 4 + th])) return kJpegMalformed;
                huff_defined |= 1u << (tc * 4 + th);
                d += 17 + total, n -= 17 + total;
            }
        } else if (m == 0xc0) {
            if (sof || n < 6) return kJpegMalformed;
            const int precision = d[0], nc = d[5];
            F.h = d[1] << 8 | d[2], F.w = d[3] << 8 | d[4];
            if (precision == 12 || nc == 2 || nc == 4 || (F.h == 0 && F.w > 0)) return kJpegUnsupported;  // h == 0: the height comes in a DNL
            if (precision != 8 || (nc != 1 && nc != 3) || n != 6 + 3 * nc || F.w == 0) return kJpegMalformed;
            for (int c = 0; c < nc; ++c) {
                const int hv = d[7 + 3 * c], ch = hv >> 4, cv = hv & 15, tq = d[8 + 3 * c];
                if (ch < 1 || ch > 4 || cv < 1 || cv > 4 || tq > 3) return kJpegMalformed;
                const bool first_ok = nc == 3 ? (hv == 0x11 || hv == 0x21 || hv == 0x22) : hv == 0x11;
                if (c == 0 ? !first_ok : hv != 0x11) return kJpegUnsupported;
                if (c == 0) F.hs = ch, F.vs = cv;
                F.id[c] = d[6 + 3 * c], F.tq[c] = tq;
            }
            if (nc == 3 && (F.id[0] == F.id[1] || F.id[0] == F.id[2] || F.id[1] == F.id[2])) return kJpegMalformed;
            F.comps = nc;
            F.mx = (F.w + 8 * F.hs - 1) / (8 * F.hs), F.my = (F.h + 8 * F.vs - 1) / (8 * F.vs);
            sof = true;
        } else if (m == 0xdd) {
            if (n != 2) return kJpegMalformed;
            F.interval = d[0] << 8 | d[1];
        } else if (m == 0xda) {
            if (!sof || n != 4 + 2 * F.comps || d[0] != F.comps) return sof && n >= 1 && d[0] >= 1 && d[0] < F.comps ? kJpegUnsupported : kJpegMalformed;
            for (int c = 0; c < F.comps; ++c) {
                const int td = d[2 + 2 * c] >> 4, ta = d[2 + 2 * c] & 15;
                if (d[1 + 2 * c] != F.id[c] || td > 3 || ta > 3) return kJpegMalformed;
                if (!(huff_defined >> td & 1u) || !(huff_defined >> (4 + ta) & 1u) || !(quant_defined >> F.tq[c] & 1u)) return kJpegMalformed;
                F.td[c] = td, F.ta[c] = ta;
            }
            const unsigned char* e = d + 1 + 2 * F.comps;
            if (e[0] != 0 || e[1] != 63 || e[2] != 0) return kJpegUnsupported;
            if (F.comps == 3 && (adobe || (!jfif && !(F.id[0] == 1 && F.id[1] == 2 && F.id[2] == 3)))) return kJpegUnsupported;
            if (jpeg_block_capacity(F.h, F.w, F.comps) > kJpegMaxBlocks) return kJpegUnsupported;
            F.scan_at = (int)(pos + 2 + seg);
            return 0;
        } else if (m == 0xc1 || m == 0xc2 || m == 0xc3 || (m >= 0xc5 && m <= 0xcf) || m == 0xdc) {
            return kJpegUnsupported;  // extended, progressive, lossless, arithmetic coding, DNL
        } else {
            return kJpegMalformed;
        }
        pos += 2 + seg;
    }
}

// the segments a file with this header must have
DAD3D_HD int jpeg_expected_segments(const JpegFile& F) {
    const int mcus = F.mx * F.my;
    return F.interval ? (mcus + F.interval - 1) / F.interval : 1;
}

// The table of entropy segments, serially (the scan kernel does the same with 64 lanes): from scan_at to the first marker that is no
// restart marker, which has to be EOI. Sets nseg and scan_end; returns the flag.
DAD3D_HD int jpeg_find_segments(const unsigned char* f, long long len, JpegFile& F, JpegSegment* segs, long long segs_cap) {
    const int expected = jpeg_expected_segments(F);
    if (expected > segs_cap) return kJpegMalformed;
    int count = 0;
    segs[0].start = F.scan_at;
    for (long long p = F.scan_at; p + 1 < len; ++p) {
        if (f[p] != 0xff || f[p + 1] == 0) continue;
        const int b = f[p + 1];
        if (b >= 0xd0 && b <= 0xd7) {
            if (b - 0xd0 != (count & 7) || count + 1 >= expected) return kJpegMalformed;  // out of sequence, or more than the grid holds
            segs[count].end = (int)p, segs[count + 1].start = (int)p + 2;
            ++count;
            continue;
        }
        if (b != 0xd9) return kJpegUnsupported;  // fill bytes in front of a marker, a second scan, DNL, tables between scans
        if (count != expected - 1) return kJpegMalformed;
        segs[count].end = (int)p;
        F.nseg = expected, F.scan_end = (int)p;
        return 0;
    }
    return kJpegMalformed;  // no EOI
}

// MSB-first bits of one segment; FF 00 is the data byte FF. `over` once a bit beyond the last byte was asked for. A refill takes up
// to four bytes by loads that do not wait for each other (a lane's walk is a chain of dependent loads, and this is its longest
// link); whether the byte behind an FF is still to be dropped is carried from one refill to the next.
struct JpegBits {
    const unsigned char* p;
    const unsigned char* end;
    unsigned long long acc;  // the low `have` bits are unread
    int have;
    bool over, bad, zero_due;

    DAD3D_HD void take(unsigned b) {
        if (zero_due) {
            if (b != 0) bad = true;  // the scan found no marker here: cannot happen
            zero_due = false;
        } else {
            acc = acc << 8 | b, have += 8;
            zero_due = b == 0xff;
        }
    }
    DAD3D_HD void fill() {
        if (have > 32 || p >= end) return;
        const long long left = end - p;
        const int n = left < 4 ? (int)left : 4;
        const unsigned b0 = p[0], b1 = p[n > 1 ? 1 : 0], b2 = p[n > 2 ? 2 : 0], b3 = p[n > 3 ? 3 : 0];
        take(b0);
        if (n > 1) take(b1);
        if (n > 2) take(b2);
        if (n > 3) take(b3);
        p += n;
    }
    DAD3D_HD unsigned peek16() {
        fill();
        return (unsigned)(have >= 16 ? acc >> (have - 16) : acc << (16 - have)) & 0xffffu;
    }
    DAD3D_HD void skip(int n) {
        if (n > have) over = true, have = 0;
        else have -= n;
    }
    DAD3D_HD int get(int n) {  // 1 .. 16 bits
        fill();
        if (have < n) {
            over = true, have = 0;
            return 0;
        }
        have -= n;
        return (int)(acc >> have) & ((1 << n) - 1);
    }
    // at the end of the segment: a whole byte nobody read, or an FF whose 00 is missing
    DAD3D_HD bool left_over() {
        if (zero_due) {
            if (p < end && *p == 0)
                ++p, zero_due = false;
            else
                bad = true;
        }
        return p < end || have >= 8 || bad;
    }
};

template <class Bits>  // JpegBits, or the reader of jpeg_sync.hpp that also knows where in the file it stands
DAD3D_HD int jpeg_symbol(Bits& in, const JpegHuff& t) {  // -1: a code no table assigns
    const unsigned v = in.peek16();
    const unsigned quick = t.look[v >> 8];  // a code of eight bits or fewer: one read
    if (quick) {
        in.skip((int)(quick >> 8));
        return (int)(quick & 255u);
    }
    for (int len = 9; len <= 16; ++len)
        if (v < t.limit[len]) {
            in.skip(len);
            return t.symbols[(t.offset[len] + (int)(v >> (16 - len))) & 255];
        }
    return -1;
}

DAD3D_HD int jpeg_extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// one block: 64 quantised coefficients in natural order, zeros included; false for a damaged stream
DAD3D_HD bool jpeg_block(JpegBits& in, const JpegHuff& dc, const JpegHuff& ac, int& pred, short* dst) {
    for (int i = 0; i < 64; ++i) dst[i] = 0;
    int s = jpeg_symbol(in, dc);
    if (s < 0 || s > 11) return false;
    if (s) pred += jpeg_extend(in.get(s), s);
    if (pred < -32768 || pred > 32767) return false;
    dst[0] = (short)pred;
    for (int k = 1; k < 64;) {  // k grows every turn
        const int rs = jpeg_symbol(in, ac);
        if (rs < 0) return false;
        const int r = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (r != 15) break;
            k += 16;
            continue;
        }
        k += r;
        if (s > 10 || k > 63) return false;
        dst[jpeg_natural(k)] = (short)jpeg_extend(in.get(s), s);
        ++k;
    }
    return !in.over && !in.bad;
}

// Segment `seg` of the file: its MCUs' blocks into coefs[block][64], component after component (jpeg_component_base), each
// component's blocks row-major over its padded grid. Returns the flag.
DAD3D_HD int jpeg_decode_segment(const unsigned char* f, const JpegFile& F, int seg, JpegSegment where, short* coefs) {
    const int mcus = F.mx * F.my;
    const int first = F.interval ? seg * F.interval : 0;
    const int last = F.interval && first + F.interval < mcus ? first + F.interval : mcus;
    JpegBits in{f + where.start, f + where.end, 0ull, 0, false, false, false};
    if (where.start < F.scan_at || where.end < where.start || where.end > F.scan_end) return kJpegMalformed;
    int pred0 = 0, pred1 = 0, pred2 = 0;
    const int hs = F.hs, luma = hs * F.vs, per_mcu = F.comps == 3 ? luma + 2 : luma, mx = F.mx;
    const int base1 = jpeg_component_base(F, 1), base2 = jpeg_component_base(F, 2);
    for (int m = first; m < last; ++m) {
        const int my_ = m / mx, mx_ = m - my_ * mx;
        for (int j = 0; j < per_mcu; ++j) {  // one place for the block decode: the luma blocks v rows of h, then Cb, then Cr
            const int c = j < luma ? 0 : j - luma + 1, v = j / hs, h = j - v * hs;
            const int at = c == 0 ? (my_ * F.vs + v) * (mx * hs) + mx_ * hs + h : (c == 1 ? base1 : base2) + m;
            int pred = c == 0 ? pred0 : c == 1 ? pred1 : pred2;
            if (!jpeg_block(in, F.huff[F.td[c]], F.huff[4 + F.ta[c]], pred, coefs + (size_t)at * 64)) return kJpegMalformed;
            pred0 = c == 0 ? pred : pred0, pred1 = c == 1 ? pred : pred1, pred2 = c == 2 ? pred : pred2;
        }
    }
    return in.over || in.left_over() || in.bad ? kJpegMalformed : 0;
}

}  // namespace dad3d
