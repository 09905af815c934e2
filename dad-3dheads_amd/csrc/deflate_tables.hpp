// The Huffman tables of one dynamic deflate block (RFC 1951 3.2.7) from the block's symbol histograms: length-limited code lengths,
// canonical codes and the bits of the block header. The single-lane part of csrc/png_encode.hip. __host__
// __device__, integers only and no indexed local arrays (every table lives in memory the caller hands in: LDS on the device), so
// the code one lane of deflate_segment_kernel runs is the code dad3d_deflate_tables_host runs on a CPU.
//
// Code lengths: the used symbols sorted by (count, symbol); minimum-redundancy depths in place (Moffat & Katajainen, "In-place
// calculation of minimum-redundancy codes", 1995); depths above the limit are clamped and the count of codes per length repaired
// until the Kraft sum is exactly 1 (lengthen the deepest code above the limit level while the sum is over, then shorten the
// code that gains most without overshooting); the lengths go back to the symbols in sorted order, rarest longest.
// One used symbol gets one bit (the incomplete code inflate accepts), none gets no code at all.
#pragma once

#include <hip/hip_runtime.h>

namespace dad3d {

constexpr int kDeflateLitCodes = 286;    // literals 0..255, end of block 256, lengths 257..285
constexpr int kDeflateDistCodes = 30;
constexpr int kDeflateClCodes = 19;      // the code-length alphabet: 0..15, 16 / 17 / 18 = repeat
constexpr int kDeflateHeaderBytes = 640; // 3 + 14 + 19 * 3 + 316 * 14 bits at the very most
constexpr unsigned kDeflateMaxCount = 1u << 22;  // a histogram entry stays below this (sort key: count << 9 | symbol)

struct DeflateTables {
    unsigned char ll_len[kDeflateLitCodes], d_len[kDeflateDistCodes], cl_len[kDeflateClCodes];
    unsigned short ll_code[kDeflateLitCodes], d_code[kDeflateDistCodes], cl_code[kDeflateClCodes];  // canonical, as RFC 1951 3.2.2 numbers them
    unsigned char header[kDeflateHeaderBytes];  // BFINAL = 0, BTYPE = 10, HLIT, HDIST, HCLEN, the code-length code, both length runs: LSB first
    int header_bits;
    unsigned dynamic_bits;  // header + every symbol of the histograms with its extra bits: the whole block
    unsigned fixed_bits;    // the same symbols as a fixed-Huffman block, its three header bits included
};

struct DeflateWork {
    unsigned key[kDeflateLitCodes], depth[kDeflateLitCodes];
    unsigned short seq[kDeflateLitCodes + kDeflateDistCodes];  // the run-length coded lengths: symbol | extra << 5
    unsigned cl_hist[kDeflateClCodes];
    int count[16], next[16];
};

#define DAD3D_HD __host__ __device__ inline

// length 3..258 -> its symbol, extra-bit count and extra value
DAD3D_HD void deflate_length_symbol(int len, int& sym, int& extra_bits, int& extra) {
    const int l = len - 3;
    if (len == 258) {
        sym = 285, extra_bits = 0, extra = 0;
    } else if (l < 8) {
        sym = 257 + l, extra_bits = 0, extra = 0;
    } else {
        int top = 3;
        while ((l >> (top + 1)) != 0) ++top;  // floor(log2 l), l in 8..254
        extra_bits = top - 2;
        sym = 261 + 4 * extra_bits + ((l >> extra_bits) & 3);
        extra = l & ((1 << extra_bits) - 1);
    }
}
DAD3D_HD int deflate_ll_extra_bits(int sym) { return sym < 265 || sym == 285 ? 0 : (sym - 261) >> 2; }
DAD3D_HD int deflate_dist_extra_bits(int sym) { return sym < 4 ? 0 : (sym >> 1) - 1; }
DAD3D_HD int deflate_fixed_ll_len(int sym) { return sym < 144 ? 8 : sym < 256 ? 9 : sym < 280 ? 7 : 8; }
// RFC 1951 3.2.7: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, five bits each
DAD3D_HD int deflate_cl_order(int i) {
    const unsigned long long lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 |
                                  5ull << 45 | 11ull << 50 | 4ull << 55;
    const unsigned long long hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (int)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31u);
}

// hist[n] -> len[n]: 0 for an unused symbol, 1..limit otherwise, Kraft sum 1 when two or more are used
DAD3D_HD void deflate_code_lengths(const unsigned* hist, int n, int limit, unsigned char* len, DeflateWork& w) {
    unsigned* key = w.key;
    unsigned* a = w.depth;
    int m = 0;
    for (int i = 0; i < n; ++i) {
        len[i] = 0;
        if (hist[i]) key[m++] = hist[i] << 9 | (unsigned)i;
    }
    if (m == 0) return;
    if (m == 1) {
        len[key[0] & 511u] = 1;
        return;
    }
    for (int gap = m >> 1; gap > 0; gap = gap == 2 ? 1 : (gap * 5) / 11) {  // shell sort, ascending (count, symbol)
        for (int i = gap; i < m; ++i) {
            const unsigned v = key[i];
            int j = i;
            for (; j >= gap && key[j - gap] > v; j -= gap) key[j] = key[j - gap];
            key[j] = v;
        }
    }
    for (int i = 0; i < m; ++i) a[i] = key[i] >> 9;
    // Moffat & Katajainen: a[] ascending weights -> a[i] = depth of leaf i
    a[0] += a[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < m - 1; ++next) {
        if (leaf >= m || a[root] < a[leaf]) {
            a[next] = a[root];
            a[root++] = (unsigned)next;
        } else {
            a[next] = a[leaf++];
        }
        if (leaf >= m || (root < next && a[root] < a[leaf])) {
            a[next] += a[root];
            a[root++] = (unsigned)next;
        } else {
            a[next] += a[leaf++];
        }
    }
    a[m - 2] = 0;
    for (int next = m - 3; next >= 0; --next) a[next] = a[a[next]] + 1;
    {
        int avail = 1, used = 0, depth = 0, r = m - 2, next = m - 1;
        while (avail > 0) {
            while (r >= 0 && (int)a[r] == depth) {
                ++used;
                --r;
            }
            while (avail > used) {
                a[next--] = (unsigned)depth;
                --avail;
            }
            avail = 2 * used;
            ++depth;
            used = 0;
        }
    }
    // codes per length, the deep ones clamped to the limit; Kraft sum in units of 2^-limit
    int* count = w.count;
    for (int l = 0; l < 16; ++l) count[l] = 0;
    unsigned kraft = 0;
    for (int i = 0; i < m; ++i) {
        const int d = (int)a[i] < limit ? (int)a[i] : limit;
        ++count[d];
        kraft += 1u << (limit - d);
    }
    const unsigned one = 1u << limit;
    while (kraft > one) {  // lengthen the deepest code above the limit level
        int l = limit - 1;
        while (count[l] == 0) --l;
        --count[l];
        ++count[l + 1];
        kraft -= 1u << (limit - l - 1);
    }
    while (kraft < one) {  // shorten the code that gains most without passing 1; the deepest level's gain always fits
        const unsigned room = one - kraft;
        int l = 2;
        while (l < limit && (count[l] == 0 || (1u << (limit - l)) > room)) ++l;
        --count[l];
        ++count[l - 1];
        kraft += 1u << (limit - l);
    }
    int i = 0;
    for (int l = limit; l >= 1; --l)
        for (int c = count[l]; c > 0; --c) len[key[i++] & 511u] = (unsigned char)l;
}

// canonical codes (RFC 1951 3.2.2) of len[n]
DAD3D_HD void deflate_canonical_codes(const unsigned char* len, int n, unsigned short* code, DeflateWork& w) {
    int* count = w.count;
    int* next = w.next;
    for (int l = 0; l < 16; ++l) count[l] = 0;
    for (int i = 0; i < n; ++i) ++count[len[i]];
    count[0] = 0;
    int c = 0;
    next[0] = 0;
    for (int l = 1; l < 16; ++l) {
        c = (c + count[l - 1]) << 1;
        next[l] = c;
    }
    for (int i = 0; i < n; ++i) code[i] = len[i] ? (unsigned short)next[len[i]]++ : (unsigned short)0;
}

DAD3D_HD unsigned deflate_reverse_bits(unsigned code, int len) {
    unsigned r = 0;
    for (int i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
    return r;
}

struct DeflateBitWriter {
    unsigned char* p;
    unsigned long long acc;
    int held, total;
    DAD3D_HD void put(unsigned value, int bits) {
        acc |= (unsigned long long)value << held;
        held += bits;
        total += bits;
        while (held >= 8) {
            *p++ = (unsigned char)acc;
            acc >>= 8;
            held -= 8;
        }
    }
    DAD3D_HD void flush() {
        if (held > 0) *p++ = (unsigned char)acc;
        acc = 0, held = 0;
    }
};

// the run-length form of len[0..n) in the code-length alphabet, appended to seq; returns the new token count
DAD3D_HD int deflate_run_lengths(const unsigned char* len, int n, unsigned short* seq, int at) {
    int i = 0;
    while (i < n) {
        const int v = len[i];
        int run = 1;
        while (i + run < n && len[i + run] == v) ++run;
        i += run;
        if (v == 0) {
            while (run >= 11) {
                const int r = run < 138 ? run : 138;
                seq[at++] = (unsigned short)(18 | (r - 11) << 5);
                run -= r;
            }
            if (run >= 3) {
                seq[at++] = (unsigned short)(17 | (run - 3) << 5);
                run = 0;
            }
            for (; run > 0; --run) seq[at++] = 0;
        } else {
            seq[at++] = (unsigned short)v;
            --run;
            while (run >= 3) {
                const int r = run < 6 ? run : 6;
                seq[at++] = (unsigned short)(16 | (r - 3) << 5);
                run -= r;
            }
            for (; run > 0; --run) seq[at++] = (unsigned short)v;
        }
    }
    return at;
}

// ll_hist[286] (end of block counted), d_hist[30], every entry < kDeflateMaxCount -> the block's tables, header and cost
DAD3D_HD void deflate_tables(const unsigned* ll_hist, const unsigned* d_hist, DeflateTables& t, DeflateWork& w) {
    deflate_code_lengths(ll_hist, kDeflateLitCodes, 15, t.ll_len, w);
    deflate_canonical_codes(t.ll_len, kDeflateLitCodes, t.ll_code, w);
    deflate_code_lengths(d_hist, kDeflateDistCodes, 15, t.d_len, w);
    deflate_canonical_codes(t.d_len, kDeflateDistCodes, t.d_code, w);
    int n_ll = kDeflateLitCodes, n_d = kDeflateDistCodes;
    while (n_ll > 257 && t.ll_len[n_ll - 1] == 0) --n_ll;
    while (n_d > 1 && t.d_len[n_d - 1] == 0) --n_d;
    int n_seq = deflate_run_lengths(t.ll_len, n_ll, w.seq, 0);  // each alphabet on its own, as zlib writes them
    n_seq = deflate_run_lengths(t.d_len, n_d, w.seq, n_seq);
    for (int i = 0; i < kDeflateClCodes; ++i) w.cl_hist[i] = 0;
    for (int i = 0; i < n_seq; ++i) ++w.cl_hist[w.seq[i] & 31];
    deflate_code_lengths(w.cl_hist, kDeflateClCodes, 7, t.cl_len, w);
    deflate_canonical_codes(t.cl_len, kDeflateClCodes, t.cl_code, w);
    int n_cl = kDeflateClCodes;
    while (n_cl > 4 && t.cl_len[deflate_cl_order(n_cl - 1)] == 0) --n_cl;

    DeflateBitWriter bw{t.header, 0ull, 0, 0};
    bw.put(0u, 1);  // BFINAL
    bw.put(2u, 2);  // BTYPE = dynamic
    bw.put((unsigned)(n_ll - 257), 5);
    bw.put((unsigned)(n_d - 1), 5);
    bw.put((unsigned)(n_cl - 4), 4);
    for (int i = 0; i < n_cl; ++i) bw.put(t.cl_len[deflate_cl_order(i)], 3);
    for (int i = 0; i < n_seq; ++i) {
        const int sym = w.seq[i] & 31, extra = w.seq[i] >> 5;
        bw.put(deflate_reverse_bits(t.cl_code[sym], t.cl_len[sym]), t.cl_len[sym]);
        if (sym == 16) bw.put((unsigned)extra, 2);
        if (sym == 17) bw.put((unsigned)extra, 3);
        if (sym == 18) bw.put((unsigned)extra, 7);
    }
    bw.flush();
    t.header_bits = bw.total;
    unsigned dyn = (unsigned)bw.total, fixed = 3;
    for (int s = 0; s < kDeflateLitCodes; ++s) {
        const unsigned extra = (unsigned)deflate_ll_extra_bits(s);
        dyn += ll_hist[s] * (t.ll_len[s] + extra);
        fixed += ll_hist[s] * ((unsigned)deflate_fixed_ll_len(s) + extra);
    }
    for (int s = 0; s < kDeflateDistCodes; ++s) {
        const unsigned extra = (unsigned)deflate_dist_extra_bits(s);
        dyn += d_hist[s] * (t.d_len[s] + extra);
        fixed += d_hist[s] * (5u + extra);
    }
    t.dynamic_bits = dyn;
    t.fixed_bits = fixed;
}

}  // namespace dad3d
