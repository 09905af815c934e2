// PNG files of a batch of uint8 images, and zlib streams of a batch of byte rows, made on the device.
//
// A file is the signature, IHDR, an IDAT that holds the zlib header 78 01, one IDAT per segment of kSeg bytes of the filtered
// stream, an IDAT with 03 00 (the empty final fixed block) + Adler-32, IEND. A segment's payload is one complete deflate block
// and the empty stored block 00 00 FF FF behind it, so it ends on a byte, depends on no neighbour and owns its chunk CRC.
//
// Three launches:
//   png_filter_kernel       one workgroup per row: the five filters' sums of |signed byte|, the smallest (lowest type on a tie),
//                           type byte + filtered row into the scratch stream
//   deflate_segment_kernel  one workgroup per (segment, item): match lengths at distances 1 and `dist2` from a reverse segmented
//                           scan of x[i] == x[i - d] held as 32-bit masks; the greedy parse's positions by pointer jumping in LDS;
//                           histograms by LDS atomics; one lane builds the tables (deflate_tables.hpp); the cheapest of stored /
//                           fixed / dynamic is packed into an LDS image at bit offsets from a prefix sum and leaves in 16-byte
//                           stores, with the segment's Adler sums and the CRC-32 of its payload
//   png_assemble_kernel     one workgroup per (segment, item): offsets from the payload lengths, chunk words around the payload,
//                           copied to its unaligned place through an LDS image (text_tile.hpp); the first workgroup of an item
//                           combines the Adler sums and writes the head, the trailer, the length and the flag
// The sums, the xor and the scan over a workgroup are those of collectives.hpp; Paeth and the Adler modulus those of png_common.hpp.
#include "common.hpp"
#include "crc32.hpp"
#include "deflate_tables.hpp"
#include "png_common.hpp"
#include "text_tile.hpp"

namespace dad3d {
namespace {

constexpr int kSeg = DAD3D_PNG_SEGMENT_BYTES;
constexpr int kLanes = 256;
constexpr int kPerLane = kSeg / kLanes;  // 32: a lane's positions are one 32-bit mask
constexpr int kSlot = kSeg + 16;         // a segment's payload in scratch: stored block (5 + n) + the empty stored block (5) at most
static_assert(kPerLane == 32 && kLanes == kTextTile, "the match masks are one word per lane");

struct SegRecord {
    int payload_bytes;
    unsigned adler_a, adler_b;  // sum of x, sum of (n - i) x[i], both mod 65521
    unsigned crc;               // CRC-32 of the payload
    int flag, kind, pad0, pad1;
};
static_assert(sizeof(SegRecord) == 32, "scratch layout");

// ---------------------------------------------------------------------------------------------------------------------------
// filter
// ---------------------------------------------------------------------------------------------------------------------------
__device__ inline unsigned png_cost(int v) { return v < 128 ? (unsigned)v : (unsigned)(256 - v); }
__device__ inline int png_filtered(int type, int x, int a, int b, int c) {
    const int pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : png_paeth(a, b, c);
    return (x - pred) & 255;
}

__global__ __launch_bounds__(kLanes) void png_filter_kernel(const unsigned char* __restrict__ images, int h, int row_bytes, int c,
                                                            unsigned char* __restrict__ stream, size_t stream_stride) {
    __shared__ unsigned long long red[kTextWaves];
    __shared__ int chosen;
    const int y = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const unsigned char* cur = images + ((size_t)b * h + y) * row_bytes;
    const unsigned char* up = y ? cur - row_bytes : nullptr;
    unsigned long long sum[5] = {0, 0, 0, 0, 0};
    for (int i = tid; i < row_bytes; i += kLanes) {
        const int x = cur[i], a = i >= c ? cur[i - c] : 0, bb = up ? up[i] : 0, cc = (up && i >= c) ? up[i - c] : 0;
#pragma unroll
        for (int t = 0; t < 5; ++t) sum[t] += png_cost(png_filtered(t, x, a, bb, cc));
    }
    unsigned long long best = 0;
    int type = 0;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        const unsigned long long s = block_sum<kTextWaves>(sum[t], red);
        if (t == 0 || s < best) best = s, type = t;  // a tie keeps the lower type
    }
    if (tid == 0) chosen = type;
    __syncthreads();
    type = chosen;
    unsigned char* dst = stream + (size_t)b * stream_stride + (size_t)y * (row_bytes + 1);
    if (tid == 0) dst[0] = (unsigned char)type;
    for (int i = tid; i < row_bytes; i += kLanes) {
        const int x = cur[i], a = i >= c ? cur[i - c] : 0, bb = up ? up[i] : 0, cc = (up && i >= c) ? up[i - c] : 0;
        dst[1 + i] = (unsigned char)png_filtered(type, x, a, bb, cc);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// deflate of one segment
// ---------------------------------------------------------------------------------------------------------------------------
// bit k of the result: byte k of `cur` equals the byte `dist` (1..4) places in front of it; prev = the dword in front of cur
__device__ inline unsigned equal_bytes(unsigned cur, unsigned prev, int dist) {
    const unsigned shifted = (unsigned)((((unsigned long long)cur << 32) | prev) >> (32 - 8 * dist));
    const unsigned x = cur ^ shifted;
    return ((x & 0xffu) == 0) | (((x & 0xff00u) == 0) << 1) | (((x & 0xff0000u) == 0) << 2) | (((x & 0xff000000u) == 0) << 3);
}
__device__ inline int run_of_ones(unsigned m) { return m == 0xffffffffu ? 32 : __ffs((int)~m) - 1; }

// OR `bits` (up to 35 of them) into the LDS image at bit offset `at`
__device__ inline void put_bits(unsigned* image, int at, unsigned long long bits) {
    const int word = at >> 5, sh = at & 31;
    const unsigned w0 = (unsigned)(bits << sh);
    const unsigned long long rest = (bits >> 1) >> (31 - sh);
    if (w0) atomicOr(&image[word], w0);
    if ((unsigned)rest) atomicOr(&image[word + 1], (unsigned)rest);
    if ((unsigned)(rest >> 32)) atomicOr(&image[word + 2], (unsigned)(rest >> 32));
}

__global__ __launch_bounds__(kLanes) void deflate_segment_kernel(const unsigned char* __restrict__ data, size_t data_stride, long long n_total,
                                                                 int dist2, int nseg, unsigned char* __restrict__ payload,
                                                                 SegRecord* __restrict__ records) {
    __shared__ uint4 xs_v[(kSeg + 16) / 16];     // byte 16 + i = x[base + i]; bytes 12..15 = the four bytes in front of the segment
    __shared__ unsigned short choice[kSeg];      // 0: literal; else match length | (second distance ? 0x8000 : 0)
    __shared__ uint4 shared_v[kSeg * 2 / 16];    // the jump table of the parse, then the payload image
    __shared__ unsigned char vis[kSeg];          // 1: the greedy parse starts a token here
    __shared__ unsigned ll_hist[kDeflateLitCodes], d_hist[kDeflateDistCodes];
    __shared__ DeflateTables tab;
    __shared__ DeflateWork work;
    __shared__ int scan1[kLanes], scan2[kLanes], red[kTextWaves];
    __shared__ unsigned long long red64[kTextWaves];

    const int seg = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const long long base = (long long)seg * kSeg;
    const int n = (int)(n_total - base < kSeg ? n_total - base : kSeg);
    const unsigned char* src = data + (size_t)b * data_stride + base;
    unsigned char* xs = reinterpret_cast<unsigned char*>(xs_v);
    unsigned* xw = reinterpret_cast<unsigned*>(xs_v);
    unsigned short* jump = reinterpret_cast<unsigned short*>(shared_v);
    unsigned* image = reinterpret_cast<unsigned*>(shared_v);
    unsigned char* image_bytes = reinterpret_cast<unsigned char*>(shared_v);

    for (int i = tid; i < (kSeg + 16) / 4; i += kLanes) xw[i] = 0;
    for (int i = tid; i < kDeflateLitCodes; i += kLanes) ll_hist[i] = i == 256 ? 1u : 0u;  // the end of block
    if (tid < kDeflateDistCodes) d_hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += kLanes) xs[16 + i] = src[i];
    if (tid < 4 && base > 0) xs[12 + tid] = src[tid - 4];
    __syncthreads();

    // ---- match lengths: masks of x[i] == x[i - d], runs of ones towards higher positions ----
    unsigned m1 = 0, m2 = 0;
    {
        unsigned prev = xw[3 + tid * 8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const unsigned cur = xw[4 + tid * 8 + q];
            m1 |= equal_bytes(cur, prev, 1) << (4 * q);
            m2 |= equal_bytes(cur, prev, dist2) << (4 * q);
            prev = cur;
        }
        const int left = n - tid * kPerLane;  // this lane's positions inside the segment
        const unsigned inside = left >= 32 ? 0xffffffffu : left <= 0 ? 0u : (1u << left) - 1u;
        m1 &= inside, m2 &= inside;
        if (base == 0 && tid == 0) m1 &= ~1u, m2 &= ~((1u << dist2) - 1u);  // nothing in front of the stream
    }
    // R[t] = run at the first position of lane t = head[t] + (all ones ? R[t + 1] : 0): a reverse segmented scan, bit 30 = all ones
    scan1[tid] = run_of_ones(m1) | (m1 == 0xffffffffu ? 1 << 30 : 0);
    scan2[tid] = run_of_ones(m2) | (m2 == 0xffffffffu ? 1 << 30 : 0);
    __syncthreads();
    for (int off = 1; off < kLanes; off <<= 1) {
        int a1 = scan1[tid], a2 = scan2[tid];
        const int b1 = tid + off < kLanes ? scan1[tid + off] : 0, b2 = tid + off < kLanes ? scan2[tid + off] : 0;
        if (a1 >> 30) a1 = ((a1 & 0xffff) + (b1 & 0xffff)) | (b1 & (1 << 30));
        if (a2 >> 30) a2 = ((a2 & 0xffff) + (b2 & 0xffff)) | (b2 & (1 << 30));
        __syncthreads();
        scan1[tid] = a1, scan2[tid] = a2;
        __syncthreads();
    }
    {
        const int carry1 = tid + 1 < kLanes ? scan1[tid + 1] & 0xffff : 0, carry2 = tid + 1 < kLanes ? scan2[tid + 1] & 0xffff : 0;
#pragma unroll 4
        for (int k = 0; k < kPerLane; ++k) {
            const int p = tid * kPerLane + k;
            if (p >= n) break;
            int l1 = run_of_ones(m1 >> k), l2 = run_of_ones(m2 >> k);  // the shifted-in zeros end a run at the lane's last position
            if (l1 == kPerLane - k) l1 += carry1;
            if (l2 == kPerLane - k) l2 += carry2;
            l1 = min(l1, 258), l2 = min(l2, 258);
            const int len = l1 >= l2 ? l1 : l2;  // the longer; on a tie distance 1
            const bool match = len >= 3;
            choice[p] = match ? (unsigned short)(len | (l1 >= l2 ? 0 : 0x8000)) : (unsigned short)0;
            jump[p] = (unsigned short)(p + (match ? len : 1));
        }
    }
    for (int i = tid; i < kSeg; i += kLanes) vis[i] = i == 0;
    __syncthreads();

    // ---- the positions the greedy parse visits: pointer jumping, jump <- jump o jump, marks follow the doubled steps ----
    for (int span = 1; span < n; span <<= 1) {
        unsigned short far[kPerLane];
#pragma unroll
        for (int k = 0; k < kPerLane; ++k) {
            const int i = k * kLanes + tid;
            far[k] = (unsigned short)n;
            if (i < n) {
                const int j = jump[i];
                if (j < n) {
                    if (vis[i]) vis[j] = 1;
                    far[k] = jump[j];
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kPerLane; ++k) {
            const int i = k * kLanes + tid;
            if (i < n) jump[i] = far[k];
        }
        __syncthreads();
    }

    // ---- histograms of the parse ----
#pragma unroll 1  // unrolled, the 32 bounds masks stay live in scalar registers and spill
    for (int k = 0; k < kPerLane; ++k) {
        const int i = k * kLanes + tid;
        if (i < n && vis[i]) {
            const int ch = choice[i];
            if (ch == 0) {
                atomicAdd(&ll_hist[xs[16 + i]], 1u);
            } else {
                int sym, eb, extra;
                deflate_length_symbol(ch & 0x7fff, sym, eb, extra);
                atomicAdd(&ll_hist[sym], 1u);
                atomicAdd(&d_hist[((ch & 0x8000) ? dist2 : 1) - 1], 1u);
            }
        }
    }
    // the payload image takes the jump table's place
    __syncthreads();
    for (int i = tid; i < kSeg * 2 / 4; i += kLanes) image[i] = 0;
    if (tid == 0) deflate_tables(ll_hist, d_hist, tab, work);
    __syncthreads();

    // ---- stored, fixed or dynamic: the fewest bits; a tie goes to the simpler block ----
    const unsigned stored_bits = 8u * (5u + (unsigned)n);
    int kind = 0;
    unsigned body_bits = stored_bits;
    if (tab.fixed_bits < body_bits) kind = 1, body_bits = tab.fixed_bits;
    if (tab.dynamic_bits < body_bits) kind = 2, body_bits = tab.dynamic_bits;
    const int header_bits = kind == 2 ? tab.header_bits : 3;
    int flag = 0, end_bits;
    __syncthreads();
    if (kind == 0) {
        if (tid == 0) {
            image_bytes[1] = (unsigned char)(n & 255), image_bytes[2] = (unsigned char)(n >> 8);
            image_bytes[3] = (unsigned char)(~n & 255), image_bytes[4] = (unsigned char)((~n >> 8) & 255);
        }
        for (int i = tid; i < n; i += kLanes) image_bytes[5 + i] = xs[16 + i];
        end_bits = (int)stored_bits;
    } else {
        // the codes as they are packed: low bit first
        for (int s = tid; s < kDeflateLitCodes + kDeflateDistCodes; s += kLanes) {
            if (s < kDeflateLitCodes) {
                int len = tab.ll_len[s];
                unsigned code = tab.ll_code[s];
                if (kind == 1) {
                    len = deflate_fixed_ll_len(s);
                    code = s < 144 ? 0x30u + s : s < 256 ? 0x190u + (s - 144) : s < 280 ? (unsigned)(s - 256) : 0xc0u + (s - 280);
                    tab.ll_len[s] = (unsigned char)len;
                }
                tab.ll_code[s] = (unsigned short)(len ? __brev(code) >> (32 - len) : 0u);
            } else {
                const int d = s - kDeflateLitCodes;
                int len = tab.d_len[d];
                unsigned code = tab.d_code[d];
                if (kind == 1) len = 5, code = (unsigned)d, tab.d_len[d] = 5;
                tab.d_code[d] = (unsigned short)(len ? __brev(code) >> (32 - len) : 0u);
            }
        }
        if (kind == 1 && tid == 0) tab.header[0] = 2;  // BFINAL = 0, BTYPE = 01
        __syncthreads();
        int bits = 0;
#pragma unroll 1
        for (int k = 0; k < kPerLane; ++k) {
            const int p = tid * kPerLane + k;
            if (p < n && vis[p]) {
                const int ch = choice[p];
                if (ch == 0) {
                    bits += tab.ll_len[xs[16 + p]];
                } else {
                    int sym, eb, extra;
                    deflate_length_symbol(ch & 0x7fff, sym, eb, extra);
                    bits += tab.ll_len[sym] + eb + tab.d_len[((ch & 0x8000) ? dist2 : 1) - 1];
                }
            }
        }
        int token_bits;
        int at = header_bits + block_exclusive_scan<kTextWaves>(bits, red, token_bits);
        for (int i = tid; i * 8 < header_bits; i += kLanes) atomicOr(&image[i >> 2], (unsigned)tab.header[i] << (8 * (i & 3)));
#pragma unroll 1
        for (int k = 0; k < kPerLane; ++k) {
            const int p = tid * kPerLane + k;
            if (p < n && vis[p]) {
                const int ch = choice[p];
                if (ch == 0) {
                    const int x = xs[16 + p];
                    put_bits(image, at, tab.ll_code[x]);
                    at += tab.ll_len[x];
                } else {
                    int sym, eb, extra;
                    deflate_length_symbol(ch & 0x7fff, sym, eb, extra);
                    const int d = ((ch & 0x8000) ? dist2 : 1) - 1, ll = tab.ll_len[sym];
                    const unsigned long long v = (unsigned long long)tab.ll_code[sym] | (unsigned long long)extra << ll |
                                                 (unsigned long long)tab.d_code[d] << (ll + eb);
                    put_bits(image, at, v);
                    at += ll + eb + tab.d_len[d];
                }
            }
        }
        end_bits = header_bits + token_bits + tab.ll_len[256];
        if (tid == 0) put_bits(image, header_bits + token_bits, tab.ll_code[256]);
        if (end_bits != (int)body_bits) flag = DAD3D_PNG_FLAG_INTERNAL;  // the cost model and the packer disagree: leave the item to the host
        end_bits = min(end_bits, (int)stored_bits);  // whatever happened, the payload stays inside its slot
    }
    __syncthreads();
    // the empty stored block: three zero bits, zeros to the byte, 00 00 FF FF
    const int tail = (end_bits + 3 + 7) >> 3;
    const int payload_bytes = tail + 4;
    if (tid == 0) image_bytes[tail + 2] = 0xff, image_bytes[tail + 3] = 0xff;

    // ---- Adler sums of the input, CRC-32 of the payload ----
    unsigned a = 0, bsum = 0;
#pragma unroll 2
    for (int k = 0; k < kPerLane; ++k) {
        const int i = k * kLanes + tid;
        if (i < n) {
            const unsigned x = xs[16 + i];
            a += x;
            bsum += (unsigned)(n - i) * x;  // 32 terms below 8192 * 255
        }
    }
    const unsigned adler_a = (unsigned)(block_sum<kTextWaves>((unsigned long long)a, red64) % kAdlerMod);
    const unsigned adler_b = (unsigned)(block_sum<kTextWaves>((unsigned long long)(bsum % kAdlerMod), red64) % kAdlerMod);
    __syncthreads();
    const int piece = (payload_bytes + kLanes - 1) / kLanes;
    const int first = min(tid * piece, payload_bytes), last = min(first + piece, payload_bytes);
    unsigned crc = 0;
    if (last > first) {
        crc = 0xffffffffu;
        for (int i = first; i < last; ++i) crc = crc_bitwise(crc, image_bytes[i]);
        crc = gf_mul(gf_x_pow_bytes((unsigned)(payload_bytes - last)), ~crc);
    }
    crc = (unsigned)block_xor<kTextWaves>((int)crc, red);

    uint4* dst = reinterpret_cast<uint4*>(payload + ((size_t)b * nseg + seg) * kSlot);
    for (int i = tid; i * 16 < payload_bytes; i += kLanes) dst[i] = shared_v[i];
    if (tid == 0) records[(size_t)b * nseg + seg] = SegRecord{payload_bytes, adler_a, adler_b, crc, flag, kind, 0, 0};
}

// ---------------------------------------------------------------------------------------------------------------------------
// assemble
// ---------------------------------------------------------------------------------------------------------------------------
__device__ inline void put_be32(unsigned char* p, unsigned v) {
    p[0] = (unsigned char)(v >> 24), p[1] = (unsigned char)(v >> 16), p[2] = (unsigned char)(v >> 8), p[3] = (unsigned char)v;
}
constexpr unsigned kCrcIdat = 0x35af061eu;  // CRC-32 of "IDAT"

__global__ __launch_bounds__(kLanes) void png_assemble_kernel(const unsigned char* __restrict__ payload, const SegRecord* __restrict__ records,
                                                              int nseg, long long n_total, int png, int h, int w, int c,
                                                              unsigned char* __restrict__ out, size_t out_stride,
                                                              long long* __restrict__ lengths, int* __restrict__ flags) {
    __shared__ uint4 stage[(kSlot + 12 + 15 + 15) / 16];
    __shared__ unsigned long long red64[kTextWaves];
    const int seg = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const SegRecord* rec = records + (size_t)b * nseg;

    unsigned long long before = 0, total = 0, s1 = 0, s2 = 0, why = 0;
    for (int j = tid; j < nseg; j += kLanes) {
        const SegRecord r = rec[j];
        total += (unsigned)r.payload_bytes;
        before += j < seg ? (unsigned)r.payload_bytes : 0u;
        why |= (unsigned)r.flag;
        if (seg == 0) {
            const long long end = (long long)(j + 1) * kSeg < n_total ? (long long)(j + 1) * kSeg : n_total;
            s1 += r.adler_a;
            s2 += r.adler_b + (unsigned long long)r.adler_a * (unsigned long long)((n_total - end) % kAdlerMod);  // 256 lanes' terms below 2^33 each
        }
    }
    before = block_sum<kTextWaves>(before, red64);
    total = block_sum<kTextWaves>(total, red64);
    why = block_sum<kTextWaves>(why ? 1ull : 0ull, red64);  // any segment's flag
    const int head = png ? 47 : 2, wrap = png ? 12 : 0;
    unsigned char* dst = out + (size_t)b * out_stride;

    if (seg == 0) {
        s1 = block_sum<kTextWaves>(s1 % kAdlerMod, red64);
        s2 = block_sum<kTextWaves>(s2 % kAdlerMod, red64);
        if (tid == 0) {
            const unsigned adler1 = (unsigned)((1 + s1) % kAdlerMod);
            const unsigned adler2 = (unsigned)(((unsigned long long)(n_total % kAdlerMod) + s2) % kAdlerMod);
            unsigned char* p = dst;
            if (png) {
                put_be32(p, 0x89504e47u);  // the signature
                put_be32(p + 4, 0x0d0a1a0au);
                put_be32(p + 8, 13);
                p[12] = 'I', p[13] = 'H', p[14] = 'D', p[15] = 'R';
                put_be32(p + 16, (unsigned)w);
                put_be32(p + 20, (unsigned)h);
                p[24] = 8;
                p[25] = (unsigned char)(c == 1 ? 0 : c == 2 ? 4 : c == 3 ? 2 : 6);
                p[26] = 0, p[27] = 0, p[28] = 0;
                unsigned crc = 0xffffffffu;
                for (int i = 12; i < 29; ++i) crc = crc_bitwise(crc, p[i]);
                put_be32(p + 29, ~crc);
                put_be32(p + 33, 2);
                p[37] = 'I', p[38] = 'D', p[39] = 'A', p[40] = 'T', p[41] = 0x78, p[42] = 0x01;
                put_be32(p + 43, 0xec1a7ed2u);  // CRC-32 of "IDAT" 78 01
            } else {
                p[0] = 0x78, p[1] = 0x01;
            }
            p = dst + head + total + (unsigned long long)nseg * wrap;
            unsigned char* t = p;
            if (png) {
                put_be32(p, 6);
                p[4] = 'I', p[5] = 'D', p[6] = 'A', p[7] = 'T';
                t = p + 8;
            }
            t[0] = 0x03, t[1] = 0x00;
            put_be32(t + 2, adler2 << 16 | adler1);
            unsigned long long length = head + total + (unsigned long long)nseg * wrap + 6;
            if (png) {
                unsigned crc = ~kCrcIdat;
                for (int i = 0; i < 6; ++i) crc = crc_bitwise(crc, t[i]);
                put_be32(t + 6, ~crc);
                put_be32(t + 10, 0);
                t[14] = 'I', t[15] = 'E', t[16] = 'N', t[17] = 'D';
                put_be32(t + 18, 0xae426082u);
                length += 12 + 12;  // the trailer chunk's words, IEND
            }
            lengths[b] = why ? 0 : (long long)length;
            flags[b] = why ? DAD3D_PNG_FLAG_INTERNAL : 0;
        }
    }

    // this segment: [length, "IDAT"] payload [CRC], through an image that starts at (offset mod 16)
    const SegRecord mine = rec[seg];
    const unsigned long long offset = head + before + (unsigned long long)seg * wrap;
    const int lead = (int)(offset & 15), len = mine.payload_bytes;
    unsigned char* s = reinterpret_cast<unsigned char*>(stage);
    const unsigned char* from = payload + ((size_t)b * nseg + seg) * kSlot;
    const int body = lead + (png ? 8 : 0);
    for (int i = tid; i < len; i += kLanes) s[body + i] = from[i];
    if (png && tid == 0) {
        put_be32(s + lead, (unsigned)len);
        s[lead + 4] = 'I', s[lead + 5] = 'D', s[lead + 6] = 'A', s[lead + 7] = 'T';
        put_be32(s + body + len, crc_append(kCrcIdat, mine.crc, (unsigned)len));
    }
    __syncthreads();
    copy_tile_out(stage, dst + (offset - lead), lead, lead + len + wrap);
}

}  // namespace

int png_segments(long long n) { return n <= 0 ? 1 : (int)((n + kSeg - 1) / kSeg); }
long long png_stream_bytes(int h, int w, int c) { return (long long)h * (1 + (long long)w * c); }
size_t zlib_max_bytes(long long n) { return 2 + (size_t)n + (size_t)png_segments(n) * 10 + 6; }
size_t png_max_bytes(int h, int w, int c) {
    const long long n = png_stream_bytes(h, w, c);
    return 47 + (size_t)n + (size_t)png_segments(n) * 22 + 18 + 12;
}
static size_t round16(size_t v) { return (v + 15) / 16 * 16; }
size_t zlib_scratch_bytes(int batch, long long n) { return (size_t)batch * png_segments(n) * (kSlot + sizeof(SegRecord)); }
size_t png_scratch_bytes(int batch, int h, int w, int c) {
    const long long n = png_stream_bytes(h, w, c);
    return (size_t)batch * round16((size_t)n) + zlib_scratch_bytes(batch, n);
}

dad3d_status launch_deflate(const DeflateArgs& a, hipStream_t s) {
    const long long n = a.png ? png_stream_bytes(a.h, a.w, a.c) : a.n;
    const int nseg = png_segments(n);
    unsigned char* scratch = static_cast<unsigned char*>(a.scratch);
    const unsigned char* data = a.data;
    size_t data_stride = (size_t)n;
    if (a.png) {
        const size_t stream_stride = round16((size_t)n);
        hipLaunchKernelGGL(png_filter_kernel, dim3(a.h, a.batch), dim3(kLanes), 0, s, a.data, a.h, a.w * a.c, a.c, scratch, stream_stride);
        DAD3D_HIP_TRY(hipGetLastError());
        data = scratch, data_stride = stream_stride;
        scratch += (size_t)a.batch * stream_stride;
    }
    unsigned char* payload = scratch;
    SegRecord* records = reinterpret_cast<SegRecord*>(scratch + (size_t)a.batch * nseg * kSlot);
    const dim3 grid(nseg, a.batch);
    hipLaunchKernelGGL(deflate_segment_kernel, grid, dim3(kLanes), 0, s, data, data_stride, n, a.png ? a.c : DAD3D_ZLIB_SECOND_DISTANCE, nseg,
                       payload, records);
    DAD3D_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(png_assemble_kernel, grid, dim3(kLanes), 0, s, payload, records, nseg, n, a.png, a.h, a.w, a.c, a.out, a.out_stride,
                       reinterpret_cast<long long*>(a.lengths), a.flags);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

dad3d_status deflate_tables_host(const unsigned* ll_hist, const unsigned* d_hist, unsigned char* ll_len, unsigned char* d_len, unsigned char* cl_len,
                                 unsigned short* ll_code, unsigned short* d_code, unsigned short* cl_code, unsigned char* header, int* header_bits,
                                 unsigned* dynamic_bits, unsigned* fixed_bits) {
    DeflateTables t;
    DeflateWork w;
    deflate_tables(ll_hist, d_hist, t, w);
    __builtin_memcpy(ll_len, t.ll_len, sizeof t.ll_len);
    __builtin_memcpy(d_len, t.d_len, sizeof t.d_len);
    __builtin_memcpy(cl_len, t.cl_len, sizeof t.cl_len);
    __builtin_memcpy(ll_code, t.ll_code, sizeof t.ll_code);
    __builtin_memcpy(d_code, t.d_code, sizeof t.d_code);
    __builtin_memcpy(cl_code, t.cl_code, sizeof t.cl_code);
    __builtin_memset(header, 0, kDeflateHeaderBytes);
    __builtin_memcpy(header, t.header, (size_t)(t.header_bits + 7) / 8);
    *header_bits = t.header_bits, *dynamic_bits = t.dynamic_bits, *fixed_bits = t.fixed_bits;
    return DAD3D_OK;
}

}  // namespace dad3d
