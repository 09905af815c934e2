// Baseline JPEG files of a batch of uint8 images, made on the device, byte-equal to PIL (libjpeg-turbo).
//
// Two launches for a batch of images of one shape:
//   jpeg_fdct_kernel   one lane per block of the scan, dummy blocks included (jpeg_fdct.hpp): colour conversion, edge replication and
//                      the box filter while the 64 samples are gathered, both DCT passes and the quantiser in registers, the
//                      coefficients in zigzag order as int16 and the AC half of the block's bit count into scratch. One further
//                      workgroup per image writes the header (jpeg_huff_encode.hpp), a lane a share of each table: it depends on
//                      the arguments alone.
//   jpeg_pack_kernel   one workgroup per image walks the scan in chunks of 256 blocks, one lane per block. A chunk: the block's bits
//                      (the AC half + the DC difference against the component's previous block, 0 at the start of an interval); an
//                      exclusive scan of the bits; a second one, over the bytes of the intervals that end in the chunk (their bits
//                      rounded up to a byte + the two bytes of RSTn), so that a block's bit offset in the chunk is 8 x its interval's
//                      byte + its bits behind the interval's start; the codes ORed into an LDS image at those offsets, the padding of
//                      1-bits and the marker by the interval's last lane; then byte stuffing: every lane counts the FF of its piece of
//                      the image, a third scan places the pieces, and the bytes leave for the file. The bits of an unfinished byte and
//                      the file offset are carried to the next chunk. The last lane writes EOI, the length and the flag.
// The interval's byte is known from the block index alone (intervals are whole MCUs, MCUs are per_mcu blocks), so no lane searches.
// An image whose blocks cannot be coded by baseline's tables, or whose file would pass its row, is flagged and left to the host.
#include "collectives.hpp"
#include "common.hpp"
#include "jpeg_huff_encode.hpp"

namespace dad3d {
namespace {

constexpr int kFdctLanes = 64;
constexpr int kLanes = 256, kWaves = kLanes / 64;
constexpr int kChunk = kLanes;  // blocks per chunk
static_assert(kLanes == kJpegAcLutWords, "a lane copies one word of each AC table");
// the image of a chunk: the carried byte, every block at its worst, a byte of padding and a marker behind every block, one word of slack
constexpr int kImageBytes = (1 + kChunk * ((kJpegEncMaxBlockBits + 7) / 8 + 3) + 4 + 15) / 16 * 16;
constexpr int kImageWords = kImageBytes / 4;
constexpr int kMarkWords = (kImageBytes + 31) / 32;
static_assert(kImageBytes + kMarkWords * 4 + 2 * kJpegAcLutWords * 4 + 1536 <= 65536, "the image, its marker bits, the AC tables and the scans' words fit one workgroup's LDS");

struct BlockMeta {
    unsigned short ac_bits, last;
};

__global__ __launch_bounds__(kFdctLanes) void jpeg_fdct_kernel(const unsigned char* __restrict__ images, JpegEncGeom g, int nblocks, int chunks,
                                                               short* __restrict__ coefs, BlockMeta* __restrict__ meta,
                                                               unsigned char* __restrict__ out, size_t out_stride) {
    const int b = blockIdx.y;
    if ((int)blockIdx.x == chunks) {  // the header's workgroup
        jpeg_enc_write_header(g, out + (size_t)b * out_stride, threadIdx.x, kFdctLanes);
        return;
    }
    const int t = blockIdx.x * kFdctLanes + threadIdx.x;
    if (t >= nblocks) return;
    const JpegEncBlock where = jpeg_enc_locate(g, t);
    int d[64];
    jpeg_enc_samples(images + (size_t)b * g.h * g.w * g.c, g, where, d);
    short zz[64];
    jpeg_fdct_quantise(d, where.comp ? 1 : 0, g.scale, where.dummy, zz);
    int bits, last;
    jpeg_enc_ac_stats(zz, where.comp ? 1 : 0, bits, last);
    const size_t at = (size_t)b * nblocks + t;
    uint4* dst = reinterpret_cast<uint4*>(coefs + at * 64);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        uint4 v;
        v.x = (unsigned short)zz[8 * i] | (unsigned)(unsigned short)zz[8 * i + 1] << 16;
        v.y = (unsigned short)zz[8 * i + 2] | (unsigned)(unsigned short)zz[8 * i + 3] << 16;
        v.z = (unsigned short)zz[8 * i + 4] | (unsigned)(unsigned short)zz[8 * i + 5] << 16;
        v.w = (unsigned short)zz[8 * i + 6] | (unsigned)(unsigned short)zz[8 * i + 7] << 16;
        dst[i] = v;
    }
    meta[at] = BlockMeta{(unsigned short)bits, (unsigned short)last};
}

// ORs `count` bits (<= 27), most significant first, into the image at bit `at`; a word holds its first bit on top
struct ImagePut {
    unsigned* image;
    int at;
    __device__ void operator()(unsigned bits, int count) {
        const int word = at >> 5, sh = at & 31;
        const unsigned long long v = (unsigned long long)bits << (64 - sh - count);
        if ((unsigned)(v >> 32)) atomicOr(&image[word], (unsigned)(v >> 32));
        if ((unsigned)v) atomicOr(&image[word + 1], (unsigned)v);
        at += count;
    }
};
__device__ inline unsigned image_byte(const unsigned* image, int i) { return image[i >> 2] >> (24 - 8 * (i & 3)) & 255u; }

__global__ __launch_bounds__(kLanes) void jpeg_pack_kernel(JpegEncGeom g, int nblocks, const short* __restrict__ coefs, const BlockMeta* __restrict__ meta,
                                                           unsigned char* __restrict__ out, size_t out_stride, long long* __restrict__ lengths,
                                                           int* __restrict__ flags) {
    __shared__ unsigned image[kImageWords];
    __shared__ unsigned mark[kMarkWords];  // bit i: byte i of the image is the FF of a marker, not entropy data
    __shared__ int starts[kChunk];         // the first scan, for the lane that needs the value at its interval's first block
    __shared__ int red[kWaves];
    __shared__ int chunk_end, chunk_bad;
    __shared__ unsigned ac_lut[2][kJpegAcLutWords];  // code << 8 | length per symbol, luma and chroma

    const int b = blockIdx.x, tid = threadIdx.x;
    ac_lut[0][tid] = jpeg_ac_lut(0)[tid], ac_lut[1][tid] = jpeg_ac_lut(1)[tid];  // kLanes == kJpegAcLutWords; the loop's first barrier orders it
    const short* zz_all = coefs + (size_t)b * nblocks * 64;
    const BlockMeta* m_all = meta + (size_t)b * nblocks;
    unsigned char* file = out + (size_t)b * out_stride;
    const int per_interval = g.interval ? g.interval * g.per_mcu : 0;  // blocks; interval <= 65535 and per_mcu <= 6
    const int luma = g.c == 1 ? 1 : g.hs * g.vs;

    size_t pos = (size_t)jpeg_enc_header_bytes(g.c, g.interval);  // bytes of the file so far
    unsigned carry = 0;                                            // the bits of an unfinished byte, on top of a byte
    int carry_bits = 0, flag = 0;

    for (int base = 0; base < nblocks && !flag; base += kChunk) {
        const int i = base + tid;
        const bool live = i < nblocks;
        // ---- this block's bits ----
        int bits = 0, last = 0, pred = 0, chroma = 0, bad = 0;
        const short* zz = zz_all + (size_t)(live ? i : 0) * 64;
        if (live) {
            const BlockMeta m = m_all[i];
            const int mcu = i / g.per_mcu, j = i - mcu * g.per_mcu;
            const int comp = j < luma ? 0 : j - luma + 1;
            chroma = comp ? 1 : 0;
            // the component's previous block: the one in front inside the MCU's luma, else the same place (the luma's last) an MCU back
            const bool fresh = j == 0 || comp != 0;  // the first block of its component in this MCU
            if (!fresh)
                pred = zz[-64];
            else if (mcu > 0 && !(per_interval && mcu % g.interval == 0))
                pred = zz_all[((size_t)(mcu - 1) * g.per_mcu + (comp ? j : luma - 1)) * 64];
            const int dc = jpeg_enc_dc_bits((int)zz[0] - pred, chroma);
            bad = dc < 0 || m.ac_bits == kJpegEncPoison || m.ac_bits > kJpegEncMaxBlockBits || m.last > 63;
            bits = bad ? 0 : dc + m.ac_bits, last = m.last;
        }
        // ---- offsets: bits behind the interval's start, bytes of the intervals that ended in front ----
        int total_bits;
        const int before = block_exclusive_scan<kWaves>(bits, red, total_bits);
        starts[tid] = before;
        if (tid == 0) chunk_bad = 0;
        __syncthreads();
        if (bad) chunk_bad = 1;
        const int first = per_interval ? max(base, i / per_interval * per_interval) : base;  // of this lane's interval, inside the chunk
        const int lead = first == base ? carry_bits : 0;                                       // an interval that began earlier brings its bits
        const int within = lead + before - starts[first - base];
        const bool ends_interval = live && per_interval && (i + 1) % per_interval == 0 && i + 1 < nblocks;
        const bool ends_image = live && i + 1 == nblocks;
        const int pad = (ends_interval || ends_image) ? (-(within + bits)) & 7 : 0;
        const int interval_bytes = ends_interval ? (within + bits + pad) / 8 + 2 : 0;
        int closed_bytes;
        const int byte_at = block_exclusive_scan<kWaves>(interval_bytes, red, closed_bytes);
        const int at = 8 * byte_at + within;
        const int end = at + bits + pad + (ends_interval ? 16 : 0);
        if (tid == min(nblocks - base, kChunk) - 1) chunk_end = end;  // the chunk's last live lane
        __syncthreads();
        const int end_bits = chunk_end, nbytes = end_bits >> 3;
        if (chunk_bad || end_bits + 64 > kImageBytes * 8 || pos + 2 * (size_t)nbytes + 4 > out_stride) {
            flag = DAD3D_JPEG_ENCODE_FLAG_INTERNAL;  // the same for every lane
            break;
        }
        // ---- the image ----
        for (int w = tid; w <= (end_bits >> 5) + 1; w += kLanes) image[w] = w == 0 ? carry << 24 : 0u;
        for (int w = tid; w <= (nbytes >> 5); w += kLanes) mark[w] = 0;
        __syncthreads();
        if (live) {
            ImagePut put{image, at};
            jpeg_enc_block_emit(zz, last, pred, chroma, ac_lut[chroma], put);
            if (pad) put((1u << pad) - 1u, pad);
            if (ends_interval) {
                const int n = (i + 1) / per_interval - 1;  // the restart markers in front of this one
                atomicOr(&mark[put.at >> 8], 1u << (put.at >> 3 & 31));
                put(0xd0u + (n & 7), 16);  // 00 Dn: the FF is written when the bytes leave
            }
        }
        __syncthreads();
        // ---- byte stuffing, and out ----
        const int piece = (nbytes + kLanes - 1) / kLanes;
        const int from = min(tid * piece, nbytes), to = min(from + piece, nbytes);
        int stuffed = 0;
        for (int k = from; k < to; ++k) stuffed += image_byte(image, k) == 255u;
        int all_stuffed;
        const int shift = block_exclusive_scan<kWaves>(stuffed, red, all_stuffed);
        unsigned char* dst = file + pos + from + shift;
        for (int k = from; k < to; ++k) {
            const unsigned v = image_byte(image, k);
            if (mark[k >> 5] >> (k & 31) & 1u) {
                *dst++ = 0xff;
            } else {
                *dst++ = (unsigned char)v;
                if (v == 255u) *dst++ = 0;
            }
        }
        carry_bits = end_bits & 7;
        carry = carry_bits ? image_byte(image, nbytes) : 0u;
        pos += (size_t)nbytes + all_stuffed;
        __syncthreads();  // the image is free for the next chunk
    }
    if (tid == 0) {
        if (!flag) file[pos] = 0xff, file[pos + 1] = 0xd9;
        lengths[b] = flag ? 0 : (long long)(pos + 2);
        flags[b] = flag;
    }
}

}  // namespace

static bool jpeg_enc_shape_ok(int h, int w, int c, int subsampling) {
    if (h < 1 || w < 1 || h > 65535 || w > 65535 || (c != 1 && c != 3) || subsampling < 0 || subsampling > 2) return false;
    return jpeg_enc_blocks(jpeg_enc_geometry(h, w, c, 50, subsampling, 0)) <= kJpegEncMaxBlocks;
}
size_t jpeg_encode_max_bytes(int h, int w, int c, int subsampling) {
    return jpeg_enc_shape_ok(h, w, c, subsampling) ? (size_t)jpeg_enc_max_bytes(h, w, c, subsampling) : 0;
}
// per image: the coefficients [blocks][64] int16, then for the whole batch the block records
size_t jpeg_encode_scratch_bytes(int batch, int h, int w, int c, int subsampling) {
    if (batch < 1 || batch > 65535 || !jpeg_enc_shape_ok(h, w, c, subsampling)) return 0;
    const size_t blocks = (size_t)jpeg_enc_blocks(jpeg_enc_geometry(h, w, c, 50, subsampling, 0));
    return (size_t)batch * blocks * (128 + sizeof(BlockMeta));
}

dad3d_status launch_jpeg_encode(const JpegEncodeArgs& a, hipStream_t s) {
    const JpegEncGeom g = jpeg_enc_geometry(a.h, a.w, a.c, a.quality, a.subsampling, a.restart_interval);
    const int nblocks = (int)jpeg_enc_blocks(g), chunks = (nblocks + kFdctLanes - 1) / kFdctLanes;
    short* coefs = static_cast<short*>(a.scratch);
    BlockMeta* meta = reinterpret_cast<BlockMeta*>(static_cast<unsigned char*>(a.scratch) + (size_t)a.batch * nblocks * 128);
    hipLaunchKernelGGL(jpeg_fdct_kernel, dim3(chunks + 1, a.batch), dim3(kFdctLanes), 0, s, a.images, g, nblocks, chunks, coefs, meta, a.out,
                       a.out_stride);
    DAD3D_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(jpeg_pack_kernel, dim3(a.batch), dim3(kLanes), 0, s, g, nblocks, coefs, meta, a.out, a.out_stride,
                       reinterpret_cast<long long*>(a.lengths), a.flags);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

// one image on the CPU through the same headers: every block in the order of the scan, a bit writer that stuffs as it goes
namespace {
struct HostPut {
    unsigned char* out;
    long long cap, n;
    unsigned long long acc;
    int held;
    void byte(unsigned v) {
        if (n < cap) out[n] = (unsigned char)v;
        ++n;
    }
    void operator()(unsigned bits, int count) {
        acc = acc << count | bits, held += count;
        for (; held >= 8; held -= 8) {
            const unsigned v = (unsigned)(acc >> (held - 8)) & 255u;
            byte(v);
            if (v == 255u) byte(0);
        }
    }
    void flush() {
        if (held) (*this)((1u << (8 - held)) - 1u, 8 - held);
    }
};
}  // namespace

int jpeg_encode_host(const unsigned char* image, int h, int w, int c, int quality, int subsampling, int restart_interval, unsigned char* out,
                     long long capacity, long long* length) {
    const JpegEncGeom g = jpeg_enc_geometry(h, w, c, quality, subsampling, restart_interval);
    const int nblocks = (int)jpeg_enc_blocks(g), luma = c == 1 ? 1 : g.hs * g.vs;
    *length = 0;
    if (capacity < jpeg_enc_header_bytes(c, restart_interval) + 2) return DAD3D_JPEG_ENCODE_FLAG_INTERNAL;
    HostPut put{out, capacity, jpeg_enc_write_header(g, out), 0, 0};
    int pred[3] = {0, 0, 0}, restarts = 0, flag = 0;
    for (int i = 0; i < nblocks && !flag; ++i) {
        const int mcu = i / g.per_mcu, j = i - mcu * g.per_mcu, comp = j < luma ? 0 : j - luma + 1;
        if (g.interval && j == 0 && mcu && mcu % g.interval == 0) {
            put.flush();
            put.byte(0xff), put.byte(0xd0 + (restarts++ & 7));
            pred[0] = pred[1] = pred[2] = 0;
        }
        const JpegEncBlock where = jpeg_enc_locate(g, i);
        int d[64], bits, last;
        alignas(16) short zz[64];
        jpeg_enc_samples(image, g, where, d);
        jpeg_fdct_quantise(d, comp ? 1 : 0, g.scale, where.dummy, zz);
        jpeg_enc_ac_stats(zz, comp ? 1 : 0, bits, last);
        if (bits == kJpegEncPoison || jpeg_enc_dc_bits((int)zz[0] - pred[comp], comp ? 1 : 0) < 0) flag = DAD3D_JPEG_ENCODE_FLAG_INTERNAL;
        if (!flag) jpeg_enc_block_emit(zz, last, pred[comp], comp ? 1 : 0, jpeg_ac_lut(comp ? 1 : 0), put);
        pred[comp] = zz[0];
    }
    put.flush();
    put.byte(0xff), put.byte(0xd9);
    if (put.n > capacity) flag = DAD3D_JPEG_ENCODE_FLAG_INTERNAL;
    *length = flag ? 0 : put.n;
    return flag;
}

}  // namespace dad3d
