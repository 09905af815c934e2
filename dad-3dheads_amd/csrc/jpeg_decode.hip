// Baseline JPEG files read back on the device, bit-equal to PIL (libjpeg-turbo). The device decodes only what it has
// fully checked; whatever it flags the caller decodes on the host.
//
// Four launches for a batch of files of any sizes, described by rows of DAD3D_JPEG_DECODE_DESC_INTS int64 (include/dad3d.h):
//   jpeg_scan_kernel     one wave per file: the descriptor against the buffers; lane 0 walks the markers up to the scan
//                        (jpeg_entropy.hpp) and leaves the header, the quantisation tables and the canonical Huffman tables in
//                        scratch; then the 64 lanes look for FF xx in the entropy data, 64 bytes a step, and compact the restart
//                        markers in order (a ballot and a count of the hits in front of the lane) into the table of segments
//   jpeg_entropy_kernel  one lane per entropy segment: the first waves take segment 0 of 64 files each, so 64 files without restart
//                        markers share a wave; the others take 64 further segments of one file each. A lane runs the bit reader and
//                        the Huffman decode over its own bytes and writes whole blocks of int16 coefficients. No lane waits for another.
//   jpeg_idct_kernel     one lane per block: dequantise, the integer IDCT, level shift, clamp, into the component's padded plane
//   jpeg_colour_kernel   one lane per pixel: chroma upsampling, YCbCr -> RGB, the channel conversion, the store at the row stride
// A kernel leaves a file alone once its flag is set; the flags are the only words two lanes may both write (atomicOr).
#include "common.hpp"
#include "jpeg_idct.hpp"
#include "jpeg_sync.hpp"

namespace dad3d {
namespace {

constexpr int kWave = 64;
constexpr int kDesc = DAD3D_JPEG_DECODE_DESC_INTS;
constexpr int kColourThreads = 256;
static_assert(sizeof(JpegFile) % 16 == 0, "the file states are the head of the scratch, and what follows is 16-byte aligned");

struct Layout {
    long long file_at, file_bytes, h, w, comps, out_at, out_stride, out_c, coef_at, planes_at, segs_at, segs_cap;
};
__device__ inline Layout load_layout(const long long* desc, int b) {
    const long long* d = desc + (size_t)b * kDesc;
    return Layout{d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10], d[11]};
}
__device__ inline bool layout_ok(const Layout& l, int batch, size_t files_bytes, size_t out_bytes, size_t scratch_bytes) {
    const long long lim = 0x7fffffffll, head = (long long)batch * (long long)sizeof(JpegFile);
    if (l.file_at < 0 || l.file_bytes < 0 || l.file_bytes > lim || (unsigned long long)l.file_at + l.file_bytes > files_bytes) return false;
    if (l.h < 1 || l.w < 1 || l.h > 65535 || l.w > 65535 || (l.comps != 1 && l.comps != 3) || (l.out_c != 1 && l.out_c != 3)) return false;
    const long long blocks = jpeg_block_capacity(l.h, l.w, l.comps);
    if (blocks > kJpegMaxBlocks) return false;
    if (l.out_at < 0 || l.out_stride < l.w * l.out_c || l.out_stride > lim) return false;
    if ((unsigned long long)l.out_at + (l.h - 1) * l.out_stride + l.w * l.out_c > out_bytes) return false;
    if (l.coef_at < head || (l.coef_at & 15) || (unsigned long long)l.coef_at + blocks * 128 > scratch_bytes) return false;
    if (l.planes_at < head || (l.planes_at & 15) || (unsigned long long)l.planes_at + blocks * 64 > scratch_bytes) return false;
    if (l.segs_at < head || (l.segs_at & 7) || l.segs_cap < 1 || l.segs_cap > kJpegMaxBlocks) return false;
    if ((unsigned long long)l.segs_at + l.segs_cap * sizeof(JpegSegment) > scratch_bytes) return false;
    return true;
}

__global__ __launch_bounds__(kWave) void jpeg_scan_kernel(const unsigned char* __restrict__ files, size_t files_bytes, const long long* __restrict__ desc,
                                                           int batch, size_t out_bytes, unsigned char* __restrict__ scratch, size_t scratch_bytes,
                                                           int* __restrict__ flags) {
    const int b = blockIdx.x, lane = threadIdx.x;
    JpegFile& F = reinterpret_cast<JpegFile*>(scratch)[b];
    const Layout l = load_layout(desc, b);
    if (!layout_ok(l, batch, files_bytes, out_bytes, scratch_bytes)) {  // a bad row is a flag, not an access
        if (lane == 0) F.flag = kJpegMalformed, flags[b] = kJpegMalformed;  // the head of the scratch holds the states: the entry point checks
        return;
    }
    const unsigned char* f = files + l.file_at;
    const int len = (int)l.file_bytes;
    JpegSegment* segs = reinterpret_cast<JpegSegment*>(scratch + l.segs_at);
    int flag = 0, scan_at = 0, expected = 0;
    if (lane == 0) {
        flag = jpeg_parse_header(f, len, F);
        if (!flag && (F.h != (int)l.h || F.w != (int)l.w || F.comps != (int)l.comps)) flag = kJpegMalformed;
        if (!flag) {
            scan_at = F.scan_at, expected = jpeg_expected_segments(F);
            if (expected > l.segs_cap) flag = kJpegMalformed;
        }
    }
    flag = __shfl(flag, 0, kWave), scan_at = __shfl(scan_at, 0, kWave), expected = __shfl(expected, 0, kWave);
    int count = 0, scan_end = -1;
    bool bad = false;
    if (!flag) {
        const unsigned long long below = (1ull << lane) - 1ull;
        for (int base = scan_at; base < len && scan_end < 0 && !flag; base += kWave) {  // the same for every lane
            const int p = base + lane;
            int kind = 0, byte = 0;  // 1 a restart marker, 2 any other marker, 3 FF FF
            if (p + 1 < len && f[p] == 0xff) {
                byte = f[p + 1];
                kind = byte == 0 ? 0 : (byte >= 0xd0 && byte <= 0xd7) ? 1 : byte == 0xff ? 3 : 2;
            }
            const unsigned long long stop = __ballot(kind >= 2);
            unsigned long long rst = __ballot(kind == 1);
            if (stop) {
                const int first = __ffsll((long long)stop) - 1;
                rst &= (1ull << first) - 1ull;
                if (__shfl(byte, first, kWave) != 0xd9)
                    flag = kJpegUnsupported;  // fill bytes in front of a marker, a second scan, DNL, tables between scans
                else
                    scan_end = base + first;
            }
            if (rst >> lane & 1ull) {
                const int idx = count + __popcll(rst & below);
                if (byte - 0xd0 != (idx & 7) || idx + 1 >= expected)
                    bad = true;  // out of sequence, or more than the grid holds
                else
                    segs[idx].end = p, segs[idx + 1].start = p + 2;
            }
            count += __popcll(rst);
        }
        if (!flag && (scan_end < 0 || __any(bad) || count != expected - 1)) flag = kJpegMalformed;
    }
    if (lane == 0) {
        if (!flag) {
            segs[0].start = scan_at, segs[expected - 1].end = scan_end;
            F.nseg = expected, F.scan_end = scan_end;
        }
        F.flag = flag;
        flags[b] = flag;
    }
}

__global__ __launch_bounds__(kWave) void jpeg_entropy_kernel(const unsigned char* __restrict__ files, const long long* __restrict__ desc, int batch,
                                                              int first_waves, int more_waves, unsigned char* __restrict__ scratch,
                                                              int* __restrict__ flags) {
    int b, seg;
    if ((int)blockIdx.x < first_waves) {
        b = blockIdx.x * kWave + threadIdx.x, seg = 0;
    } else {
        const int r = blockIdx.x - first_waves;
        b = r / more_waves, seg = 1 + (r - b * more_waves) * kWave + threadIdx.x;
    }
    if (b >= batch) return;
    const JpegFile& F = reinterpret_cast<const JpegFile*>(scratch)[b];
    if (F.flag || seg >= F.nseg) return;  // the scan's flag: what this launch adds goes to flags[b] alone
    const long long* d = desc + (size_t)b * kDesc;
    const JpegSegment where = reinterpret_cast<const JpegSegment*>(scratch + d[10])[seg];
    const int flag = jpeg_decode_segment(files + d[0], F, seg, where, reinterpret_cast<short*>(scratch + d[8]));
    if (flag) atomicOr(&flags[b], flag);
}

__global__ __launch_bounds__(kWave) void jpeg_idct_kernel(const long long* __restrict__ desc, unsigned char* __restrict__ scratch, int* __restrict__ flags) {
    const int b = blockIdx.y, t = blockIdx.x * kWave + threadIdx.x;
    const JpegFile& F = reinterpret_cast<const JpegFile*>(scratch)[b];
    if (F.flag || t >= jpeg_total_blocks(F)) return;
    if (__builtin_amdgcn_readfirstlane(flags[b])) return;  // a segment was damaged
    const long long* d = desc + (size_t)b * kDesc;
    const int c = t < jpeg_component_base(F, 1) ? 0 : t < jpeg_component_base(F, 2) ? 1 : 2;
    const int across = jpeg_blocks_across(F, c), k = t - jpeg_component_base(F, c), by = k / across, bx = k - by * across;
    unsigned char* plane = scratch + d[9] + (size_t)64 * jpeg_component_base(F, c);
    const int flag = jpeg_idct_block(reinterpret_cast<const short*>(scratch + d[8]) + (size_t)t * 64, F.quant[F.tq[c]],
                                     plane + (size_t)by * 8 * (across * 8) + bx * 8, across * 8);
    if (flag) atomicOr(&flags[b], flag);
}

__global__ __launch_bounds__(kColourThreads) void jpeg_colour_kernel(const long long* __restrict__ desc, const unsigned char* __restrict__ scratch,
                                                                      unsigned char* __restrict__ out, const int* __restrict__ flags) {
    const int b = blockIdx.y;
    if (flags[b]) return;
    const JpegFile& F = reinterpret_cast<const JpegFile*>(scratch)[b];
    const int t = blockIdx.x * kColourThreads + threadIdx.x;
    if (t >= F.h * F.w) return;  // h, w <= 65535 and the block capacity bound the product
    const long long* d = desc + (size_t)b * kDesc;
    const int y = t / F.w, x = t - y * F.w, oc = (int)d[7];
    jpeg_pixel(F, scratch + d[9], x, y, oc, out + d[5] + (size_t)y * (size_t)d[6] + (size_t)x * oc);
}

}  // namespace

// fills columns 8 .. 11 of the HOST descriptor rows, grid[0 .. 2] = the most segments, blocks and pixels a file of the batch may have,
// and returns the scratch bytes; 0 for a row outside the limits
size_t jpeg_decode_layout(long long* desc, int batch, int* grid) {
    size_t at = (size_t)batch * sizeof(JpegFile);
    long long most_segs = 1, most_blocks = 1, most_pixels = 1;
    for (int b = 0; b < batch; ++b) {
        long long* d = desc + (size_t)b * kDesc;
        if (d[1] < 0 || d[1] > 0x7fffffffll || d[2] < 1 || d[3] < 1 || d[2] > 65535 || d[3] > 65535 || (d[4] != 1 && d[4] != 3)) return 0;
        const long long blocks = jpeg_block_capacity(d[2], d[3], d[4]);
        if (blocks > kJpegMaxBlocks) return 0;
        long long segs = jpeg_segment_capacity(d[2], d[3], d[1]);
        segs = segs < 1 ? 1 : segs;
        d[8] = (long long)at, at += (size_t)blocks * 128;
        d[9] = (long long)at, at += (size_t)blocks * 64;
        d[10] = (long long)at, at += ((size_t)segs * sizeof(JpegSegment) + 15) / 16 * 16;
        d[11] = segs;
        most_segs = segs > most_segs ? segs : most_segs;
        most_blocks = blocks > most_blocks ? blocks : most_blocks;
        most_pixels = d[2] * d[3] > most_pixels ? d[2] * d[3] : most_pixels;
    }
    grid[0] = (int)most_segs, grid[1] = (int)most_blocks, grid[2] = (int)most_pixels;
    return at;
}

size_t jpeg_decode_state_bytes() { return sizeof(JpegFile); }

// the first and the last two of the four launches, which csrc/jpeg_decode_sync.hip puts around an entropy stage of its own
dad3d_status launch_jpeg_scan(const JpegDecodeArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3(a.batch), dim3(kWave), 0, s, a.files, a.files_bytes, a.desc, a.batch, a.out_bytes, a.scratch,
                       a.scratch_bytes, a.flags);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

dad3d_status launch_jpeg_pixels(const JpegDecodeArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((a.max_blocks + kWave - 1) / kWave, a.batch), dim3(kWave), 0, s, a.desc, a.scratch, a.flags);
    DAD3D_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3((a.max_pixels + kColourThreads - 1) / kColourThreads, a.batch), dim3(kColourThreads), 0, s, a.desc,
                       a.scratch, a.out, a.flags);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

dad3d_status launch_jpeg_decode(const JpegDecodeArgs& a, hipStream_t s) {
    const dad3d_status scanned = launch_jpeg_scan(a, s);
    if (scanned != DAD3D_OK) return scanned;
    const int first_waves = (a.batch + kWave - 1) / kWave, more_waves = (a.max_segments - 1 + kWave - 1) / kWave;
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(first_waves + a.batch * more_waves), dim3(kWave), 0, s, a.files, a.desc, a.batch, first_waves,
                       more_waves, a.scratch, a.flags);
    DAD3D_HIP_TRY(hipGetLastError());
    return launch_jpeg_pixels(a, s);
}

// one file on the CPU through the same headers; `out` may be null to read the header alone. piece_bytes != 0: the entropy stage in
// pieces, which fills info[4]. Returns the flag.
int jpeg_decode_host(const unsigned char* file, long long size, int channels, unsigned char* out, long long out_bytes, int* h, int* w, int* c,
                     bool* fits, int piece_bytes, int* info) {
    JpegFile* F = new JpegFile();
    *h = *w = *c = 0, *fits = true;
    int flag = jpeg_parse_header(file, size, *F);
    if (!flag) {
        const int oc = channels ? channels : F->comps;
        *h = F->h, *w = F->w, *c = oc;
        if (out) {
            const long long blocks = jpeg_block_capacity(F->h, F->w, F->comps);
            long long cap = jpeg_segment_capacity(F->h, F->w, size);
            cap = cap < 1 ? 1 : cap;
            JpegSegment* segs = new JpegSegment[cap];
            short* coefs = new short[(size_t)blocks * 64];
            unsigned char* planes = new unsigned char[(size_t)blocks * 64];
            flag = jpeg_find_segments(file, size, *F, segs, cap);
            if (!flag && piece_bytes)  // the entropy stage of csrc/jpeg_sync.hpp
                flag = jpeg_sync_entropy_host(file, *F, segs, piece_bytes, coefs, info);
            else
                for (int seg = 0; !flag && seg < F->nseg; ++seg) flag = jpeg_decode_segment(file, *F, seg, segs[seg], coefs);
            const int total = flag ? 0 : jpeg_total_blocks(*F);
            for (int t = 0; !flag && t < total; ++t) {
                const int comp = t < jpeg_component_base(*F, 1) ? 0 : t < jpeg_component_base(*F, 2) ? 1 : 2;
                const int across = jpeg_blocks_across(*F, comp), k = t - jpeg_component_base(*F, comp), by = k / across, bx = k - by * across;
                flag = jpeg_idct_block(coefs + (size_t)t * 64, F->quant[F->tq[comp]],
                                       planes + (size_t)64 * jpeg_component_base(*F, comp) + (size_t)by * 8 * (across * 8) + bx * 8, across * 8);
            }
            if (!flag) {
                if ((long long)F->h * F->w * oc > out_bytes)
                    *fits = false;
                else
                    for (int y = 0; y < F->h; ++y)
                        for (int x = 0; x < F->w; ++x) jpeg_pixel(*F, planes, x, y, oc, out + ((size_t)y * F->w + x) * oc);
            }
            delete[] segs;
            delete[] coefs;
            delete[] planes;
        }
    }
    delete F;
    return flag;
}

}  // namespace dad3d
