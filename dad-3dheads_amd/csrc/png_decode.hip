// PNG files and zlib streams read back on the device, bit-equal to PIL and zlib: the inverse of png_encode.hip.
//
// Five launches for a batch of files of any sizes, described by rows of DAD3D_PNG_DECODE_DESC_INTS int64 (include/dad3d.h):
//   png_scan_kernel      one wave per file: the descriptor against the buffers, signature, IHDR against the descriptor, the chunk walk
//                        (IHDR first, IDATs consecutive, IEND, ancillary chunks skipped, unknown critical chunks refused), the CRC-32
//                        of every chunk in 64 pieces (crc32.hpp), the table of IDAT ranges, and whether the file has the layout of
//                        png_encode.hip: zlib header | segments ending in 00 00 FF FF | 03 00 + Adler-32 (every lane walks the
//                        chunks with the same values: nothing the wave wrote is read back)
//   png_segment_kernel   one wave per (IDAT, candidate file): the IDAT alone through inflate.hpp in kInflateSegment mode, from its own
//                        first bit, straight to its place in the filtered stream; a record of ok / Adler sums / how far a distance
//                        reached in front of the segment (at most kLead bytes), and the segment's last kLead bytes, each as a
//                        value or as the number of the byte in front of the segment that it is a copy of (see below)
//   png_segment_fix_kernel  one wave per (IDAT, candidate file), at work only where a distance reached in front of the segment: the
//                        IDAT again, with the last kLead bytes of the stream in front of it as its history
//   png_inflate_kernel   one wave per file: accepts the segments (all ok, sizes exact, combined Adler-32 == trailer) or inflates the
//                        whole stream through inflate.hpp; zlib_inflate_kernel is the same for a plain stream
//
// The encoder's matches have the distances 1 and C, and its match finder sees the four bytes in front of a segment, so a segment of
// its files may copy from up to kLead = 4 bytes of the segment before. The parse of a segment does not depend on those bytes, only the
// values of the output bytes copied from them, directly or through later copies, and a copy is the identity: such an output byte IS
// one of the kLead bytes. So the first pass inflates such a segment twice, the lead bytes 00 01 02 03 and then FF FE FD FC. An output
// byte that is the same both times has its final value; one that is j the first time and FF - j the second is lead byte j. That turns
// the last kLead bytes of every segment into values or references to the segment before, the second pass follows the references back
// to values (segment 0 has no lead, so the walk ends), and with the true history its output for segment k is the serial decoder's.
//   png_unfilter_kernel  one wave per file: 64 rows in flight, lane r one pixel behind lane r - 1, the neighbours in registers and
//                        one shuffle; converts to the requested channels and stores at the caller's row stride
//
// The 64 lanes of a wave run inflate.hpp with the same values; the policies below use the lane: the input is staged through LDS in
// pieces of kStage bytes, the output goes into a circular window in LDS (history and write buffer in one), copies and stored bytes
// are spread over the lanes, and each full piece of kFlush bytes leaves in 4-byte stores with its Adler sums taken on the way.
#include "collectives.hpp"
#include "common.hpp"
#include "crc32.hpp"
#include "inflate.hpp"
#include "png_common.hpp"

namespace dad3d {
namespace {

constexpr int kSeg = DAD3D_PNG_SEGMENT_BYTES;
constexpr int kWave = 64;
constexpr int kStage = 2048;   // input bytes staged in LDS
constexpr int kFlush = 4096;   // output leaves the window in pieces of this size
constexpr int kWindow = 32768;     // the general path: the whole history of deflate
constexpr int kSegWindow = 16384;  // a segment yields kSeg bytes at most
constexpr int kLead = 4;           // a segment's distances may reach this far into the segment before
constexpr int kDesc = DAD3D_PNG_DECODE_DESC_INTS;
constexpr int kMalformed = DAD3D_PNG_DECODE_FLAG_MALFORMED, kUnsupported = DAD3D_PNG_DECODE_FLAG_UNSUPPORTED;
static_assert(kMalformed == kInflateMalformed && DAD3D_PNG_DECODE_FLAG_OVERFLOW == kInflateOverflow, "inflate.hpp sets the public flags");
static_assert(kStage + kFlush + 258 <= kSegWindow && kSeg + kLead <= kSegWindow, "unflushed output and the lead stay inside the window");
static_assert(kLead == 4 && kSeg >= kLead, "the lead is one word, and a whole segment holds it");

struct FileState {
    int flag, ranges, candidate, pad;
};
struct SegResult {
    int ok;
    unsigned a, b;
    int reach;  // the furthest a distance went in front of the segment's own output, 0 .. kLead
};
struct SegTail {
    unsigned bytes;  // the segment's last kLead bytes after the first pass, the first of them in the low byte
    unsigned from;   // per byte: kTailValue, or j = it is byte j of the kLead bytes in front of the segment
};
constexpr unsigned kTailValue = 0xffu, kLeadFirst = 0x03020100u, kLeadSecond = 0xfcfdfeffu;
struct Range {
    int at, bytes;  // from the start of the file
};

// ---------------------------------------------------------------------------------------------------------------------------
// the policies of inflate.hpp for one wave
// ---------------------------------------------------------------------------------------------------------------------------
struct WaveIn {
    const unsigned char* base;
    const Range* ranges;  // nullptr: the one range [0, single)
    int n, single, r, roff, have, at;
    unsigned char* stage;

    __device__ int range_bytes(int i) const { return ranges ? __builtin_amdgcn_readfirstlane(ranges[i].bytes) : single; }
    __device__ bool refill() {
        while (r < n && roff >= range_bytes(r)) ++r, roff = 0;
        if (r >= n) return false;
        const int k = min(kStage, range_bytes(r) - roff);
        const unsigned char* src = base + (ranges ? __builtin_amdgcn_readfirstlane(ranges[r].at) : 0) + roff;
        __syncthreads();
#pragma unroll 1
        for (int i = threadIdx.x; i < k; i += kWave) stage[i] = src[i];
        __syncthreads();
        have = k, at = 0, roff += k;
        return true;
    }
    __device__ int byte() {
        if (at >= have && !refill()) return -1;
        return __builtin_amdgcn_readfirstlane(stage[at++]);
    }
    __device__ int chunk(int want) {
        if (at >= have && !refill()) return 0;
        return min(want, have - at);
    }
    __device__ const unsigned char* ptr() const { return stage + at; }
    __device__ void skip(int k) { at += k; }
    __device__ bool at_end() const {
        if (at < have) return false;
        int rr = r, ro = roff;
        while (rr < n && ro >= range_bytes(rr)) ++rr, ro = 0;
        return rr >= n;
    }
};

template <int kWin>
struct WaveOut {
    unsigned char* win;  // LDS, kWin bytes, position p at p & (kWin - 1)
    unsigned char* out;  // 4-byte aligned
    int cap, n, flushed;  // a stream is below 2^31 bytes
    unsigned a, b;
    int lead_bytes, reach;  // history at the positions -lead_bytes .. -1 of the window; the furthest a copy went into it

    __device__ int produced() const { return n; }
    __device__ int lead() const { return lead_bytes; }
    __device__ bool room(int k) const { return k <= cap - n; }
    __device__ void flush(int m) {  // [flushed, flushed + m) never wraps: flushed is a multiple of kFlush
        __syncthreads();
        const unsigned* src = reinterpret_cast<const unsigned*>(win + (flushed & (kWin - 1)));
        unsigned* dst = reinterpret_cast<unsigned*>(out + flushed);
        unsigned sa = 0, sb = 0;  // a lane's share of sum x and sum (m - i) x[i]: below 2^29
#pragma unroll 1
        for (int j = threadIdx.x; j < (m >> 2); j += kWave) {
            const unsigned v = src[j];
            dst[j] = v;
            const unsigned x0 = v & 255u, x1 = (v >> 8) & 255u, x2 = (v >> 16) & 255u, x3 = v >> 24;
            const unsigned wgt = (unsigned)(m - 4 * j);
            sa += x0 + x1 + x2 + x3;
            sb += wgt * x0 + (wgt - 1) * x1 + (wgt - 2) * x2 + (wgt - 3) * x3;
        }
        const int tail = m & ~3;
        if ((int)threadIdx.x < m - tail) {
            const int i = tail + threadIdx.x;
            const unsigned x = win[(flushed + i) & (kWin - 1)];
            out[flushed + i] = (unsigned char)x;
            sa += x, sb += (unsigned)(m - i) * x;
        }
        sa = __builtin_amdgcn_readfirstlane(wave_sum(sa)) % kAdlerMod;
        sb = __builtin_amdgcn_readfirstlane(wave_sum(sb % kAdlerMod)) % kAdlerMod;
        b = (b + (unsigned)m * a + sb) % kAdlerMod;  // m a < 2^28
        a = (a + sa) % kAdlerMod;
        flushed += m;
    }
    __device__ void flush_full() {
        while (n - flushed >= kFlush) flush(kFlush);
    }
    __device__ void lit(int x) {
        win[n & (kWin - 1)] = (unsigned char)x;
        ++n;
        if ((n & (kFlush - 1)) == 0) flush_full();
    }
    // Every source byte is in front of n, so the lanes need no order among themselves for the values. A destination slot aliases
    // a source slot of the same copy only for dist == kWin (n + i and n - dist + i' meet mod kWin only where i == i'), and then
    // the same lane reads it before it writes it; the barrier behind the loop orders this copy before the next. `lit` needs no
    // barrier because every lane writes every literal, so each lane later reads what it wrote itself. All of this assumes a
    // workgroup of ONE wave: with more waves, `lit` and the reads of the next symbol race, and barriers have to go in.
    __device__ void copy(int dist, int len) {
        reach = max(reach, dist - n);
#pragma unroll 1
        for (int i = threadIdx.x; i < len; i += kWave) {
            const int back = dist >= len ? i : i % dist;
            win[(n + i) & (kWin - 1)] = win[(n - dist + back) & (kWin - 1)];
        }
        n += len;
        __syncthreads();
        flush_full();
    }
    __device__ void bytes(const unsigned char* p, int k) {
#pragma unroll 1
        for (int i = threadIdx.x; i < k; i += kWave) win[(n + i) & (kWin - 1)] = p[i];
        n += k;
        __syncthreads();
        flush_full();
    }
    __device__ unsigned finish() {
        if (n > flushed) flush(n - flushed);
        return b << 16 | a;
    }
};

template <int kWin>
struct InflateShared {
    unsigned char win[kWin];
    unsigned char stage[kStage];
    InflateWork work;
};

// one wave: the ranges -> out[0, cap); returns the flag, *produced = the bytes written, *adler = the sums of the output. With
// lead = kLead the four bytes of `history` (the first in the low byte) stand in front of the output and *reach says how far into
// them a distance went.
template <int kWin>
__device__ int wave_inflate(InflateShared<kWin>& sh, const unsigned char* base, const Range* ranges, int n_ranges, int single, unsigned char* out,
                            long long cap, int mode, long long* produced, unsigned* adler, int lead = 0, unsigned history = 0,
                            int* reach = nullptr) {
    __syncthreads();
    if ((int)threadIdx.x < lead) sh.win[kWin - lead + threadIdx.x] = (unsigned char)(history >> (8 * threadIdx.x));
    __syncthreads();
    WaveIn in{base, ranges, n_ranges, single, 0, 0, 0, 0, sh.stage};
    WaveOut<kWin> o{sh.win, out, (int)cap, 0, 0, mode == kInflateZlib ? 1u : 0u, 0u, lead, 0};
    Inflater<WaveIn, WaveOut<kWin>> inf(in, o, sh.work);
    const int flag = inf.run(mode);
    *produced = o.flushed;
    *adler = o.b << 16 | o.a;
    if (reach) *reach = o.reach;
    return flag;
}

// the last kLead bytes of a whole segment's output, still in the window
__device__ inline unsigned segment_tail(const unsigned char* win, long long produced) {
    unsigned v = 0;
    if (produced >= kLead && produced <= kSeg)
        for (int j = 0; j < kLead; ++j) v |= (unsigned)win[produced - kLead + j] << (8 * j);
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------------
// scan
// ---------------------------------------------------------------------------------------------------------------------------
__device__ inline unsigned be32(const unsigned char* p) { return (unsigned)p[0] << 24 | (unsigned)p[1] << 16 | (unsigned)p[2] << 8 | p[3]; }

// CRC-32 of p[0, len) by the wave
__device__ inline unsigned wave_crc(const unsigned char* p, unsigned len) {
    const unsigned piece = (len + kWave - 1) / kWave;
    const unsigned first = min(threadIdx.x * piece, len), last = min(first + piece, len);
    unsigned crc = 0;
    if (last > first) {
        crc = 0xffffffffu;
        for (unsigned i = first; i < last; ++i) crc = crc_bitwise(crc, p[i]);
        crc = gf_mul(gf_x_pow_bytes_wide(len - last), ~crc);
    }
    return wave_xor(crc);
}

struct Layout {
    long long file_at, file_bytes, h, w, src_c, out_at, out_stride, out_c, stream_at, ranges_at, ranges_cap, records_at;
};
__device__ inline Layout load_layout(const long long* desc, int b) {
    const long long* d = desc + (size_t)b * kDesc;
    return Layout{d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10], d[11]};
}
__device__ inline bool layout_ok(const Layout& l, int batch, size_t files_bytes, size_t out_bytes, size_t scratch_bytes) {
    const long long lim = 0x7fffffffll, head = (long long)batch * (long long)sizeof(FileState);
    if (l.file_at < 0 || l.file_bytes < 0 || l.file_bytes > lim || (unsigned long long)l.file_at + l.file_bytes > files_bytes) return false;
    if (l.h < 1 || l.w < 1 || l.h > lim || l.w > lim || l.src_c < 1 || l.src_c > 4 || l.out_c < 1 || l.out_c > 4) return false;
    if (l.w * 4 > lim || l.h * (1 + l.w * l.src_c) > lim) return false;
    const long long n = l.h * (1 + l.w * l.src_c), nseg = (n + kSeg - 1) / kSeg;
    if (l.out_at < 0 || l.out_stride < l.w * l.out_c || l.out_stride > lim) return false;
    if ((unsigned long long)l.out_at + (l.h - 1) * l.out_stride + l.w * l.out_c > out_bytes) return false;
    if (l.stream_at < head || (l.stream_at & 15) || (unsigned long long)l.stream_at + n > scratch_bytes) return false;
    if (l.ranges_at < head || (l.ranges_at & 7) || l.ranges_cap < 0 || l.ranges_cap > lim) return false;
    if ((unsigned long long)l.ranges_at + l.ranges_cap * sizeof(Range) > scratch_bytes) return false;
    if (l.records_at < head || (l.records_at & 15) || (unsigned long long)l.records_at + nseg * (sizeof(SegResult) + sizeof(SegTail)) > scratch_bytes)
        return false;
    return true;
}

constexpr unsigned fourcc(char a, char b, char c, char d) { return (unsigned)a << 24 | (unsigned)b << 16 | (unsigned)c << 8 | (unsigned)d; }

__device__ inline bool zlib_header_ok(unsigned cmf, unsigned flg) {
    return (cmf & 15u) == 8u && (cmf >> 4) <= 7u && ((cmf << 8) | flg) % 31u == 0u && !(flg & 0x20u);
}

__global__ __launch_bounds__(kWave) void png_scan_kernel(const unsigned char* __restrict__ files, size_t files_bytes, const long long* __restrict__ desc,
                                                          int batch, size_t out_bytes, unsigned char* __restrict__ scratch, size_t scratch_bytes,
                                                          int max_segments, int* __restrict__ flags, int* __restrict__ info) {
    const int b = blockIdx.x, lane = threadIdx.x;
    FileState* state = reinterpret_cast<FileState*>(scratch) + b;
    const Layout l = load_layout(desc, b);
    int flag = 0, nr = 0, candidate = 0;
    if (!layout_ok(l, batch, files_bytes, out_bytes, scratch_bytes)) {
        flag = kMalformed;
    } else {
        const unsigned char* f = files + l.file_at;
        const long long len = l.file_bytes;
        Range* ranges = reinterpret_cast<Range*>(scratch + l.ranges_at);
        // what the walk needs of the row, in words: the whole row live in scalar registers spills them
        const unsigned want_w = (unsigned)l.w, want_h = (unsigned)l.h;
        const int want_c = (int)l.src_c, ranges_cap = (int)l.ranges_cap;
        const int nseg = (int)((l.h * (1 + l.w * l.src_c) + kSeg - 1) / kSeg);
        bool seen_idat = false, idat_over = false, seen_iend = false;
        bool head_ok = false, middle_ok = true, last_is_middle = false, tail_ok = false;  // of the IDATs seen so far
        if (len < 8 + 25 + 12 || be32(f) != 0x89504e47u || be32(f + 4) != 0x0d0a1a0au) flag = kMalformed;
        long long pos = 8;
        for (int index = 0; !flag && !seen_iend; ++index) {
            if (pos + 12 > len) {
                flag = kMalformed;
                break;
            }
            const unsigned n = be32(f + pos), type = be32(f + pos + 4);
            if (n > 0x7fffffffu || pos + 12 + (long long)n > len || wave_crc(f + pos + 4, n + 4) != be32(f + pos + 8 + n)) {
                flag = kMalformed;
                break;
            }
            const unsigned char* body = f + pos + 8;
            if (index == 0) {
                if (type != fourcc('I', 'H', 'D', 'R') || n != 13) {
                    flag = kMalformed;
                    break;
                }
                const unsigned w = be32(body), h = be32(body + 4), depth = body[8], colour = body[9];
                const bool depth_ok = colour == 0   ? (depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16)
                                      : colour == 3 ? (depth == 1 || depth == 2 || depth == 4 || depth == 8)
                                                    : ((colour == 2 || colour == 4 || colour == 6) && (depth == 8 || depth == 16));
                if (!depth_ok || body[10] != 0 || body[11] != 0 || body[12] > 1 || w == 0 || h == 0 || w > 0x7fffffffu || h > 0x7fffffffu) {
                    flag = kMalformed;
                } else if (depth != 8 || colour == 3 || body[12] == 1) {
                    flag = kUnsupported;
                } else {
                    const int c = colour == 0 ? 1 : colour == 4 ? 2 : colour == 2 ? 3 : 4;
                    if (w != want_w || h != want_h || c != want_c) flag = kMalformed;
                }
            } else if (type == fourcc('I', 'D', 'A', 'T')) {
                if (idat_over || nr >= ranges_cap) {
                    flag = kMalformed;
                    break;
                }
                seen_idat = true;
                if (lane == 0) ranges[nr] = Range{(int)(pos + 8), (int)n};
                // the layout of png_encode.hip, from the data alone: header | .. 00 00 FF FF | .. | 03 00 + Adler-32
                if (nr == 0) head_ok = n == 2 && zlib_header_ok(body[0], body[1]);
                if (nr >= 2) middle_ok = middle_ok && last_is_middle;
                last_is_middle = n >= 5 && be32(body + n - 4) == 0x0000ffffu;
                tail_ok = n == 6 && body[0] == 0x03 && body[1] == 0x00;
                ++nr;
            } else {
                idat_over = seen_idat;
                if (type == fourcc('I', 'E', 'N', 'D'))
                    seen_iend = true;
                else if (type == fourcc('I', 'H', 'D', 'R') || (!(type & 0x20000000u) && type != fourcc('P', 'L', 'T', 'E')))
                    flag = kMalformed;  // a critical chunk this reader does not know
            }
            pos += 12 + (long long)n;
        }
        if (!flag && (!seen_idat || !seen_iend)) flag = kMalformed;
        candidate = !flag && head_ok && middle_ok && tail_ok && nr >= 3 && nr - 2 == nseg && nseg <= max_segments;
    }
    if (lane == 0) {
        *state = FileState{flag, nr, candidate, 0};
        flags[b] = flag;
        info[b] = 0;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// inflate
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWave) void png_segment_kernel(const unsigned char* __restrict__ files, const long long* __restrict__ desc,
                                                             unsigned char* __restrict__ scratch) {
    __shared__ InflateShared<kSegWindow> sh;
    const int seg = blockIdx.x, b = blockIdx.y;
    const FileState st = reinterpret_cast<const FileState*>(scratch)[b];
    if (st.flag || !st.candidate || seg >= st.ranges - 2) return;
    const Layout l = load_layout(desc, b);
    const long long n_stream = l.h * (1 + l.w * l.src_c), from = (long long)seg * kSeg;
    const long long cap = min((long long)kSeg, n_stream - from);
    const Range* ranges = reinterpret_cast<const Range*>(scratch + l.ranges_at);
    const int lead = seg ? kLead : 0;  // from >= kSeg >= kLead behind the first segment
    long long produced;
    unsigned adler;
    int reach;
    int flag = wave_inflate(sh, files + l.file_at, ranges + 1 + seg, 1, 0, scratch + l.stream_at + from, cap, kInflateSegment, &produced, &adler, lead,
                            kLeadFirst, &reach);
    int ok = flag == 0 && produced == cap;
    const unsigned tail = segment_tail(sh.win, produced);
    unsigned tail_from = kTailValue * 0x01010101u;
    if (ok && reach > 0) {  // the same parse with the other lead: a byte that differs is a copy of a lead byte
        long long again;
        unsigned sums;
        int r;
        flag = wave_inflate(sh, files + l.file_at, ranges + 1 + seg, 1, 0, scratch + l.stream_at + from, cap, kInflateSegment, &again, &sums, lead,
                            kLeadSecond, &r);
        const unsigned other = segment_tail(sh.win, again);
        ok = flag == 0 && again == produced;
        tail_from = 0;
        for (int j = 0; j < kLead; ++j) {
            const unsigned x = (tail >> (8 * j)) & 255u, y = (other >> (8 * j)) & 255u;
            if (x != y && (x >= (unsigned)kLead || y != 255u - x)) ok = 0;  // cannot happen: a copy is the identity
            tail_from |= (x == y ? kTailValue : x) << (8 * j);
        }
    }
    if (threadIdx.x == 0) {
        SegResult* rec = reinterpret_cast<SegResult*>(scratch + l.records_at);
        SegTail* tails = reinterpret_cast<SegTail*>(rec + (st.ranges - 2));
        rec[seg] = SegResult{ok, adler & 0xffffu, adler >> 16, reach};
        tails[seg] = SegTail{tail, tail_from};
    }
}

// A wave reads the tails of the segments before, which the first pass wrote and this pass leaves alone, and writes its own segment
// and its own record: the waves of this launch share nothing. The walk back ends at a value, at segment 0 at the latest; where a
// long run crosses many segments it is as long as the run, a few loads a step.
__global__ __launch_bounds__(kWave) void png_segment_fix_kernel(const unsigned char* __restrict__ files, const long long* __restrict__ desc,
                                                                 unsigned char* __restrict__ scratch) {
    __shared__ InflateShared<kSegWindow> sh;
    const int seg = blockIdx.x, b = blockIdx.y;
    const FileState st = reinterpret_cast<const FileState*>(scratch)[b];
    if (st.flag || !st.candidate || seg < 1 || seg >= st.ranges - 2) return;
    const Layout l = load_layout(desc, b);
    SegResult* rec = reinterpret_cast<SegResult*>(scratch + l.records_at);
    const SegTail* tails = reinterpret_cast<const SegTail*>(rec + (st.ranges - 2));
    const SegResult mine = rec[seg];
    if (!mine.ok || mine.reach <= 0) return;
    unsigned history = 0;
    bool resolved = true;
#pragma unroll 1
    for (int j = 0; j < kLead; ++j) {
        int m = seg - 1;
        unsigned at = (unsigned)j, value = 0;
#pragma unroll 1
        for (;;) {
            const SegTail t = tails[m];
            const unsigned f = (t.from >> (8 * at)) & 255u;
            if (f == kTailValue) {
                value = (t.bytes >> (8 * at)) & 255u;
                break;
            }
            if (m == 0 || f >= (unsigned)kLead) {  // a record the first pass did not leave: the file goes the general way
                resolved = false;
                break;
            }
            at = f, --m;
        }
        history |= value << (8 * j);
    }
    int ok = 0;
    unsigned adler = 0;
    if (resolved) {
        const long long n_stream = l.h * (1 + l.w * l.src_c), from = (long long)seg * kSeg;
        const long long cap = min((long long)kSeg, n_stream - from);
        const Range* ranges = reinterpret_cast<const Range*>(scratch + l.ranges_at);
        long long produced;
        int reach;
        const int flag = wave_inflate(sh, files + l.file_at, ranges + 1 + seg, 1, 0, scratch + l.stream_at + from, cap, kInflateSegment, &produced,
                                      &adler, kLead, history, &reach);
        ok = flag == 0 && produced == cap;
    }
    if (threadIdx.x == 0) rec[seg] = SegResult{ok, adler & 0xffffu, adler >> 16, mine.reach};
}

__global__ __launch_bounds__(kWave) void png_inflate_kernel(const unsigned char* __restrict__ files, const long long* __restrict__ desc,
                                                             unsigned char* __restrict__ scratch, int force_general, int* __restrict__ flags,
                                                             int* __restrict__ info) {
    __shared__ InflateShared<kWindow> sh;
    const int b = blockIdx.x, lane = threadIdx.x;
    FileState* state = reinterpret_cast<FileState*>(scratch) + b;
    const FileState st = *state;
    if (st.flag) return;
    const Layout l = load_layout(desc, b);
    const long long n_stream = l.h * (1 + l.w * l.src_c);
    const Range* ranges = reinterpret_cast<const Range*>(scratch + l.ranges_at);
    const unsigned char* f = files + l.file_at;
    if (st.candidate && !force_general) {
        // the segments' Adler sums combined as png_assemble_kernel combines them
        const SegResult* rec = reinterpret_cast<const SegResult*>(scratch + l.records_at);
        const int nseg = st.ranges - 2;
        bool ok = true;
        unsigned long long s1 = 0, s2 = 0;
        for (int j = lane; j < nseg; j += kWave) {
            const SegResult r = rec[j];
            ok = ok && r.ok;
            const long long end = min((long long)(j + 1) * kSeg, n_stream);
            s1 += r.a;
            s2 = (s2 + r.b + (unsigned long long)r.a * (unsigned long long)((n_stream - end) % kAdlerMod)) % kAdlerMod;
        }
        s1 = wave_sum(s1 % kAdlerMod), s2 = wave_sum(s2);
        const unsigned a = (unsigned)((1 + s1) % kAdlerMod);
        const unsigned bb = (unsigned)(((unsigned long long)(n_stream % kAdlerMod) + s2) % kAdlerMod);
        if (__all(ok) && be32(f + ranges[st.ranges - 1].at + 2) == (bb << 16 | a)) {
            if (lane == 0) info[b] = DAD3D_PNG_DECODE_INFO_SEGMENTED;
            return;
        }
    }
    long long produced;
    unsigned adler;
    int flag = wave_inflate(sh, f, ranges, st.ranges, 0, scratch + l.stream_at, n_stream, kInflateZlib, &produced, &adler);
    if (flag || produced != n_stream) flag = kMalformed;  // a filtered stream too long or too short for the IHDR
    if (flag && lane == 0) state->flag = flag, flags[b] = flag;
}

__global__ __launch_bounds__(kWave) void zlib_inflate_kernel(const unsigned char* __restrict__ streams, size_t streams_bytes,
                                                              const long long* __restrict__ desc, unsigned char* __restrict__ out, size_t out_bytes,
                                                              long long* __restrict__ lengths, int* __restrict__ flags) {
    __shared__ InflateShared<kWindow> sh;
    const int b = blockIdx.x;
    const long long* d = desc + (size_t)b * DAD3D_ZLIB_DECODE_DESC_INTS;
    const long long at = d[0], bytes = d[1], out_at = d[2], cap = d[3];
    int flag = 0;
    long long produced = 0;
    if (at < 0 || bytes < 0 || bytes > 0x7fffffffll || (unsigned long long)at + bytes > streams_bytes || out_at < 0 || (out_at & 15) || cap < 0 ||
        (unsigned long long)out_at + cap > out_bytes) {
        flag = kMalformed;  // a row that points outside the buffers: nothing is read or written
    } else {
        unsigned adler;
        flag = wave_inflate(sh, streams + at, nullptr, 1, (int)bytes, out + out_at, min(cap, 0x7fffffffll), kInflateZlib, &produced, &adler);
    }
    if (threadIdx.x == 0) lengths[b] = flag ? 0 : produced, flags[b] = flag;
}

// ---------------------------------------------------------------------------------------------------------------------------
// unfilter and store
// ---------------------------------------------------------------------------------------------------------------------------
// Lane r holds row 64 band + r and is at pixel t - r in step t. Its left pixel is its own last result, the pixel above is lane
// r - 1's last result (one shuffle) and the pixel above left is what that shuffle gave one step before. Lane 63 writes its row back
// over the filtered bytes; after a fence lane 0 of the next band reads it as the row above.
__global__ __launch_bounds__(kWave) void png_unfilter_kernel(const long long* __restrict__ desc, unsigned char* scratch, unsigned char* __restrict__ out,
                                                              int* __restrict__ flags) {
    const int b = blockIdx.x, lane = threadIdx.x;
    FileState* state = reinterpret_cast<FileState*>(scratch) + b;
    if (state->flag) return;
    const Layout l = load_layout(desc, b);
    const int h = (int)l.h, w = (int)l.w, sc = (int)l.src_c, oc = (int)l.out_c;
    const size_t pitch = 1 + (size_t)w * sc;
    unsigned char* stream = scratch + l.stream_at;
    unsigned char* image = out + l.out_at;
    bool bad = false;
    for (int band = 0; band * kWave < h; ++band) {
        const int y = band * kWave + lane;
        const bool active = y < h;
        unsigned char* row = stream + (size_t)(active ? y : 0) * pitch;
        int type = active ? row[0] : 0;
        if (type > 4) bad = true, type = 0;
        const unsigned char* above = (lane == 0 && band > 0) ? row - pitch + 1 : nullptr;
        unsigned char* dst = image + (size_t)(active ? y : 0) * (size_t)l.out_stride;
        unsigned left = 0, up_before = 0;
        for (int t = 0; t < w + kWave - 1; ++t) {
            const int x = t - lane;
            const bool valid = active && x >= 0 && x < w;
            unsigned up = __shfl_up(left, 1, kWave);
            if (lane == 0) {
                up = 0;
                if (above && valid)
                    for (int k = 0; k < sc; ++k) up |= (unsigned)above[(size_t)x * sc + k] << (8 * k);
            }
            if (!valid) continue;
            unsigned f = 0;
            for (int k = 0; k < sc; ++k) f |= (unsigned)row[1 + (size_t)x * sc + k] << (8 * k);
            const unsigned a = x > 0 ? left : 0u, c = x > 0 ? up_before : 0u;
            unsigned raw = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int fa = (a >> (8 * k)) & 255, fb = (up >> (8 * k)) & 255, fc = (c >> (8 * k)) & 255;
                const int pred = type == 0 ? 0 : type == 1 ? fa : type == 2 ? fb : type == 3 ? (fa + fb) >> 1 : png_paeth(fa, fb, fc);
                raw |= (((f >> (8 * k)) + (unsigned)pred) & 255u) << (8 * k);
            }
            left = raw, up_before = up;
            if (lane == kWave - 1)
                for (int k = 0; k < sc; ++k) row[1 + (size_t)x * sc + k] = (unsigned char)(raw >> (8 * k));
            // PIL's convert: grey replicated, alpha dropped or 255, L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16
            const unsigned r0 = raw & 255u, r1 = (raw >> 8) & 255u, r2 = (raw >> 16) & 255u, r3 = raw >> 24;
            const bool grey = sc <= 2;
            const unsigned alpha = sc == 2 ? r1 : sc == 4 ? r3 : 255u;
            unsigned char* px = dst + (size_t)x * oc;
            if (oc <= 2) {
                px[0] = (unsigned char)(grey ? r0 : (r0 * 19595u + r1 * 38470u + r2 * 7471u + 0x8000u) >> 16);
                if (oc == 2) px[1] = (unsigned char)alpha;
            } else {
                px[0] = (unsigned char)r0, px[1] = (unsigned char)(grey ? r0 : r1), px[2] = (unsigned char)(grey ? r0 : r2);
                if (oc == 4) px[3] = (unsigned char)alpha;
            }
        }
        __threadfence();
        __syncthreads();
    }
    if (__any(bad) && lane == 0) state->flag = kMalformed, flags[b] = kMalformed;
}

}  // namespace

// fills columns 8 .. 11 of the HOST descriptor rows and returns the scratch bytes; 0 for a row outside the limits
size_t png_decode_layout(long long* desc, int batch, int* max_segments) {
    size_t at = ((size_t)batch * sizeof(FileState) + 15) / 16 * 16;
    int most = 1;
    for (int b = 0; b < batch; ++b) {
        long long* d = desc + (size_t)b * kDesc;
        const long long lim = 0x7fffffffll;
        if (d[1] < 0 || d[1] > lim || d[2] < 1 || d[3] < 1 || d[2] > lim || d[3] > lim || d[4] < 1 || d[4] > 4 || d[7] < 1 || d[7] > 4) return 0;
        if (d[3] * 4 > lim || d[2] * (1 + d[3] * d[4]) > lim) return 0;
        const long long n = d[2] * (1 + d[3] * d[4]), nseg = (n + kSeg - 1) / kSeg, cap = d[1] / 12 + 1;
        d[8] = (long long)at, at += ((size_t)n + 15) / 16 * 16;
        d[9] = (long long)at, at += ((size_t)cap * sizeof(Range) + 15) / 16 * 16;
        d[10] = cap;
        d[11] = (long long)at, at += ((size_t)nseg * (sizeof(SegResult) + sizeof(SegTail)) + 15) / 16 * 16;
        most = nseg > most ? (int)nseg : most;
    }
    *max_segments = most;
    return at;
}

dad3d_status launch_png_decode(const PngDecodeArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(png_scan_kernel, dim3(a.batch), dim3(kWave), 0, s, a.files, a.files_bytes, a.desc, a.batch, a.out_bytes, a.scratch,
                       a.scratch_bytes, a.max_segments, a.flags, a.info);
    DAD3D_HIP_TRY(hipGetLastError());
    if (!a.force_general) {
        hipLaunchKernelGGL(png_segment_kernel, dim3(a.max_segments, a.batch), dim3(kWave), 0, s, a.files, a.desc, a.scratch);
        DAD3D_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(png_segment_fix_kernel, dim3(a.max_segments, a.batch), dim3(kWave), 0, s, a.files, a.desc, a.scratch);
        DAD3D_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(png_inflate_kernel, dim3(a.batch), dim3(kWave), 0, s, a.files, a.desc, a.scratch, a.force_general, a.flags, a.info);
    DAD3D_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(png_unfilter_kernel, dim3(a.batch), dim3(kWave), 0, s, a.desc, a.scratch, a.out, a.flags);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

dad3d_status launch_zlib_decompress(const ZlibDecompressArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(zlib_inflate_kernel, dim3(a.batch), dim3(kWave), 0, s, a.streams, a.streams_bytes, a.desc, a.out, a.out_bytes,
                       reinterpret_cast<long long*>(a.lengths), a.flags);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

int inflate_host(const unsigned char* const* ranges, const long long* range_bytes, int n_ranges, unsigned char* out, long long capacity,
                 long long* length) {
    HostInflateIn in(ranges, range_bytes, n_ranges);
    HostInflateOut o(out, capacity, 1u);
    InflateWork work;
    Inflater<HostInflateIn, HostInflateOut> inf(in, o, work);
    const int flag = inf.run(kInflateZlib);
    *length = o.n;
    return flag;
}

}  // namespace dad3d
