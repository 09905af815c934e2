// Baseline JPEG files read back on the device with the entropy data of a file WITHOUT restart markers decoded in pieces, one lane per
// piece (the rules and the routines are csrc/jpeg_sync.hpp). The header scan, the IDCT, the colour conversion and
// all flags are the launches of csrc/jpeg_decode.hip; between them, in this order:
//   jpeg_sync_clear_kernel     zeroes the coefficients of every file without restart markers: a block can span pieces
//   jpeg_sync_groups_kernel    launch A: one workgroup per group of 256 pieces, one lane per piece. Every piece walks leniently from
//                              its guess; then, round after round, every piece whose input (the state the piece in front handed on,
//                              kept in LDS) has changed walks again, until no input changes: 256 rounds at the most, a barrier
//                              between them. Leaves every piece's input, output and counts, and the group's exit.
//                              launch B: the same from where launch A stood, with the group's input taken from the exit launch A
//                              left for the group in front; then a scan over the group gives every piece the blocks and the DC
//                              sums in front of it within the group
//   jpeg_sync_totals_kernel    one workgroup per file: the scan over the groups' totals, and the verification: every group's exit
//                              behind launch B equals its exit behind launch A. Writes info[b] = mode, pieces, groups, 0.
//   jpeg_sync_write_kernel     a verified file: one lane per piece walks strictly from its state, block index and predictors and
//                              writes coefficients
//   jpeg_sync_segments_kernel  one lane per segment (jpeg_decode_segment), as jpeg_entropy_kernel does: the segments of a file WITH
//                              restart markers, and the one segment of a file whose pieces the totals launch has not verified. A
//                              launch of its own: the serial walk beside the strict walk of a piece needs more registers than a
//                              kernel has without spilling. The lanes of a wave take the same segment of 64 files.
// No workgroup waits for another: what one launch leaves the next one reads. The Huffman tables of the file and the states a group
// hands on lie in LDS.
#include "collectives.hpp"
#include "common.hpp"
#include "jpeg_idct.hpp"
#include "jpeg_sync.hpp"

namespace dad3d {
namespace {

constexpr int kWave = 64;
constexpr int kDesc = DAD3D_JPEG_DECODE_DESC_INTS;
constexpr int kMore = DAD3D_JPEG_DECODE_SYNC_DESC_INTS - DAD3D_JPEG_DECODE_DESC_INTS;  // the columns behind the batch's rows of kDesc
constexpr int kThreads = kSyncGroup;
constexpr int kWaves = kThreads / kWave;
constexpr int kHuffWords = sizeof(JpegHuff) / 4;
static_assert(sizeof(JpegHuff) % 4 == 0 && kMore == 4, "the tables are copied by words; four columns describe the tables of a file");

// What a file without restart markers is cut into, and where its tables lie. `run`: the file takes the pieces' way; `bad`: it would,
// but its columns point outside the scratch or hold less than the file needs.
struct Plan {
    bool run, bad;
    int len, pieces, groups;
    const unsigned char* d;
    JpegSyncPiece* piece;
    JpegSyncGroup* group;
};
__device__ inline Plan plan_of(const JpegFile& F, const unsigned char* files, const long long* desc, int batch, int b, int piece_bytes,
                               unsigned char* scratch, size_t scratch_bytes) {
    Plan p{false, false, 0, 0, 0, nullptr, nullptr, nullptr};
    if (F.flag || F.interval) return p;
    const long long* more = desc + (size_t)batch * kDesc + (size_t)b * kMore;
    const long long pieces_at = more[0], pieces_cap = more[1], groups_at = more[2], groups_cap = more[3];
    const long long head = (long long)batch * (long long)sizeof(JpegFile);
    p.len = F.scan_end - F.scan_at;
    const long long pieces = jpeg_sync_pieces(p.len, piece_bytes), groups = jpeg_sync_groups(pieces);
    p.bad = p.len < 0 || pieces_at < head || (pieces_at & 15) || groups_at < head || (groups_at & 15) || pieces > pieces_cap || groups > groups_cap ||
            pieces_cap > 0x7fffffffll || groups_cap > 0x7fffffffll ||
            (unsigned long long)pieces_at + (unsigned long long)pieces_cap * sizeof(JpegSyncPiece) > scratch_bytes ||
            (unsigned long long)groups_at + (unsigned long long)groups_cap * sizeof(JpegSyncGroup) > scratch_bytes;
    if (p.bad) return p;
    p.run = true, p.pieces = (int)pieces, p.groups = (int)groups;
    p.d = files + desc[(size_t)b * kDesc] + F.scan_at;
    p.piece = reinterpret_cast<JpegSyncPiece*>(scratch + pieces_at), p.group = reinterpret_cast<JpegSyncGroup*>(scratch + groups_at);
    return p;
}

// the file's tables by component into LDS; every lane of the workgroup makes the call
__device__ inline void load_tables(const JpegFile& F, JpegHuff* tabs) {
    for (int slot = 0; slot < 2 * F.comps; ++slot) {
        const unsigned* from = reinterpret_cast<const unsigned*>(&jpeg_sync_table(F, slot));
        unsigned* to = reinterpret_cast<unsigned*>(tabs + slot);
        for (int i = threadIdx.x; i < kHuffWords; i += kThreads) to[i] = from[i];
    }
    __syncthreads();
}

__global__ __launch_bounds__(kThreads) void jpeg_sync_clear_kernel(const long long* __restrict__ desc, unsigned char* __restrict__ scratch) {
    const int b = blockIdx.y;
    const JpegFile& F = reinterpret_cast<const JpegFile*>(scratch)[b];
    if (F.flag || F.interval) return;
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= (long long)jpeg_total_blocks(F) * 8) return;  // 128 bytes a block, 16 a lane; the scan has checked the place
    reinterpret_cast<uint4*>(scratch + desc[(size_t)b * kDesc + 8])[t] = make_uint4(0u, 0u, 0u, 0u);
}

// lane t takes segment t / batch of file t % batch: the lanes of a wave walk the same segment of 64 files, each with its own tables.
// A file without restart markers is one segment, and is walked here only where the totals launch has not verified its pieces.
__global__ __launch_bounds__(kWave) void jpeg_sync_segments_kernel(const unsigned char* __restrict__ files, const long long* __restrict__ desc,
                                                                    int batch, unsigned char* __restrict__ scratch, int* __restrict__ flags,
                                                                    const int* __restrict__ info) {
    const long long t = (long long)blockIdx.x * kWave + threadIdx.x;
    const int seg = (int)(t / batch), b = (int)(t - (long long)seg * batch);
    const JpegFile& F = reinterpret_cast<const JpegFile*>(scratch)[b];
    if (F.flag || seg >= F.nseg || (!F.interval && info[4 * b] != DAD3D_JPEG_DECODE_SYNC_MODE_SERIAL)) return;
    const long long* d = desc + (size_t)b * kDesc;
    const JpegSegment where = reinterpret_cast<const JpegSegment*>(scratch + d[10])[seg];
    const int flag = jpeg_decode_segment(files + d[0], F, seg, where, reinterpret_cast<short*>(scratch + d[8]));
    if (flag) atomicOr(&flags[b], flag);
}

__global__ __launch_bounds__(kThreads) void jpeg_sync_groups_kernel(const unsigned char* __restrict__ files, const long long* __restrict__ desc,
                                                                     int batch, int piece_bytes, int second, unsigned char* __restrict__ scratch,
                                                                     size_t scratch_bytes) {
    __shared__ JpegHuff tabs[6];
    __shared__ unsigned long long outs[kThreads];
    __shared__ int red[kWaves];
    const int b = blockIdx.y, g = blockIdx.x, tid = threadIdx.x;
    const JpegFile& F = reinterpret_cast<const JpegFile*>(scratch)[b];
    const Plan p = plan_of(F, files, desc, batch, b, piece_bytes, scratch, scratch_bytes);
    if (!p.run || g >= p.groups) return;  // the same for every lane
    load_tables(F, tabs);
    const int luma = F.hs * F.vs, per_mcu = F.comps == 3 ? luma + 2 : luma;
    const int u = g * kThreads + tid;
    const bool active = u < p.pieces;
    const long long end_bit = jpeg_sync_end_bit(p.len, u, piece_bytes);
    unsigned long long in = kSyncEnd, out = kSyncEnd, handed = 0ull;
    int blocks = 0;
    unsigned dc[3] = {0u, 0u, 0u};
    if (active) {
        if (!second) {
            in = jpeg_sync_state(jpeg_sync_first_bit(p.d, p.len, u, piece_bytes), 0, 0);
            out = jpeg_sync_piece(p.d, p.len, end_bit, piece_bytes, in, tabs, luma, per_mcu, blocks, dc);
        } else {
            const JpegSyncPiece was = p.piece[u];
            in = was.in, out = was.out, blocks = was.blocks, dc[0] = was.dc[0], dc[1] = was.dc[1], dc[2] = was.dc[2];
        }
    }
    if (tid == 0) handed = second && g ? p.group[g - 1].exit_a : in;
    outs[tid] = out;
    __syncthreads();
    for (int round = 0; round < kThreads; ++round) {  // behind round r the first r pieces stand: no more rounds than pieces
        const unsigned long long want = tid == 0 ? handed : outs[tid - 1];
        const bool changed = active && want != in;
        if (!__syncthreads_or(changed)) break;  // and every lane has read before any lane writes
        if (changed) {
            in = want;
            out = jpeg_sync_piece(p.d, p.len, end_bit, piece_bytes, in, tabs, luma, per_mcu, blocks, dc);
            outs[tid] = out;
        }
        __syncthreads();
    }
    const bool last = u == (p.pieces - 1 < g * kThreads + kThreads - 1 ? p.pieces - 1 : g * kThreads + kThreads - 1);
    if (!second) {
        if (active) p.piece[u] = JpegSyncPiece{in, out, blocks, {dc[0], dc[1], dc[2]}};
        if (last) p.group[g].exit_a = out;
        return;
    }
    int sum_blocks, sum0, sum1, sum2;
    const int before_blocks = block_exclusive_scan<kWaves>(blocks, red, sum_blocks);
    const int before0 = block_exclusive_scan<kWaves>((int)dc[0], red, sum0), before1 = block_exclusive_scan<kWaves>((int)dc[1], red, sum1);
    const int before2 = block_exclusive_scan<kWaves>((int)dc[2], red, sum2);
    if (active) p.piece[u] = JpegSyncPiece{in, out, before_blocks, {(unsigned)before0, (unsigned)before1, (unsigned)before2}};
    if (last) {
        JpegSyncGroup& own = p.group[g];
        own.exit_b = out, own.blocks = sum_blocks, own.dc[0] = (unsigned)sum0, own.dc[1] = (unsigned)sum1, own.dc[2] = (unsigned)sum2;
    }
}

__global__ __launch_bounds__(kThreads) void jpeg_sync_totals_kernel(const unsigned char* __restrict__ files, const long long* __restrict__ desc,
                                                                     int batch, int piece_bytes, unsigned char* __restrict__ scratch,
                                                                     size_t scratch_bytes, int* __restrict__ flags, int* __restrict__ info) {
    __shared__ int red[kWaves];
    const int b = blockIdx.x, tid = threadIdx.x;
    const JpegFile& F = reinterpret_cast<const JpegFile*>(scratch)[b];
    const Plan p = plan_of(F, files, desc, batch, b, piece_bytes, scratch, scratch_bytes);
    if (!p.run) {
        if (tid == 0) {
            if (p.bad) atomicOr(&flags[b], kJpegMalformed);  // a row that points outside the scratch
            info[4 * b] = info[4 * b + 1] = info[4 * b + 2] = info[4 * b + 3] = 0;
        }
        return;
    }
    bool differs = false;
    int blocks = 0, dc0 = 0, dc1 = 0, dc2 = 0;  // of the groups in front of this turn's
    for (int base = 0; base < p.groups; base += kThreads) {
        const int g = base + tid;
        JpegSyncGroup own{0ull, 0ull, 0, {0u, 0u, 0u}};
        if (g < p.groups) own = p.group[g];
        differs = differs || own.exit_a != own.exit_b;
        int sum_blocks, sum0, sum1, sum2;
        const int before_blocks = block_exclusive_scan<kWaves>(own.blocks, red, sum_blocks);
        const int before0 = block_exclusive_scan<kWaves>((int)own.dc[0], red, sum0), before1 = block_exclusive_scan<kWaves>((int)own.dc[1], red, sum1);
        const int before2 = block_exclusive_scan<kWaves>((int)own.dc[2], red, sum2);
        if (g < p.groups) {
            JpegSyncGroup& to = p.group[g];
            to.blocks = blocks + before_blocks, to.dc[0] = (unsigned)(dc0 + before0), to.dc[1] = (unsigned)(dc1 + before1), to.dc[2] = (unsigned)(dc2 + before2);
        }
        blocks += sum_blocks, dc0 += sum0, dc1 += sum1, dc2 += sum2;
    }
    const int unverified = __syncthreads_or(differs);
    if (tid == 0) info[4 * b] = unverified ? 2 : 1, info[4 * b + 1] = p.pieces, info[4 * b + 2] = p.groups, info[4 * b + 3] = 0;
}

__global__ __launch_bounds__(kThreads) void jpeg_sync_write_kernel(const unsigned char* __restrict__ files, const long long* __restrict__ desc,
                                                                    int batch, int piece_bytes, unsigned char* __restrict__ scratch,
                                                                    size_t scratch_bytes, int* __restrict__ flags, const int* __restrict__ info) {
    __shared__ JpegHuff tabs[6];
    const int b = blockIdx.y, g = blockIdx.x, tid = threadIdx.x;
    const JpegFile& F = reinterpret_cast<const JpegFile*>(scratch)[b];
    const Plan p = plan_of(F, files, desc, batch, b, piece_bytes, scratch, scratch_bytes);
    if (!p.run || g >= p.groups || info[4 * b] != 1) return;
    short* coefs = reinterpret_cast<short*>(scratch + desc[(size_t)b * kDesc + 8]);
    load_tables(F, tabs);
    const int u = g * kThreads + tid;
    if (u >= p.pieces) return;
    const JpegSyncPiece own = p.piece[u];
    const JpegSyncGroup& front = p.group[g];
    const unsigned pred[3] = {front.dc[0] + own.dc[0], front.dc[1] + own.dc[1], front.dc[2] + own.dc[2]};
    const int flag = jpeg_sync_write_piece(p.d, p.len, jpeg_sync_end_bit(p.len, u, piece_bytes), piece_bytes, u == p.pieces - 1, own.in, tabs, F,
                                           (int)((unsigned)front.blocks + (unsigned)own.blocks), pred, coefs);
    if (flag) atomicOr(&flags[b], flag);
}

}  // namespace

// jpeg_decode_layout, and behind the batch's rows of DAD3D_JPEG_DECODE_DESC_INTS four columns a file: where its piece table and its
// group table lie in the scratch, and what they hold. grid[3] = the most groups a file of the batch may have.
size_t jpeg_decode_sync_layout(long long* desc, int batch, int* grid, int piece_bytes) {
    if (!jpeg_sync_piece_bytes_ok(piece_bytes)) return 0;
    size_t at = jpeg_decode_layout(desc, batch, grid);
    if (at == 0) return 0;
    long long most_groups = 1;
    for (int b = 0; b < batch; ++b) {
        long long* more = desc + (size_t)batch * kDesc + (size_t)b * kMore;
        const long long pieces = jpeg_sync_pieces(desc[(size_t)b * kDesc + 1], piece_bytes), groups = jpeg_sync_groups(pieces);
        more[0] = (long long)at, at += (size_t)pieces * sizeof(JpegSyncPiece);
        more[1] = pieces;
        more[2] = (long long)at, at += (size_t)groups * sizeof(JpegSyncGroup);
        more[3] = groups;
        most_groups = groups > most_groups ? groups : most_groups;
    }
    grid[3] = (int)most_groups;
    return at;
}

dad3d_status launch_jpeg_decode_sync(const JpegDecodeSyncArgs& a, hipStream_t s) {
    const JpegDecodeArgs& j = a.base;
    const dad3d_status scanned = launch_jpeg_scan(j, s);
    if (scanned != DAD3D_OK) return scanned;
    const unsigned clear_x = (unsigned)(((long long)j.max_blocks * 8 + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(jpeg_sync_clear_kernel, dim3(clear_x, j.batch), dim3(kThreads), 0, s, j.desc, j.scratch);
    DAD3D_HIP_TRY(hipGetLastError());
    for (int second = 0; second < 2; ++second) {
        hipLaunchKernelGGL(jpeg_sync_groups_kernel, dim3(a.max_groups, j.batch), dim3(kThreads), 0, s, j.files, j.desc, j.batch, a.piece_bytes, second,
                           j.scratch, j.scratch_bytes);
        DAD3D_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(jpeg_sync_totals_kernel, dim3(j.batch), dim3(kThreads), 0, s, j.files, j.desc, j.batch, a.piece_bytes, j.scratch,
                       j.scratch_bytes, j.flags, a.info);
    DAD3D_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(jpeg_sync_write_kernel, dim3(a.max_groups, j.batch), dim3(kThreads), 0, s, j.files, j.desc, j.batch, a.piece_bytes, j.scratch,
                       j.scratch_bytes, j.flags, a.info);
    DAD3D_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(jpeg_sync_segments_kernel, dim3((unsigned)(((long long)j.max_segments * j.batch + kWave - 1) / kWave)), dim3(kWave), 0, s, j.files,
                       j.desc, j.batch, j.scratch, j.flags, a.info);
    DAD3D_HIP_TRY(hipGetLastError());
    return launch_jpeg_pixels(j, s);
}

}  // namespace dad3d
