// Baseline JPEG, the entropy data of a file WITHOUT restart markers decoded in pieces. Huffman-coded data falls
// into step: a walk started at an arbitrary bit with a guessed state almost always meets the true walk after some bytes. The
// routines here are what one piece does; csrc/jpeg_decode_sync.hip runs them one lane per piece, and jpeg_sync_entropy_host below
// runs them on a CPU, group after group, so tests/test_jpeg_sync_host.py holds to PIL the code the kernels run.
//
//   pieces   the entropy bytes d[0, len) = file[scan_at, scan_end) are cut into pieces of P bytes (a power of two, 16 .. 256);
//            piece u owns the codes whose first bit lies in d[u P, (u + 1) P). A 00 behind an FF is no data: no position rests on it.
//   state    (bit position in d, block j within the MCU, zigzag index k; k = 0: a DC code is next), packed into 64 bits, or kSyncEnd
//   guess    piece u starts at its first data bit with j = 0, k = 0; for piece 0 that is the truth
//   lenient  jpeg_sync_piece: total and deterministic, equal to jpeg_block's walk wherever that walk accepts: a DC symbol skips
//            its value bits, an AC (run, size) moves k on, EOB or k >= 64 ends the block and moves j on, a code no table assigns
//            costs one bit, a bit beyond d[len) gives kSyncEnd. Every step takes a bit or more: at most 8 P steps a piece.
//   strict   jpeg_sync_write_piece: the same walk with the checks of jpeg_block and jpeg_decode_segment, from a state, a block
//            index and three predictors, writing coefficients until the piece or the header's block count ends
// A routine reads nothing outside d[0, len) and writes nothing outside the places it is handed.
#pragma once

#include "jpeg_entropy.hpp"

namespace dad3d {

constexpr int kSyncGroup = 256;                  // pieces a group (one workgroup) hands states through
constexpr unsigned long long kSyncEnd = ~0ull;   // the state behind a walk that needed a bit beyond the data

struct JpegSyncPiece {       // what a piece leaves for the launches behind it
    unsigned long long in, out;  // the state it started from and the state it handed on
    int blocks;                  // blocks that end in it; behind launch B: blocks that end in the pieces of its group in front of it
    unsigned dc[3];              // the DC differences it read, summed per component (wrapping); behind launch B: likewise in front of it
};
struct JpegSyncGroup {
    unsigned long long exit_a, exit_b;  // the last piece's `out` behind launch A and behind launch B
    int blocks;                         // the group's blocks; behind the totals launch: the blocks of the groups in front
    unsigned dc[3];
};
static_assert(sizeof(JpegSyncPiece) == 32 && sizeof(JpegSyncGroup) == 32, "the scratch is laid out by these sizes");

DAD3D_HD bool jpeg_sync_piece_bytes_ok(int p) { return p >= 16 && p <= 256 && (p & (p - 1)) == 0; }
DAD3D_HD long long jpeg_sync_pieces(long long len, int piece_bytes) { return len <= 0 ? 1 : (len + piece_bytes - 1) / piece_bytes; }
DAD3D_HD long long jpeg_sync_groups(long long pieces) { return (pieces + kSyncGroup - 1) / kSyncGroup; }

DAD3D_HD unsigned long long jpeg_sync_state(long long pos, int j, int k) { return (unsigned long long)pos << 10 | (unsigned)j << 6 | (unsigned)k; }
DAD3D_HD long long jpeg_sync_pos(unsigned long long s) { return (long long)(s >> 10); }

// the first data bit of piece u, and the bit at which the piece ends
DAD3D_HD long long jpeg_sync_first_bit(const unsigned char* d, int len, long long u, int piece_bytes) {
    long long at = u * piece_bytes;
    if (at >= len) return 8ll * len;
    if (at > 0 && d[at] == 0 && d[at - 1] == 0xff) ++at;
    return 8 * (at < len ? at : (long long)len);
}
DAD3D_HD long long jpeg_sync_end_bit(int len, long long u, int piece_bytes) {
    const long long end = (u + 1) * piece_bytes;
    return 8 * (end < len ? end : (long long)len);
}

// JpegBits that knows where it stands: `q` never rests on a stuffed 00 (the byte behind an FF is skipped when the FF is taken: the
// segment scan has found no marker in d[0, len), so it is a 00), and `ff` keeps, one bit per taken byte, whether it was an FF.
struct JpegSyncBits {
    const unsigned char* d;
    int len, q;
    unsigned long long acc;  // the low `have` bits are unread
    int have;
    unsigned ff;
    bool over;

    DAD3D_HD void open(const unsigned char* data, int n, long long pos) {
        d = data, len = n, acc = 0ull, have = 0, ff = 0u, over = false;
        const long long byte = pos >> 3;
        q = byte < 0 ? 0 : byte > n ? n : (int)byte;
        fill();
        skip((int)(pos & 7));
        over = false;
    }
    DAD3D_HD void take(unsigned b, bool& stuffed) {
        if (stuffed) {
            stuffed = false;
        } else {
            acc = acc << 8 | b, have += 8, ff = ff << 1 | (b == 0xffu ? 1u : 0u);
            stuffed = b == 0xffu;
        }
    }
    DAD3D_HD void fill() {
        if (have > 32 || q >= len) return;
        const int left = len - q, n = left < 4 ? left : 4;
        const unsigned b0 = d[q], b1 = d[q + (n > 1 ? 1 : 0)], b2 = d[q + (n > 2 ? 2 : 0)], b3 = d[q + (n > 3 ? 3 : 0)];
        bool stuffed = false;
        take(b0, stuffed);
        if (n > 1) take(b1, stuffed);
        if (n > 2) take(b2, stuffed);
        if (n > 3) take(b3, stuffed);
        q += n + (stuffed ? 1 : 0);
        q = q > len ? len : q;
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
    // the position in d of the first unread bit: behind q lie the unread bytes and the stuffed bytes behind those of them that are FF
    DAD3D_HD long long at() const {
        const int bytes = (have + 7) >> 3;
        const int stuffed = __builtin_popcount(ff & ((1u << bytes) - 1u));
        return 8ll * (q - bytes - stuffed) + ((8 - (have & 7)) & 7);
    }
    DAD3D_HD bool left_over() const { return q < len || have >= 8; }  // a whole byte nobody read
};

// The Huffman tables of a file by component, for the lookups of a piece: tabs[2 c] the DC table of component c, tabs[2 c + 1] its AC table.
DAD3D_HD const JpegHuff& jpeg_sync_table(const JpegFile& F, int slot) { return F.huff[slot & 1 ? 4 + F.ta[slot >> 1] : F.td[slot >> 1]]; }

// The lenient walk over the codes piece u owns, from `in`; returns the state it hands on, and counts the blocks that end in the
// piece and its DC differences. `luma` blocks of component 0 come first in an MCU of `per_mcu` blocks.
DAD3D_HD unsigned long long jpeg_sync_piece(const unsigned char* d, int len, long long end_bit, int piece_bytes, unsigned long long in,
                                            const JpegHuff* tabs, int luma, int per_mcu, int& blocks, unsigned* dc) {
    blocks = 0, dc[0] = dc[1] = dc[2] = 0u;
    if (in == kSyncEnd) return kSyncEnd;
    long long pos = jpeg_sync_pos(in);
    if (pos >= end_bit) return in;
    int j = (int)(in >> 6) & 15, k = (int)in & 63;
    JpegSyncBits bits;
    bits.open(d, len, pos);
    for (int step = 0; step < 8 * piece_bytes; ++step) {  // every turn takes a bit or more of the piece's 8 P
        const int c = j < luma ? 0 : j - luma + 1;
        if (k == 0) {
            const int s = jpeg_symbol(bits, tabs[2 * c]);
            if (s < 0) {
                bits.skip(1);
            } else {
                if (s) dc[c] += (unsigned)jpeg_extend(bits.get(s), s);
                k = 1;
            }
        } else {
            const int rs = jpeg_symbol(bits, tabs[2 * c + 1]);
            if (rs < 0) {
                bits.skip(1);
            } else if ((rs & 15) == 0) {
                k = (rs >> 4) == 15 ? k + 16 : 64;
            } else {
                bits.get(rs & 15);
                k += (rs >> 4) + 1;
            }
        }
        if (bits.over) return kSyncEnd;
        if (k >= 64) k = 0, j = j + 1 == per_mcu ? 0 : j + 1, ++blocks;
        pos = bits.at();
        if (pos >= end_bit) break;
    }
    return jpeg_sync_state(pos, j, k);
}

// where block j of MCU m lies among the file's blocks (jpeg_decode_segment's order)
DAD3D_HD int jpeg_sync_block_at(const JpegFile& F, int m, int j) {
    const int luma = F.hs * F.vs;
    if (j >= luma) return jpeg_component_base(F, j - luma + 1) + m;
    const int my_ = m / F.mx, mx_ = m - my_ * F.mx, v = j / F.hs, h = j - v * F.hs;
    return (my_ * F.vs + v) * (F.mx * F.hs) + mx_ * F.hs + h;
}

// The strict walk over the codes piece u owns, from the state `in`, with `block` blocks and the predictors `pred` in front of it.
// The coefficients it reads go to coefs[block][64] (cleared by the caller: a block can span pieces). Stops at the header's block
// count; the piece that ends the last block checks what is left of the data, and the file's last piece that its blocks were all
// there. Returns the flag.
DAD3D_HD int jpeg_sync_write_piece(const unsigned char* d, int len, long long end_bit, int piece_bytes, bool last_piece, unsigned long long in,
                                   const JpegHuff* tabs, const JpegFile& F, int block, const unsigned* pred_in, short* coefs) {
    const int total = jpeg_total_blocks(F);
    if (block < 0 || block >= total) return 0;  // the piece begins at or behind the last block
    if (in == kSyncEnd) return kJpegMalformed;  // a piece in front needed a bit beyond the data
    long long pos = jpeg_sync_pos(in);
    int j = (int)(in >> 6) & 15, k = (int)in & 63;
    const int luma = F.hs * F.vs, per_mcu = F.comps == 3 ? luma + 2 : luma;
    if (j >= per_mcu) return kJpegMalformed;
    const int mcus = F.mx * F.my;
    int m = block / per_mcu;
    int pred[3] = {(int)pred_in[0], (int)pred_in[1], (int)pred_in[2]};
    JpegSyncBits bits;
    bits.open(d, len, pos);
    short* dst = coefs + (size_t)jpeg_sync_block_at(F, m, j) * 64;
    bool done = false;
    for (int step = 0; step < 8 * piece_bytes && pos < end_bit && !done; ++step) {
        const int c = j < luma ? 0 : j - luma + 1;
        if (k == 0) {
            const int s = jpeg_symbol(bits, tabs[2 * c]);
            if (s < 0 || s > 11) return kJpegMalformed;
            if (s) pred[c] = (int)((unsigned)pred[c] + (unsigned)jpeg_extend(bits.get(s), s));
            if (bits.over || pred[c] < -32768 || pred[c] > 32767) return kJpegMalformed;
            dst[0] = (short)pred[c];
            k = 1;
        } else {
            const int rs = jpeg_symbol(bits, tabs[2 * c + 1]);
            if (rs < 0) return kJpegMalformed;
            const int r = rs >> 4, s = rs & 15;
            if (s == 0) {
                k = r == 15 ? k + 16 : 64;
            } else {
                k += r;
                if (s > 10 || k > 63) return kJpegMalformed;
                dst[jpeg_natural(k)] = (short)jpeg_extend(bits.get(s), s);
                ++k;
            }
        }
        if (bits.over) return kJpegMalformed;
        if (k >= 64) {
            k = 0, ++block;
            if (++j == per_mcu) j = 0, ++m;
            if (block == total) done = true;
            else if (m >= mcus) return kJpegMalformed;  // j and the block index disagree: cannot happen in a verified chain
            else dst = coefs + (size_t)jpeg_sync_block_at(F, m, j) * 64;
        }
        pos = bits.at();
    }
    if (done) return bits.left_over() ? kJpegMalformed : 0;
    return last_piece ? kJpegMalformed : 0;  // the data ended in front of the last block
}

// The entropy stage of one file on the CPU, by the rules the launches follow: launch A (every group from its guess), launch B (every
// group from the exit of the group in front), the totals and the verification, then the strict walk of every piece -- or, for a
// file that is not verified, jpeg_decode_segment. A group's hand-over has one fixed point, the chain of its pieces from the group's
// input, so the CPU walks that chain once where the workgroup repeats rounds. info = mode, pieces, groups, 0. Returns the flag.
inline int jpeg_sync_entropy_host(const unsigned char* file, const JpegFile& F, const JpegSegment* segs, int piece_bytes, short* coefs, int* info) {
    info[0] = info[1] = info[2] = info[3] = 0;
    int flag = 0;
    if (F.interval) {  // mode 0: segment after segment
        for (int seg = 0; !flag && seg < F.nseg; ++seg) flag = jpeg_decode_segment(file, F, seg, segs[seg], coefs);
        return flag;
    }
    const unsigned char* d = file + F.scan_at;
    const int len = F.scan_end - F.scan_at;
    const long long pieces = jpeg_sync_pieces(len, piece_bytes), groups = jpeg_sync_groups(pieces);
    const int luma = F.hs * F.vs, per_mcu = F.comps == 3 ? luma + 2 : luma;
    JpegHuff* tabs = new JpegHuff[6];
    for (int slot = 0; slot < 2 * F.comps; ++slot) tabs[slot] = jpeg_sync_table(F, slot);
    JpegSyncPiece* piece = new JpegSyncPiece[pieces];
    JpegSyncGroup* group = new JpegSyncGroup[groups];
    for (int launch = 0; launch < 2; ++launch)
        for (long long g = 0; g < groups; ++g) {
            const long long first = g * kSyncGroup, last = first + kSyncGroup < pieces ? first + kSyncGroup : pieces;
            unsigned long long state = launch && g ? group[g - 1].exit_a : jpeg_sync_state(jpeg_sync_first_bit(d, len, first, piece_bytes), 0, 0);
            JpegSyncGroup sum{0ull, 0ull, 0, {0u, 0u, 0u}};
            for (long long u = first; u < last; ++u) {
                JpegSyncPiece& p = piece[u];
                int blocks;
                unsigned dc[3];
                p.in = state;
                p.out = state = jpeg_sync_piece(d, len, jpeg_sync_end_bit(len, u, piece_bytes), piece_bytes, state, tabs, luma, per_mcu, blocks, dc);
                p.blocks = sum.blocks, p.dc[0] = sum.dc[0], p.dc[1] = sum.dc[1], p.dc[2] = sum.dc[2];
                sum.blocks = (int)((unsigned)sum.blocks + (unsigned)blocks), sum.dc[0] += dc[0], sum.dc[1] += dc[1], sum.dc[2] += dc[2];
            }
            if (launch == 0) {
                group[g].exit_a = state;
            } else {
                group[g].exit_b = state, group[g].blocks = sum.blocks;
                group[g].dc[0] = sum.dc[0], group[g].dc[1] = sum.dc[1], group[g].dc[2] = sum.dc[2];
            }
        }
    bool verified = true;
    JpegSyncGroup before{0ull, 0ull, 0, {0u, 0u, 0u}};
    for (long long g = 0; g < groups; ++g) {
        verified = verified && group[g].exit_a == group[g].exit_b;
        const JpegSyncGroup own = group[g];
        group[g].blocks = before.blocks, group[g].dc[0] = before.dc[0], group[g].dc[1] = before.dc[1], group[g].dc[2] = before.dc[2];
        before.blocks = (int)((unsigned)before.blocks + (unsigned)own.blocks);
        before.dc[0] += own.dc[0], before.dc[1] += own.dc[1], before.dc[2] += own.dc[2];
    }
    info[0] = verified ? 1 : 2, info[1] = (int)pieces, info[2] = (int)groups;
    if (!verified) {
        flag = jpeg_decode_segment(file, F, 0, JpegSegment{F.scan_at, F.scan_end}, coefs);
    } else {
        const int total = jpeg_total_blocks(F);
        for (size_t i = 0; i < (size_t)total * 64; ++i) coefs[i] = 0;
        for (long long u = 0; u < pieces; ++u) {
            const JpegSyncGroup& g = group[u / kSyncGroup];
            const unsigned pred[3] = {g.dc[0] + piece[u].dc[0], g.dc[1] + piece[u].dc[1], g.dc[2] + piece[u].dc[2]};
            flag |= jpeg_sync_write_piece(d, len, jpeg_sync_end_bit(len, u, piece_bytes), piece_bytes, u == pieces - 1, piece[u].in, tabs, F,
                                          (int)((unsigned)g.blocks + (unsigned)piece[u].blocks), pred, coefs);
        }
    }
    delete[] tabs;
    delete[] piece;
    delete[] group;
    return flag;
}
}  // namespace dad3d
