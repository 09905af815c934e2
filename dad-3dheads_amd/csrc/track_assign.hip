// Detections into tracks, for gfx950 (MI355X): the edge where a caller's detector meets the tracker's slots, in ONE launch over state
// that stays on the device. Held word for word to its host statement (boxes.assign_detections; the rule is in include/dad3d.h), so
// the unit is built with -ffp-contract=off: `match_iou * double(union)` is one rounded product.
//
// assign_detections_kernel  One workgroup of 1024 lanes; lane t is detection t and slot t.
//   1. The live slots' boxes and frames are staged in LDS, a slot that is not live as the zero box, whose intersection with
//      anything is 0. The detections are NOT staged (see LDS below): a lane keeps its own detection in registers, and another lane
//      that needs it reads it again from global memory, where the 16 KiB of detections stay in the CU's vector L1.
//   2. All n * m pair tests are made in parallel into a bit matrix, pass[d] = {live s : same frame, inter > 0,
//      inter >= match_iou * union}, a row of 32 words per detection.
//   3. Best-first one-to-one matching, as rounds that give exactly the sorted walk of the rule: every unmatched detection knows its
//      best unmatched slot (the exact ratio, ties to the lower slot), every unmatched slot its best unmatched detection over ALL
//      unmatched detections (ties to the lower detection); mutual pairs are taken; until a round takes nothing. The globally best
//      remaining pair is always mutual, so every round with a passing pair takes one, and min(n, m) bounds the rounds (every box
//      identical in one frame: one pair a round). A lane's best stays its best while that partner is free -- the sets only shrink
//      -- so a lane looks again only after its partner went to somebody else. A look walks the set bits of (row & free slots), or
//      the free detections of a column, in ascending order, and stops at a ratio of exactly 1, which nothing later can beat.
//      Ratios are compared as inter_a * union_b against inter_b * union_a: in double first, where the two products differ by more
//      than their rounding can explain, otherwise as 128-bit integers.
//   4. Covered, spawned and full detections, retired slots and the spawned mask are two prefix sums (collectives.hpp) over the
//      lanes and per-lane stores. Every slot word is written by the lane of that slot, every detection word by the lane of that
//      detection, after the last read of the state: the launch is in place.
//   LDS, static, whatever n and m are (one workgroup either way): 1024 * 1024 / 8 bytes of pass bits, 16 KiB of slot boxes, 4 KiB
//   of slot frames, two lists of 1024 ints (a round's best detection per slot, then the free slots in order; the spawn candidates
//   in order), 2 * 32 words of free masks, 16 words for the scans and 2 for the rounds: 160 072 bytes of the CU's 163 840. Staging
//   the detections too would be 16 KiB more than there is.
#include "collectives.hpp"
#include "common.hpp"

namespace dad3d {
namespace {

constexpr int kThreads = 1024, kWaves = kThreads / 64, kWords = 32;
constexpr int kMissesMax = 1 << 30;
static_assert(DAD3D_TRACK_MAX_SLOTS == kThreads && DAD3D_TRACK_MAX_DETECTIONS == kThreads, "lane t is slot t and detection t");
static_assert(kWords * 32 == kThreads, "a row of pass bits is one 32-bit word per 32 slots");

struct Ratio {
    long long inter, uni;  // inter >= 0, uni > 0 where inter > 0
};

// the areas of the rule: int64 corners, so no int32 box overflows; a zero box (w == 0) gives inter == 0
__device__ __forceinline__ Ratio overlap(const int4& a, const int4& b) {
    const long long ax0 = a.x, ay0 = a.y, ax1 = ax0 + a.z, ay1 = ay0 + a.w, bx0 = b.x, by0 = b.y, bx1 = bx0 + b.z, by1 = by0 + b.w;
    const long long iw = min(ax1, bx1) - max(ax0, bx0), ih = min(ay1, by1) - max(ay0, by0);
    if (iw <= 0 || ih <= 0) return {0, 1};
    const long long inter = iw * ih;
    return {inter, (long long)a.z * a.w + (long long)b.z * b.w - inter};
}

// a.inter / a.uni > b.inter / b.uni, exactly. All four are in (0, 2^63).
__device__ __forceinline__ bool greater(const Ratio& a, const Ratio& b) {
#pragma clang fp contract(off)
    const double l = (double)a.inter * (double)b.uni, r = (double)b.inter * (double)a.uni;  // each within 2^-51 of its product
    if (l > r * (1.0 + 0x1p-40)) return true;
    if (r > l * (1.0 + 0x1p-40)) return false;
    const unsigned long long ai = a.inter, au = a.uni, bi = b.inter, bu = b.uni;
    const unsigned long long lh = __umul64hi(ai, bu), ll = ai * bu, rh = __umul64hi(bi, au), rl = bi * au;
    return lh != rh ? lh > rh : ll > rl;
}

__device__ __forceinline__ int4 load_box(const int32_t* boxes, int i) {
    const int32_t* b = boxes + (size_t)i * 4;
    return make_int4(b[0], b[1], b[2], b[3]);
}

__device__ __forceinline__ void store_box(int32_t* boxes, int i, const int4& v) {
    int32_t* b = boxes + (size_t)i * 4;
    b[0] = v.x, b[1] = v.y, b[2] = v.z, b[3] = v.w;
}

__global__ __launch_bounds__(kThreads) void assign_detections_kernel(AssignDetectionsArgs a) {
#pragma clang fp contract(off)
    __shared__ unsigned pass[kThreads * kWords];
    __shared__ int4 sbox[kThreads];  // (x, y, w, h); all zero for a slot that is not live
    __shared__ int sframe[kThreads];
    __shared__ int list_a[kThreads];  // in the rounds: a slot's best detection; after them: the free slots, ascending
    __shared__ int list_b[kThreads];  // the spawn candidates, ascending
    __shared__ unsigned sfree[kWords], dfree[kWords];  // live slots / valid detections that no pair has taken
    __shared__ int red[kWaves];
    __shared__ int took_any[2];  // did round r take a pair: word r & 1, cleared by lane 0 during round r - 1
    const int t = threadIdx.x, lane = t & 63, n = a.n, m = a.m;
    const int swords = (n + 31) >> 5, dwords = (m + 31) >> 5;
    int count = m;
    if (a.det_count) count = min(max(*a.det_count, 0), m);

    // 1. this lane's slot and this lane's detection
    int4 my_slot = make_int4(0, 0, 0, 0);
    int my_frame = -1, my_flags = 0;
    if (t < n) my_slot = load_box(a.boxes, t), my_frame = a.image_index[t], my_flags = a.flags[t];
    const bool live = t < n && my_flags == 0 && my_slot.z > 0 && my_slot.w > 0;  // as it stands at entry
    sbox[t] = live ? my_slot : make_int4(0, 0, 0, 0);
    sframe[t] = my_frame;
    int4 my_det = make_int4(0, 0, 0, 0);
    int my_det_frame = -1;
    if (t < count) my_det = load_box(a.det_boxes, t), my_det_frame = a.det_index[t];
    const bool valid = t < count && my_det.z > 0 && my_det.w > 0 && my_det_frame >= 0 && my_det_frame < a.n_frames;
    {
        const unsigned long long sl = __ballot(live), dv = __ballot(valid);
        if (lane == 0) {
            sfree[t >> 5] = (unsigned)sl, sfree[(t >> 5) + 1] = (unsigned)(sl >> 32);
            dfree[t >> 5] = (unsigned)dv, dfree[(t >> 5) + 1] = (unsigned)(dv >> 32);
        }
        if (t == 0) took_any[0] = 0;
    }
    __syncthreads();

    // 2. the pass bits: one word (a detection against 32 slots) per trip
    for (int k = t; k < m * swords; k += kThreads) {
        const int d = k / swords, w = k - d * swords;
        unsigned word = 0;
        if (d < count) {
            const int4 bd = load_box(a.det_boxes, d);
            const int fd = a.det_index[d];
            if (bd.z > 0 && bd.w > 0 && fd >= 0 && fd < a.n_frames) {
                for (int i = 0; i < 32; ++i) {
                    const int s = w * 32 + i;
                    if (sframe[s] != fd) continue;
                    const Ratio r = overlap(bd, sbox[s]);
                    if (r.inter > 0 && (double)r.inter >= a.match_iou * (double)r.uni) word |= 1u << i;  // one product, no division
                }
            }
        }
        pass[d * kWords + w] = word;
    }
    __syncthreads();

    // 3. the rounds
    bool det_open = valid, slot_open = live;  // not taken yet
    bool det_look = valid, slot_look = live;  // the kept best went to somebody else (or there is none yet)
    int det_best = -1, slot_best = -1;
    for (int round = 0;; ++round) {
        if (det_open && det_look) {
            det_best = -1;
            Ratio best{0, 1};
            bool done = false;
            for (int w = 0; w < swords && !done; ++w) {
                unsigned bits = pass[t * kWords + w] & sfree[w];
                while (bits) {
                    const int s = w * 32 + __ffs(bits) - 1;
                    bits &= bits - 1;
                    const Ratio r = overlap(my_det, sbox[s]);
                    if (det_best < 0 || greater(r, best)) det_best = s, best = r;  // strictly: a tie stays with the lower slot
                    if (r.inter == r.uni) {  // the ratio 1: no later slot is better, and an equal one is higher
                        done = true;
                        break;
                    }
                }
            }
            det_look = false;
        }
        if (slot_open && slot_look) {
            slot_best = -1;
            Ratio best{0, 1};
            bool done = false;
            for (int w = 0; w < dwords && !done; ++w) {
                unsigned bits = dfree[w];
                while (bits) {
                    const int d = w * 32 + __ffs(bits) - 1;
                    bits &= bits - 1;
                    if (!(pass[d * kWords + (t >> 5)] >> (t & 31) & 1)) continue;
                    const Ratio r = overlap(load_box(a.det_boxes, d), my_slot);
                    if (slot_best < 0 || greater(r, best)) slot_best = d, best = r;  // a tie stays with the lower detection
                    if (r.inter == r.uni) {
                        done = true;
                        break;
                    }
                }
            }
            slot_look = false;
        }
        list_a[t] = slot_open ? slot_best : -1;
        __syncthreads();
        if (t == 0) took_any[(round + 1) & 1] = 0;  // last read in front of this barrier, next written behind the next round's
        const bool took = det_open && det_best >= 0 && list_a[det_best] == t;
        if (took) {
            took_any[round & 1] = 1;
            atomicAnd(&dfree[t >> 5], ~(1u << (t & 31)));
            atomicAnd(&sfree[det_best >> 5], ~(1u << (det_best & 31)));
            det_open = false;
        }
        __syncthreads();
        if (!took_any[round & 1]) break;
        if (slot_open && !(sfree[t >> 5] >> (t & 31) & 1)) slot_open = false;  // taken by slot_best: the pair was mutual
        if (det_open && det_best >= 0) det_look = !(sfree[det_best >> 5] >> (det_best & 31) & 1);
        if (slot_open && slot_best >= 0) slot_look = !(dfree[slot_best >> 5] >> (slot_best & 31) & 1);
    }
    const bool det_matched = valid && !det_open, slot_matched = live && !slot_open;

    // 4. the rest: covered, spawned, full; retired; the spawned mask
    bool covered = false;
    if (valid && !det_matched)
        for (int w = 0; w < swords; ++w) covered |= pass[t * kWords + w] != 0;
    const bool candidate = valid && !det_matched && !covered, vacant = t < n && !live;
    int n_candidates, n_vacant;
    const int cand_rank = block_exclusive_scan<kWaves>(candidate ? 1 : 0, red, n_candidates);
    const int vacant_rank = block_exclusive_scan<kWaves>(vacant ? 1 : 0, red, n_vacant);
    if (vacant) list_a[vacant_rank] = t;  // the last read of list_a stands in front of the scans' barriers
    if (candidate) list_b[cand_rank] = t;
    __syncthreads();

    if (t < m) {
        int to = -1, how = 0;
        if (t >= count) how = DAD3D_ASSIGN_FLAG_PADDING;
        else if (!valid) how = DAD3D_ASSIGN_FLAG_INVALID;
        else if (det_matched) to = det_best;
        else if (covered) how = DAD3D_ASSIGN_FLAG_COVERED;
        else if (cand_rank < n_vacant) to = list_a[cand_rank], how = DAD3D_ASSIGN_FLAG_SPAWNED;
        else how = DAD3D_ASSIGN_FLAG_FULL;
        a.assign[t] = to, a.det_flags[t] = how;
    }
    if (t >= n) return;
    int spawned = 0;
    if (vacant) {
        if (vacant_rank < n_candidates) {  // free at entry: the candidate of the same rank comes here
            const int d = list_b[vacant_rank];
            store_box(a.boxes, t, load_box(a.det_boxes, d));
            a.image_index[t] = a.det_index[d];
            a.flags[t] = 0;
            if (a.misses) a.misses[t] = 0;
            spawned = 1;
        }
    } else if (slot_matched) {
        if (a.misses) a.misses[t] = 0;
        if (a.refresh) store_box(a.boxes, t, load_box(a.det_boxes, slot_best));
    } else if (a.misses) {  // live and unconfirmed; without a counter there is nothing to count and nothing retires
        const bool searched = !a.frame_searched || (my_frame >= 0 && my_frame < a.n_frames && a.frame_searched[my_frame] != 0);
        if (searched) {
            const int seen = a.misses[t], now = seen >= kMissesMax ? kMissesMax : seen + 1;
            a.misses[t] = now;
            if (a.max_misses >= 0 && now > a.max_misses) {
                a.flags[t] = DAD3D_TRACK_FLAG_RETIRED;
                store_box(a.boxes, t, make_int4(0, 0, 0, 0));
            }
        }
    }
    a.spawned[t] = spawned;
}

}  // namespace

dad3d_status launch_assign_detections(const AssignDetectionsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(assign_detections_kernel, dim3(1), dim3(kThreads), 0, s, a);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

}  // namespace dad3d
