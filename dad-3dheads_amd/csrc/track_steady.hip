// Steady tracks, for gfx950 (MI355X): the two per-slot rules a video loop needs on top of track_boxes.hip, each ONE launch over
// state that stays on the device. Both are held bit for bit to their host statements (steady.one_euro_rows, boxes.suppress_duplicates),
// so the unit is built with -ffp-contract=off and every operation below rounds once.
//
// one_euro_rows_kernel  A One-Euro filter (Casiez et al. 2012) over the rows of a float32 matrix [N,D]. One wave per row, four rows
//   per 256-lane workgroup. A row's fate depends on all of its elements (a NaN anywhere, an overflow anywhere), so a wave makes two
//   passes over its row: the first computes what the second would write and keeps only two bits, ONE wave_reduce of
//   collectives.hpp (or) gives them to every lane, and the second pass writes. A lane reads and writes the same elements in both
//   passes, so `out == x` needs nothing more. No LDS, no barrier, no atomics.
//
// suppress_duplicates_kernel  Greedy suppression of slots that converged on one head. One workgroup of 1024 lanes. The rule is
//   sequential (slot j is a duplicate of a KEPT earlier slot), but the pair tests are not: all N^2/2 of them are made in parallel
//   into a bit matrix in LDS, conflict[j] = {i < j : same frame, inter > 0, inter >= merge_iou * union}; after one barrier the
//   first wave walks j upward holding the kept slots as one 32-bit word in each of its first 32 lanes, and a slot is a duplicate if
//   the ballot of (conflict[j][lane] & kept[lane]) is not empty; bit j of conflict[j], which no pair uses, says that slot j takes
//   part. The next row is read while this one is decided, and there is no barrier in the walk. The boxes are staged once in LDS
//   with a slot that takes no part (flagged, or a side <= 0) as the zero box, whose intersection with anything is 0. LDS:
//   1024 * 1024 / 8 bytes of bits, 16 KiB of boxes and 4 KiB of frame numbers of the CU's 160 KiB, which is where
//   DAD3D_TRACK_MAX_SLOTS comes from. The allocation is static: a launch of 64 slots reserves the same 151 552 bytes (it is one
//   workgroup either way, and only the first n rows of ceil(n / 32) words are touched).
#include "collectives.hpp"
#include "common.hpp"

namespace dad3d {
namespace {

constexpr int kEuroThreads = 256, kEuroRows = kEuroThreads / 64;
constexpr int kAgeMax = 1 << 30;
constexpr int kBitInput = 1, kBitOverflow = 2;

struct OpOr {
    template <typename T>
    __device__ static __forceinline__ T of(T a, T b) { return a | b; }
};

__device__ __forceinline__ bool finite32(float v) { return fabsf(v) < __builtin_inff(); }  // a NaN compares false

// rule 4 of include/dad3d.h on one element: every operation once, in this order
__device__ __forceinline__ void one_euro(const OneEuroArgs& a, float x, float xp, float dxp, float mc, float beta, float& out, float& dxh) {
#pragma clang fp contract(off)
    const float dx = (x - xp) * a.rate;
    dxh = dxp + a.alpha_d * (dx - dxp);
    const float fc = mc + beta * fabsf(dxh);
    const float r = a.two_pi_dt * fc;
    const float al = r / (r + 1.0f);
    out = xp + al * (x - xp);
}

__global__ __launch_bounds__(kEuroThreads) void one_euro_rows_kernel(OneEuroArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * kEuroRows + (threadIdx.x >> 6);
    if (row >= a.n) return;  // the whole wave: nothing below meets another wave
    const float* x = a.x + row * a.x_stride;
    float* out = a.out + row * a.out_stride;
    float* sx = a.state_x + row * a.d;
    float* sdx = a.state_dx + row * a.d;
    const int age = a.age[row];
    const bool flagged = a.flags && a.flags[row] != 0, first = age <= 0;
    int bits = 0;
    if (!flagged) {
        for (int d = lane; d < a.d; d += 64) {
            const float v = x[d];
            if (!finite32(v)) {
                bits |= kBitInput;
            } else if (!first) {
                float o, dxh;
                one_euro(a, v, sx[d], sdx[d], a.min_cutoff[d], a.beta[d], o, dxh);
                if (!finite32(o) || !finite32(dxh)) bits |= kBitOverflow;
            }
        }
        bits = wave_reduce<OpOr>(bits);
    }
    if (flagged || (bits & kBitInput)) {  // rules 1 and 2: the values pass, the track restarts, the state stays
        if (out != x)
            for (int d = lane; d < a.d; d += 64) out[d] = x[d];
        if (lane == 0) a.age[row] = 0;
        return;
    }
    if (first || (bits & kBitOverflow)) {  // rules 3 and 5
        for (int d = lane; d < a.d; d += 64) {
            const float v = x[d];
            out[d] = v, sx[d] = v, sdx[d] = 0.0f;
        }
        if (lane == 0) a.age[row] = 1;
        return;
    }
    for (int d = lane; d < a.d; d += 64) {  // rule 4, the bits of the first pass again
        float o, dxh;
        one_euro(a, x[d], sx[d], sdx[d], a.min_cutoff[d], a.beta[d], o, dxh);
        out[d] = o, sx[d] = o, sdx[d] = dxh;
    }
    if (lane == 0) a.age[row] = age >= kAgeMax ? kAgeMax : age + 1;
}

constexpr int kDupThreads = 1024, kDupWords = DAD3D_TRACK_MAX_SLOTS / 32;
static_assert(DAD3D_TRACK_MAX_SLOTS == 32 * 32, "the resolving wave keeps one 32-bit word of kept slots in each of 32 lanes");

__global__ __launch_bounds__(kDupThreads) void suppress_duplicates_kernel(SuppressDuplicatesArgs a) {
#pragma clang fp contract(off)
    __shared__ unsigned conflict[DAD3D_TRACK_MAX_SLOTS * kDupWords];
    __shared__ int4 box[DAD3D_TRACK_MAX_SLOTS];  // (x, y, w, h); all zero for a slot that takes no part
    __shared__ int frame[DAD3D_TRACK_MAX_SLOTS];
    const int t = threadIdx.x, n = a.n, words = (n + 31) >> 5;
    for (int i = t; i < n; i += kDupThreads) {
        const int32_t* b = a.boxes + (size_t)i * 4;
        const bool part = a.flags[i] == 0 && b[2] > 0 && b[3] > 0;
        box[i] = part ? make_int4(b[0], b[1], b[2], b[3]) : make_int4(0, 0, 0, 0);
        frame[i] = a.image_index[i];
    }
    __syncthreads();
    for (int k = t; k < n * words; k += kDupThreads) {
        const int j = k / words, w = k - j * words;
        const int4 bj = box[j];
        const int fj = frame[j];
        const long long jx0 = bj.x, jy0 = bj.y, jx1 = jx0 + bj.z, jy1 = jy0 + bj.w, area_j = (long long)bj.z * bj.w;
        unsigned word = (j >> 5) == w && bj.z > 0 ? 1u << (j & 31) : 0u;  // the diagonal, which no pair uses: slot j takes part
        const int end = min(w * 32 + 32, j);  // only earlier slots
        for (int i = w * 32; i < end; ++i) {
            if (frame[i] != fj) continue;
            const int4 bi = box[i];
            const long long ix0 = bi.x, iy0 = bi.y, ix1 = ix0 + bi.z, iy1 = iy0 + bi.w;
            const long long iw = min(ix1, jx1) - max(ix0, jx0), ih = min(iy1, jy1) - max(iy0, jy0);
            if (iw <= 0 || ih <= 0) continue;  // inter == 0 is never a duplicate; most pairs end here
            const long long inter = iw * ih, uni = (long long)bi.z * bi.w + area_j - inter;
            if ((double)inter >= a.merge_iou * (double)uni) word |= 1u << (i & 31);  // one product, no division
        }
        conflict[j * kDupWords + w] = word;
    }
    __syncthreads();
    if (t >= 64) return;
    // the first wave, in slot order; lane l < 32 holds the kept slots 32 l .. 32 l + 31
    unsigned kept = 0;
    unsigned next = t < words ? conflict[t] : 0u;
    for (int j = 0; j < n; ++j) {
        const unsigned row = next;
        if (j + 1 < n) next = t < words ? conflict[(j + 1) * kDupWords + t] : 0u;  // does not depend on this slot's fate
        const bool dup = __ballot((row & kept) != 0) != 0;  // kept holds earlier slots only, so the diagonal bit does not meet it
        if (!dup && t == (j >> 5)) kept |= row & (1u << (j & 31));
    }
    for (int base = 0; base < n; base += 64) {  // every lane makes every trip: the shuffle reads lanes that must still be here
        const int j = base + t;
        const unsigned word = __shfl(kept, (j >> 5) & 31, 64);
        if (j < n && box[j].z > 0 && !(word >> (j & 31) & 1)) {
            int32_t* b = a.boxes + (size_t)j * 4;
            b[0] = 0, b[1] = 0, b[2] = 0, b[3] = 0;
            a.flags[j] = DAD3D_TRACK_FLAG_DUPLICATE;
        }
    }
}

}  // namespace

dad3d_status launch_one_euro_rows(const OneEuroArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(one_euro_rows_kernel, dim3((unsigned)(((long long)a.n + kEuroRows - 1) / kEuroRows)), dim3(kEuroThreads), 0, s, a);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

dad3d_status launch_suppress_duplicates(const SuppressDuplicatesArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(suppress_duplicates_kernel, dim3(1), dim3(kDupThreads), 0, s, a);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

}  // namespace dad3d
