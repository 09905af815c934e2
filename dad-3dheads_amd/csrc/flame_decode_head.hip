// FLAME / HeadMesh decode for gfx950 (MI355X): whole-mesh launches of 33..64 images, "48 + 16".
//
// The pipelined kernel (flame_decode_pipe.hip) multiplies such a launch as two half-blocks of 32 images. Its first GEMM runs at the pace
// of the basis stream (104 KB per CU, over ~13 k cycles after the launch whenever the requests go out) with the matrix pipe a third idle,
// and the second half-block is ~9 k cycles of pure matrix-pipe work behind the stream. Here the SAME arithmetic is cut differently:
//
//   pass 1  rows 0..47 as THREE row blocks of 16 images against each basis group as it lands: 12 MFMAs per group instead of 8 under the
//           stream. The basis requests are an issue-ahead ring: DAD3D_HEAD_DEPTH of them up front, then one per k-group between the MFMAs,
//           so the first MFMA waits for group 0 and not for 26 issues, and a stager's request never stands behind the whole slice.
//           A step's request and its LDS reads of the next A fragments stand BETWEEN the step's MFMAs: a wave issues in order, in one
//           clump in front of the step they cost ~50 cycles of matrix pipe a step, which is what looked like a wait for the stream.
//           The stagers ask for slab 0 (k 0..127) of the 48 rows in front of the start-up barrier and for the rest behind it.
//   pass 2  (B > 48) rows 48..63 as ONE row block, a chain of 104 dependent MFMAs. Rows 0..31 are finished in its hooks by the mma waves
//           (the pipelined kernel's hook layout and its first two pieces), rows 32..47 and vertices 16..19 of rows 0..31 (the half-empty
//           third piece) by the stagers, which have nothing else to do -- in two calls: vertices 0..15 of rows 32..47, then vertices
//           16..19 of rows 0..47 as ONE call of 48 lanes, so that the stagers are not the late party at barrier P2. Multiplying part of
//           this chain inside pass 1 was measured and loses (profiles/r11_kernel_log.md); so does starting it without barrier P1, on
//           arrival words, with the park and the hook set-up between its first MFMAs (profiles/r12_kernel_log.md).
//   tail    all eight waves finish rows 48..63 -- or rows 0..47 when B <= 48: there is no pass 2 then. B > 48: what the tail does not get
//           from the chain (constants, vertex-table row, masks, offsets) is read in front of barrier P2, by the mma waves inside the
//           chain's last groups and by the stagers in front of their two calls; behind P2 it reads the jaw and three accumulator values.
//
// Every accumulator sums G = 0..25, s = 0..3 from zero and every (vertex, image) goes through finish_vertex (flame_pipe_epilogue.hpp) with
// the constants of write_round below, which is flame_decode_pipe.hip's: a row's bits do not depend on the kernel, the pass or the wave that
// finishes it (tests/test_gpu_decode_head.py). Same argument list (fourteen preloaded dwords + one struct behind them), same LDS layout,
// same trace slots as the pipelined kernel; capi.cpp sends a launch here. The small device helpers are copies: the pipelined unit's three
// kernels are held to their instruction streams (tests/test_decode_pipe_entry.py), so nothing of theirs moved into a header.
#pragma clang fp contract(off)
#include <type_traits>

#include "common.hpp"
#include "flame_math.hpp"
#include "flame_pipe_epilogue.hpp"

#ifndef DAD3D_HEAD_DEPTH   // basis requests in flight ahead of the GEMM, per mma wave (4 KB per CU each). 26 = all of them up front, the
#define DAD3D_HEAD_DEPTH 6  // pipelined kernel's order. 6 / 8 / 10 tie at B <= 48, 12 and more lose 0.1-0.4 us at B > 48; not below 6: ~15 KB per CU
#endif                      // in flight is what the stream's rate needs (profiles/r10_kernel_log.md section 2)
#ifndef DAD3D_HEAD_R0_AT   // constants round 0 sits behind this one of the up-front basis requests (flame_decode_pipe.hip: DAD3D_PIPE_R0_AT);
#define DAD3D_HEAD_R0_AT 1  // behind the last of them: 0.05-0.2 us slower at every size
#endif

#ifndef DAD3D_HEAD_SPREAD  // 1: pass 1 issues a step's basis request and LDS reads between its MFMAs; 0: all in front of the step's first MFMA
#define DAD3D_HEAD_SPREAD 1
#endif
#ifndef DAD3D_HEAD_SPREAD_REQ_AT  // the MFMA row (s = 0..3, three MFMAs each) behind which the request goes: 2 never lost, 0 and 1 read 0.05-0.1 us slower
#define DAD3D_HEAD_SPREAD_REQ_AT 2
#endif
#ifndef DAD3D_HEAD_SPREAD_LDS_AT  // ... and the three LDS reads go; 4: one read behind each MFMA of row 0 (0.03-0.1 us better than all behind row 0 at 49..64)
#define DAD3D_HEAD_SPREAD_LDS_AT 4
#endif
#ifndef DAD3D_HEAD_V16_STAGERS  // 1: vertices 16..19 of rows 0..31 (B > 48) are finished by the stagers, which wait at P2, not in the chain's last hook
#define DAD3D_HEAD_V16_STAGERS 1
#endif
#ifndef DAD3D_HEAD_V16_MERGED  // 1: the stagers' two mostly empty calls (vertices 16..19 of rows 32..47 and of rows 0..31) are ONE call of 48 lanes
#define DAD3D_HEAD_V16_MERGED 1
#endif
#ifndef DAD3D_HEAD_TAIL_PRE  // 1 (B > 48): the tail's constants, vertex-table row, masks and offsets are read in front of barrier P2, by both roles
#define DAD3D_HEAD_TAIL_PRE 1
#endif
#ifndef DAD3D_HEAD_TAIL_PRE_AT  // ... by the mma waves behind this group of the chain (in front of barrier P1, where they wait, ties: profiles/r12_kernel_log.md)
#define DAD3D_HEAD_TAIL_PRE_AT 22
#endif

namespace dad3d {

namespace {

using namespace pipe;
constexpr bool kSpread = DAD3D_HEAD_SPREAD != 0;
constexpr int kSpreadReqAt = DAD3D_HEAD_SPREAD_REQ_AT, kSpreadLdsAt = DAD3D_HEAD_SPREAD_LDS_AT;
constexpr bool kV16Stagers = DAD3D_HEAD_V16_STAGERS != 0;
static_assert(kSpreadReqAt >= 0 && kSpreadReqAt < 4 && kSpreadLdsAt >= 0 && kSpreadLdsAt <= 4, "rows of a step's MFMAs");
constexpr bool kV16Merged = DAD3D_HEAD_V16_STAGERS != 0 && DAD3D_HEAD_V16_MERGED != 0;
constexpr bool kTailPre = DAD3D_HEAD_TAIL_PRE != 0;
constexpr int kTailPreAt = DAD3D_HEAD_TAIL_PRE_AT;
static_assert(kTailPreAt >= 0 && kTailPreAt < 26, "a group of the chain");

constexpr int KG = kPipeKGroups;       // MFMA groups of 16 k
constexpr int TV = kPipeTileVerts;     // vertices per tile
constexpr int kNumBeta = 400;
constexpr int kJawCol = 3 * TV;        // columns 60..62 of a tile: the jaw joint
constexpr int LD = 424;                // A image row stride (floats), as in flame_decode_pipe.hip
constexpr int OS = 76;                 // accumulator tile row stride
constexpr int CS = 24;                 // per-image constants: D 9 | G 9 | s tx ty | 3 pad
constexpr int kRows = 64;              // rows of the A image and of the accumulator tile
constexpr int kRows1 = 48;             // rows of pass 1
constexpr int kRound = 128;            // images per constants round (one round here: the ring's second half stays unused)
constexpr int D = DAD3D_HEAD_DEPTH < KG ? DAD3D_HEAD_DEPTH : KG;
static_assert(D >= 6 && DAD3D_HEAD_R0_AT < D, "issue-ahead depth");
struct Lds {  // flame_decode_pipe.hip's layout and size: its two A images and two accumulator tiles are one of 64 rows each here
    static constexpr int a_off = 0;                          // [64][LD]         params rows
    static constexpr int o_off = a_off + kRows * LD;         // [64][OS]         accumulators
    static constexpr int c_off = o_off + kRows * OS;         // [2][kRound][CS]  per-image constants
    static constexpr int y_off = c_off + 2 * kRound * CS;    // [4] arrival words
    static constexpr int v_off = y_off + 4;                  // [TV] float4: the tile's rows of the vertex table
    static constexpr int total = v_off + 4 * TV;
    static_assert(total * 4 <= 160 * 1024, "LDS budget of one CU");
};

__device__ __forceinline__ int lds_peek(lds_int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void wait_ge(lds_int* p, int target) {
    while (lds_peek(p) < target) __builtin_amdgcn_s_sleep(1);
    asm volatile("" ::: "memory");  // the LDS reads this wait guards stay behind it (a wave's LDS operations execute in order)
}
__device__ __forceinline__ void wait_ge2(lds_int* p, int target, lds_int* q, int target_q) {
    while ((int)(lds_peek(p) < target) | (int)(lds_peek(q) < target_q)) __builtin_amdgcn_s_sleep(1);
    asm volatile("" ::: "memory");
}
__device__ __forceinline__ void arrive(lds_int* p, int lane) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's LDS writes have completed
    if (lane == 0) __hip_atomic_fetch_add(p, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// workgroup barrier that does not drain the wave's outstanding global loads / stores
__device__ __forceinline__ void phase_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

}  // namespace

// Barriers (every wave executes the same ones; B is launch-uniform): start-up | P1: pass 1 is parked, rows 48..63 and the vertex table are
// in LDS | P2 (B > 48 only): pass 2 is parked. Arrival words inside pass 1: parts + 0 .. 2 = slab 0, 1, 2 of rows 0..47 are in LDS (the
// third counts the four stagers and mma waves 0 and 1, which write k = 400..415 of all 64 rows), parts + 3 = constants round 0 is in LDS.
constexpr int kHeadPreloadDwords = 14;  // params 2 | bpack 2 | vtab 2 | trace 2 | batch | n_verts | n_params | span_half | geom | n_lmk
static_assert(4 * kHeadPreloadDwords == 4 * sizeof(void*) + 6 * sizeof(int), "the preloaded range ends with n_lmk");
struct PipeLateArgs {  // the arguments behind the preloaded range -- the same struct as flame_decode_pipe.hip's, member for member
    const int* lmk_next;
    float *verts3d, *proj, *lmk_xy;
    int32_t* lmk_px;
    float image_size;
};
static_assert((4 * kHeadPreloadDwords) % alignof(PipeLateArgs) == 0, "`late` starts where the preloaded range ends: late_args() reads it there");
template <bool TO2D>
__global__ __launch_bounds__(512, 2) void flame_decode_head_kernel(float* params, const float* bpack, const float4* vtab, unsigned long long* trace_buf, int batch,
                                                                   int n_verts, int n_params, int span_half, unsigned geom, int n_lmk, PipeLateArgs late) {
    PipeArgs a;
    a.params = params, a.bpack = bpack, a.vtab = vtab, a.trace = trace_buf, a.n_params = n_params, a.batch = batch, a.n_half = span_half, a.n_verts = n_verts, a.n_lmk = n_lmk;
    a.flags = pipe_geom_unpack(geom).flags;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* abuf = smem + Lds::a_off;
    float* otile = smem + Lds::o_off;
    float* cst = smem + Lds::c_off;
    lds_int* parts = (lds_int*)(smem + Lds::y_off);

    // (`wave` stays a per-lane value: the role split is an exec-mask branch, as in flame_decode_pipe.hip)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x, v0 = tile * TV;
    const int B = a.batch, P = a.n_params;
    const bool two = B > kRows1;  // there is a pass 2
    unsigned long long* trace = a.trace ? a.trace + ((size_t)tile * 8 + wave) * 32 : nullptr;
    auto stamp = [&](int slot) {
        if (trace && lane == 0) trace[slot] = __builtin_readcyclecounter();
    };
    if (trace && lane == 0) trace[12] = wall_clock64();
    stamp(0);
    if (tid < 4) __hip_atomic_store(parts + tid, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    const unsigned nl = (unsigned)a.n_lmk;
    // the arguments behind the preloaded range, once per role and where the role waits anyway (flame_decode_pipe.hip, late_args)
    EpiCtx cx;
    __amdgpu_buffer_rsrc_t rs3, rsp;
    unsigned outs = 0;
    auto late_args = [&]() {
        typedef const __attribute__((address_space(4))) char* kernarg_ptr;
        typedef const __attribute__((address_space(4))) PipeLateArgs* late_ptr;
        kernarg_ptr kp = (kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(kp));
        const late_ptr lp = reinterpret_cast<late_ptr>(kp + 4 * kHeadPreloadDwords);
        a.lmk_next = lp->lmk_next, a.verts3d = lp->verts3d, a.proj = lp->proj, a.lmk_xy = lp->lmk_xy, a.lmk_px = lp->lmk_px, a.image_size = lp->image_size;
        rs3 = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<char*>(a.verts3d), 0, 0x7fffffff, 0x00020000);
        rsp = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<char*>(a.proj), 0, 0x7fffffff, 0x00020000);
        cx.lx = reinterpret_cast<char*>(a.lmk_xy), cx.lp = reinterpret_cast<char*>(a.lmk_px);
        outs = __builtin_amdgcn_readfirstlane((a.verts3d ? 1u : 0u) | (a.proj ? 2u : 0u));
        asm volatile("" : "+s"(outs));
        cx.lmk_next = a.lmk_next;
        cx.image_size = a.image_size;
    };
    cx.zsign = (a.flags & DAD3D_FLIP_Z) ? -1.0f : 1.0f;
    float4* const vt_lds = reinterpret_cast<float4*>(smem + Lds::v_off);
    // Rows finished outside a GEMM, out of the accumulator tile, the constants ring and the vertex table in LDS. fin4: flame_decode_pipe.hip's
    // final_epilogue -- wave w of a set takes rows row0 + 4 w .. + 3, lane = (row fi of four, vertex fu of sixteen) -> vertices fu and, for
    // fu < 4, fu + 16. fin2: all eight waves on sixteen rows -- rows row0 + 2 wave + {0, 1}, lane = (row fi of two, vertex fu of 32), one
    // vertex a lane.
    auto fin4 = [&](int row0, int w, auto both) {  // both: std::false_type = vertices 0..15 only
        const int fi = lane & 3, fu = lane >> 2, b = row0 + 4 * w + fi;
        const float4* cp = reinterpret_cast<const float4*>(cst + b * CS);
        const float4 c0 = cp[0], c1 = cp[1], c2 = cp[2], c3 = cp[3], c4 = cp[4], c5 = cp[5];
        const float* ot = otile + b * OS;
        const float jx = ot[kJawCol], jy = ot[kJawCol + 1], jz = ot[kJawCol + 2];
        const unsigned vrow = (unsigned)b * (unsigned)a.n_verts + (unsigned)(v0 + fu), bnl = (unsigned)b * nl;
        {
            const float4 t = vt_lds[fu];
            const bool live = b < B && v0 + fu < a.n_verts;
            finish_vertex<TO2D, 0>(cx, rs3, rsp, c0, c1, c2, c3, c4, c5, jx, jy, jz, ot[3 * fu], ot[3 * fu + 1], ot[3 * fu + 2], t.x, t.y, __float_as_int(t.z), __float_as_int(t.w),
                                   live && (outs & 1u), live && (outs & 2u), live && nl > 0 && __float_as_int(t.z) >= 0, vrow, bnl);
        }
        if (decltype(both)::value && fu < TV - 16) {
            const int j = fu + 16;
            const float4 t = vt_lds[j];
            const bool live = b < B && v0 + j < a.n_verts;
            finish_vertex<TO2D, 16>(cx, rs3, rsp, c0, c1, c2, c3, c4, c5, jx, jy, jz, ot[3 * j], ot[3 * j + 1], ot[3 * j + 2], t.x, t.y, __float_as_int(t.z), __float_as_int(t.w),
                                    live && (outs & 1u), live && (outs & 2u), live && nl > 0 && __float_as_int(t.z) >= 0, vrow, bnl);
        }
    };
    // fin_v16: vertices 16..19 of rows 8 w .. 8 w + 7, lanes 0..31 = (row of eight, vertex of four): the hooks' third piece
    auto fin_v16 = [&](int w) {
        const int fu = (lane >> 3) & 3, j = fu + 16, b = 8 * w + (lane & 7);
        const float4* cp = reinterpret_cast<const float4*>(cst + b * CS);
        const float4 c0 = cp[0], c1 = cp[1], c2 = cp[2], c3 = cp[3], c4 = cp[4], c5 = cp[5];
        const float* ot = otile + b * OS;
        const float jx = ot[kJawCol], jy = ot[kJawCol + 1], jz = ot[kJawCol + 2];
        const unsigned vrow = (unsigned)b * (unsigned)a.n_verts + (unsigned)(v0 + fu), bnl = (unsigned)b * nl;
        const float4 t = vt_lds[j];
        const bool live = lane < 32 && v0 + j < a.n_verts;  // (b < 32 < B)
        finish_vertex<TO2D, 16>(cx, rs3, rsp, c0, c1, c2, c3, c4, c5, jx, jy, jz, ot[3 * j], ot[3 * j + 1], ot[3 * j + 2], t.x, t.y, __float_as_int(t.z), __float_as_int(t.w),
                                live && (outs & 1u), live && (outs & 2u), live && nl > 0 && __float_as_int(t.z) >= 0, vrow, bnl);
    };
    // fin_v16_both (kV16Merged): that piece and fin4(32, w)'s second one in ONE call of 48 lanes -- lanes 0..31 as in fin_v16, lanes 32..47 =
    // (row 32 + 4 w + (lane & 3), vertex 16 + ((lane >> 2) & 3)), fin4's lanes 0..15. Constants, jaw and accumulators are per lane: the same
    // pairs with the same arithmetic, two calls beside the chain instead of three. (Lanes 48..63 compute lanes 32..47's pairs and store nothing.)
    auto fin_v16_both = [&](int w) {
        const bool hi = lane >= 32;
        const int fu = hi ? (lane >> 2) & 3 : (lane >> 3) & 3, j = fu + 16, b = hi ? 32 + 4 * w + (lane & 3) : 8 * w + (lane & 7);
        const float4* cp = reinterpret_cast<const float4*>(cst + b * CS);
        const float4 c0 = cp[0], c1 = cp[1], c2 = cp[2], c3 = cp[3], c4 = cp[4], c5 = cp[5];
        const float* ot = otile + b * OS;
        const float jx = ot[kJawCol], jy = ot[kJawCol + 1], jz = ot[kJawCol + 2];
        const unsigned vrow = (unsigned)b * (unsigned)a.n_verts + (unsigned)(v0 + fu), bnl = (unsigned)b * nl;
        const float4 t = vt_lds[j];
        const bool live = lane < 48 && v0 + j < a.n_verts;  // (b < 48 < B)
        finish_vertex<TO2D, 16>(cx, rs3, rsp, c0, c1, c2, c3, c4, c5, jx, jy, jz, ot[3 * j], ot[3 * j + 1], ot[3 * j + 2], t.x, t.y, __float_as_int(t.z), __float_as_int(t.w),
                                live && (outs & 1u), live && (outs & 2u), live && nl > 0 && __float_as_int(t.z) >= 0, vrow, bnl);
    };
    auto fin2 = [&](int row0) {
        const int fi = lane & 1, fu = min(lane >> 1, TV - 1), b = row0 + 2 * wave + fi;
        const float4* cp = reinterpret_cast<const float4*>(cst + b * CS);
        const float4 c0 = cp[0], c1 = cp[1], c2 = cp[2], c3 = cp[3], c4 = cp[4], c5 = cp[5];
        const float* ot = otile + b * OS;
        const float jx = ot[kJawCol], jy = ot[kJawCol + 1], jz = ot[kJawCol + 2];
        const unsigned vrow = (unsigned)b * (unsigned)a.n_verts + (unsigned)(v0 + fu), bnl = (unsigned)b * nl;
        const float4 t = vt_lds[fu];
        const bool live = b < B && (lane >> 1) < TV && v0 + fu < a.n_verts;
        finish_vertex<TO2D, 0>(cx, rs3, rsp, c0, c1, c2, c3, c4, c5, jx, jy, jz, ot[3 * fu], ot[3 * fu + 1], ot[3 * fu + 2], t.x, t.y, __float_as_int(t.z), __float_as_int(t.w),
                               live && (outs & 1u), live && (outs & 2u), live && nl > 0 && __float_as_int(t.z) >= 0, vrow, bnl);
    };

    // The tail of a launch with a pass 2 in two halves (kTailPre): what does not come out of the chain -- the constants and the vertex-table row
    // of the lane's pair, masks and offsets -- in front of barrier P2, where each role has time (round 0 and the vertex table are in LDS behind
    // P1); behind it the jaw and three accumulator values: fin2(kRows1)'s arithmetic on fin2's operands.
    float4 t0, t1, t2, t3, t4, t5, tvt;
    unsigned t_vrow = 0, t_bnl = 0;
    bool t_live3 = false, t_livep = false, t_livel = false;
    auto tail_pre = [&]() {
        const int fu = min(lane >> 1, TV - 1), b = kRows1 + 2 * wave + (lane & 1);
        const float4* cp = reinterpret_cast<const float4*>(cst + b * CS);
        t0 = cp[0], t1 = cp[1], t2 = cp[2], t3 = cp[3], t4 = cp[4], t5 = cp[5];
        tvt = vt_lds[fu];
        t_vrow = (unsigned)b * (unsigned)a.n_verts + (unsigned)(v0 + fu), t_bnl = (unsigned)b * nl;
        const bool live = b < B && (lane >> 1) < TV && v0 + fu < a.n_verts;
        t_live3 = live && (outs & 1u), t_livep = live && (outs & 2u), t_livel = live && nl > 0 && __float_as_int(tvt.z) >= 0;
    };
    auto tail_post = [&]() {
        const int fu = min(lane >> 1, TV - 1), b = kRows1 + 2 * wave + (lane & 1);
        const float* ot = otile + b * OS;
        const float jx = ot[kJawCol], jy = ot[kJawCol + 1], jz = ot[kJawCol + 2];
        finish_vertex<TO2D, 0>(cx, rs3, rsp, t0, t1, t2, t3, t4, t5, jx, jy, jz, ot[3 * fu], ot[3 * fu + 1], ot[3 * fu + 2], tvt.x, tvt.y, __float_as_int(tvt.z), __float_as_int(tvt.w),
                               t_live3, t_livep, t_livel, t_vrow, t_bnl);
    };

    if (wave >= 4) {
        // =============================================== stager waves =====================================================
        // Rows 0..47, twelve a wave, k 0..383 as three slabs of 128: a wave request covers 512 contiguous bytes of each of two rows (lane >> 5
        // picks the row) -- pre[6 s + jj]: slab s, rows 12 fw + 2 jj + {0, 1}; pre[18]: k 384..399 of the wave's twelve rows (lanes 0..47).
        // Rows past the batch re-read its last row.
        const int fw = wave - 4;
        const int lr = lane >> 5, lc = lane & 31;
        float4 pre[19];
        const float* prow[6];
#pragma unroll
        for (int jj = 0; jj < 6; ++jj) prow[jj] = a.params + (size_t)min(12 * fw + 2 * jj + lr, B - 1) * P + 4 * lc;
        auto load_slab = [&](int sl) {
#pragma unroll
            for (int jj = 0; jj < 6; ++jj) {
                const f4u v = *reinterpret_cast<const f4u*>(prow[jj] + 128 * sl);
                pre[6 * sl + jj] = float4{v.x, v.y, v.z, v.w};
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        auto write_slab = [&](int sl) {
#pragma unroll
            for (int jj = 0; jj < 6; ++jj) *reinterpret_cast<float4*>(abuf + (12 * fw + 2 * jj + lr) * LD + 128 * sl + 4 * lc) = pre[6 * sl + jj];
        };
        load_slab(0);  // in front of the start-up barrier: what the first MFMA needs and no more (24 wave requests in the workgroup)
        // (by every stager wave, from a clamped row: a branch around a load ends in a wait for it)
        const float4 vt_row = a.vtab[min(v0 + min(lane, TV - 1), a.n_verts - 1)];
        stamp(1);
        phase_barrier();  // nothing in front of it waits for data (and: the arrival words are zero)
        stamp(6);
        // behind the barrier, between the mma waves' up-front basis requests and in the order the GEMM wants them
        // (slab 2 asked for only once slab 0 is published: slab 0 is there ~0.9 k cycles earlier and nothing ends earlier -- profiles/r10_kernel_log.md)
        load_slab(1);
        load_slab(2);
        {
            const int r = min(lane >> 2, 11);
            const f4u v = *reinterpret_cast<const f4u*>(a.params + (size_t)min(12 * fw + r, B - 1) * P + 384 + 4 * (lane & 3));
            pre[18] = float4{v.x, v.y, v.z, v.w};
        }
        late_args();  // (the wait hides behind the one for slab 0)
        write_slab(0);
        arrive(parts, lane);
        stamp(7);
        write_slab(1);
        arrive(parts + 1, lane);
        write_slab(2);
        if (lane < 48) *reinterpret_cast<float4*>(abuf + (12 * fw + (lane >> 2)) * LD + 384 + 4 * (lane & 3)) = pre[18];
        arrive(parts + 2, lane);
        if (fw == 3 && lane < TV) vt_lds[lane] = vt_row;  // the tile's rows of the vertex table, read behind P1
        stamp(2);
        if (two) {
            // Rows 48..63, four a wave, for pass 2: asked for now, with at most D basis requests of each mma wave in the queue in front of them
            // (asked for behind ALL of the basis they would come back behind the stream).
            float4 q[7];
            const float* qrow[2];
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) qrow[jj] = a.params + (size_t)min(kRows1 + 4 * fw + 2 * jj + lr, B - 1) * P + 4 * lc;
#pragma unroll
            for (int sl = 0; sl < 3; ++sl)
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const f4u v = *reinterpret_cast<const f4u*>(qrow[jj] + 128 * sl);
                    q[2 * sl + jj] = float4{v.x, v.y, v.z, v.w};
                }
            {
                const f4u v = *reinterpret_cast<const f4u*>(a.params + (size_t)min(kRows1 + 4 * fw + min(lane >> 2, 3), B - 1) * P + 384 + 4 * (lane & 3));
                q[6] = float4{v.x, v.y, v.z, v.w};
            }
            stamp(16);
#pragma unroll
            for (int sl = 0; sl < 3; ++sl)
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) *reinterpret_cast<float4*>(abuf + (kRows1 + 4 * fw + 2 * jj + lr) * LD + 128 * sl + 4 * lc) = q[2 * sl + jj];
            if (lane < 16) *reinterpret_cast<float4*>(abuf + (kRows1 + 4 * fw + (lane >> 2)) * LD + 384 + 4 * (lane & 3)) = q[6];
            stamp(17);
        }
        stamp(18);
        phase_barrier();  // P1
        stamp(19);
        if (two) {
            if (kTailPre) tail_pre();
            fin4(32, fw, std::bool_constant<!kV16Merged>{});  // rows 32..47, while the mma waves multiply rows 48..63 and finish rows 0..31
            stamp(21);
            if (kV16Merged) fin_v16_both(fw);  // vertices 16..19 of rows 0..31 (not in the chain's last hook) and of rows 32..47
            else if (kV16Stagers) fin_v16(fw);
            stamp(9);
            phase_barrier();  // P2
            stamp(23);
            if (kTailPre) tail_post();
            else fin2(kRows1);
        } else {
            fin4(0, wave, std::true_type{});
            fin2(32);
        }
        stamp(5);
        if (trace && lane == 0) trace[13] = wall_clock64();
        return;
    }

    // ================================================== mma waves ===========================================================
    // wave w owns columns [16 w, 16 w + 16) of the tile; fragments and the basis pack as in flame_decode_pipe.hip.
    const float4* bsrc = reinterpret_cast<const float4*>(a.bpack) + ((size_t)tile * KG * 4 + wave) * 64 + lane;
    // -- the constants of the launch's rows: lanes 0..31 of wave w take rows 32 w + lane (rows past the batch: its last row) ------------
    f4u raw0 = {}, raw1 = {};
    f3u raw2 = {};  // (three floats, not four with translation z along: flame_decode_pipe.hip)
    float raw_scale = 0.f;
    {
        const float* prow = a.params + (size_t)min(32 * wave + (lane & 31), B - 1) * P + kNumBeta;
        raw0 = *reinterpret_cast<const f4u*>(prow), raw1 = *reinterpret_cast<const f4u*>(prow + 4), raw2 = *reinterpret_cast<const f3u*>(prow + 8);
        raw_scale = prow[12];
    }
    auto write_round = [&]() {
        // [400,403) jaw | [403,409) 6-DoF rotation | [409,412) translation | [412] scale   (FlameParams.from_3dmm, flame.py:48-73)
        const float jaw[3] = {raw0.x, raw0.y, raw0.z};
        const float rot6[6] = {raw0.w, raw1.x, raw1.y, raw1.z, raw1.w, raw2.x};
        float Dm[9], G[9];
        rodrigues_minus_identity_lean(jaw, Dm);  // pose feature of the jaw (smplx lbs step 3) = R_jaw - I
        rot6_to_matrix_lean(rot6, G);
        const float sp1 = raw_scale + 1.0f;
        const float s = sp1 < 1e-8f ? 1e-8f : sp1;  // head_mesh.py:39 torch.clamp(min=): a NaN scale stays NaN
        if (wave < 2 && lane < 32) {
            // rows of the A image past the betas, k = 400..415, of all 64 rows: pose feature R_jaw - I, the template's 1, zero padding
            float4* tail = reinterpret_cast<float4*>(abuf + (32 * wave + lane) * LD + kNumBeta);
            tail[0] = float4{Dm[0], Dm[1], Dm[2], Dm[3]};
            tail[1] = float4{Dm[4], Dm[5], Dm[6], Dm[7]};
            tail[2] = float4{Dm[8], 1.0f, 0.f, 0.f};
            tail[3] = float4{0.f, 0.f, 0.f, 0.f};
        }
        if (lane < 32) {
            float4* c = reinterpret_cast<float4*>(cst + (32 * wave + lane) * CS);
            c[0] = float4{Dm[0], Dm[1], Dm[2], Dm[3]};
            c[1] = float4{Dm[4], Dm[5], Dm[6], Dm[7]};
            c[2] = float4{Dm[8], G[0], G[1], G[2]};
            c[3] = float4{G[3], G[4], G[5], G[6]};
            c[4] = float4{G[7], G[8], s, raw2.y};
            c[5] = float4{raw2.z, 0.f, 0.f, 0.f};
            const int b = 32 * wave + lane;
            if ((a.flags & DAD3D_MUTATE_PARAMS) && tile == 0 && b < B)
                store_tz(a.params + ((unsigned)b * (unsigned)P + (unsigned)(kNumBeta + 11)));  // translation z := 0 (head_mesh.py:41), written through
        }
    };
    float4 bq[KG];  // the wave's basis slice, resident for the launch
    const float* afrag0 = abuf + (lane & 15) * LD + 4 * (lane >> 4);
    float* const ot0 = otile + ((lane >> 4) * 4) * OS + wave * 16 + (lane & 15);

    late_args();  // (here, where the mma waves are about to wait for the stagers anyway)
    stamp(6);
    phase_barrier();  // the stagers' requests for slab 0 are in the load queue (and the arrival words are zero)
    stamp(7);
    // The first D basis requests, in order (requests come back in order and group 0 is what the first MFMA waits for), constants round 0
    // behind request DAD3D_HEAD_R0_AT: the params' tails were asked for in front of the barrier, and no MFMA streams yet.
#pragma unroll
    for (int G = 0; G < D; ++G) {
        bq[G] = bsrc[(size_t)G * 256];
        __builtin_amdgcn_sched_barrier(0);
        if (G == DAD3D_HEAD_R0_AT) {
            // (no stamp in front of the round: a stamp is a store under a branch, the wait for the params' tails is counted for the path
            // without it, and a traced launch would wait here for basis group 0 as well -- slot 1 stays empty in the mma waves)
            write_round();
            if (wave < 2) arrive(parts + 2, lane);  // k = 400..415 of the A rows
            arrive(parts + 3, lane);                // constants round 0 is in LDS
            stamp(4);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    {   // ---- pass 1: rows 0..47, three row blocks; request G + D rides in front of the MFMAs of group G -----------------------------
        f32x4 acc[3] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
        float4 af[3], an[3] = {};
        stamp(16);
        wait_ge(parts, 4);
#pragma unroll
        for (int m = 0; m < 3; ++m) af[m] = *reinterpret_cast<const float4*>(afrag0 + m * 16 * LD);
#pragma unroll
        for (int G = 0; G < KG; ++G) {
            // The step's request and its three LDS reads each stand behind a row of three MFMAs (kSpread), not all in front of the step:
            // a wave issues in order, and only what is issued while an MFMA still runs costs the matrix pipe nothing.
            auto request = [&]() {
                if (G + D < KG) bq[G + D] = bsrc[(size_t)(G + D) * 256];
            };
            auto next_a = [&]() {
                if (G + 1 < KG) {
#pragma unroll
                    for (int m = 0; m < 3; ++m) an[m] = *reinterpret_cast<const float4*>(afrag0 + m * 16 * LD + 16 * (G + 1));
                }
            };
            if (!kSpread) request();
            if (G + 1 == 8) wait_ge(parts + 1, 4);
            if (G + 1 == 16) wait_ge2(parts + 2, 6, parts + 3, 4);
            if (!kSpread) next_a();
            __builtin_amdgcn_sched_barrier(0);
            if (G == 0) stamp(8);  // first MFMA: basis group 0 and slab 0 are here
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const float bv = s == 0 ? bq[G].x : s == 1 ? bq[G].y : s == 2 ? bq[G].z : bq[G].w;
#pragma unroll
                for (int m = 0; m < 3; ++m) {
                    const float av = s == 0 ? af[m].x : s == 1 ? af[m].y : s == 2 ? af[m].z : af[m].w;
                    acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[m], 0, 0, 0);
                    if (kSpread && kSpreadLdsAt == 4 && s == 0 && G + 1 < KG) {  // (4: one read behind each MFMA of row 0)
                        __builtin_amdgcn_sched_barrier(0);
                        an[m] = *reinterpret_cast<const float4*>(afrag0 + m * 16 * LD + 16 * (G + 1));
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                if (kSpread && s == kSpreadReqAt) {
                    __builtin_amdgcn_sched_barrier(0);
                    request();
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (kSpread && s == kSpreadLdsAt) {
                    __builtin_amdgcn_sched_barrier(0);
                    next_a();
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int m = 0; m < 3; ++m) af[m] = an[m];
        }
        stamp(2);
        // accumulators -> LDS tile [image][column]; D layout: row = (lane >> 4) * 4 + reg, column = lane & 15
#pragma unroll
        for (int m = 0; m < 3; ++m)
#pragma unroll
            for (int q = 0; q < 4; ++q) ot0[(m * 16 + q) * OS] = acc[m][q];
        stamp(17);
    }
    if (!two) {
        phase_barrier();  // P1
        stamp(18);
        stamp(3);
        fin4(0, wave, std::true_type{});
        fin2(32);
        stamp(5);
        if (trace && lane == 0) trace[13] = wall_clock64();
        return;
    }
    // ---- pass 2: rows 48..63, one row block; rows 0..31 are finished in its hooks: the wave finishes rows [8 w, 8 w + 8), lane = (row ei,
    // vertex group eu) walks the vertices eu, eu + 8, eu + 16 of the tile (flame_decode_pipe.hip's epilogue role, its pieces at its groups)
    const int ei = lane & 7, eu = lane >> 3, li = 8 * wave + ei;
    float4 k0, k1, k2, k3, k4, k5;
    {   // (round 0 is in LDS: pass 1 waited for parts + 3 at group 16; read where the wave is about to wait at P1 anyway)
        const float4* c = reinterpret_cast<const float4*>(cst + li * CS);
        k0 = c[0], k1 = c[1], k2 = c[2], k3 = c[3], k4 = c[4], k5 = c[5];
    }
    phase_barrier();  // P1: every wave's share of rows 0..47 is parked, rows 48..63 of A and the vertex table are in LDS
    stamp(18);
    float vW[3], vw2[3];
    int lh[3], ln[3];
    bool vl[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float4 t = vt_lds[min(eu + 8 * k, TV - 1)];
        vW[k] = t.x, vw2[k] = t.y, lh[k] = __float_as_int(t.z), ln[k] = __float_as_int(t.w);
        vl[k] = eu + 8 * k < TV && v0 + eu + 8 * k < a.n_verts;
    }
    float jx = 0.f, jy = 0.f, jz = 0.f, ex = 0.f, ey = 0.f, ez = 0.f;
    const float* const ot_e = otile + li * OS;
    const unsigned e_vrow = (unsigned)li * (unsigned)a.n_verts + (unsigned)(v0 + eu), e_bnl = (unsigned)li * nl;
    bool live3[3], livep[3], livel[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) live3[k] = vl[k] && (outs & 1u), livep[k] = vl[k] && (outs & 2u), livel[k] = vl[k] && nl > 0 && lh[k] >= 0;  // (li < 32 < B)
    auto epi_fetch = [&](int k) {
        const int j = eu + 8 * k;
        ex = ot_e[3 * j], ey = ot_e[3 * j + 1], ez = ot_e[3 * j + 2];  // v_posed (template + blend shapes + pose correctives)
    };
    auto epi_finish = [&](int k) {
        if (k == 0) finish_vertex<TO2D, 0>(cx, rs3, rsp, k0, k1, k2, k3, k4, k5, jx, jy, jz, ex, ey, ez, vW[0], vw2[0], lh[0], ln[0], live3[0], livep[0], livel[0], e_vrow, e_bnl);
        if (k == 1) finish_vertex<TO2D, 8>(cx, rs3, rsp, k0, k1, k2, k3, k4, k5, jx, jy, jz, ex, ey, ez, vW[1], vw2[1], lh[1], ln[1], live3[1], livep[1], livel[1], e_vrow, e_bnl);
        if (k == 2) finish_vertex<TO2D, 16>(cx, rs3, rsp, k0, k1, k2, k3, k4, k5, jx, jy, jz, ex, ey, ez, vW[2], vw2[2], lh[2], ln[2], live3[2], livep[2], livel[2], e_vrow, e_bnl);
    };
    {
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        const float* afrag = afrag0 + kRows1 * LD;
        float4 af = *reinterpret_cast<const float4*>(afrag), an = {};
        stamp(20);
#pragma unroll
        for (int G = 0; G < KG; ++G) {
            if (G + 1 < KG) an = *reinterpret_cast<const float4*>(afrag + 16 * (G + 1));
            __builtin_amdgcn_sched_barrier(0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af.x, bq[G].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af.y, bq[G].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af.z, bq[G].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af.w, bq[G].w, acc, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            af = an;
            if (G == 0) {
                jx = ot_e[kJawCol], jy = ot_e[kJawCol + 1], jz = ot_e[kJawCol + 2];  // J_jaw of this row, from pass 1
                epi_fetch(0);
            }
            if (G == 3) epi_finish(0), epi_fetch(1);
            if (G == 11) {
                epi_finish(1);
                if (!kV16Stagers) epi_fetch(2);
            }
            if (G == 19 && !kV16Stagers) epi_finish(2);
            if (kTailPre && G == kTailPreAt) tail_pre();  // (the basis registers of the groups behind are free, and the reads land under the groups in front)
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) ot0[(kRows1 + q) * OS] = acc[q];
        stamp(21);
    }
    phase_barrier();  // P2
    stamp(22);
    stamp(3);
    if (kTailPre) tail_post();
    else fin2(kRows1);
    stamp(5);
    if (trace && lane == 0) trace[13] = wall_clock64();
}

dad3d_status launch_flame_decode_head(const PipeArgs& a, hipStream_t s) {
    static PerDeviceOnce attr_done;
    const int dev = PerDeviceOnce::current();
    const size_t lds = (size_t)Lds::total * sizeof(float);
    DAD3D_REQUIRE(a.batch > kPipeHalf && a.batch <= kRows && a.chunk_half == 0 && (a.verts3d || a.proj),
                  "launch_flame_decode_head: a whole-mesh launch of 33..64 rows with a vertex output, not %d rows", a.batch);
    if (!attr_done.done(dev)) {
        for (const void* k : {reinterpret_cast<const void*>(&flame_decode_head_kernel<true>), reinterpret_cast<const void*>(&flame_decode_head_kernel<false>)})
            DAD3D_HIP_TRY(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_done.set(dev);
    }
    // without a projection output the two instantiations differ in nothing that runs
    const bool to2d = (a.flags & DAD3D_TO_2D) || !a.proj;
    const unsigned geom = pipe_geom_word(a.flags, 0, 1, 0);
    const PipeLateArgs late{a.lmk_next, a.verts3d, a.proj, a.lmk_xy, a.lmk_px, a.image_size};
    if (to2d)
        hipLaunchKernelGGL((flame_decode_head_kernel<true>), dim3(a.n_tiles), dim3(512), lds, s, a.params, a.bpack, a.vtab, a.trace, a.batch, a.n_verts, a.n_params, a.n_half, geom,
                           a.n_lmk, late);
    else
        hipLaunchKernelGGL((flame_decode_head_kernel<false>), dim3(a.n_tiles), dim3(512), lds, s, a.params, a.bpack, a.vtab, a.trace, a.batch, a.n_verts, a.n_params, a.n_half, geom,
                           a.n_lmk, late);
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

}  // namespace dad3d
