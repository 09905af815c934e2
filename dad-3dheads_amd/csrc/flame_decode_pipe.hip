// FLAME / HeadMesh decode for gfx950 (MI355X), round 4: ONE role, persistent workgroups, a software pipeline over the batch.
//
// Why (profiles/r04_kernel_log.md section 1, tools/coissue_probe.hip): v_mfma_f32_16x16x4_f32 runs at the fp32 vector rate and
// every VALU instruction issued on its SIMD -- by the multiplying wave itself or by a second wave; fp32, integer, packed or a
// plain move alike -- costs the matrix pipe ~6 cycles (transcendentals ~9). A second wave's VALU work is moreover THROTTLED
// beside a streaming MFMA wave (~0.3 instructions per MFMA issued), while its LDS and memory instructions get ~1 slot per MFMA
// and cost the matrix pipe nothing. So: arithmetic belongs in the multiplying wave's own stream, data movement in a second
// wave, and a block of 64 images x 64 columns costs its SIMD 13.3 k cycles of MFMA + ~6 x (VALU instructions) + whatever
// nothing overlaps. The two-role kernel of rounds 1-3 (flame_decode.hip) spends ~1.2 k non-MFMA instructions per SIMD and
// block and overlaps nothing: 24.4 k cycles per block. This kernel:
//
//   * one workgroup per tile of 20 vertices (252 tiles) walks the whole batch in HALF-BLOCKS of 32 images. Its four "mma"
//     waves (one per SIMD) keep their basis slice (26 KB each) in registers for the whole launch; per half-block they run
//     ds_read_b128 + MFMA, park the accumulators in LDS, meet at ONE s_barrier and finish their share of the half-block
//     (8 images x 20 vertices each) themselves. Its four "stager" waves do nothing but move the params rows of half-block h + 1
//     into the other LDS image while half-block h multiplies (global loads a phase ahead, ds_write_b128, the same barrier).
//   * no pose role and no hand-off: the only joint the jaw-only skinning needs, J_jaw = J0 + Jdirs.betas, is linear in the
//     betas and rides the GEMM as columns 60..62 of every tile. With R_j = I for every joint but the jaw the reference's
//     T.[v;1] = sum_j w_j A_j [v;1] collapses to  W v + w_jaw (R_jaw - I)(v - J_jaw)  (W = sum of the weights): the
//     translations of the other joints and the jaw's (J_jaw - J_neck) + (J_neck - J_root) + J_root chain cancel to fp32
//     rounding (<= 2e-8 in model units; bar 5e-6, north star 1e-4). The other per-image constants (Rodrigues of the jaw,
//     6-DoF rotation, scale, translation) are computed by the mma waves for 128 images at a time -- the first round in front
//     of the first MFMA, among their basis requests -- into an LDS ring.
//   * epilogue with the per-image constants in REGISTERS: lane (image i of the wave's 8, vertex group u) holds the image's 24
//     constants for the half-block and the weights / landmark slots of its <= 3 vertices for the launch, so a (vertex, image)
//     costs 3 LDS reads + ~30 VALU and leaves as one 12-byte and one 8-byte store (eight lanes = eight consecutive vertices
//     of one image: 96 / 64 contiguous bytes). ~110 VALU instructions per mma wave and half-block, ~220 per SIMD and block
//     instead of ~860.
//
// Reference arithmetic: model_training/model/flame.py:191-228 (betas, pose feature, lbs, +MESH_OFFSET_Z, 6-DoF rotation),
// smplx.lbs steps 1-6, model_training/model/utils.py:92-101, model_training/head_mesh.py:39-45,
// demo_utils.py:42-46 (int truncation of the landmark pixels).
// No implicit fp contraction in this translation unit: the epilogue and the constants code are inlined at several places (first
// half-block, steady state, last half-block) and every copy has to round identically -- duplicate params rows give bit-identical
// outputs whichever half-block they land in (tests/test_gpu_decode.py). The fused multiply-adds are written out.
#pragma clang fp contract(off)
#include "common.hpp"
#include "flame_math.hpp"
#include "flame_pipe_epilogue.hpp"

#ifndef DAD3D_PIPE_R0_AT  // constants round 0 sits behind this one of the mma waves' 26 basis requests (0..25), in all four waves at once.
#define DAD3D_PIPE_R0_AT 1  // 12.27 / 12.29 / 12.31 us at B = 64 for 1 / 4 / 12 against 12.51 with the round inside the first GEMM; staggered
#endif                      // over the waves (request 4 + 5 w) 12.53, a tie with the parent: profiles/r08_kernel_log.md section 3
#ifndef DAD3D_PIPE_STAGER_PRIO  // s_setprio of the stager waves (the mma waves stay at 0). Their instructions are few and every
#define DAD3D_PIPE_STAGER_PRIO 0  // one of them sits on a latency chain -- but priority 1 measured slower at every size (14.9 / 23.7 / 40.5 / 139.2
                                  // against 14.0 / 22.6 / 39.5 / 138.4 us at B = 64 / 128 / 256 / 1024, same call; 3: as 1)
#endif

namespace dad3d {

namespace {

using namespace pipe;

constexpr int KG = kPipeKGroups;       // MFMA groups of 16 k
constexpr int HB = kPipeHalf;          // images per half-block
constexpr int TV = kPipeTileVerts;     // vertices per tile
constexpr int kNumBeta = 400;
constexpr int kJawCol = 3 * TV;        // columns 60..62 of a tile: the jaw joint
constexpr int LD = 424;                // A image row stride (floats): LD / 4 odd -> conflict-free ds_read_b128 of the fragments
constexpr int OS = 76;                 // accumulator tile row stride: 76 = 12 (mod 32) -> the epilogue's (image, vertex) reads
                                       // of a half-wave hit 32 different banks (12 i covers the multiples of 4, 3 u the rest)
constexpr int CS = 24;                 // per-image constants: D 9 | G 9 | s tx ty | 3 pad
constexpr int kRound = 128;            // images per constants round: 4 mma waves x 32 lanes; ring of two rounds
struct Lds {
    static constexpr int a_off = 0;                          // [2][HB][LD]      params rows, double buffered
    static constexpr int o_off = a_off + 2 * HB * LD;        // [2][HB][OS]      accumulators, double buffered
    static constexpr int c_off = o_off + 2 * HB * OS;        // [2][kRound][CS]  per-image constants, two rounds
    static constexpr int y_off = c_off + 2 * kRound * CS;    // [4] arrival words of the first A image's three parts
    static constexpr int v_off = y_off + 4;                  // [TV] float4: the tile's rows of the vertex table (last half-block)
    static constexpr int total = v_off + 4 * TV;
    static_assert(total * 4 <= 160 * 1024, "LDS budget of one CU");
};

__device__ __forceinline__ int lds_peek(lds_int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void wait_ge(lds_int* p, int target) {
    while (lds_peek(p) < target) __builtin_amdgcn_s_sleep(1);
    asm volatile("" ::: "memory");  // the LDS reads this wait guards stay behind it (a wave's LDS operations execute in order)
}
__device__ __forceinline__ void wait_ge2(lds_int* p, int target, lds_int* q, int target_q) {  // two words, one LDS round trip per look
    while ((int)(lds_peek(p) < target) | (int)(lds_peek(q) < target_q)) __builtin_amdgcn_s_sleep(1);
    asm volatile("" ::: "memory");
}
__device__ __forceinline__ void arrive(lds_int* p, int lane) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's LDS writes have completed
    if (lane == 0) __hip_atomic_fetch_add(p, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// workgroup barrier that does NOT drain the wave's outstanding global loads / stores (__syncthreads would: vmcnt(0)); the
// stagers keep the next A image in flight across it, the mma waves their stores
__device__ __forceinline__ void phase_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// ---- the GEMM of one half-block on one mma wave: acc[m] += A[16 m .. 16 m + 16][k] * basis[k][16 columns] --------------------
// Groups [G0, G1) of 16 k, RB row blocks of 16 images (2 = a half-block); `af` carries the prefetched A fragments from one call to
// the next. FIRST: the launch's first
// half-block -- the A image arrives in three parts (arrival words) and the basis slice is still on its way into the registers: the
// first half-block of a launch runs at the pace of the basis stream (25.6 MB through every CU's share of the memory system),
// not at the pace of the matrix pipe.
// hook(G) runs between the MFMAs of group G and those of group G + 1: the previous half-block's epilogue rides here in pieces,
// so that its LDS round trips hide and its stores leave spread over the GEMM instead of as one burst of every CU.
template <bool FIRST, int G0, int G1, int RB, class Hook>
__device__ __forceinline__ void gemm_groups(const float* afrag, const float4 (&bq)[KG], f32x4 (&acc)[RB], float4 (&af)[RB], lds_int* parts,
                                            Hook&& hook) {
    float4 an[RB] = {};
    if (G0 == 0) {
        if (FIRST) wait_ge(parts, 4);
#pragma unroll
        for (int m = 0; m < RB; ++m) af[m] = *reinterpret_cast<const float4*>(afrag + m * 16 * LD);
    }
#pragma unroll
    for (int G = G0; G < G1; ++G) {
        if (FIRST && G + 1 == 8) wait_ge(parts + 1, 4);
        // the last part of A(0): four stagers and the mma wave that wrote the tail rows. And constants round 0 of all four mma waves, for
        // load_consts(0) behind this GEMM: written in front of group 7 at the latest, so the second word costs no LDS round trip of its own
        if (FIRST && G + 1 == 16) wait_ge2(parts + 2, 4 + RB / 2, parts + 3, 4);
        if (G + 1 < KG) {
#pragma unroll
            for (int m = 0; m < RB; ++m) an[m] = *reinterpret_cast<const float4*>(afrag + m * 16 * LD + 16 * (G + 1));
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float bv = s == 0 ? bq[G].x : s == 1 ? bq[G].y : s == 2 ? bq[G].z : bq[G].w;
#pragma unroll
            for (int m = 0; m < RB; ++m) {
                const float av = s == 0 ? af[m].x : s == 1 ? af[m].y : s == 2 ? af[m].z : af[m].w;
                acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[m], 0, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int m = 0; m < RB; ++m) af[m] = an[m];
        hook(G);
        __builtin_amdgcn_sched_barrier(0);
    }
}

}  // namespace

// Barrier protocol (every wave of the workgroup executes exactly 1 + H phase barriers: the start-up barrier and A(0 .. H - 1)):
//   start   the stagers' requests for the first A image (the mma waves': for the params' tails of round 0) are in the load queue
//   A(h)    after the mma waves have parked half-block h, the stagers have written A(h + 1) (and its tail rows)
// Inside the first phase four arrival words in LDS stand for barriers: parts + 0 .. 2 = the three parts of A(0) are in LDS (the third
// counts the four stagers and mma wave 0, which writes the tail rows k = 400..415), parts + 3 = constants round 0 is in LDS (the four
// mma waves; read by the stagers before write_tail(1) and by the mma waves before load_consts(0)). Every arrival is unconditional.
// Between A(h - 1) and A(h): mma waves [write a constants round,] multiply half-block h out of image h & 1 -- finishing half-block
// h - 1 (accumulator tile (h - 1) & 1, constants already in registers) in the gaps -- park it in tile h & 1 and load its constants
// into registers; stagers write image (h + 1) & 1 -- last read by GEMM(h - 1) -- and request the rows of half-block h + 2.
// TO2D: `proj` is [B,V,2] (head_mesh.py:44-45 `to_2d`), else [B,V,3]. DAD3D_ZERO_ROTATION launches take the two-role kernel.
// (Measured and dropped, profiles/r04_kernel_log.md: a launch of 33..64 images as ONE pass of four row blocks over both A images,
// all eight waves finishing both half-blocks -- 13.2 us at B = 64 against 12.8 for the two-phase pipeline: every store of the
// launch then leaves at the very end. Round 4's "48 + 16" -- three row blocks under the basis stream, one behind it -- lost there too, because it
// kept all 26 basis requests in front of the first MFMA; with the requests as an issue-ahead ring it wins 0.8 us at B = 64 and 2 us at 33..48 and
// is what whole-mesh launches of 33..64 rows with a vertex output now take: flame_decode_head.hip, profiles/r10_kernel_log.md (capi.cpp sends
// them there; DAD3D_DECODE_KERNEL=halfblocks keeps them here). And profiles/r07_kernel_log.md: the LAST half-block as two row blocks of 16 images with a barrier
// between them, rows 0..15 finished inside row block 1's GEMM and only rows 16..31 behind A(H - 1) -- bit-identical, 12.50 against 12.47 us
// at B = 64 on top of the write-through landmark stores, 12.78 against 12.68 alone: the tail behind the last barrier is ~1.5 k cycles of
// latency whether a lane finishes one vertex or two, and two chains of 104 dependent MFMAs are slower than one of 208 independent pairs.)
// The two ends of a launch: nothing waits for data in front of the first barrier -- not for the kernel's own arguments either (below:
// preloaded, and the rest read where a wave waits anyway) --, and no store is left to the end-of-kernel write-back --
// vertex stores, landmark slots and `translation z := 0` are all written through (flame_pipe_epilogue.hpp).
// CHUNKED (models of few tiles: the landmark sub-model's 23 for the 445 list): the batch is cut into a.n_chunks chunks of a.chunk_half
// half-blocks and a workgroup is one (tile, chunk) -- the kernel below on rows [b0, b0 + chunk) with every pointer moved there, so a
// row's results are the bits of an unchunked launch. Workgroups w = tile * n_chunks + chunk are dealt to the XCDs in runs of a.wg_per_xcd
// (<= 32, one per CU); workgroup id -> XCD id % 8 is the observed placement (MI355X_MICROARCH.md, "for speed only"): the chunks of one
// tile sit on one XCD (two at a run's end) and its basis slice crosses the fabric once or twice, not once per chunk.
// Arguments: flat scalars in the order of first use, not one by-value struct -- the unit is built with -mllvm -amdgpu-kernarg-preload-count
// (Makefile) and the first kPipePreloadDwords dwords of the kernarg segment arrive in SGPRs with the wave: everything the code in front of
// the start-up barrier reads, so no wave starts with a scalar load from a kernarg slot that is fresh with every launch and a wait for it. The
// compiler preloads scalar arguments only (a by-value struct: none) and whole arguments only, so the fourteen dwords are four pointers and
// six words with no padding between them; 14 is what the hardware takes (16 user SGPRs, two of them the kernarg pointer). `span_half`: the
// half-blocks a workgroup walks at most -- PipeArgs::n_half, CHUNKED PipeArgs::chunk_half (n_half is then the chunk's own). `geom`:
// pipe_geom_word (common.hpp: the flags and a chunked launch's wg_per_xcd, n_chunks, n_tiles). The rest is one struct behind them, read from the kernarg segment by late_args() below. (The compiler keeps a prologue in
// front of the entry that loads the preloaded range, for firmware that does not preload.) tests/test_decode_pipe_entry.py holds the
// descriptor to this list. Measured: 11.85 against 12.19 us at B = 64 (profiles/r09_kernel_log.md).
constexpr int kPipePreloadDwords = 14;  // params 2 | bpack 2 | vtab 2 | trace 2 | batch | n_verts | n_params | span_half | geom | n_lmk
static_assert(4 * kPipePreloadDwords == 4 * sizeof(void*) + 6 * sizeof(int), "the preloaded range ends with n_lmk");
struct PipeLateArgs {  // the arguments behind the preloaded range: one by-value struct, read where late_args() stands
    const int* lmk_next;
    float *verts3d, *proj, *lmk_xy;
    int32_t* lmk_px;
    float image_size;
};
static_assert((4 * kPipePreloadDwords) % alignof(PipeLateArgs) == 0, "`late` starts where the preloaded range ends: late_args() reads it there");
template <bool TO2D, bool CHUNKED>
__global__ __launch_bounds__(512, 2) void flame_decode_pipe_kernel(float* params, const float* bpack, const float4* vtab, unsigned long long* trace_buf, int batch,
                                                                   int n_verts, int n_params, int span_half, unsigned geom, int n_lmk, PipeLateArgs late) {
    // (dissolved by the compiler: the body below reads the launch's geometry under the names the host gives it. ORDER: lmk_next, verts3d, proj,
    // lmk_xy, lmk_px and image_size are NOT set here -- late_args() sets them, and with them cx, rs3, rsp and outs; nothing may read any of
    // those in front of a role's late_args() call. n_half and chunk_half both start as span_half: a chunked launch sends its chunk_half there and
    // computes n_half below, any other launch never reads chunk_half. Rewritten on two fully initialised local structs the kernel is tidier
    // and its chunked instantiation slower than the by-value struct at 2048 landmark-only rows -- profiles/r09_kernel_log.md section 3.)
    PipeArgs a;
    a.params = params, a.bpack = bpack, a.vtab = vtab, a.trace = trace_buf, a.n_params = n_params, a.batch = batch, a.n_half = span_half, a.n_verts = n_verts, a.n_lmk = n_lmk;
    const PipeGeom g = pipe_geom_unpack(geom);
    a.flags = g.flags, a.chunk_half = span_half, a.wg_per_xcd = g.wg_per_xcd, a.n_chunks = g.n_chunks, a.n_tiles = g.n_tiles;
    // (`late` is read through the kernarg pointer in late_args(), not here: named here, its load would sit at the top of the kernel)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* abuf = smem + Lds::a_off;
    float* otile = smem + Lds::o_off;
    float* cst = smem + Lds::c_off;
    lds_int* parts = (lds_int*)(smem + Lds::y_off);

    // (`wave` stays a per-lane value on purpose. The compiler cannot prove it uniform, so the role split below is an exec-mask branch and
    // its saved mask is this kernel's "2 SGPR spills": one v_writelane pair at the top, one v_readlane pair at the very end, once per
    // launch, no scratch. Made uniform with readfirstlane the branch turns scalar -- and 30-odd values turn into SGPRs with it: 7 spills
    // inside the loops instead of 2 outside them. tests/test_kernel_resources.py holds the line: scratch 0, VGPR spills 0.)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int tile_id = blockIdx.x, chunk_b0 = 0;
    if (CHUNKED) {
        const int w = (blockIdx.x & 7) * a.wg_per_xcd + (blockIdx.x >> 3);
        if ((int)(blockIdx.x >> 3) >= a.wg_per_xcd || w >= a.n_tiles * a.n_chunks) return;
        tile_id = w / a.n_chunks;
        const int b0 = (w % a.n_chunks) * a.chunk_half * HB;
        chunk_b0 = b0;  // (the output pointers move there in late_args())
        a.params += (size_t)b0 * a.n_params;
        a.batch = min(a.batch - b0, a.chunk_half * HB);
        a.n_half = (a.batch + HB - 1) / HB;
    }
    const int tile = tile_id, v0 = tile * TV;
    const int H = a.n_half, B = a.batch, P = a.n_params;
    unsigned long long* trace = a.trace ? a.trace + ((size_t)tile * 8 + wave) * 32 : nullptr;
    auto stamp = [&](int slot) {
        if (trace && lane == 0) trace[slot] = __builtin_readcyclecounter();
    };
    if (trace && lane == 0) trace[12] = wall_clock64();
    stamp(0);
    if (tid < 4) __hip_atomic_store(parts + tid, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    const unsigned nl = (unsigned)a.n_lmk;
    // What hangs on the arguments behind the preloaded range -- the output pointers, lmk_next, image_size -- is formed by late_args(): a scalar
    // load of `late` through the kernarg pointer (a miss, ~450 cycles: the slot is fresh with every launch) and the wait for it, once per role
    // and where the role waits anyway. In front of the role split it would put back what the preload takes away; as ONE load at the top with
    // the wait further down its eleven registers live through both roles beside what is made of them: 10-12 SGPR spills.
    EpiCtx cx;
    __amdgpu_buffer_rsrc_t rs3, rsp;
    unsigned outs = 0;
    auto late_args = [&]() {
        typedef const __attribute__((address_space(4))) char* kernarg_ptr;
        typedef const __attribute__((address_space(4))) PipeLateArgs* late_ptr;
        kernarg_ptr kp = (kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(kp));  // (opaque: otherwise the loads below are one load at the top of the kernel, and its values live through both roles)
        const late_ptr lp = reinterpret_cast<late_ptr>(kp + 4 * kPipePreloadDwords);
        a.lmk_next = lp->lmk_next, a.verts3d = lp->verts3d, a.proj = lp->proj, a.lmk_xy = lp->lmk_xy, a.lmk_px = lp->lmk_px, a.image_size = lp->image_size;
        if (CHUNKED) {
            const size_t b0 = (size_t)chunk_b0;
            if (a.verts3d) a.verts3d += b0 * a.n_verts * 3;
            if (a.proj) a.proj += b0 * a.n_verts * (TO2D ? 2 : 3);
            if (a.lmk_xy) a.lmk_xy += b0 * a.n_lmk * 2;
            if (a.lmk_px) a.lmk_px += b0 * a.n_lmk * 2;
        }
        // 3d_vertices / projection leave as raw buffer stores: (uniform resource) + (32-bit byte offset of the lane) + immediate
        rs3 = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<char*>(a.verts3d), 0, 0x7fffffff, 0x00020000);
        rsp = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<char*>(a.proj), 0, 0x7fffffff, 0x00020000);
        // (the landmark slots and `translation z := 0` leave as write-through stores too -- DAD3D_PIPE_LMK_STORE_AUX, flame_pipe_epilogue.hpp:
        // no store of this kernel is left to the end-of-kernel write-back of the XCDs' L2s)
        cx.lx = reinterpret_cast<char*>(a.lmk_xy), cx.lp = reinterpret_cast<char*>(a.lmk_px);
        // whether the launch has the two vertex outputs, as ONE opaque scalar word (bit 0 verts3d, bit 1 proj) tested where it is used: left
        // to itself the compiler holds a 64-bit lane mask of each for the whole launch, and the scalar file is full -- the write-through stores
        // took the CHUNKED instantiation from 3 SGPR spills to 5 without this (tests/test_kernel_resources.py allows 3). Timing: the same.
        outs = __builtin_amdgcn_readfirstlane((a.verts3d ? 1u : 0u) | (a.proj ? 2u : 0u));
        asm volatile("" : "+s"(outs));
        cx.lmk_next = a.lmk_next;
        cx.image_size = a.image_size;
    };
    cx.zsign = (a.flags & DAD3D_FLIP_Z) ? -1.0f : 1.0f;
    float4* const vt_lds = reinterpret_cast<float4*>(smem + Lds::v_off);
    // The LAST half-block has no GEMM to ride in and nothing left to stage: all eight waves finish it, four images each, lane =
    // (image fi of the wave's four, vertex fu of sixteen) -> vertices fu and, for fu < 4, fu + 16; sixteen lanes = sixteen
    // consecutive vertices of one image. The vertex table comes from LDS (parked there at the start by a stager wave).
    auto final_epilogue = [&](int hb) {
        const int fi = lane & 3, fu = lane >> 2, fli = 4 * wave + fi, b = hb * HB + fli;
        const float4* cp = reinterpret_cast<const float4*>(cst + (((hb >> 2) & 1) * kRound + (hb & 3) * HB + fli) * CS);
        const float4 c0 = cp[0], c1 = cp[1], c2 = cp[2], c3 = cp[3], c4 = cp[4], c5 = cp[5];
        const float* ot = otile + (hb & 1) * (HB * OS) + fli * OS;
        const float jx = ot[kJawCol], jy = ot[kJawCol + 1], jz = ot[kJawCol + 2];
        const unsigned vrow = (unsigned)b * (unsigned)a.n_verts + (unsigned)(v0 + fu), bnl = (unsigned)b * nl;
        {
            const float4 t = vt_lds[fu];
            const bool live = b < B && v0 + fu < a.n_verts;
            finish_vertex<TO2D, 0>(cx, rs3, rsp, c0, c1, c2, c3, c4, c5, jx, jy, jz, ot[3 * fu], ot[3 * fu + 1], ot[3 * fu + 2], t.x, t.y, __float_as_int(t.z), __float_as_int(t.w),
                                   live && (outs & 1u), live && (outs & 2u), live && nl > 0 && __float_as_int(t.z) >= 0, vrow, bnl);
        }
        if (fu < TV - 16) {
            const int j = fu + 16;
            const float4 t = vt_lds[j];
            const bool live = b < B && v0 + j < a.n_verts;
            finish_vertex<TO2D, 16>(cx, rs3, rsp, c0, c1, c2, c3, c4, c5, jx, jy, jz, ot[3 * j], ot[3 * j + 1], ot[3 * j + 2], t.x, t.y, __float_as_int(t.z), __float_as_int(t.w),
                                    live && (outs & 1u), live && (outs & 2u), live && nl > 0 && __float_as_int(t.z) >= 0, vrow, bnl);
        }
    };

    if (wave >= 4) {
        // =============================================== stager waves =====================================================
        if (DAD3D_PIPE_STAGER_PRIO) __builtin_amdgcn_s_setprio(DAD3D_PIPE_STAGER_PRIO);
        const int fw = wave - 4;
        // The half-block's 32 params rows x 400 betas (params[:, 0:400]: shape 300 + expression 100, flame.py:192-200 with nothing
        // to pad) as three slabs of 128 k and one of 16: a wave request covers 512 contiguous bytes of each of TWO rows (lane >> 5
        // picks the row), 10 cache lines -- eight rows x 128 bytes per request were 16, and the CU's one address unit is what the
        // launch's first microsecond waits for. Rows are 4-byte aligned (413 floats). pre[4 s + jj]: slab s, rows 8 fw + 2 jj + {0, 1};
        // pre[12]: k = 384..399 of the wave's eight rows (lanes 0..31).
        const int lr = lane >> 5, lc = lane & 31;
        float4 pre[13];   // the thread's share of the NEXT A image, requested a phase ahead
        float4 pre1[13];  // ... and of the launch's SECOND image, requested while the first is still in `pre`
        auto load_rows = [&](int hb, float4 (&dst)[13]) {
            const int r0 = hb * HB + 8 * fw;
            const float* prow[4];
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) prow[jj] = a.params + (size_t)min(r0 + 2 * jj + lr, B - 1) * P + 4 * lc;  // rows past the batch re-read its last row
#pragma unroll
            for (int sl = 0; sl < 3; ++sl)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const f4u v = *reinterpret_cast<const f4u*>(prow[jj] + 128 * sl);
                    dst[4 * sl + jj] = float4{v.x, v.y, v.z, v.w};
                    __builtin_amdgcn_sched_barrier(0);  // slab by slab, as the GEMM will want them
                }
            const f4u v = *reinterpret_cast<const f4u*>(a.params + (size_t)min(r0 + (lc >> 2), B - 1) * P + 384 + 4 * (lane & 3));
            dst[12] = float4{v.x, v.y, v.z, v.w};
        };
        auto write_rows = [&](int hb, int j0, int j1, const float4 (&src)[13]) {  // MFMA groups [0,8) [8,16) [16,26) = pre[0,4) [4,8) [8,13)
            float* img = abuf + (hb & 1) * (HB * LD);
#pragma unroll
            for (int idx = 0; idx < 12; ++idx)
                if (idx >= j0 && idx < j1) *reinterpret_cast<float4*>(img + (8 * fw + 2 * (idx & 3) + lr) * LD + 128 * (idx >> 2) + 4 * lc) = src[idx];
            if (j1 == 13 && lane < 32) *reinterpret_cast<float4*>(img + (8 * fw + (lane >> 2)) * LD + 384 + 4 * (lane & 3)) = src[12];
        };
        auto load_a = [&](int hb) { load_rows(hb, pre); };
        auto write_a = [&](int hb, int j0, int j1) { write_rows(hb, j0, j1, pre); };
        // rows of the A image past the betas, k = 400..415: pose feature R_jaw - I (9), the template's 1, zero padding -- copied
        // from the constants ring; lanes 0..31 of the wave: image 8 fw + (lane >> 2), float4 number lane & 3
        auto write_tail = [&](int hb) {
            if (lane < 32) {
                const int r = 8 * fw + (lane >> 2), q = lane & 3;
                const float* c = cst + (((hb >> 2) & 1) * kRound + (hb & 3) * HB + r) * CS;
                float4 v = *reinterpret_cast<const float4*>(c + 4 * min(q, 2));  // D0..3 | D4..7 | D8 G0 G1 G2
                if (q == 2) v = float4{v.x, 1.0f, 0.f, 0.f};
                if (q == 3) v = float4{0.f, 0.f, 0.f, 0.f};
                *reinterpret_cast<float4*>(abuf + (hb & 1) * (HB * LD) + r * LD + kNumBeta + 4 * q) = v;
            }
        };
        load_a(0);  // in flight before anything else happens in this workgroup
        // (by every stager wave, from a clamped row: a branch around a load -- even a wave-uniform one -- ends in a wait for it)
        const float4 vt_row = a.vtab[min(v0 + min(lane, TV - 1), a.n_verts - 1)];
        stamp(1);
        // Nothing in front of this barrier waits for data: it only tells the mma waves that the first A image's requests are in the
        // CU's load queue, ahead of the 104 KB of basis they are about to ask for.
        phase_barrier();  // (and: the arrival words are zero)
        stamp(6);
        late_args();  // (the wait hides behind the one for the first rows of A(0))
        write_a(0, 0, 4);
        arrive(parts, lane);
        stamp(7);
        // The second A image, NOW: a CU's requests come back in order, so what is asked for once the basis requests are queued comes
        // back behind the whole basis stream -- asked for ~8 k cycles into the launch these rows arrived 1.5 k cycles after the mma waves had
        // parked the first half-block. Here they interleave with the first basis requests and are back long before that. (In front of
        // the first barrier they would hold the basis back: 13.1 against 12.8 us at B = 64.)
        if (H > 1) load_rows(1, pre1);
        write_a(0, 4, 8);
        arrive(parts + 1, lane);
        write_a(0, 8, 13);
        arrive(parts + 2, lane);
        // the tile's rows of the vertex table, for the last half-block (read behind the last barrier)
        if (fw == 3 && lane < TV) vt_lds[lane] = vt_row;
        stamp(2);
        // constants round 0 is in LDS: write_tail(1) copies rows of it. This used to be a workgroup barrier, B0. (One half-block: nothing
        // here reads the ring in front of A(0), and a wave polling LDS for thousands of cycles takes issue slots from the mma wave on its SIMD.)
        if (H > 1) wait_ge(parts + 3, 4);
#pragma unroll 1
        for (int h = 0; h < H; ++h) {
            if (h < 4) stamp(16 + 4 * h);
            if (h + 1 < H) {
                // phase 0: the rows have been here since the first thousands of cycles; written ahead of the MFMAs (the third image's
                // requests below block this wave until the basis stream has drained)
                if (h == 0) __builtin_amdgcn_s_setprio(2);
                if (h == 0) write_rows(1, 0, 13, pre1);
                else write_a(h + 1, 0, 13);
                write_tail(h + 1);
                if (h == 0) __builtin_amdgcn_s_setprio(DAD3D_PIPE_STAGER_PRIO);
            }
            if (h < 4) stamp(17 + 4 * h);
            if (h + 2 < H) load_a(h + 2);
            if (h < 4) stamp(18 + 4 * h);
            phase_barrier();  // A(h)
            if (h < 4) stamp(19 + 4 * h);
        }
        final_epilogue(H - 1);
        stamp(5);
        if (trace && lane == 0) trace[13] = wall_clock64();
        return;
    }

    // ================================================== mma waves ===========================================================
    // wave w owns columns [16 w, 16 w + 16) of the tile for both 16-image row blocks of every half-block. MFMA step (G, s):
    // lane (q = lane >> 4, n = lane & 15) contributes basis row k = 16 G + 4 q + s, so its A operand for s = 0..3 is the
    // float4 at A[16 m + n][16 G + 4 q] of the row-major LDS image and its B operand the float4 packed for (G, w, lane).
    const float4* bsrc = reinterpret_cast<const float4*>(a.bpack) + ((size_t)tile * KG * 4 + wave) * 64 + lane;
    // -- constants of 128 images at a time (a "round"): lanes 0..31 of wave w take images 128 r + 32 w + lane ------------------
    f4u raw0 = {}, raw1 = {};  // (kept in the loaded type: a copy would make the wave wait for the load on the spot)
    f3u raw2 = {};             // (three floats, not four with translation z along: the compiler recycles a loaded register nobody reads, and waits for the load to do so)
    float raw_scale = 0.f;
    auto load_raw = [&](int r) {  // params[400..412] of the row, a phase before they are needed
        const float* prow = a.params + (size_t)min(r * kRound + 32 * wave + (lane & 31), B - 1) * P + kNumBeta;
        raw0 = *reinterpret_cast<const f4u*>(prow), raw1 = *reinterpret_cast<const f4u*>(prow + 4), raw2 = *reinterpret_cast<const f3u*>(prow + 8);
        raw_scale = prow[12];
    };
    auto write_round = [&](int r, bool first) {
        // [400,403) jaw | [403,409) 6-DoF rotation | [409,412) translation | [412] scale   (FlameParams.from_3dmm, flame.py:48-73)
        const float jaw[3] = {raw0.x, raw0.y, raw0.z};
        const float rot6[6] = {raw0.w, raw1.x, raw1.y, raw1.z, raw1.w, raw2.x};
        float D[9], G[9];
        rodrigues_minus_identity_lean(jaw, D);  // pose feature of the jaw (smplx lbs step 3) = R_jaw - I
        rot6_to_matrix_lean(rot6, G);
        const float sp1 = raw_scale + 1.0f;
        const float s = sp1 < 1e-8f ? 1e-8f : sp1;  // head_mesh.py:39 torch.clamp(min=): a NaN scale stays NaN (fmaxf would return 1e-8)
        if (first && wave == 0 && lane < 32) {
            // rows of the first A image past the betas, k = 400..415: pose feature R_jaw - I, the template's 1, zero padding
            // (later half-blocks: the stagers copy them out of the ring)
            float4* tail = reinterpret_cast<float4*>(abuf + lane * LD + kNumBeta);
            tail[0] = float4{D[0], D[1], D[2], D[3]};
            tail[1] = float4{D[4], D[5], D[6], D[7]};
            tail[2] = float4{D[8], 1.0f, 0.f, 0.f};
            tail[3] = float4{0.f, 0.f, 0.f, 0.f};
        }
        if (lane < 32) {
            float4* c = reinterpret_cast<float4*>(cst + ((r & 1) * kRound + 32 * wave + lane) * CS);
            c[0] = float4{D[0], D[1], D[2], D[3]};
            c[1] = float4{D[4], D[5], D[6], D[7]};
            c[2] = float4{D[8], G[0], G[1], G[2]};
            c[3] = float4{G[3], G[4], G[5], G[6]};
            c[4] = float4{G[7], G[8], s, raw2.y};
            c[5] = float4{raw2.z, 0.f, 0.f, 0.f};
            const int b = r * kRound + 32 * wave + lane;
            if ((a.flags & DAD3D_MUTATE_PARAMS) && tile == 0 && b < B)
                store_tz(a.params + ((unsigned)b * (unsigned)P + (unsigned)(kNumBeta + 11)));  // translation z := 0 (head_mesh.py:41), written through
                                                                                              // (32-bit index: b P < b V, capi.cpp resolve_kernel)
        }
    };
    load_raw(0);  // with the stagers' requests, ahead of the basis: needed among the first basis requests
    float4 bq[KG];  // the wave's basis slice, resident for the launch
    // -- epilogue role: the wave finishes images [8 w, 8 w + 8) of every half-block; lane = (image ei, vertex group eu) walks the
    // vertices eu, eu + 8, eu + 16 of the tile. Their weights and landmark slots stay in registers for the launch.
    const int ei = lane & 7, eu = lane >> 3, li = 8 * wave + ei;
    float vW[3], vw2[3];
    int lh[3], ln[3];
    bool vl[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) vl[k] = eu + 8 * k < TV && v0 + eu + 8 * k < a.n_verts;
    float4 k0, k1, k2, k3, k4, k5;  // the constants of this lane's image for the half-block about to be finished
    auto load_consts = [&](int hb) {
        const float4* c = reinterpret_cast<const float4*>(cst + (((hb >> 2) & 1) * kRound + (hb & 3) * HB + li) * CS);
        k0 = c[0], k1 = c[1], k2 = c[2], k3 = c[3], k4 = c[4], k5 = c[5];
    };
    // The epilogue of one half-block in pieces (the constants of the lane's image were loaded before the barrier that closed the
    // half-block): begin = J_jaw + output offsets; fetch(k) = v_posed of the lane's k-th vertex out of the accumulator tile;
    // finish(k) = skinning, rotation, projection, stores. The pieces ride in the next GEMM's hooks.
    float jx = 0.f, jy = 0.f, jz = 0.f, ex = 0.f, ey = 0.f, ez = 0.f;
    const float* ot_e = nullptr;
    unsigned e_vrow = 0, e_bnl = 0;  // b V + v0 + eu, b n_lmk
    bool live3[3] = {false, false, false}, livep[3] = {false, false, false}, livel[3] = {false, false, false};
    auto epi_begin = [&](int hb) {
        ot_e = otile + (hb & 1) * (HB * OS) + li * OS;
        jx = ot_e[kJawCol], jy = ot_e[kJawCol + 1], jz = ot_e[kJawCol + 2];  // J_jaw of this image, from the GEMM
        const int b = hb * HB + li;
        e_vrow = (unsigned)b * (unsigned)a.n_verts + (unsigned)(v0 + eu);
        e_bnl = (unsigned)b * nl;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const bool live = b < B && vl[k];
            live3[k] = live && (outs & 1u), livep[k] = live && (outs & 2u), livel[k] = live && nl > 0 && lh[k] >= 0;
        }
    };
    auto epi_fetch = [&](int k) {
        const int j = eu + 8 * k;
        ex = ot_e[3 * j], ey = ot_e[3 * j + 1], ez = ot_e[3 * j + 2];  // v_posed (template + blend shapes + pose correctives)
    };
    auto epi_finish = [&](int k) {
        if (k == 0) finish_vertex<TO2D, 0>(cx, rs3, rsp, k0, k1, k2, k3, k4, k5, jx, jy, jz, ex, ey, ez, vW[0], vw2[0], lh[0], ln[0], live3[0], livep[0], livel[0], e_vrow, e_bnl);
        if (k == 1) finish_vertex<TO2D, 8>(cx, rs3, rsp, k0, k1, k2, k3, k4, k5, jx, jy, jz, ex, ey, ez, vW[1], vw2[1], lh[1], ln[1], live3[1], livep[1], livel[1], e_vrow, e_bnl);
        if (k == 2) finish_vertex<TO2D, 16>(cx, rs3, rsp, k0, k1, k2, k3, k4, k5, jx, jy, jz, ex, ey, ez, vW[2], vw2[2], lh[2], ln[2], live3[2], livep[2], livel[2], e_vrow, e_bnl);
    };
    // hook of the steady-state GEMM: pieces of the previous half-block's epilogue, a fetch two groups before its finish
    int hook_hb = 0;
    auto epi_hook = [&](int G) {
        if (DAD3D_PIPE_ABLATE & 2) return;
        if (G == 0) epi_begin(hook_hb), epi_fetch(0);
        if (G == 3) epi_finish(0), epi_fetch(1);
        if (G == 11) epi_finish(1), epi_fetch(2);
        if (G == 19) epi_finish(2);
    };
    const float* afrag0 = abuf + (lane & 15) * LD + 4 * (lane >> 4);
    float* const ot0 = otile + ((lane >> 4) * 4) * OS + wave * 16 + (lane & 15);
    // accumulators -> LDS tile [image][column]; D layout: row = (lane >> 4) * 4 + reg, column = lane & 15
    auto park = [&](int h, const f32x4 (&acc)[2]) {
        float* ot = ot0 + (h & 1) * (HB * OS);
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int q = 0; q < 4; ++q) ot[(m * 16 + q) * OS] = acc[m][q];
    };
    const int n_rounds = (B + kRound - 1) / kRound;

    // (here, where the mma waves are about to wait for the stagers anyway -- those reach the barrier ~1 k cycles later. Behind the basis requests
    // the same scalar load sits under the basis stream and the headline LOSES 0.1 us against the by-value struct: profiles/r09_kernel_log.md)
    late_args();
    stamp(6);
    phase_barrier();  // the stagers' requests for the first A image are in the load queue (and the arrival words are zero)
    stamp(7);
    // The basis slice, ALL of it in flight from here: the CU's vector memory requests are served in order, so the A image -- asked
    // for in front of the barrier -- is not behind these 104 KB (asked for together with it, they put the first MFMA at 6.3 k
    // cycles instead of 4.5 k), while the basis stream neither waits for the GEMM to ask for it a few groups at a time (first
    // half-block 12.2 k cycles at that pace) nor for anybody's data: no wave waits for a load in front of the barrier above.
    // (in THIS order -- the requests come back in order and group 0 is what the first MFMA waits for; left alone, the scheduler
    // issued group 0 twenty-fifth)
    // Constants round 0 sits INSIDE this issue loop, behind request DAD3D_PIPE_R0_AT: the params' tails were asked for in front of the
    // barrier and are back first -- requests return in order -- and no MFMA streams yet, so the round's VALU work costs the matrix
    // pipe nothing. The address unit does not run dry meanwhile: it serves the stagers' requests for the second A image, which
    // otherwise queue between the basis requests until ~7 k cycles. (The round used to sit between groups 6 and 7 of the first GEMM,
    // on the reading that it fills time the GEMM would spend waiting for the basis anyway. The stamps say the MFMA chain of all four
    // waves stopped for ~1.4 k cycles there. What the move buys is less than that: the first MFMA now starts ~1.3 k cycles later and
    // the GEMM behind it runs at ~300 cycles a group instead of ~320 + the stop -- the first half-block is parked ~0.3-0.5 k cycles
    // earlier, the rest the basis stream takes back. profiles/r08_kernel_log.md.)
    // A launch (or chunk) of ONE half-block has no second A image: nothing would feed the address unit during the round and every
    // cycle of it would delay the basis, which is all such a launch waits for (landmark-only chunks 8.05 -> 8.34 us at 256 rows, B = 32
    // 8.30 -> 8.37). There the round stays between groups 6 and 7 of the GEMM. Launch-uniform: a wave runs the round, and arrives, at
    // exactly one of the two places.
    const bool round0_early = H > 1;
    auto round0 = [&]() {
        stamp(1);
        write_round(0, true);
        if (wave == 0) arrive(parts + 2, lane);  // the tail rows of A(0)
        arrive(parts + 3, lane);                 // "round 0 is in LDS": what barrier B0 used to say
        stamp(4);
    };
#pragma unroll
    for (int G = 0; G < KG; ++G) {
        bq[G] = bsrc[(size_t)G * 256];
        __builtin_amdgcn_sched_barrier(0);
        if (G == DAD3D_PIPE_R0_AT && round0_early) {
            round0();
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // the lanes' rows of the vertex table: weights and landmark slots, first used by the first epilogue -- behind the basis
    // (unconditional, from a clamped row: a branch around a load makes the wave wait for it on the spot; vl[k] gates every use)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float4 t = a.vtab[min(v0 + eu + 8 * k, a.n_verts - 1)];
        vW[k] = t.x, vw2[k] = t.y, lh[k] = __float_as_int(t.z), ln[k] = __float_as_int(t.w);
    }
    {   // the first half-block: A arrives in parts, the basis slice is still streaming into the registers. Nothing but LDS reads and
        // MFMAs: the constants of the first 128 images were written above, among the basis requests (one half-block: behind group 6).
        f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
        float4 af[2];
        stamp(16);
        gemm_groups<true, 0, KG, 2>(afrag0, bq, acc, af, parts, [&](int G) {
            if (G == 6 && !round0_early) {
                // (the loaded values made opaque: left alone the compiler sees one computation at two places, hoists it in front of
                // the first basis request -- behind a wait for the params' tails -- and every launch starts its basis stream late)
                asm volatile("" : "+v"(raw0), "+v"(raw1), "+v"(raw2), "+v"(raw_scale));
                round0();
            }
        });
        stamp(2);
        park(0, acc);
        stamp(17);
    }
    if (H > 1) load_consts(0);  // (round 0 is in LDS: the GEMM waited for parts + 3 at group 16)
    phase_barrier();  // A(0)
    stamp(18);
#pragma unroll 1
    for (int h = 1; h < H; ++h) {
        // round r covers half-blocks 4 r .. 4 r + 3: written in phase 4 r - 2 (the stagers read it from phase 4 r - 1 on), its
        // params requested a phase before that. The ring slot's previous tenant (round r - 2) was consumed by phase 4 r - 5.
        const int r = (h + 2) >> 2;
        if (!(DAD3D_PIPE_ABLATE & 4) && (h & 3) == 2 && r < n_rounds) write_round(r, false);
        if ((h & 3) == 1 && ((h + 3) >> 2) < n_rounds) load_raw((h + 3) >> 2);
        if (h < 4) stamp(16 + 4 * h);
        f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
        float4 af[2];
        hook_hb = h - 1;  // half-block h - 1 is finished inside the GEMM of half-block h
        gemm_groups<false, 0, KG, 2>(afrag0 + (h & 1) * (HB * LD), bq, acc, af, parts, epi_hook);
        park(h, acc);
        if (h < 4) stamp(17 + 4 * h);
        if (h + 1 < H) load_consts(h);  // (the last half-block is finished by all eight waves, in another lane layout)
        phase_barrier();  // A(h)
        if (h < 4) stamp(18 + 4 * h);
    }
    stamp(3);
    final_epilogue(H - 1);
    stamp(5);
    if (trace && lane == 0) trace[13] = wall_clock64();
}

size_t flame_decode_pipe_lds_bytes() { return (size_t)Lds::total * sizeof(float); }

dad3d_status launch_flame_decode_pipe(const PipeArgs& a, hipStream_t s) {
    static PerDeviceOnce attr_done;
    const int dev = PerDeviceOnce::current();
    const size_t lds = flame_decode_pipe_lds_bytes();
    if (!attr_done.done(dev)) {
        for (const void* k : {reinterpret_cast<const void*>(&flame_decode_pipe_kernel<true, false>),
                              reinterpret_cast<const void*>(&flame_decode_pipe_kernel<false, false>),
                              reinterpret_cast<const void*>(&flame_decode_pipe_kernel<true, true>)})
            DAD3D_HIP_TRY(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_done.set(dev);
    }
    // without a projection output the two instantiations differ in nothing that runs
    const bool to2d = (a.flags & DAD3D_TO_2D) || !a.proj;
    const bool chunked = a.chunk_half > 0 && to2d;
    DAD3D_REQUIRE(!chunked || pipe_geom_fits(a.wg_per_xcd, a.n_chunks, a.n_tiles), "launch_flame_decode_pipe: chunk geometry %d x %d in runs of %d "
                  "does not fit the kernel's geometry word", a.n_tiles, a.n_chunks, a.wg_per_xcd);  // (nothing pipe_chunking gives: tests/test_pipe_geom_word.py)
    const unsigned geom = chunked ? pipe_geom_word(a.flags, a.wg_per_xcd, a.n_chunks, a.n_tiles) : pipe_geom_word(a.flags, 0, 1, 0);
    const int span_half = chunked ? a.chunk_half : a.n_half;
    const PipeLateArgs late{a.lmk_next, a.verts3d, a.proj, a.lmk_xy, a.lmk_px, a.image_size};
#define DAD3D_PIPE_LAUNCH(TO2D_, CHUNKED_, GRID_)                                                                                              \
    hipLaunchKernelGGL((flame_decode_pipe_kernel<TO2D_, CHUNKED_>), dim3(GRID_), dim3(512), lds, s, a.params, a.bpack, a.vtab, a.trace, a.batch, \
                       a.n_verts, a.n_params, span_half, geom, a.n_lmk, late)
    if (chunked) DAD3D_PIPE_LAUNCH(true, true, 8 * a.wg_per_xcd);
    else if (to2d) DAD3D_PIPE_LAUNCH(true, false, a.n_tiles);
    else DAD3D_PIPE_LAUNCH(false, false, a.n_tiles);
#undef DAD3D_PIPE_LAUNCH
    DAD3D_HIP_TRY(hipGetLastError());
    return DAD3D_OK;
}

}  // namespace dad3d
