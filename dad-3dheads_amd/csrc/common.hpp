// Shared host-side declarations for libdad3d_hip.so (gfx950 only; no portability layer).
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/dad3d.h"

namespace dad3d {

void set_error(const char* fmt, ...);

#define DAD3D_HIP_TRY(expr)                                                                      \
    do {                                                                                         \
        hipError_t e__ = (expr);                                                                 \
        if (e__ != hipSuccess) {                                                                 \
            ::dad3d::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, \
                               __LINE__);                                                        \
            return DAD3D_E_HIP;                                                                  \
        }                                                                                        \
    } while (0)

#define DAD3D_REQUIRE(cond, ...)            \
    do {                                    \
        if (!(cond)) {                      \
            ::dad3d::set_error(__VA_ARGS__); \
            return DAD3D_E_INVALID;         \
        }                                   \
    } while (0)

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a property of a kernel ON ONE DEVICE: a launcher remembers per
// device whether it has raised the limit there (a process-wide flag let a second device launch a 150 KB-LDS kernel
// without the attribute). The launchers run with the handle's device current (DeviceGuard in the C ABI).
struct PerDeviceOnce {
    std::atomic<unsigned long long> mask[4] = {};  // 256 devices
    static int current() {
        int d = 0;
        (void)hipGetDevice(&d);
        return d & 255;
    }
    bool done(int d) const { return (mask[d >> 6].load(std::memory_order_acquire) >> (d & 63)) & 1ull; }
    void set(int d) { mask[d >> 6].fetch_or(1ull << (d & 63), std::memory_order_release); }
};

// RAII: make `device` current for the scope of a C-ABI call, restore afterwards.
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) ok = (hipSetDevice(device) == hipSuccess);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// ---------------------------------------------------------------------------------------------
// FLAME decode: geometry of the packed operands (see DESIGN.md "Data layout in HBM")
// ---------------------------------------------------------------------------------------------
constexpr int kTileVerts = 21;   // vertices per column tile: 63 basis columns + 1 zero pad = 64
constexpr int kTileCols = 64;    // 4 waves x one 16-wide MFMA column block
constexpr int kBlockImages = 64; // images (GEMM rows) per workgroup: 4 MFMA row blocks of 16
constexpr int kImgConsts = 84;   // floats per image: A_j 5x12 (jaw first) | R 9 | s tx ty | 4 compact translations
constexpr int kNumJoints = 5;    // FLAME: global, neck, jaw, left eye, right eye
constexpr int kOutStride = 68;   // LDS row stride of the accumulator tile (conflict-free ds_write_b32)
constexpr int kSyncWords = 1025;  // dad3d_flame sync block: words 0..5 + the ticket in the last word
constexpr unsigned kDeviceEpoch = 0x100u;  // internal decode flag: hand-off epoch kept on the device (graph capture)

// Offsets into one params row, `FlameParams.from_3dmm` order (flame.py:48-73).
struct ParamLayout {
    int n_params;
    int shape_off, shape_n;
    int expr_off, expr_n;
    int jaw_off, jaw_n;
    int rot_off;
    int eye_off, eye_n;
    int neck_off, neck_n;
    int trans_off;
    int scale_off;
};

struct DecodeArgs {
    float* params;          // [B,P] (tz written when DAD3D_MUTATE_PARAMS)
    const float* bpack;     // [n_tiles][kgroups][4 waves][64 lanes][4]: basis in MFMA B-fragment order
    const float* jdirs;     // [15][n_betas]  J_regressor . shapedirs
    const float* j0;        // [15]           J_regressor . v_template
    const float* weights8;  // [V][8] skinning weights w0..w4, S = w0+w1+w3+w4, 0, 0
    const int* lmk_head;    // [V][2] first landmark slot of a vertex or -1, and the slot chained after it (or -1)
    const int* lmk_next;    // [n_lmk] next slot with the same vertex or -1
    float* imgc;            // [B][kImgConsts] per-image constants: pose role -> decode role hand-off
    unsigned* sync;         // [0] arrivals, one per pose workgroup (monotonic over launches)  [1] hand-off time-outs (sticky)
                            // device-epoch launches (graph capture): [4] their arrivals  [5] arrivals of all earlier
                            // such launches (advanced by the kernel)  [kSyncWords-1] launch ticket
    float* verts3d;         // [B,V,3] or null
    float* proj;            // [B,V,2|3] or null
    float* lmk_xy;          // [B,n_lmk,2] or null
    int32_t* lmk_px;        // [B,n_lmk,2] or null
    unsigned long long* trace;  // diagnostics: [decode blocks][4 waves][32] s_memtime stamps, or null
    ParamLayout lay;
    int parents[kNumJoints];
    int batch, nbb, n_tiles, n_tiles_pad8, n_verts, n_lmk;
    int n_pose_blocks, n_pose_blocks_pad8;
    int n_betas, max_shape;  // 400, 300
    int betas_contiguous;    // params[0:400] are the betas (shape == 300 and expression == 100)
    int kgroups;
    unsigned arrive_target;  // host-side epoch: value of sync[0] once every pose workgroup of this launch has arrived
    unsigned spin_limit;
    float image_size;
    unsigned flags;
    float* posed;            // [B,V,3] v_posed (before skinning) for the backward pass, or null. Last on purpose: the
                             // inference instantiations never read it and their kernarg offsets stay what they were
};

dad3d_status launch_flame_decode(const DecodeArgs& a, hipStream_t s);

// Single-role, persistent, software-pipelined decode (flame_decode_pipe.hip, round 4): one workgroup per tile of 20 vertices
// walks the batch in half-blocks of 32 images. No pose role, no hand-off: the jaw joint rides the GEMM as columns 60..62 of
// every tile (J_jaw = J0_jaw + Jdirs_jaw . betas is linear in the betas), the other per-image constants come straight from
// the params row. Jaw-only models with the dad_3dnet.yaml params layout; inference outputs only.
constexpr int kPipeTileVerts = 20;  // 60 basis columns + 3 jaw-joint columns + 1 zero pad = 64
constexpr int kPipeHalf = 32;       // images per pipeline stage: 2 MFMA row blocks of 16
constexpr int kPipeKGroups = 26;    // K = 400 betas + 9 jaw pose features + the template row -> 416
struct PipeArgs {
    float* params;           // [B,P] (tz written when DAD3D_MUTATE_PARAMS)
    const float* bpack;      // [n_tiles][26][4 waves][64 lanes][4]: basis of the 20-vertex tiles + the jaw-joint columns
    const float4* vtab;      // [V] {W = sum of the five skinning weights, w_jaw, first landmark slot, slot chained after it} (the
                             //      last two as int bits; -1 = none)
    const int* lmk_next;     // [n_lmk] next slot with the same vertex or -1
    float* verts3d;          // [B,V,3] or null
    float* proj;             // [B,V,2|3] or null
    float* lmk_xy;           // [B,n_lmk,2] or null
    int32_t* lmk_px;         // [B,n_lmk,2] or null
    unsigned long long* trace;  // diagnostics: [n_tiles][8 waves][32] stamps, or null
    int n_params, batch, n_half, n_tiles, n_verts, n_lmk;
    float image_size;
    unsigned flags;
    int chunk_half, n_chunks, wg_per_xcd;  // chunk_half > 0: workgroup = (tile, chunk of chunk_half half-blocks) (pipe_chunking)
};
// Models of few tiles (the landmark sub-model): cut the batch into as many chunks of whole half-blocks as keep tiles x chunks within
// the 256 CUs (one workgroup per CU: 152 KB of LDS), dealt to the XCDs in runs of wg_per_xcd <= 32. chunk_half = 0: one workgroup per
// tile walks the whole batch (the whole mesh: 252 tiles).
inline void pipe_chunking(int n_tiles, int n_half, int* chunk_half, int* n_chunks, int* wg_per_xcd) {
    *chunk_half = 0, *n_chunks = 1, *wg_per_xcd = 0;
    const int max_chunks = 256 / n_tiles;
    if (max_chunks < 2 || n_half < 2) return;
    *chunk_half = (n_half + max_chunks - 1) / max_chunks;
    *n_chunks = (n_half + *chunk_half - 1) / *chunk_half;
    *wg_per_xcd = (n_tiles * *n_chunks + 7) / 8;
}
// The kernel's `geom` argument (flame_decode_pipe.hip: one preloaded dword): the flags and a chunked launch's geometry in one word, a byte
// each: flags | wg_per_xcd (<= 32) | n_chunks - 1 | n_tiles. pipe_chunking gives tiles x chunks <= 256 with at least two chunks: n_tiles <= 128,
// but n_chunks up to 256 -- a sub-model of ONE tile (a landmark list of up to 20 vertices) whose n_half is a multiple of 256 -- hence the
// "- 1". A launch that is not chunked sends the flags alone and reads n_chunks = 1, which is what PipeArgs says of it. (Bytes on purpose:
// the kernel divides the workgroup number by n_chunks in front of its first address, and a divisor the compiler knows to be <= 256 takes
// the short form of that division.)
struct PipeGeom {
    unsigned flags;
    int wg_per_xcd, n_chunks, n_tiles;
};
constexpr bool pipe_geom_fits(int wg_per_xcd, int n_chunks, int n_tiles) {
    return wg_per_xcd >= 0 && wg_per_xcd < 256 && n_chunks >= 1 && n_chunks <= 256 && n_tiles >= 0 && n_tiles < 256;
}
constexpr unsigned pipe_geom_word(unsigned flags, int wg_per_xcd, int n_chunks, int n_tiles) {
    return (flags & 0xFFu) | (unsigned)wg_per_xcd << 8 | (unsigned)(n_chunks - 1) << 16 | (unsigned)n_tiles << 24;
}
constexpr PipeGeom pipe_geom_unpack(unsigned w) {
    return PipeGeom{w & 0xFFu, (int)(w >> 8 & 0xFFu), (int)(w >> 16 & 0xFFu) + 1, (int)(w >> 24)};
}
dad3d_status launch_flame_decode_pipe(const PipeArgs& a, hipStream_t s);
size_t flame_decode_pipe_lds_bytes();
// The same decode for whole-mesh launches of 33..64 rows with a vertex output (flame_decode_head.hip): rows 0..47 multiply while the basis
// streams in, rows 48..63 behind it. Same arguments (chunk_half = 0), same bits.
dad3d_status launch_flame_decode_head(const PipeArgs& a, hipStream_t s);

// The exact-product splits of the same decode (flame_decode_split.hip, round 6; gated: DAD3D_KERNEL_SPLIT_BF16 -- three bf16 planes, six
// products -- and DAD3D_KERNEL_SPLIT_F16 -- two fp16 planes, three products). Two launches:
// a pre-pass that splits the params rows into planes and computes the per-image constants once, and the tile kernel, which
// reads the pipelined kernel's basis pack as it is and walks the batch in phases of 16 images.
constexpr int kSplitRows = 16;        // images per phase: one MFMA row block
constexpr int kSplitKGroups = 13;     // K = 416 in MFMA groups of 32
constexpr int kSplitRowBytes = 848;   // one plane row: 416 bf16 + 16 bytes of padding (conflict-free 16-byte fragment reads)
constexpr int kSplitPlaneBytes = (3 * kSplitRows * kSplitRowBytes + 1023) / 1024 * 1024;  // a phase's planes [3][16 rows][848], in whole KB
constexpr int kSplitConstBytes = (kSplitRows * 24 * 4 + 1023) / 1024 * 1024;              // its per-image constants [16][24 floats]
constexpr int kSplitBlockBytes = kSplitPlaneBytes + kSplitConstBytes;                     // one phase in HBM: planes | constants
struct SplitArgs {
    float* params;           // [B,P] (tz written when DAD3D_MUTATE_PARAMS)
    const float* bpack;      // the pipelined kernel's pack (PipeArgs::bpack)
    const float* bpack_f16;  // DAD3D_KERNEL_SPLIT_F16: the same pack split into its two fp16 planes (launch_split_basis_f16), same size and addressing
    const float4* vtab;      // [V] as PipeArgs::vtab
    const int* lmk_next;     // [n_lmk]
    float* verts3d;          // [B,V,3] or null
    float* proj;             // [B,V,2|3] or null
    float* lmk_xy;           // [B,n_lmk,2] or null
    int32_t* lmk_px;         // [B,n_lmk,2] or null
    char* aplanes;           // [n_phase][kSplitBlockBytes] scratch, pre-pass -> tile kernel: the params rows as bf16 planes, then the
                             // per-image constants D 9 | G 9 | s tx ty | pad of the phase
    float b_scale;           // DAD3D_KERNEL_SPLIT_F16: the power of two the basis is multiplied by in front of its fp16 split (split_basis_scale)
    int n_params, batch, n_phase, n_tiles, n_verts, n_lmk;
    int n_chunks, phases_per_chunk;  // split_chunking: (1, n_phase) for the whole mesh
    float image_size;
    unsigned flags;
};
// A model of few tiles (the landmark sub-model: 23) cuts the launch's phases into chunks, one workgroup per (tile, chunk), up to 256 workgroups
inline void split_chunking(int n_tiles, int n_phase, int* n_chunks, int* phases_per_chunk) {
    *n_chunks = 1, *phases_per_chunk = n_phase;
    const int max_chunks = 256 / n_tiles;
    if (max_chunks < 2 || n_phase < 2) return;
    *phases_per_chunk = (n_phase + max_chunks - 1) / max_chunks;
    *n_chunks = (n_phase + *phases_per_chunk - 1) / *phases_per_chunk;
}
dad3d_status launch_flame_decode_split(const SplitArgs& a, int form, hipStream_t s);  // form: DAD3D_KERNEL_SPLIT_BF16 | DAD3D_KERNEL_SPLIT_F16
float split_basis_scale(float max_abs);
dad3d_status launch_split_basis_f16(const float* bpack, float* bpack_f16, int n_tiles, float scale, hipStream_t s);
size_t flame_decode_split_lds_bytes();

// Backward of the per-vertex half of the decode (flame_backward.hip). Per-image constants, natural joint order:
//   [0,60) A_j rows 0..2 of the relative transforms (j = 0..4, 12 floats each)   [60,69) G row-major   [69] s   [70,72) tx ty
constexpr int kBackwardConsts = 72;
struct BackwardArgs {
    const float* weights8;   // [V][8] as in DecodeArgs
    const float* consts;     // [B][72]
    const float* posed;      // [B,V,3] v_posed (template + blend shapes + pose correctives)
    const float* g_verts3d;  // [B,V,3] or null
    const float* g_proj;     // [B,V,2|3] or null
    float* g_posed;          // [B,V,3]
    float* g_consts;         // [B][72]
    float* partials;         // [B][nsplit][72] scratch when nsplit > 1
    int batch, n_verts, nsplit;
    float image_size;
    unsigned flags;          // DAD3D_ZERO_ROTATION | DAD3D_TO_2D | DAD3D_FLIP_Z as passed to the forward call
};
dad3d_status launch_flame_backward(const BackwardArgs& a, hipStream_t s);
constexpr int kBackwardMaxSplit = 8;

// dL/d[betas | pose feature] = dL/d(v_posed) . basis^T (flame_backward.hip): split over the 3V axis in chunks of kGradChunk
constexpr int kGradChunk = 256;        // columns (vertex coordinates) per workgroup
constexpr int kGradQuarters = 4;       // output quarters: a workgroup's four waves take two 16-row MFMA tiles each
constexpr int kGradQuarterRows = 128;
constexpr int kGradRows = kGradQuarters * kGradQuarterRows;    // 512 >= n_betas + 36
struct GradPackArgs {      // builds the MFMA B-fragment pack of basis^T from the forward pack, once per model
    const float* bpack;    // forward pack (DecodeArgs::bpack)
    float* gpack;          // [n_chunks][4 quarters][4 waves][16 groups][2 tiles][64][4]
    int kgroups, n_betas, n_pose_feats, pose_feat_first, n_inputs, n_cols, n_chunks;
};
struct GradInputsArgs {
    const float* g_posed;  // [B][n_cols]
    const float* gpack;
    float* partials;       // [n_slices][batch_pad][kGradRows]
    float* g_inputs;       // [B][n_inputs]
    int batch, batch_pad, n_cols, n_chunks, n_inputs;
    int chunks_per_slice, n_slices;  // a workgroup multiplies `chunks_per_slice` consecutive chunks: partials [n_slices][batch_pad][kGradRows]
};
inline int grad_chunks_per_slice(int batch_pad) { return batch_pad / kBlockImages >= 4 ? 4 : batch_pad / kBlockImages >= 2 ? 2 : 1; }
size_t grad_pack_floats(int n_chunks);
dad3d_status launch_grad_pack(const GradPackArgs& a, hipStream_t s);
dad3d_status launch_grad_inputs(const GradInputsArgs& a, hipStream_t s);

// Per-image chain (flame_backward.hip): forward writes `inputs` and `consts`; vjp reads g_inputs / g_consts, writes g_params.
struct ChainArgs {
    const float* params;    // [B,P]
    const float* jdirs;     // [15][n_betas]
    const float* j0;        // [15]
    float* inputs;          // [B][n_betas + 36]  betas | pose feature      (forward)
    float* consts;          // [B][72]                                      (forward)
    const float* g_inputs;  // [B][n_betas + 36]                            (vjp)
    const float* g_consts;  // [B][72]                                      (vjp)
    float* g_params;        // [B,P], every entry written                   (vjp)
    ParamLayout lay;
    int parents[kNumJoints];
    int batch, n_betas, max_shape;
};
dad3d_status launch_pose_chain(const ChainArgs& a, bool vjp, hipStream_t s);
dad3d_status launch_readjust(float* params, int batch, ParamLayout lay, const float* pads_scale, float pad_left,
                             float pad_top, float scale, float img_size, hipStream_t s);
size_t flame_decode_lds_bytes(int kgroups);

// ---------------------------------------------------------------------------------------------
// Sim3DR
// ---------------------------------------------------------------------------------------------
struct MeshDev {
    const int* tri;       // [ntri,3]
    const int* adj_ptr;   // [nver+1]   CSR rows: (face, corner) incidences of a vertex, ascending face order
    const int* adj_face;  // [3*ntri]
    const int4* adj_tri;  // [3*ntri]   the three corner indices of adj_face[e] (and the face index)
    int ntri, nver;
};

// Face lists of vertex chunks (normals, round 3): the vertices are cut into `chunks` ranges of `vpb`; chunk c lists every
// face with a corner in its range (ascending face index). A workgroup computes each of those face normals ONCE into an
// LDS table, then a vertex sums its table entries in ascending face order -- the serial scatter-add order of
// rasterize_kernel.cpp:188-198 -- instead of recomputing every incident face from its corners.
constexpr int kNormalChunkings = 4;  // 1, 2, 4, 8 chunks per image
struct NormalChunksDev {
    const uint2* faces;   // [face_ptr[chunks]]  (i0 | i1 << 16, i2), chunk after chunk: 8 bytes per face -- these static lists are
                          // as much load traffic per block as the vertices themselves, hence 16-bit indices
    int face_ptr[9];      // [chunks + 1] offsets into faces (by value: no dependent round trip in front of the face loads)
    const unsigned short* slot;  // [3*ntri]  aligned with adj_face: position of adj_face[e] in the list of its vertex's chunk
    const uint4* row8;    // [nver]  the first eight slots of a vertex as 8 x u16 in ONE aligned 16-byte load (0xFFFF = no more
                          // faces; a vertex with more than eight keeps seven here and 0xFFFE in the last: the rest from slot[])
    int chunks, vpb, max_faces;  // chunks == 0: not built (mesh too large for the LDS table)
};

dad3d_status launch_tri_normal(const MeshDev& m, float* tri_normal, const float* vertices, int batch, int norm_flg,
                               hipStream_t s);
dad3d_status launch_ver_normal(const MeshDev& m, float* ver_normal, const float* tri_normal, int batch,
                               unsigned flags, hipStream_t s);
dad3d_status launch_get_normal(const MeshDev& m, const NormalChunksDev* nc, float* ver_normal, const float* vertices,
                               int batch, unsigned flags, hipStream_t s);
// bytes of LDS the face-normal-table kernels need for a chunking with `max_faces` faces in its largest chunk
size_t normal_table_lds_bytes(int nver, int max_faces);
// Which kernel form a launch takes and over how many vertex chunks per image: decided here once, for the launchers
// and for dad3d_mesh_normal_plan alike. form = DAD3D_FORM_*; nc = the table chunking (table form only); lds = dynamic bytes.
struct NormalPlan {
    int form, chunks, vpb;
    const NormalChunksDev* nc;
    size_t lds;
};
NormalPlan plan_get_normal(const MeshDev& m, const NormalChunksDev* nc, int batch);
NormalPlan plan_phong(const MeshDev& m, const NormalChunksDev* nc, bool normals_given, int batch);  // refused: lds = what it would need
NormalPlan plan_render_light(const MeshDev& m, const NormalChunksDev* nc, int h, int w);            // the light inside the geometry kernel
// scratch: raster_scratch_bytes(..) bytes of device memory (per-image triangle boxes, setup planes, per-tile
// triangle lists), zeroed once with raster_scratch_init before its first use
size_t raster_scratch_bytes(const MeshDev& m, int batch, int h, int w);
dad3d_status raster_scratch_init(const MeshDev& m, void* scratch, int batch, int h, int w, hipStream_t s);
dad3d_status launch_rasterize(const MeshDev& m, const NormalChunksDev* nc, void* scratch, unsigned long long* trace, uint8_t* image, const float* vertices,
                              const float* colors, float* depth, int32_t* tri_buf, float* bary, int batch, int h,
                              int w, int c, int render_flags, int mode, const dad3d_light* light_cfg, hipStream_t s, float alpha = 1.0f);
// _render_texture_core: tex_tri [ntri][2] float4 = the texel coordinates of every triangle's corners (x0 y0 x1 y1 | x2 y2 - -);
// image / texture float32 or uint8; tex_image_stride = elements between two images' textures, 0 for one shared texture
dad3d_status launch_render_texture(const MeshDev& m, void* scratch, void* image, int image_u8, const float* vertices, const float4* tex_tri,
                                   const void* texture, int texture_u8, size_t tex_image_stride, float* depth, int batch, int h, int w, int c,
                                   int tex_h, int tex_w, int tex_c, int nearest, hipStream_t s);
dad3d_status launch_phong(const MeshDev& m, const NormalChunksDev* nc, float* light, const float* vertices, const float* normals,
                          float* normals_out, int batch, const dad3d_light& cfg, hipStream_t s);
// Heads into frames (sim3dr_frames.hip). frames_check_shapes: the host copy of the frame table against the limits, *total_tiles =
// the 64 x 64 tiles of all frames; nothing touches the device. scratch: frames_scratch_bytes(..) bytes, no initialisation needed.
dad3d_status frames_check_shapes(const char* who, const int64_t* frames_host, int n_frames, int* total_tiles);
size_t frames_scratch_bytes(int ntri, int n_frames, int n_heads, int total_tiles);
dad3d_status launch_rasterize_frames(const MeshDev& m, void* scratch, const int64_t* frames, int n_frames, int total_tiles, const float* vertices,
                                     const float* colors, const int32_t* image_index, int n_heads, int reverse, int32_t* flags, hipStream_t s);
// Textured heads into frames (sim3dr_frames_texture.hip): the same lists, then a tile kernel with _render_texture_core's pixel test and
// resolve. tex_tri as for launch_render_texture; tex_head_stride = elements between two heads' textures, 0 for one shared texture.
dad3d_status launch_render_texture_frames(const MeshDev& m, void* scratch, const int64_t* frames, int n_frames, int total_tiles,
                                          const float* vertices, const float4* tex_tri, const void* texture, int texture_u8, size_t tex_head_stride,
                                          int tex_h, int tex_w, int tex_c, int nearest, const int32_t* image_index, int n_heads, int32_t* flags,
                                          hipStream_t s);

// matrix projection (flame_dataset.py:115-141): frame = [B][3] (image height, crop x, crop y)
dad3d_status launch_project_vertices(const float* vertices, const float* model_view, const float* projection,
                                     const float* frame, int batch, int nver, float* world_homo, float* xy, int32_t* xy_int,
                                     hipStream_t s);

// the reference's mesh losses, value and gradient (mesh_losses.hip)
constexpr int kCubeStats = 28;  // floats per (region, image): see cube_stats_kernel
struct CubeLossArgs {
    const float* pred;           // [B,V,3]
    const float* target;         // [B,V,3]
    const int* region_ptr;       // [R+1] offsets into region_idx
    const int* region_idx;       // [sum N_r] vertex indices, region after region (duplicates allowed)
    const float* region_weight;  // [R]
    const int* vert_ptr;         // [V+1] incidence list vertex -> (region, position in the region), ascending region
    const int* vert_region;      // [sum N_r]
    const int* vert_pos;         // [sum N_r]
    float* stats;                // [R][B][kCubeStats] scratch
    float* loss_terms;           // [R][B] weighted mean of the region on image b (their sum is the loss)
    float* grad_pred;            // [B,V,3] dL/dpred, every element written; null: value only
    int batch, n_verts, n_regions, criterion;
};
struct PointLossArgs {
    const float* pred;          // [B,N,comps]
    const float* target;        // [B,N,comps]
    const float* point_weight;  // [N] sum over the regions of w_r * multiplicity / N_r
    float* loss_terms;          // [B][point_loss_blocks(N)]
    float* grad_pred;           // [B,N,comps] or null
    float scale;                // 1 / (B * comps): the rest of the mean
    int batch, n_points, comps, criterion;
};
int point_loss_blocks(int n_points);
dad3d_status launch_cube_loss(const CubeLossArgs& a, hipStream_t s);
dad3d_status launch_point_loss(const PointLossArgs& a, hipStream_t s);

// the benchmark scorer's point-set steps (mesh_eval.hip)
constexpr int kEvalMaxK = 8;        // nearest neighbours kept per query
constexpr int kEvalMaxHead = 4096;  // head-subset size the Z5 sort holds in LDS (8-byte keys: 32 KB)
constexpr int kEvalMaxAnchors = 8;
struct EvalNearestArgs {
    const float* query;       // [B,Q,3]
    const float* points;      // [B,N,3]; rows of item b past counts[b] are never read
    const int* counts;        // [B] or null (every item has N points)
    const float* similarity;  // [B][13] = s, R (3x3 row-major), t: p' = s * p . R + t; or null (identity)
    float* min_dist2;         // [B,Q]
    int* knn_index;           // [B,Q,k] or null; -1 where fewer than k points exist
    float* knn_dist2;         // [B,Q,k] or null; +inf there
    int batch, n_query, n_points, k, self_exclude;
};
struct EvalZ5Args {
    const float* gt_head;    // [B,K,3] (the GT head subset, already negated as the scorer does)
    const float* pred_head;  // [B,K,3]
    int* counts;             // [B][n_anchors]
    int* order;              // [B][n_anchors][K] or null
    int anchors[kEvalMaxAnchors];
    int batch, n_head, sort_len, n_anchors;
};
dad3d_status launch_eval_nearest(const EvalNearestArgs& a, hipStream_t s);
dad3d_status launch_eval_z5(const EvalZ5Args& a, hipStream_t s);

// the UV-texture bake (uv_texture.hip, uv_texture_frames.hip): uv_texture.hpp, included below, outside this namespace

// the demo's overlays (overlay.hip): segments and discs over a per-image point table, drawn per pixel
struct OverlaySegmentsArgs {
    const uint8_t* src;     // [B,h,w,3]
    uint8_t* dst;           // [B,h,w,3], every byte written; may be src
    const float* points;    // [B,n_points,2] (x, y)
    const int* edges;       // [n_edges,2] into the point table, shared by the batch
    const uint8_t* colors;  // [n_edges,3] or null: `color` for every segment
    unsigned color;         // channel c in bits 8c .. 8c + 7
    int batch, h, w, n_points, n_edges;
    int thickness;          // 0: anti-aliased, one pixel wide; 1 .. 255: solid
};
struct OverlayDiscsArgs {
    const uint8_t* src;
    uint8_t* dst;
    const float* points;  // [B,n_points,2]
    const int* index;     // [n_discs] into the point table, or null: the first n_discs points
    unsigned color;
    int batch, h, w, n_points, n_discs, radius;
};
dad3d_status launch_overlay_segments(const OverlaySegmentsArgs& a, hipStream_t s);
dad3d_status launch_overlay_discs(const OverlayDiscsArgs& a, hipStream_t s);

// head pose and similarity alignment (head_pose.hip, pose_math.hpp): the same routines on the device and, `_host`, on the CPU
struct HeadPoseArgs {
    const float* params;        // row i's six rotation floats at params[i * row_stride + rot_offset ..]
    long long row_stride;       // in floats
    int rot_offset;
    int n;
    const long long* frames;    // [n_frames][4] {address, h, w, row stride}, or null: `h` x `w` for every row
    const int* image_index;     // [n] with `frames`
    int n_frames, h, w;
    float* rotation;            // [n,3,3] or null
    double* rpy;                // [n,3] or null
    float* points;              // [n,10,2] or null
    int* flags;                 // [n] or null
};
struct ProcrustesArgs {
    const double* x;            // [B,n,3]
    const double* y;            // [B,n,3]
    int batch, n_points;
    double* b;                  // [B]
    double* t;                  // [B,3,3]
    double* c;                  // [B,3]
    int* flags;                 // [B]
};
dad3d_status launch_head_pose(const HeadPoseArgs& a, hipStream_t s);
dad3d_status launch_procrustes(const ProcrustesArgs& a, hipStream_t s);
void head_pose_host(const HeadPoseArgs& a);
void procrustes_host(const ProcrustesArgs& a);

// the rest of the reference's training objective (train_objective.hip): heatmap target, heatmap IoU, visibility landmark
// loss, keypoint metrics
struct HeatmapEncodeArgs {
    void* out;                // [channels][size][size] float32 or uint8 (form), 16-byte aligned, every element written
    const float* keypoints;   // [channels][2] resized-image pixels
    const uint8_t* presence;  // [channels] (bool / uint8, non-zero = present)
    const void* table;        // [(2r+1)^2] the stamp in the output's form
    int* invalid;             // [1] += present points whose centre is NaN / inf, or null
    size_t channels;          // B * C
    float stride;
    int size, radius, form;
};
constexpr double kIouEps = 1e-6;  // keypoint_losses.py:12, metrics/iou.py:15
struct IouArgs {
    const float* pred;    // [channels][hw] logits (or probabilities: no sigmoid)
    const void* target;   // [channels][hw] float32 or uint8 (/ 255 fused in)
    double* sums;         // [channels][3] sum(t s), sum(t^2), sum(s^2)
    float* iou;           // [channels] or null
    float* loss;          // [2] = 1 - mean, mean; or null (terms only)
    float* accum;         // [2] += mean, += 1 (SoftIoUMetric's ious / total), or null
    const float* grad_out;  // [1] upstream gradient of the loss (backward)
    float* grad;            // [channels][hw] (backward)
    size_t channels;
    int hw;
    bool target_u8;
};
struct VisibilityLossArgs {
    const float* pred;             // [B,N,2]
    const float* pred_presence;    // [B,N]
    const float* target;           // [B,N,2]
    const float* target_presence;  // [B,N]
    float* loss;                   // [1]
    float* grad_pred;              // [B,N,2] dL/dpred for an upstream gradient of 1, or null
    int batch, n_points, criterion;
};
constexpr int kMaxThresholds = 8;
struct KeypointErrArgs {
    const float* pred;       // [B,V,D]
    const float* target;     // [B,V,D]
    const int* index;        // [n_points] into V, or null (the first n_points)
    const float* presence;   // [B,V] multiplies both, or null
    const int* bbox;         // [B,4] (x, y, w, h): norm sqrt(w h); null: 2.0
    double* err;             // [B][2] scratch: err, norm
    float* out;              // [1 + n_thresholds] NME, failure fractions; or null (per-item errors only)
    float* accum;            // [2 (1 + n_thresholds)] += (value, 1) pairs, or null
    double pred_scale, target_scale;
    double thresholds[kMaxThresholds];
    int batch, n_verts, n_points, dims, n_thresholds;
    bool cube, below;
};
dad3d_status launch_heatmap_encode(const HeatmapEncodeArgs& a, hipStream_t s);
dad3d_status launch_heatmap_iou(const IouArgs& a, bool sigmoid, bool vec, hipStream_t s);
dad3d_status launch_heatmap_iou_grad(const IouArgs& a, bool vec, hipStream_t s);
dad3d_status launch_visibility_loss(const VisibilityLossArgs& a, hipStream_t s);
dad3d_status launch_keypoint_errors(const KeypointErrArgs& a, hipStream_t s);

// training-batch ground truth (train_batch.hip): one lane per (item, subset point or vertex)
struct GtKeypointsArgs {
    const float* vertices;    // [B,nver,3]
    const float* model_view;  // [B,16] row-major
    const float* projection;  // [B,16] row-major
    const int* frames;        // [B,8] image height, crop x, y, w, h, pad_top, pad_left, 0
    const int* index;         // [n_subset] vertex ids (index mode), or null
    const int* corners;       // [n_subset,3] vertex ids of the embedding faces (68-landmark mode), or null
    const float* weights;     // [n_subset,3] barycentric weights (68-landmark mode)
    float* full;              // [B,nver,2]
    float* subset_px;         // [B,n_subset,2]
    float* subset_norm;       // [B,n_subset,2]
    uint8_t* presence;        // [B,n_subset]
    int nver, n_subset, out_size, mode;
};
dad3d_status launch_gt_keypoints(const GtKeypointsArgs& a, int batch, hipStream_t s);

// the .obj vertex text (obj_text.hip): `v %.8f %.8f %.8f\n` per vertex, the bytes MeshSaver writes (demo_utils.py:130-144)
struct ObjFormatArgs {
    const float* vertices;  // [B,N,3]
    unsigned char* text;    // [B][text_stride], 16-byte aligned rows; mesh b's lines start at b * text_stride
    size_t text_stride;     // >= N * DAD3D_OBJ_MAX_LINE_BYTES, a multiple of 16
    int64_t* lengths;       // [B] bytes of mesh b's text; 0 for a flagged mesh
    int32_t* flags;         // [B] DAD3D_OBJ_FLAG_* bits: the mesh holds a value outside the domain and has no text
    void* scratch;          // obj_format_scratch_bytes(B, N): {length, flag bits} per tile of 256 lines
    int batch, nver;
};
inline int obj_format_tiles(int nver) { return nver > 256 ? (nver + 255) / 256 : 1; }
size_t obj_format_scratch_bytes(int batch, int nver);
dad3d_status launch_obj_format(const ObjFormatArgs& a, hipStream_t s);

// JSON text from a layout template (json_text.hip): per item, literal bytes in front of each of n_slots numbers and a suffix; the
// numbers as json.dump prints a float32 widened to double (json_number.hpp)
struct JsonFormatArgs {
    const float* values;   // [B,n_slots]
    const void* literals;  // the template image: int32 offsets [n_slots + 2], then the literal bytes they index
    unsigned char* text;   // [B][text_stride], 16-byte aligned rows
    size_t text_stride;    // >= literal bytes + n_slots * DAD3D_JSON_MAX_NUMBER_BYTES, a multiple of 16
    int64_t* lengths;      // [B] bytes of item b's text; 0 for a flagged item
    int32_t* flags;        // [B] DAD3D_JSON_FLAG_* bits: the item holds NaN / inf and has no text
    void* scratch;         // json_format_scratch_bytes(B, n_slots): {length, flag bits} per tile of 256 slots
    int batch, n_slots;
};
inline int json_format_tiles(int n_slots) { return (n_slots + 255) / 256; }
size_t json_format_scratch_bytes(int batch, int n_slots);
dad3d_status launch_json_format(const JsonFormatArgs& a, hipStream_t s);
// host: text of values[i] at out + i * out_stride (DAD3D_JSON_MAX_NUMBER_BYTES at most), its length in lengths[i]; -1 for NaN / inf
void json_number_host(const float* values, size_t n, unsigned char* out, size_t out_stride, int* lengths);

// PNG files / zlib streams (png_encode.hip): filter, deflate per segment of DAD3D_PNG_SEGMENT_BYTES, assemble
struct DeflateArgs {
    const unsigned char* data;  // png: images [B,h,w,c]; else the streams [B,n]
    unsigned char* out;         // [B][out_stride], 16-byte aligned rows
    size_t out_stride;
    int64_t* lengths;           // [B]
    int32_t* flags;             // [B] DAD3D_PNG_FLAG_*
    void* scratch;              // png_scratch_bytes / zlib_scratch_bytes: the filtered streams | payload slots | segment records
    long long n;                // bytes per stream (zlib)
    int batch, png, h, w, c;
};
int png_segments(long long n);
long long png_stream_bytes(int h, int w, int c);
size_t png_max_bytes(int h, int w, int c);
size_t png_scratch_bytes(int batch, int h, int w, int c);
size_t zlib_max_bytes(long long n);
size_t zlib_scratch_bytes(int batch, long long n);
dad3d_status launch_deflate(const DeflateArgs& a, hipStream_t s);
// host: deflate_tables (deflate_tables.hpp) on one pair of histograms
dad3d_status deflate_tables_host(const unsigned* ll_hist, const unsigned* d_hist, unsigned char* ll_len, unsigned char* d_len, unsigned char* cl_len,
                                 unsigned short* ll_code, unsigned short* d_code, unsigned short* cl_code, unsigned char* header, int* header_bits,
                                 unsigned* dynamic_bits, unsigned* fixed_bits);

// PNG files / zlib streams read back (png_decode.hip): scan, inflate per segment, inflate or accept, unfilter and store
struct PngDecodeArgs {
    const unsigned char* files;  // every file of the batch, at the offsets of the descriptor rows
    size_t files_bytes;
    const long long* desc;       // DEVICE [B][DAD3D_PNG_DECODE_DESC_INTS]
    int batch, max_segments, force_general;
    unsigned char* out;
    size_t out_bytes;
    int32_t* flags;              // [B] DAD3D_PNG_DECODE_FLAG_*
    int32_t* info;               // [B] DAD3D_PNG_DECODE_INFO_*
    unsigned char* scratch;      // png_decode_layout: file states | per file: filtered stream, IDAT ranges, segment records
    size_t scratch_bytes;
};
size_t png_decode_layout(long long* desc_host, int batch, int* max_segments);
dad3d_status launch_png_decode(const PngDecodeArgs& a, hipStream_t s);
struct ZlibDecompressArgs {
    const unsigned char* streams;
    size_t streams_bytes;
    const long long* desc;  // DEVICE [B][DAD3D_ZLIB_DECODE_DESC_INTS]
    int batch;
    unsigned char* out;
    size_t out_bytes;
    int64_t* lengths;
    int32_t* flags;
};
dad3d_status launch_zlib_decompress(const ZlibDecompressArgs& a, hipStream_t s);
// JPEG files read back (jpeg_decode.hip): scan, entropy decode per segment, IDCT per block, upsampling and colour per pixel
struct JpegDecodeArgs {
    const unsigned char* files;  // every file of the batch, at the offsets of the descriptor rows
    size_t files_bytes;
    const long long* desc;       // DEVICE [B][DAD3D_JPEG_DECODE_DESC_INTS]
    int batch, max_segments, max_blocks, max_pixels;  // the grid dad3d_jpeg_decode_scratch_bytes gave
    unsigned char* out;
    size_t out_bytes;
    int32_t* flags;              // [B] DAD3D_JPEG_DECODE_FLAG_*
    unsigned char* scratch;      // jpeg_decode_layout: file states | per file: coefficients, planes, segment table
    size_t scratch_bytes;
};
size_t jpeg_decode_layout(long long* desc_host, int batch, int* grid);
size_t jpeg_decode_state_bytes();
dad3d_status launch_jpeg_decode(const JpegDecodeArgs& a, hipStream_t s);
dad3d_status launch_jpeg_scan(const JpegDecodeArgs& a, hipStream_t s);    // the scan alone, and the IDCT and the colour launch alone:
dad3d_status launch_jpeg_pixels(const JpegDecodeArgs& a, hipStream_t s);  // around the entropy stage of jpeg_decode_sync.hip
// host: one file through jpeg_entropy.hpp / jpeg_idct.hpp; returns the flag (out null: the header alone). piece_bytes != 0: the
// entropy stage of jpeg_sync.hpp, which fills info[4] (mode, pieces, groups, 0)
int jpeg_decode_host(const unsigned char* file, long long size, int channels, unsigned char* out, long long out_bytes, int* h, int* w, int* c,
                     bool* fits, int piece_bytes = 0, int* info = nullptr);
// JPEG files read back, the entropy data of a file without restart markers decoded in pieces (jpeg_decode_sync.hip, jpeg_sync.hpp)
struct JpegDecodeSyncArgs {
    JpegDecodeArgs base;  // desc: DEVICE [B][DAD3D_JPEG_DECODE_DESC_INTS] and behind them [B][4]: the piece and group tables
    int piece_bytes, max_groups;
    int32_t* info;        // [B][4]
};
size_t jpeg_decode_sync_layout(long long* desc_host, int batch, int* grid, int piece_bytes);
dad3d_status launch_jpeg_decode_sync(const JpegDecodeSyncArgs& a, hipStream_t s);
// JPEG files written (jpeg_encode.hip): samples to coefficients per block, then per image the bits, byte stuffing and the framing
struct JpegEncodeArgs {
    const unsigned char* images;  // [B,h,w,c]
    int batch, h, w, c, quality, subsampling, restart_interval;
    unsigned char* out;           // [B][out_stride], 16-byte aligned rows
    size_t out_stride;
    int64_t* lengths;             // [B]
    int32_t* flags;               // [B] DAD3D_JPEG_ENCODE_FLAG_*
    void* scratch;                // jpeg_encode_scratch_bytes: coefficients [B][blocks][64] int16 | block records [B][blocks]
};
size_t jpeg_encode_max_bytes(int h, int w, int c, int subsampling);  // 0 for a shape outside the limits
size_t jpeg_encode_scratch_bytes(int batch, int h, int w, int c, int subsampling);
dad3d_status launch_jpeg_encode(const JpegEncodeArgs& a, hipStream_t s);
// host: one image through jpeg_fdct.hpp / jpeg_huff_encode.hpp; returns the flag
int jpeg_encode_host(const unsigned char* image, int h, int w, int c, int quality, int subsampling, int restart_interval, unsigned char* out,
                     long long capacity, long long* length);
// host: inflate.hpp on a list of byte ranges; returns the flag
int inflate_host(const unsigned char* const* ranges, const long long* range_bytes, int n_ranges, unsigned char* out, long long capacity,
                 long long* length);

// JSON read back on the device (json_parse.hip): index the document, compact its token and bracket lists, check candidate arrays, extract
// the values of the lifted ones; the entries of include/dad3d.h one to one
struct JsonParseListsArgs {
    const void* scratch;
    int32_t *tok_pos, *tok_brk, *brk_pos, *brk_key, *brk_nonnum, *brk_tok;
    long long n_bytes, tok_cap, brk_cap;
};
struct JsonParseCheckArgs {
    const unsigned char* text;
    const int32_t *tok_pos, *tok_brk, *brk_pos, *brk_key, *brk_tok, *arr_open, *arr_close;
    int32_t* arr_rows;
    long long n_bytes, n_tokens, n_brackets, n_arrays;
};
struct JsonParseExtractArgs {
    const unsigned char* text;
    const int32_t *tok_pos, *records;
    double* values;
    unsigned char* is_int;
    long long n_bytes, n_tokens, n_records, n_values;
};
int json_parse_tiles(long long n_bytes);
size_t json_parse_scratch_bytes(long long n_bytes);
dad3d_status launch_json_parse_index(const unsigned char* text, long long n_bytes, void* scratch, int* counts, hipStream_t s);
dad3d_status launch_json_parse_lists(const JsonParseListsArgs& a, hipStream_t s);
dad3d_status launch_json_parse_check_arrays(const JsonParseCheckArgs& a, hipStream_t s);
dad3d_status launch_json_parse_extract(const JsonParseExtractArgs& a, hipStream_t s);
// host: the number routine on token i = text[starts[i], ends[i])
void json_parse_number_host(const unsigned char* text, const long long* starts, const long long* ends, size_t n, unsigned long long* bits,
                            unsigned char* is_int, unsigned* flags);

// DAD-3DHeads annotation files read on the device (annotation_parse.hip): one workgroup per document, one launch per batch
struct AnnotationParseArgs {
    const unsigned char* text;
    long long n_bytes;
    const long long *doc_offsets, *doc_sizes;
    int batch, n_verts;
    float *vertices, *model_view, *projection;
    int32_t* status;
};
dad3d_status launch_annotation_parse(const AnnotationParseArgs& a, hipStream_t s);

// predictor preprocessing (preprocess.hip): descs = [B][8] int64 on the device: {src pointer, h, w, new_h, new_w, pad_top,
// pad_left, row stride in bytes}
dad3d_status launch_preprocess(const long long* descs, int batch, int out_size, const float mean[3], const float std[3],
                               float* out, hipStream_t s);

// DAD-3DNet glue (cnn_glue.hip): NHWC tensors, dtype = DAD3D_DTYPE_*
dad3d_status launch_nhwc_bias_act(void* y, const void* bias, const void* z, size_t n_pixels, int channels, int dtype, int relu,
                                  hipStream_t s);
dad3d_status launch_nhwc_resize_sum(void* out, int n, int oh, int ow, int channels, int dtype, int n_inputs, const void* const* xs,
                                    const int* hs, const int* ws, const float* weights, hipStream_t s);

// the forward's tail (net_tail.hip): the fusion layer's input and output, the regression heads
dad3d_status launch_nhwc_fusion_concat(void* out, const void* x, const void* heat, const void* level, int n, int oh, int ow, int hh, int hw,
                                       int cx, int ch, int cl, int dtype, hipStream_t s);
dad3d_status launch_nhwc_bias_mul(void* y, const void* bias, const void* x, size_t n_pixels, int channels, int dtype, hipStream_t s);
struct RegressionHeadsArgs {
    const void* top;  // [batch, hw, channels]
    int batch, channels, hw, dtype, n_heads;
    dad3d_head_desc head[DAD3D_HEADS_MAX];
    float *pooled, *hidden;  // float32 [batch, channels] and [batch, sum of hidden]: the stages between the three launches
};
dad3d_status launch_regression_heads(const RegressionHeadsArgs& a, hipStream_t s);

// heatmap peaks and the landmark readjustment (heatmap_points.hip): dtype = DAD3D_DTYPE_* or DAD3D_HEATMAP_DTYPE_U8, layout = DAD3D_LAYOUT_*
struct HeatmapArgmaxArgs {
    const void* heatmap;
    int dtype, batch, channels, h, w, layout, sigmoid;
    int32_t* yx;  // [B,C,2] (k // H, k % H)
    float* peak;  // [B,C] or null
    int n_split;  // set by the launcher: workgroups per channels-last image
};
dad3d_status launch_heatmap_argmax(const HeatmapArgmaxArgs& a, hipStream_t s);
struct PointsReadjustArgs {
    const void* src;  // src_kind 0: float32 (x, y); 1: int32 (row, col)
    int src_kind, batch, n_points;
    float mul, limit;
    const double* geometry;  // [B,3] (pad_left, pad_top, scale) or null: the triple below
    int pad_left, pad_top;
    double scale;
    int32_t* points;
};
dad3d_status launch_points_readjust(const PointsReadjustArgs& a, hipStream_t s);

// frames + bounding boxes -> network input, and a crop's results moved into its frame (preprocess_boxes.hip)
struct PreprocessBoxesArgs {
    const long long* images;  // [M][4] {address, h, w, row stride in bytes}
    int n_images;
    const void* boxes;  // [N][4] (x, y, w, h) of box_dtype
    int box_dtype;
    const int32_t* image_index;  // [N]
    int n_boxes;
    int has_offset;
    double left, right, top, bottom;  // extend_bbox's factors
    int out_size, out_format;
    float3 mean255, inv_std255;
    void* out;
    int32_t* crops;    // [N][4]
    double* geometry;  // [N][5] (pad_left, pad_top, scale, x, y)
    int32_t* flags;    // [N]
};
dad3d_status launch_preprocess_boxes(PreprocessBoxesArgs a, const float mean[3], const float std[3], hipStream_t s);
// geometry: [B][5] as above
dad3d_status launch_readjust_frame(float* params, int batch, ParamLayout lay, const double* geometry, float img_size, hipStream_t s);
dad3d_status launch_points_readjust_frame(const PointsReadjustArgs& a, hipStream_t s);  // a.geometry is [B][5]

// the projected vertices of a call's heads -> the boxes of the next call (track_boxes.hip)
struct TrackBoxesArgs {
    const float* proj;  // head i's vertex v at proj + i*head_stride + v*vertex_stride: x at +0, y at +1
    int n_heads, n_verts;
    long long head_stride;
    int vertex_stride;
    const int32_t* subset;  // [n_subset] vertex indices, or null: all
    int n_subset;
    const long long* frames;  // [M][4] {address, h, w, row stride in bytes}
    int n_frames;
    const int32_t* image_index;  // [N]
    const int32_t* prev_flags;   // [N] or null
    int min_side;
    double min_visible;
    int32_t* boxes;  // [N][4] (x, y, w, h)
    int32_t* flags;  // [N]
};
dad3d_status launch_boxes_from_heads(const TrackBoxesArgs& a, hipStream_t s);

// steady tracks (track_steady.hip): the One-Euro filter over the rows of a matrix, and the suppression of duplicate slots
struct OneEuroArgs {
    const float* x;  // row i at x + i*x_stride
    long long x_stride;
    float* out;  // may be x itself (then with x's stride)
    long long out_stride;
    int n, d;
    const int32_t* flags;                 // [N] or null
    const float *min_cutoff, *beta;       // [D]
    float rate, two_pi_dt, alpha_d;       // the host's three scalars
    float *state_x, *state_dx;            // [N][D], contiguous
    int32_t* age;                         // [N]
};
dad3d_status launch_one_euro_rows(const OneEuroArgs& a, hipStream_t s);
struct SuppressDuplicatesArgs {
    int32_t* boxes;  // [N][4] (x, y, w, h), in place
    int32_t* flags;  // [N], in place
    const int32_t* image_index;  // [N]
    int n;  // 1 .. DAD3D_TRACK_MAX_SLOTS
    double merge_iou;
};
dad3d_status launch_suppress_duplicates(const SuppressDuplicatesArgs& a, hipStream_t s);

// detections into tracks (track_assign.hip): match, spawn and retire slots in one launch
struct AssignDetectionsArgs {
    int32_t* boxes;        // [N][4] (x, y, w, h), in place
    int32_t* flags;        // [N], in place
    int32_t* image_index;  // [N], in place
    int32_t* misses;       // [N], in place, or null
    int n;                 // 0 .. DAD3D_TRACK_MAX_SLOTS
    const int32_t* det_boxes;       // [M][4]
    const int32_t* det_index;       // [M]
    const int32_t* det_count;       // one word, or null: all M
    int m;                          // 0 .. DAD3D_TRACK_MAX_DETECTIONS
    const int32_t* frame_searched;  // [n_frames] or null: all
    int n_frames;
    double match_iou;
    int refresh, max_misses;
    int32_t *assign, *det_flags;  // [M]
    int32_t* spawned;             // [N]
};
dad3d_status launch_assign_detections(const AssignDetectionsArgs& a, hipStream_t s);

}  // namespace dad3d

#include "uv_texture.hpp"
