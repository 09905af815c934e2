/*
 * dad3d.h -- C ABI of libdad3d_hip.so, the MI355X (gfx950) implementation of the DAD-3DNet
 * mesh-decode hot path: FLAME/HeadMesh decode -> weak-perspective projection -> landmark gather,
 * and the Sim3DR vertex-normal / z-buffer rasterisation loops.
 *
 * Plain C, no torch types: pointers + sizes only. Unless a function says "host", every buffer is a
 * DEVICE pointer (HBM of the device the handle was created on) and every call is ASYNCHRONOUS on the
 * `hipStream_t` passed as `void* stream` (NULL = the default stream). Every function returns a
 * dad3d_status; nothing throws across the boundary. dad3d_last_error() gives a thread-local message.
 *
 * Each entry point cites the reference interface it replaces (paths relative to the reference root).
 */
#ifndef DAD3D_H_
#define DAD3D_H_

#include <stddef.h>
#include <stdint.h>

/* libdad3d_hip.so is built with -fvisibility=hidden: the functions declared here and the five C++-linkage Sim3DR doubles of
 * csrc/sim3dr_compat.cpp are its ENTIRE dynamic symbol table (tests/test_capi_symbols.py holds `nm -D` to that). */
#ifndef DAD3D_EXPORT
#define DAD3D_EXPORT __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define DAD3D_VERSION 100 /* 0.1.0 */

typedef enum dad3d_status {
    DAD3D_OK = 0,
    DAD3D_E_INVALID = 1,     /* bad argument (NULL, negative size, shape mismatch) */
    DAD3D_E_HIP = 2,         /* a HIP runtime call failed; see dad3d_last_error() */
    DAD3D_E_UNSUPPORTED = 3, /* valid in the reference but not implemented here (documented) */
    DAD3D_E_NOMEM = 4
} dad3d_status;

DAD3D_EXPORT const char* dad3d_last_error(void);
DAD3D_EXPORT void dad3d_clear_error(void); /* reset the thread-local message to "" */
DAD3D_EXPORT int dad3d_version(void);
/* The toolchain pair, for benchmark records: "built: clang <version>, HIP headers a.b.c; running: HIP runtime <n>, driver <n>" -- the
 * compiler and headers this library was built with (the authoring container) and the runtime it is loaded against (the GPU box). */
DAD3D_EXPORT const char* dad3d_build_info(void);
/* Number of visible HIP devices (0 when there is none). Host-only, launches nothing. */
DAD3D_EXPORT int dad3d_device_count(void);

/* ------------------------------------------------------------------------------------------------
 * FLAME / HeadMesh decode
 * ---------------------------------------------------------------------------------------------- */

/* HOST pointers to the FLAME constants exactly as `FLAMELayer.__init__` registers them
 * (model_training/model/flame.py:124-180), all C-contiguous fp32 unless noted. */
typedef struct dad3d_flame_model {
    int32_t n_verts;          /* V = 5023 */
    int32_t n_betas;          /* MAX_SHAPE + MAX_EXPRESSION = 400 (flame.py:107-108) */
    int32_t n_joints;         /* J = 5 */
    const float* v_template;  /* [V,3]                       flame.py:157 */
    const float* shapedirs;   /* [V,3,n_betas]               flame.py:160-163 */
    const float* posedirs;    /* [(J-1)*9, 3V] (already reshaped+transposed, flame.py:169-173) */
    const float* j_regressor; /* [J,V] dense                 flame.py:165-166 */
    const int32_t* parents;   /* [J], root = -1              flame.py:175-178 */
    const float* lbs_weights; /* [V,J]                       flame.py:180 */
} dad3d_flame_model;

/* The `constants` dict of dad_3dnet.yaml:4-12 / FLAME_CONSTS (flame.py:17-26). The params vector is
 * sliced in `FlameParams.from_3dmm` order (flame.py:48-73):
 *   shape | expression | jaw | rotation | eyeballs | neck | translation | scale                   */
typedef struct dad3d_flame_consts {
    int32_t shape, expression, jaw, rotation, eyeballs, neck, translation, scale;
} dad3d_flame_consts;

typedef struct dad3d_flame dad3d_flame; /* opaque: packed basis + scratch resident in HBM */

/* decode flags */
#define DAD3D_ZERO_ROTATION 0x1u /* skip the 6-DoF rotation        (flame.py:225 `zero_rot`) */
#define DAD3D_TO_2D 0x2u         /* `proj` is [B,V,2] not [B,V,3]  (head_mesh.py:44-45 `to_2d`) */
#define DAD3D_MUTATE_PARAMS 0x4u /* write translation z := 0 back into `params`, the side effect of
                                    HeadMesh.reprojected_vertices (head_mesh.py:41) */
#define DAD3D_FLIP_Z 0x8u        /* negate proj z (inference/pncc_estimator.py:88), needs !TO_2D */
#define DAD3D_COMPAT_CROSS_B3 0x10u /* opt-in bug compatibility: model_training/model/utils.py:98-99 calls torch.cross WITHOUT
                                    `dim`; for a batch of EXACTLY three rows torch's legacy rule takes the first axis of size
                                    3 -- the batch axis -- so the three images' 6-DoF rotations mix. With this flag a batch of
                                    three reproduces that (every other batch size is unaffected); without it (default) every
                                    image gets its own Gram-Schmidt rotation, as for any other batch size. INFERENCE ONLY:
                                    dad3d_flame_decode_posed refuses it (the backward pass differentiates the per-image rotation) */

/* Upload + repack the model for `device`. Replaces FLAMELayer.__init__ (flame.py:124-180) and
 * HeadMesh.__init__ (head_mesh.py:10-22). `image_size` is HeadMesh._image_size (256). */
DAD3D_EXPORT dad3d_status dad3d_flame_create(const dad3d_flame_model* model, const dad3d_flame_consts* consts, float image_size,
                                int device, dad3d_flame** out);
DAD3D_EXPORT void dad3d_flame_destroy(dad3d_flame* h);
/* A second handle on the same device that SHARES the model constants of `parent` (26 MB, reference counted: either may
 * be destroyed first) and its current landmark list (until either handle calls dad3d_flame_set_landmarks, which changes that
 * handle's list only), and owns its hand-off buffers and scratch. A handle serves one stream at a time -- its pose-role ->
 * decode-role hand-off block and its split-kernel scratch, which landmark-only launches use too, are per handle -- so a serving
 * loop that keeps several batches in flight uses one fork per stream (bench.py does, with two). */
DAD3D_EXPORT dad3d_status dad3d_flame_fork(dad3d_flame* parent, dad3d_flame** out);

/* Number of floats per params row (sum of the consts; 413 for dad_3dnet.yaml). */
DAD3D_EXPORT int dad3d_flame_num_params(const dad3d_flame* h);
DAD3D_EXPORT int dad3d_flame_num_verts(const dad3d_flame* h);

/* Ordered landmark index list (HOST int64, e.g. the 445 list of model_training/utils.py:62-105 or the
 * per-file lists demo_utils.py:44-46 walks). Duplicates allowed. Replaces np.take(..., indices, axis=0). */
DAD3D_EXPORT dad3d_status dad3d_flame_set_landmarks(dad3d_flame* h, const int64_t* indices, int n);
DAD3D_EXPORT int dad3d_flame_num_landmarks(const dad3d_flame* h);
/* Landmark-only launches (every vertex output NULL, a landmark output given -- BASELINE configs[3]'s per-GPU work, the landmark-only fast
 * path of SURVEY 7.1) on the pipelined or a split kernel run on the SUB-MODEL of the distinct vertices the list names, built by
 * dad3d_flame_set_landmarks: 445 of 5023 vertices = 23 column tiles instead of 252, with the batch cut into chunks across workgroups so that
 * the launch still fills the GPU. Same kernel, same basis values in the same order: lmk_xy / lmk_px of such a launch are BIT-IDENTICAL to
 * those of a full-output launch of the same handle, at every batch size (tests/test_gpu_landmark_subset.py). This returns the number of
 * vertices of that sub-model, 0 when there is none (empty list, a list naming more than a third of the mesh, a model the pipelined kernel
 * does not cover, DAD3D_LANDMARK_SUBSET=0). A launch that takes the two-role kernel (DAD3D_ZERO_ROTATION, outputs of the whole mesh past
 * 2 GB, an uncovered model), a handle pinned with dad3d_flame_select_kernel(TWO_ROLE / PIPELINED) and a tracing handle decode the whole
 * mesh for such a launch like for any other. */
DAD3D_EXPORT int dad3d_flame_num_landmark_vertices(const dad3d_flame* h);

/* One fused decode of B parameter rows. Any output pointer may be NULL (not produced).
 *   params  [B,P] fp32 (read; tz written when DAD3D_MUTATE_PARAMS)
 *   verts3d [B,V,3]  == HeadMesh.vertices_3d(params, zero_rotation)            head_mesh.py:28-31
 *   proj    [B,V,2|3]== HeadMesh.reprojected_vertices(params, to_2d)           head_mesh.py:33-46
 *                       (always rotated; DAD3D_ZERO_ROTATION applies to verts3d only, as in the reference)
 *   lmk_xy  [B,n,2] fp32 = proj[:, idx, :2]
 *   lmk_px  [B,n,2] int32 = projected.astype(int)[idx]  (truncation)           demo_utils.py:42,46
 * The reference needs two full decodes for verts3d + proj (predictor.py:136-137); this is one.
 * A call with verts3d == proj == NULL and a landmark output decodes only the vertices the landmark list names (see
 * dad3d_flame_num_landmark_vertices above), with the same bits a full-output launch returns for them.
 * hipGraph: the call may be captured (hipStreamBeginCapture on `stream`) after one warm-up call with the same batch
 * size; a captured launch keeps its hand-off bookkeeping on the device, so the graph can be replayed any number of
 * times and interleaved with direct calls (about 1.6 us slower per launch than a direct call). The raster and
 * lighting entry points below are capturable as they are (warm up once with the same shapes). */
DAD3D_EXPORT dad3d_status dad3d_flame_decode(dad3d_flame* h, float* params, int batch, unsigned flags, float* verts3d, float* proj,
                                float* lmk_xy, int32_t* lmk_px, void* stream);

/* The same launch for callers that will differentiate: additionally stores posed [B,V,3] = v_posed (template + blend
 * shapes + pose correctives, i.e. smplx lbs before skinning), the operand dad3d_flame_decode_backward needs. No
 * landmark outputs. */
DAD3D_EXPORT dad3d_status dad3d_flame_decode_posed(dad3d_flame* h, float* params, int batch, unsigned flags, float* verts3d, float* proj,
                                      float* posed, void* stream);

/* Vertex half of the BACKWARD pass of dad3d_flame_decode, for the reference's training callers that differentiate
 * through HeadMesh (model_training/losses/vertices_3d_loss.py:41 `vertices_3d(..., zero_rotation=True)`,
 * reprojection_loss.py:33 `reprojected_vertices(..., to_2d=True)`; the reference gets these gradients from torch
 * autograd over flame.py:182-229 + smplx.lbs.lbs). All pointers are DEVICE pointers; `flags` as in the forward call.
 *   consts       [B,72]  per-image constants of the forward pass: rows 0..2 of the five relative joint transforms A_j
 *                        (smplx batch_rigid_transform, natural joint order, 12 floats each), the 6-DoF rotation matrix
 *                        (9, row-major), s = clamp(scale + 1, 1e-8), tx, ty
 *   posed        [B,V,3] v_posed = template + blend shapes + pose correctives (smplx lbs, before skinning)
 *   grad_verts3d [B,V,3] dL/d(verts3d) or NULL      grad_proj [B,V,2|3] dL/d(proj) or NULL (at least one given)
 *   grad_posed   [B,V,3] OUT: dL/d(v_posed) -- multiply by the blend-shape basis transposed for dL/d(betas, pose feature)
 *   grad_consts  [B,72]  OUT: dL/d(consts), summed over the vertices (deterministic: one workgroup per image)
 * The constants are small differentiable functions of (jaw/neck/eye pose, joints(betas), rot6d, scale, translation);
 * the host mirror (dad_3dheads_amd/autograd.py) takes their derivatives and runs the two library GEMMs. */
DAD3D_EXPORT dad3d_status dad3d_flame_decode_backward(dad3d_flame* h, int batch, unsigned flags, const float* consts, const float* posed,
                                         const float* grad_verts3d, const float* grad_proj, float* grad_posed,
                                         float* grad_consts, void* stream);

/* dL/d[betas | pose feature] = dL/d(v_posed) . basis^T: the transpose of the blend-shape GEMM of flame.py:212-221 (what torch
 * autograd does for the reference's losses, vertices_3d_loss.py:41), a split-K fp32 MFMA kernel + a fixed-order reduction.
 *   grad_posed [B, 3V] (from dad3d_flame_decode_backward)  ->  grad_inputs [B, dad3d_flame_num_chain_inputs(h)]
 * The basis^T pack and the scratch are created by the first dad3d_flame_decode_posed of the handle (of a larger batch) when
 * the batch is at most DAD3D_GRAD_INPUTS_MAX_BATCH -- the range the host mirror uses this entry for (above it a library GEMM
 * is faster) -- and by the first call of this entry otherwise: run one step before capturing a graph. */
#define DAD3D_GRAD_INPUTS_MAX_BATCH 96
DAD3D_EXPORT dad3d_status dad3d_flame_grad_inputs(dad3d_flame* h, const float* grad_posed, int batch, float* grad_inputs, void* stream);

/* Per-image half of the same differentiable decode: everything between a params row and the operands of the per-vertex
 * work (flame.py:191-210 betas / full_pose assembly, smplx batch_rodrigues + batch_rigid_transform + vertices2joints,
 * model/utils.py:92-101 rot_mat_from_6dof, head_mesh.py:39-41 scale / translation).
 *   inputs  [B, K] fp32, K = dad3d_flame_num_chain_inputs() = 400 + 36: [betas | pose feature], the A operand of the
 *           blend-shape contraction (v_posed = template + inputs . basis)
 *   consts  [B,72] as described above
 * ..._backward is its vector-Jacobian product: grad_params [B,P] (every entry written; translation z gets 0) from
 * grad_inputs [B,K] and grad_consts [B,72]. The derivative is taken with dual numbers over the SAME device code that
 * computes the forward values (one lane per input direction), so the two cannot drift apart. */
DAD3D_EXPORT int dad3d_flame_num_chain_inputs(const dad3d_flame* h);
DAD3D_EXPORT dad3d_status dad3d_flame_pose_chain(dad3d_flame* h, const float* params, int batch, float* inputs, float* consts, void* stream);
DAD3D_EXPORT dad3d_status dad3d_flame_pose_chain_backward(dad3d_flame* h, const float* params, int batch, const float* grad_inputs,
                                             const float* grad_consts, float* grad_params, void* stream);

/* Same, HOST buffers in and out (synchronous; PCIe-inclusive convenience for non-HIP callers). */
DAD3D_EXPORT dad3d_status dad3d_flame_decode_host(dad3d_flame* h, float* params, int batch, unsigned flags, float* verts3d,
                                     float* proj, float* lmk_xy, int32_t* lmk_px);

/* predictor.readjust_3dmm_to_the_input_image (predictor.py:154-176), in place on device params:
 *   s' = (s+1)/scale - 1 ;  t' = (t + 1 - [pad_left,pad_top,0]*2/img_size)/scale - 1
 * `pads_scale` is a DEVICE array [B,3] = (pad_left, pad_top, scale) per row, or NULL with the three
 * scalars applied to every row. */
DAD3D_EXPORT dad3d_status dad3d_flame_readjust_params(dad3d_flame* h, float* params, int batch, const float* pads_scale,
                                         float pad_left, float pad_top, float scale, void* stream);

/* Timing aid for bench.py: `_begin` records a hipEvent on `stream`, `_end` records a second one on the same
 * stream, synchronises on it and returns the elapsed milliseconds and the number of decode launches issued
 * through this handle in between. With one fused kernel per decode and launches issued back to back,
 * total_ms / launches is that kernel's average duration including the inter-launch gap. */
DAD3D_EXPORT dad3d_status dad3d_flame_profile_begin(dad3d_flame* h, void* stream);
DAD3D_EXPORT dad3d_status dad3d_flame_profile_end(dad3d_flame* h, void* stream, double* total_ms, int* launches);
/* How many decode workgroups ever gave up waiting for the pose role's hand-off and recomputed the per-image
 * constants themselves (still correct, slower). Expected 0; synchronises the device. */
DAD3D_EXPORT dad3d_status dad3d_flame_handoff_timeouts(dad3d_flame* h, unsigned* count);
/* Which kernel a decode launch of this handle takes: DAD3D_KERNEL_AUTO (default) = the pipelined single-role kernel
 * (csrc/flame_decode_pipe.hip) whenever it covers the launch -- jaw-only model with the dad_3dnet.yaml params layout, inference outputs,
 * no DAD3D_ZERO_ROTATION / DAD3D_COMPAT_CROSS_B3 -- and the two-role kernel (csrc/flame_decode.hip) otherwise; DAD3D_KERNEL_TWO_ROLE
 * forces the latter; DAD3D_KERNEL_PIPELINED returns DAD3D_E_UNSUPPORTED from a decode the pipelined kernel does not cover instead of
 * falling back. DAD3D_KERNEL_SPLIT_BF16 (round 6, never chosen automatically) = the same decode with the blend-shape contraction on the
 * bf16 matrix pipe as an exact-product split (csrc/flame_decode_split.hip): params rows and basis are each split into three bf16
 * planes with exact residuals and six of the nine plane products are accumulated in fp32 -- measured MORE accurate against float64 than
 * the fp32 MFMA chain (profiles/r06_split_error.md) and held to the same bars by the same tests, but NOT bit-identical to the default
 * kernel; same model coverage as the pipelined kernel (DAD3D_E_UNSUPPORTED otherwise), two launches per decode, its first call at a
 * batch size allocates (warm up before capturing a graph). DAD3D_KERNEL_SPLIT_F16 = the same kernel with the operands as TWO fp16
 * planes (22 significant bits; params rows x 16 and the basis x a power of two chosen at dad3d_flame_create so that no residual
 * underflows -- exact scalings) and three products: half the matrix instructions, about 1.4x the speed of the bf16 form at large
 * batches, error against float64 between the bf16 form's and the fp32 chain's (same file); a params entry beyond +-4094 makes ITS
 * row inf/NaN in this form only. The first decode of a model in this form also builds the
 * basis as two fp16 planes on the device (26.7 MB for the whole mesh, shared by forks; not inside a graph capture). A handle on a split form runs its
 * landmark-only launches on the sub-model in the SAME form (bit-identical
 * to its whole-mesh launches). The environment variable DAD3D_DECODE_KERNEL=v1|force_pipe|split|split_f16 sets the
 * process-wide default for handles that have not chosen (A/B timing; anything else = automatic). */
#define DAD3D_KERNEL_AUTO 0
#define DAD3D_KERNEL_TWO_ROLE 1
#define DAD3D_KERNEL_PIPELINED 2
#define DAD3D_KERNEL_SPLIT_BF16 3
#define DAD3D_KERNEL_SPLIT_F16 4
DAD3D_EXPORT dad3d_status dad3d_flame_select_kernel(dad3d_flame* h, int which);
/* Diagnostics: a DEVICE buffer of `capacity` uint64 entries that every wave of the decode kernel fills with shader-clock stamps
 * (32 entries per wave; slots 12 / 13 = the 100 MHz wall clock at the wave's start / end); NULL switches it off. The two kernels
 * lay it out differently:
 *   pipelined   [tiles = ceil(V/20)][8 waves][32]                       slots 0.. = per half-block phase stamps (tools/trace_pipe.py)
 *   two-role    [8*ceil(ceil(V/21)/8) * ceil(B/64) decode workgroups][8 waves][32], then [4*ceil(B/4) pose waves, padded to 8
 *               workgroups][32]: 0 start, 1 loads issued, 2 operands landed, 3 GEMM done, 4 tile staged, 5 end (tools/trace_decode.py)
 * dad3d_flame_debug_trace_entries(h, batch) = the entries a launch of `batch` images can write (the larger of the two layouts);
 * while a trace buffer is set, a decode whose stamps would not fit its `capacity` returns DAD3D_E_INVALID instead of launching. */
DAD3D_EXPORT dad3d_status dad3d_flame_debug_trace(dad3d_flame* h, unsigned long long* device_buffer, uint64_t capacity);
DAD3D_EXPORT uint64_t dad3d_flame_debug_trace_entries(const dad3d_flame* h, int batch);

/* ------------------------------------------------------------------------------------------------
 * Sim3DR: vertex normals + z-buffer rasterisation
 * ---------------------------------------------------------------------------------------------- */

typedef struct dad3d_mesh dad3d_mesh; /* opaque: triangle list + vertex->face adjacency in HBM */

/* `triangles` HOST int32 [ntri,3] (numpy intc, as Sim3DR/lib/rasterize.pyx:63-69 requires). */
DAD3D_EXPORT dad3d_status dad3d_mesh_create(const int32_t* triangles, int ntri, int nver, int device, dad3d_mesh** out);
DAD3D_EXPORT void dad3d_mesh_destroy(dad3d_mesh* m);

#define DAD3D_NORMAL_ACCUMULATE 0x1u /* add onto the existing content of `ver_normal` like the C function does;
                                        default = start from zero like Sim3DR/Sim3DR.py:9 */
/* Batched `_get_normal` (Sim3DR/lib/rasterize_kernel.cpp:158-215; rasterize.h:92).
 *   vertices [B,nver,3] fp32 -> ver_normal [B,nver,3] fp32. Bit-exact with the reference. */
DAD3D_EXPORT dad3d_status dad3d_mesh_get_normal(dad3d_mesh* m, float* ver_normal, const float* vertices, int batch,
                                   unsigned flags, void* stream);
/* Batched `_get_tri_normal` (rasterize_kernel.cpp:87-120): tri_normal [B,ntri,3]. */
DAD3D_EXPORT dad3d_status dad3d_mesh_get_tri_normal(dad3d_mesh* m, float* tri_normal, const float* vertices, int batch,
                                       int norm_flg, void* stream);
/* Batched `_get_ver_normal` (rasterize_kernel.cpp:125-153): tri_normal [B,ntri,3] -> ver_normal [B,nver,3]. */
DAD3D_EXPORT dad3d_status dad3d_mesh_get_ver_normal(dad3d_mesh* m, float* ver_normal, const float* tri_normal, int batch,
                                       unsigned flags, void* stream);

/* Batched `_rasterize` (rasterize_kernel.cpp:219-292; rasterize.h:98-100).
 *   image    [B,h,w,c] uint8, read-modify-write (background in, render out)
 *   vertices [B,nver,3] fp32 (pixel x, pixel y, depth); colors [B,nver,c] fp32 in [0,1]
 *   depth    [B,h,w] fp32 in/out, or NULL = start from -1e8 (Sim3DR/Sim3DR.py:23) and discard
 *   alpha == 1 (the only value Python can reach: Sim3DR.py:27-28, rasterize.pyx:95): the z-buffer kernels below.
 *   alpha != 1: the reference blends every triangle that improves a pixel's depth, in triangle order (rasterize_kernel.cpp:276-281);
 *   `raster_blend_kernel` replays exactly that chain per pixel -- bit-exact, for c = 1..4 channels. NaN alpha and c outside 1..4
 *   return DAD3D_E_INVALID (the reference accepts any c; nothing in it passes another).
 * Bit-exact with the reference for alpha == 1: strict-interior test, `>` depth test, ties to the
 * lowest triangle index, (unsigned char) truncation.
 * Scratch: the handle owns device memory for the per-image triangle records, the 64x64-tile lists and the work queue
 * (about (48 + 4 * tiles) * ntri bytes per image, allocated on first use and when (B, h, w) grows -- that call
 * synchronises the device). One handle serves one stream at a time; use one handle per concurrent stream.
 * Limits: at most 4096 tiles of 64x64 pixels per image (4096 x 4096, 16384 x 1024, ...), B * tiles < 2^24,
 * ntri < 2^28; beyond them DAD3D_E_INVALID with a message. */
DAD3D_EXPORT dad3d_status dad3d_mesh_rasterize(dad3d_mesh* m, uint8_t* image, const float* vertices, const float* colors,
                                  float* depth, int batch, int h, int w, int c, float alpha, int reverse,
                                  void* stream);
/* Batched `_rasterize_triangles` (rasterize_kernel.cpp:295-353): depth [B,h,w] in/out (required),
 * triangle_buffer [B,h,w] int32 and barycentric [B,h,w,3] fp32 written where a triangle wins. */
DAD3D_EXPORT dad3d_status dad3d_mesh_rasterize_triangles(dad3d_mesh* m, const float* vertices, float* depth,
                                            int32_t* triangle_buffer, float* barycentric, int batch, int h, int w,
                                            void* stream);

/* Per-vertex Phong lighting of Sim3DR/lighting.py:37-62 (`RenderPipeline.__call__`, texture=None):
 * normals [B,nver,3] + vertices [B,nver,3] -> light [B,nver,3] in [0,1]. Float op order follows the
 * numpy code; agreement with numpy is to rounding (pow), not bitwise. */
typedef struct dad3d_light {
    float intensity_ambient, intensity_directional, intensity_specular, specular_exp;
    float color_ambient[3], color_directional[3], light_pos[3], view_pos[3];
} dad3d_light;
DAD3D_EXPORT dad3d_status dad3d_mesh_phong_light(dad3d_mesh* m, float* light, const float* vertices, const float* normals,
                                    int batch, const dad3d_light* cfg, void* stream);
/* RenderPipeline's first two steps in ONE launch (lighting.py:64-67: `_get_normal` on a zeroed buffer, then the Phong
 * terms): light [B,nver,3] from the vertices alone; `ver_normal` [B,nver,3] receives the normals, or NULL. */
DAD3D_EXPORT dad3d_status dad3d_mesh_normal_phong_light(dad3d_mesh* m, float* light, float* ver_normal, const float* vertices,
                                           int batch, const dad3d_light* cfg, void* stream);
/* Read-only: which kernel form a launch on this mesh would take, computed by the functions the launchers themselves call;
 * nothing is launched. `entry`: DAD3D_PLAN_GET_NORMAL (dad3d_mesh_get_normal at `batch`), DAD3D_PLAN_PHONG
 * (dad3d_mesh_normal_phong_light at `batch`) or DAD3D_PLAN_RENDER (the light inside dad3d_mesh_render's geometry kernel on
 * h x w images, a shape the raster accepts; it does not depend on the batch). h and w are read for DAD3D_PLAN_RENDER only.
 *   *form        DAD3D_FORM_TABLE (face-normal table in LDS), DAD3D_FORM_LDS (vertices staged in LDS, faces gathered per
 *                vertex), DAD3D_FORM_GLOBAL (gathered from global memory) or DAD3D_FORM_REFUSED (the call returns DAD3D_E_INVALID)
 *   *chunks      workgroups per image that compute normals (vertex chunks); 0 when refused
 *   *built_mask  bit k set: dad3d_mesh_create built the table of 1 << k chunks (k = 0..3) */
#define DAD3D_PLAN_GET_NORMAL 0
#define DAD3D_PLAN_PHONG 1
#define DAD3D_PLAN_RENDER 2
#define DAD3D_FORM_REFUSED 0
#define DAD3D_FORM_TABLE 1
#define DAD3D_FORM_LDS 2
#define DAD3D_FORM_GLOBAL 3
DAD3D_EXPORT dad3d_status dad3d_mesh_normal_plan(dad3d_mesh* m, int entry, int batch, int h, int w, int* form, int* chunks,
                                    int* built_mask);
/* Diagnostics: DEVICE buffer of [B * tiles][8 waves][16] uint64 that every wave of the raster kernel fills with
 * 100 MHz wall-clock stamps at its phase boundaries (slots 0-6: start, list sorted, fragments done, after barrier,
 * shaded, after barrier, end; 7: triangles in the tile list; 8-11 / 12-15: wave steps, ticks waiting for records,
 * ticks working, pixel tests of the busiest lane, for the fragment / shading walk); NULL switches it off.
 * tiles = ceil(w/64) * ceil(h/64). */
DAD3D_EXPORT dad3d_status dad3d_mesh_debug_trace(dad3d_mesh* m, unsigned long long* device_buffer);

/* `RenderPipeline.__call__` with texture=None (Sim3DR/lighting.py:64-71) for a batch, in TWO launches: the geometry kernel
 * of the raster also computes the vertex normals and the Phong light of its share of the vertices (same arithmetic as
 * dad3d_mesh_normal_phong_light) into `light` [B,nver,3], the tile kernel rasterises with `light` as the colours into the
 * 3-channel `image` [B,h,w,3]. `depth` as in dad3d_mesh_rasterize. `flags`: DAD3D_RENDER_REVERSE = the `reverse` argument of
 * Sim3DR.rasterize (1, as before); DAD3D_RENDER_CLEAR = render onto a black background (`bg = np.zeros_like(img)`, the
 * `with_bg_flag=False` call of the reference's demo): the image is zeroed by the geometry launch itself, no fill in front. */
enum { DAD3D_RENDER_REVERSE = 1, DAD3D_RENDER_CLEAR = 2 };
DAD3D_EXPORT dad3d_status dad3d_mesh_render(dad3d_mesh* m, uint8_t* image, const float* vertices, float* light, float* depth, int batch,
                               int h, int w, const dad3d_light* cfg, int flags, void* stream);

/* Several heads into their frames in one chain of seven launches: the loop `for k: frame[image_index[k]] = Sim3DR.rasterize(
 * vertices[k], triangles, colors[k], bg=frame[image_index[k]], reverse=reverse)` (Sim3DR/Sim3DR.py:14-29 around _rasterize,
 * rasterize_kernel.cpp:219-292) for frames of any sizes, and with dad3d_mesh_render_frames RenderPipeline.__call__
 * (lighting.py:37-71, texture=None) per head. Every call of that loop has a z-buffer of its own starting at -1e8, so a later
 * head paints over an earlier one wherever it covers a pixel, also where it lies behind; within a head: strict-interior test,
 * `>` depth test, ties to the lowest triangle index, (unsigned char) truncation. A frame without heads is not written, and a
 * pixel no head covers is not written. alpha == 1 and three channels only; no depth output.
 *   frames       DEVICE int64 [n_frames][4], the table of dad3d_preprocess_boxes: {address of the first byte, h, w, row stride in
 *                bytes}; uint8 RGB pixels, HWC, unit pixel stride. The stride may exceed 3 * w; neither it nor the address need be
 *                aligned: pixels are written as single bytes, and no byte outside [row, row + 3 * w) of a row is touched.
 *   frames_host  HOST copy of the same table: shapes are checked and the scratch is sized from it, before any device work
 *   vertices     DEVICE [n_heads,nver,3] fp32 (frame pixel x, pixel y, depth); colors / light [n_heads,nver,3] fp32
 *   image_index  DEVICE int32 [n_heads], in any order; never read on the host
 *   flags        DEVICE int32 [n_heads], written: 0 = drawn; DAD3D_FRAME_FLAG_INDEX = image_index outside [0, n_frames);
 *                DAD3D_FRAME_FLAG_CAPACITY = the head did not fit the list pool. A flagged head is not drawn at all and changes
 *                no byte of any frame.
 * List pool: every (64 x 64 tile, triangle) pair a head touches takes one entry of a pool of 4 * ntri * n_heads; heads take
 * theirs in ascending order, and a head that no longer fits is dropped whole. A triangle whose box inside the frame is at most
 * 64 x 64 pixels touches at most 2 x 2 tiles, so a call in which every such box is that small always fits.
 * dad3d_mesh_render_frames: `light` [n_heads,nver,3] receives the Phong light of every head (the arithmetic of
 * dad3d_mesh_normal_phong_light: per-head norm_vertices bounds and normals), which is then the colours; one launch more.
 * `render_flags`: DAD3D_RENDER_REVERSE; DAD3D_RENDER_CLEAR is DAD3D_E_INVALID (a frame is the caller's picture).
 * Scratch: owned by the handle, bounded by n_heads * ntri, n_frames and the tile total of the frames (about 24 * ntri bytes a
 * head and 12 bytes a tile), allocated on first use and on growth -- that call synchronises the device. A call whose scratch
 * is large enough allocates nothing, does not synchronise and can be captured into a graph. One handle serves one stream at a time.
 * Limits: at most DAD3D_FRAME_MAX_TILES tiles a frame, less than 2^24 tiles in all, n_frames and n_heads at most
 * DAD3D_FRAME_MAX_COUNT each, ntri at most 65535 and 4 * ntri * n_heads < 2^31; beyond them DAD3D_E_INVALID with a message.
 * n_frames == 0 or n_heads == 0: nothing to do, DAD3D_OK. Every argument check happens before any device work. */
#define DAD3D_FRAME_FLAG_INDEX 1
#define DAD3D_FRAME_FLAG_CAPACITY 2
#define DAD3D_FRAME_MAX_TILES 4096
#define DAD3D_FRAME_MAX_COUNT 65535
DAD3D_EXPORT dad3d_status dad3d_mesh_rasterize_frames(dad3d_mesh* m, const int64_t* frames, const int64_t* frames_host, int n_frames,
                                                      const float* vertices, const float* colors, const int32_t* image_index, int n_heads,
                                                      int reverse, int32_t* flags, void* stream);
DAD3D_EXPORT dad3d_status dad3d_mesh_render_frames(dad3d_mesh* m, const int64_t* frames, const int64_t* frames_host, int n_frames,
                                                   const float* vertices, float* light, const int32_t* image_index, int n_heads,
                                                   const dad3d_light* cfg, int render_flags, int32_t* flags, void* stream);
/* Read-only: the bytes of device scratch the handle holds for the two entries above (0 before the first call). */
DAD3D_EXPORT dad3d_status dad3d_mesh_frames_scratch_bytes(dad3d_mesh* m, size_t* bytes);

/* Batched `_render_texture_core` (rasterize_kernel.cpp:358-463, declared in rasterize.h:102-109; the reference's Cython binding
 * comments it out): a head drawn with a texture instead of per-vertex colours. Two launches: the geometry kernel of
 * dad3d_mesh_rasterize (same boxes), then a tile kernel with
 *   coverage (:423)  is_point_in_tri (u >= 0, v >= 0, u + v < 1) OR the pixel lies in the two-pixel border band of the image
 *                    (x < 2 || x > w - 3 || y < 2 || y > h - 3): there every triangle whose box reaches the pixel competes with
 *                    extrapolated weights. Reference behaviour, kept.
 *   depth (:425-427) `>`: the deepest fragment, ties to the lowest triangle index, NaN never wins.
 *   texel (:432-453) tex_p = tex_p0 * w0 + tex_p1 * w1 + tex_p2 * w2, clamped to [0, size - 1]; mapping_type 0 = nearest
 *                    (round half away from zero), otherwise bilinear over the floor / ceil texels. Unfused, in the reference's
 *                    order: bit-exact on the float path.
 * dad3d_mesh_set_texcoords attaches the (static) texture coordinates, HOST arrays uploaded once: tex_coords [n_tex, stride] fp32
 * in texel units (x = column, y = row; stride 2 or 3, a third column is ignored), tex_triangles int32 [ntri,3] with indices in
 * [0, n_tex). It synchronises the device and may be called again to replace them. Both indexing modes are laid out from it:
 *   DAD3D_TEX_INDEX_CORNER     x and y of corner k of triangle i from row tex_triangles[i][k]: what a UV layout with seams needs.
 *                              The reference gives the same image when it is called on the unrolled mesh (one vertex per corner).
 *   DAD3D_TEX_INDEX_REFERENCE  the reference as it is (:398-403): x from row tex_triangles[i][k], y from row triangles[i][k] (the
 *                              MESH triangle), rows of 3 floats. Available when stride == 3 and every vertex index is < n_tex.
 * dad3d_mesh_render_texture, DEVICE buffers:
 *   image    [B,h,w,c] float32 or uint8 (image_dtype), written where a fragment wins, untouched elsewhere. uint8: the float
 *            result through (unsigned char), i.e. the float image's astype(uint8).
 *   vertices [B,nver,3] fp32 (pixel x, pixel y, depth)
 *   texture  [B,tex_h,tex_w,tex_c] (texture_batched != 0) or one [tex_h,tex_w,tex_c] for all images, float32 or uint8
 *            (texture_dtype; uint8 texels are widened to float first). The first c channels are used.
 *   depth    [B,h,w] fp32 in/out, or NULL = start from -1e8 and discard
 * c outside 1..4 or above tex_c, an unknown dtype or indexing mode, a missing table -> DAD3D_E_INVALID. Where the reference
 * indexes the texture with whatever a non-finite coordinate converts to, the row / column here is clamped into the texture after
 * the conversion (NaN reads row / column 0): nothing outside the texture is read and a non-finite image of a batch changes only
 * its own pixels. `nver` and `tex_nver` of the reference are unused there and have no counterpart. Scratch, stream rule and limits
 * as for dad3d_mesh_rasterize. */
enum { DAD3D_TEX_INDEX_CORNER = 0, DAD3D_TEX_INDEX_REFERENCE = 1 };
enum { DAD3D_DTYPE_F32 = 0, DAD3D_DTYPE_U8 = 1 };
DAD3D_EXPORT dad3d_status dad3d_mesh_set_texcoords(dad3d_mesh* m, const float* tex_coords, int n_tex, int stride,
                                                   const int32_t* tex_triangles);
DAD3D_EXPORT dad3d_status dad3d_mesh_render_texture(dad3d_mesh* m, void* image, int image_dtype, const float* vertices,
                                                    const void* texture, int texture_dtype, int texture_batched, float* depth,
                                                    int batch, int h, int w, int c, int tex_h, int tex_w, int tex_c,
                                                    int mapping_type, int indexing, void* stream);

/* Textured heads through the frames chain. Per frame, in ascending head order:
 *   frame = (unsigned char) _render_texture_core(image = float(frame), vertices[k], .., texture[k], a fresh depth buffer at -1e8)
 * A later head paints over an earlier one wherever it covers a pixel; an uncovered pixel is not written. Seven launches: the six
 * list-building launches of dad3d_mesh_rasterize_frames, then a tile kernel with dad3d_mesh_render_texture's coverage, depth test and
 * texel arithmetic (see there). The two-pixel border band is that of the FRAME (x < 2 || x > w - 3 || y < 2 || y > h - 3) and is kept
 * on purpose, as the reference has it; it only matters for a head whose triangle boxes reach the frame's outer two pixels.
 *   frames, frames_host, vertices, image_index, flags   as for dad3d_mesh_rasterize_frames (DAD3D_FRAME_FLAG_INDEX / _CAPACITY; a
 *                flagged head changes no byte of any frame)
 *   texture      DEVICE [n_heads,tex_h,tex_w,tex_c] (texture_batched != 0: head k samples texture k) or one [tex_h,tex_w,tex_c] for
 *                all heads, float32 or uint8 (texture_dtype); tex_c >= 3, the first three channels are used
 *   mapping_type 0 = nearest, otherwise bilinear; indexing DAD3D_TEX_INDEX_CORNER or _REFERENCE (dad3d_mesh_set_texcoords)
 * Pixels are written as three single bytes, (unsigned char) of the float result; no byte outside [row, row + 3 * w) of a row is
 * touched. `reverse` is not offered; alpha == 1; no depth output and no depth buffer shared between heads. A missing texcoord table,
 * tex_c < 3, an unknown dtype or indexing mode -> DAD3D_E_INVALID. Limits, list pool, scratch ownership (shared with the two entries
 * above), stream and graph rule: exactly those of dad3d_mesh_rasterize_frames. Every argument check happens before any device work. */
DAD3D_EXPORT dad3d_status dad3d_mesh_render_texture_frames(dad3d_mesh* m, const int64_t* frames, const int64_t* frames_host, int n_frames,
                                                           const float* vertices, const void* texture, int texture_dtype,
                                                           int texture_batched, int tex_h, int tex_w, int tex_c, int mapping_type,
                                                           int indexing, const int32_t* image_index, int n_heads, int32_t* flags,
                                                           void* stream);

/* ---------------------------------------------------------------------------------------------
 * Matrix projection of meshes (GT annotations): model_training/data/flame_dataset.py:115-141 (`_load_mesh`,
 * `_project_vertices_onto_image`), visualize.py:10-22 (`get_2d_keypoints`). All DEVICE pointers:
 *   vertices [B,nver,3], model_view [B,4,4], projection [B,4,4] (row-major, as the annotation JSON stores them),
 *   frame [B,3] = (image height, crop_point_x, crop_point_y) -- zeros for no crop.
 * Outputs, each optional (NULL): world_homo [B,nver,4] = (MV . [v;1])^T, xy [B,nver,2] = (x/w, H - y/w) - crop,
 * xy_int [B,nver,2] = (int) xy: truncation toward zero; a NaN gives 0, +inf or a value >= 2^31 gives INT32_MAX, -inf or a
 * value < -2^31 gives INT32_MIN (the gfx950 conversion saturates). A vertex with clip w = 0 or w < 0 is divided like any other
 * (+-inf, NaN or a mirrored point), never clipped.
 * The arithmetic is fixed: both 4x4 products are summed k = 0..3 in order in fp32 without fused multiply-adds, then one
 * correctly rounded divide, flip and crop shift, so the outputs are reproducible to the bit (the tests hold them to a NumPy
 * restatement of that order). It is numpy's own sgemm that may fuse or reorder the products: agreement with the numpy
 * REFERENCE is therefore to fp32 rounding, not bitwise. batch > 65535 (the launch grid) -> DAD3D_E_INVALID before any device work.
 * --------------------------------------------------------------------------------------------- */
DAD3D_EXPORT dad3d_status dad3d_project_vertices(const float* vertices, const float* model_view, const float* projection,
                                    const float* frame, int batch, int nver, float* world_homo, float* xy,
                                    int32_t* xy_int, int device, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Ground-truth keypoints of a training batch: FlameDataset's per-sample geometry (model_training/data/flame_dataset.py:115-199)
 * for B items in one launch, replacing `_load_mesh` (:115-127), `_project_vertices_onto_image` (:130-141),
 * `_get_2d_landmarks_w_presence` (:143-171, with get_68_landmarks of data/utils.py:120-206), the keypoint half of
 * `_transform` (albumentations 1.0.0 LongestMaxSize + PadIfNeeded or Resize on KeypointParams("xy"), :173-191) and the
 * `landmarks / img_size` of `_form_anno_dict` (:198). All DEVICE pointers:
 *   vertices [B,nver,3], model_view [B,4,4], projection [B,4,4] float32, row-major (the annotation JSON's layout)
 *   frames   [B,8] int32 = (full image height, crop x, crop y, crop w, crop h, pad_top, pad_left, 0); the pads are
 *            PadIfNeeded's on the LongestMaxSize-resized crop (ignored in DAD3D_RESIZE_RESIZE mode); w, h > 0
 *   subset   index mode: index [n_subset] vertex ids, corners = weights = NULL;
 *            68-landmark mode: corners [n_subset,3] vertex ids of the embedding faces, weights [n_subset,3], index = NULL.
 *            Ids outside [0, nver) give a NaN point (absent), never a read.
 * Outputs: full [B,nver,2] (TARGET_2D_FULL_LANDMARKS, out_size pixels), subset_px [B,n_subset,2] (out_size pixels: the heatmap
 * coder's input), subset_norm [B,n_subset,2] = subset_px / out_size (TARGET_2D_LANDMARKS), presence [B,n_subset] uint8
 * (0 < x < w and 0 < y < h in crop pixels). The resize step runs in float64 and rounds to fp32 once (the pinned numpy 1.22
 * promotes np.float32 * float to float64). Agreement with the numpy reference is fp32 rounding in the two 4x4 products
 * (sgemm order), exact after them. Stream-ordered, no allocation, no atomics, no host sync.
 * --------------------------------------------------------------------------------------------- */
enum { DAD3D_RESIZE_LONGEST_MAX_SIZE = 0, DAD3D_RESIZE_RESIZE = 1 };
DAD3D_EXPORT dad3d_status dad3d_gt_keypoints(const float* vertices, const float* model_view, const float* projection,
                                const int32_t* frames, int batch, int nver, const int32_t* index, const int32_t* corners,
                                const float* weights, int n_subset, int out_size, int resize_mode, float* full, float* subset_px,
                                float* subset_norm, uint8_t* presence, int device, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The reference's mesh losses, VALUE and GRADIENT w.r.t. the prediction, on vertices that are already in HBM (the outputs of
 * the differentiable decode). All pointers are DEVICE pointers; nothing is allocated, both calls can be captured into a graph.
 *
 * dad3d_cube_region_loss  = Vertices3DLoss.forward after its decode (model_training/losses/vertices_3d_loss.py:43-49):
 *     sum_r w_r * criterion(normalize_to_cube(pred[:, idx_r]), normalize_to_cube(target[:, idx_r]))
 *   normalize_to_cube: model_training/model/utils.py:55-68; criterion: nn.L1Loss / MSELoss / SmoothL1Loss, reduction "mean"
 *   (vertices_3d_loss.py:11). The gradient of a min / max goes to its arg position, as torch autograd routes it.
 *     region_ptr [R+1], region_idx [sum N_r]  the index lists of indices_reweighing (model_training/utils.py:108-117)
 *     vert_ptr [V+1], vert_region, vert_pos   the same incidence transposed: for every vertex the (region, position) pairs
 *     stats [R][B][28] scratch; loss_terms [R][B] (the loss is their sum); grad_pred [B,V,3] or NULL (value only)
 * dad3d_weighted_point_loss = ReprojectionLoss.forward after its decode (model_training/losses/reprojection_loss.py:42-46):
 *     sum_r w_r * criterion(pred[:, idx_r], target[:, idx_r]) = sum_{b,n,c} point_weight[n] * scale * criterion(pred - target)
 *   with point_weight[n] = sum_r w_r * multiplicity_r(n) / N_r and scale = 1 / (B * comps).
 *     loss_terms [B][dad3d_point_loss_terms(n_points)] (the loss is their sum); grad_pred [B,N,comps] or NULL */
enum { DAD3D_LOSS_L1 = 0, DAD3D_LOSS_L2 = 1, DAD3D_LOSS_SMOOTH_L1 = 2 };
DAD3D_EXPORT dad3d_status dad3d_cube_region_loss(const float* pred, const float* target, int batch, int n_verts,
                                    const int32_t* region_ptr, const int32_t* region_idx, const float* region_weight,
                                    int n_regions, const int32_t* vert_ptr, const int32_t* vert_region,
                                    const int32_t* vert_pos, int criterion, float* stats, float* loss_terms,
                                    float* grad_pred, int device, void* stream);
DAD3D_EXPORT int dad3d_point_loss_terms(int n_points);
DAD3D_EXPORT dad3d_status dad3d_weighted_point_loss(const float* pred, const float* target, int batch, int n_points, int comps,
                                       const float* point_weight, float scale, int criterion, float* loss_terms,
                                       float* grad_pred, int device, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The rest of the reference's training objective: the heatmap target, the heatmap IoU loss, the landmark loss with visibility
 * and the keypoint metrics of a training step. All pointers are DEVICE pointers; nothing is allocated, no call waits for the
 * device, every call can be captured into a graph. Sums run in a fixed order (no float atomics): two runs give the same bits.
 * Bad sizes, an unknown form / criterion or a NULL pointer -> DAD3D_E_INVALID before any device work.
 *
 * dad3d_heatmap_encode  HeatmapCoder.__call__ (model_training/data/coder.py:17-24; draw_gaussian data/utils.py:48-71) for
 *   B * C channels: keypoints [B*C,2] fp32 (resized-image pixels), presence [B*C] bool / uint8. A present point stamps the
 *   (2r+1)^2 `table` around int(point // stride) (numpy's float32 floor_divide), clipped to the size x size channel; every
 *   other element is 0. `table` holds the stamp in the output's form (DAD3D_HEATMAP_RAW float32 = the coder's return,
 *   DAD3D_HEATMAP_UINT8 = flame_dataset.py:198 `np.uint8(255.0 * heatmap)`, DAD3D_HEATMAP_FLOAT = mixins.py:50
 *   `uint8 / 255.0`). out [B*C,size,size] float32 / uint8, 16-byte aligned. A present point whose centre is NaN or inf (the
 *   reference raises) leaves its channel zero and adds 1 to invalid[0] (invalid may be NULL).
 * dad3d_heatmap_iou  IoULoss (losses/keypoint_losses.py:11-30), SoftIoUMetric / soft_iou (metrics/iou.py:15-72):
 *   per channel N = sum(t s) + 1e-6, D = sum(t^2) + sum(s^2) - sum(t s) + 1e-6 over hw elements, s = sigmoid(pred) when
 *   `sigmoid` (the loss) or pred itself (the metric), t = target (float32) or target / 255 (uint8, target_u8 = 1).
 *   sums [channels,3] float64 (saved for the gradient); iou [channels] fp32 or NULL; loss [2] = (1 - mean N/D, mean N/D)
 *   or NULL; accum [2] += (mean, 1) or NULL.
 * dad3d_heatmap_iou_grad  dL/dpred of the loss for an upstream gradient grad_out [1] (read on the device):
 *   -g / channels * (t D - N (2 s - t)) / D^2 * s (1 - s), with the sums of dad3d_heatmap_iou. grad [channels,hw] fp32.
 * dad3d_visibility_point_loss  LandmarksLossWVisibility (losses/landmarks_loss_w_visibility.py:17-26):
 *   criterion(pred * pred_presence[..., None], target * target_presence[..., None]), mean over B*N*2; pred, target [B,N,2],
 *   presences [B,N] fp32. loss [1]; grad_pred [B,N,2] (for an upstream gradient of 1) or NULL.
 * dad3d_keypoint_errors  metrics/keypoints.py:19-53 (`keypoints_nme`, `percentage_of_errors_below_IOD`): per item
 *   err = mean_n |p_n - q_n|_2 over index [n_points] (NULL: the first n_points of n_verts) with p = pred * pred_scale * presence,
 *   q = target * presence * target_scale (presence [B,n_verts] or NULL), both normalize_to_cube'd (model/utils.py:55-68)
 *   when `cube`; norm = sqrt(w h) of bbox [B,4] int32 (x, y, w, h), or 2.0 when bbox is NULL. Float64 throughout. An index
 *   outside [0,n_verts) reads as NaN. thresholds [n_thresholds] is a HOST float64 array.
 *   err [B,2] float64 = (err, norm). out [1 + n_thresholds] = (mean(err / norm), count(err < thr_k norm) / B ...) (`below` = 0:
 *   err > thr_k norm), or NULL; accum [2 (1 + n_thresholds)] += (value, 1) pairs, or NULL. n_thresholds <= 8, dims 2 or 3.
 * --------------------------------------------------------------------------------------------- */
enum { DAD3D_HEATMAP_RAW = 0, DAD3D_HEATMAP_UINT8 = 1, DAD3D_HEATMAP_FLOAT = 2 };
DAD3D_EXPORT dad3d_status dad3d_heatmap_encode(void* out, int form, const float* keypoints, const uint8_t* presence, int batch,
                                  int n_classes, float stride, int size, int radius, const void* table, int32_t* invalid,
                                  int device, void* stream);
DAD3D_EXPORT dad3d_status dad3d_heatmap_iou(const float* pred, const void* target, int target_u8, int batch, int channels,
                               int hw, int sigmoid, double* sums, float* iou, float* loss, float* accum, int device,
                               void* stream);
DAD3D_EXPORT dad3d_status dad3d_heatmap_iou_grad(const float* pred, const void* target, int target_u8, int batch, int channels,
                                    int hw, const double* sums, const float* grad_out, float* grad, int device, void* stream);
DAD3D_EXPORT dad3d_status dad3d_visibility_point_loss(const float* pred, const float* pred_presence, const float* target,
                                         const float* target_presence, int batch, int n_points, int criterion, float* loss,
                                         float* grad_pred, int device, void* stream);
DAD3D_EXPORT dad3d_status dad3d_keypoint_errors(const float* pred, const float* target, int batch, int n_verts, int dims,
                                   const int32_t* index, int n_points, const float* presence, float pred_scale,
                                   float target_scale, int cube, const int32_t* bbox, const double* thresholds,
                                   int n_thresholds, int below, double* err, float* out, float* accum, int device,
                                   void* stream);

/* ---------------------------------------------------------------------------------------------
 * The DAD-3DHeads benchmark scorer's two dense point-set steps (dad_3dheads_benchmark/benchmark.py `DADEvaluator`, utils.py).
 * All pointers are DEVICE pointers unless noted; nothing is allocated, both calls can be captured into a graph. Distances are
 * squared, fp32, in the direct-difference form (qx-px)^2 + (qy-py)^2 + (qz-pz)^2 (no |q|^2 + |p|^2 - 2 q.p expansion).
 * Sizes are validated before any device work: B, Q, N, K <= 0, k outside 1..8, K > 4096 or a NULL pointer -> DAD3D_E_INVALID.
 *
 * dad3d_eval_nearest  one-sided nearest neighbours (utils.py:119-133 `calc_ch_dist`: kaolin's `chamfer_distance(gt, pred,
 *   1.0, 0.0)` = mean over the GT points of min_dist2, its alignment loop utils.py:154-171 `align_pred_to_gt` fused):
 *     query [B,Q,3]; points [B,N,3]; counts [B] int32 or NULL: item b uses points[b, :counts[b]] (clamped to 0..N)
 *     similarity [B][13] = (s, R row-major 3x3, t) or NULL: every point is mapped to s * p . R + t (row vector) first
 *     flags: DAD3D_EVAL_SELF_EXCLUDE = query and points are the same set in the same order: point q is not a neighbour of
 *            query q. Requires Q == N (else DAD3D_E_INVALID)
 *     min_dist2 [B,Q] (required); knn_index [B,Q,k] int32, knn_dist2 [B,Q,k]: the k nearest in ascending distance, ties to
 *     the lower index, -1 / +inf where fewer than k points exist (each optional, NULL)
 *     Non-finite input: only a FINITE distance is ever reported. A point whose distance to the query is NaN or +inf (a NaN or
 *     infinite coordinate, after the similarity) is skipped as if it were absent, and a query with a NaN or infinite coordinate
 *     gets -1 / +inf at every rank (min_dist2 = +inf). Nothing propagates a NaN: where the reference's Chamfer mean would turn
 *     NaN on a NaN vertex, the caller has to look for non-finite input itself. Rows past counts[b] are never read.
 * dad3d_eval_z5_ranks  benchmark.py:126-160 `calc_zn` / `zn` as the script computes it: for every anchor a (head-subset
 *   positions, HOST array anchors[n_anchors], n_anchors <= 8), all K head vertices ordered by fp32 distance to gt_head[a]
 *   (ties to the lower index, rank 0 included) = o_a, then
 *     counts[b][a] = #{ i < K : (g_z[i] >= g_z[o_a[i]]) == (w_z[i] >= w_z[o_a[i]]) }
 *     gt_head [B,K,3] (the GT world head subset TIMES -1, benchmark.py:155), pred_head [B,K,3], counts [B][n_anchors] int32,
 *     order [B][n_anchors][K] int32 (o_a) or NULL
 *   Non-finite vertices: the sort key is the distance's bit pattern, then the index. +inf distances sort behind every finite
 *   one (among themselves by index) and a NaN distance behind those, where a stable float64 argsort places them; SEVERAL NaN
 *   distances order by their bit patterns (sign and payload) first, so not necessarily by index as that argsort would.
 *   The z comparisons are IEEE: any comparison with a NaN z is false.
 * --------------------------------------------------------------------------------------------- */
#define DAD3D_EVAL_SELF_EXCLUDE 0x1
#define DAD3D_EVAL_MAX_K 8
#define DAD3D_EVAL_MAX_HEAD 4096
#define DAD3D_EVAL_MAX_ANCHORS 8
DAD3D_EXPORT dad3d_status dad3d_eval_nearest(const float* query, const float* points, const int32_t* counts, const float* similarity,
                                int batch, int n_query, int n_points, int k, int flags, float* min_dist2, int32_t* knn_index,
                                float* knn_dist2, int device, void* stream);
DAD3D_EXPORT dad3d_status dad3d_eval_z5_ranks(const float* gt_head, const float* pred_head, int batch, int n_head,
                                 const int32_t* anchors, int n_anchors, int32_t* counts, int32_t* order, int device, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The reference demo's UV-texture bake (inference/uv_texture.py `UVTextureCreator._compute_texture_map`), float64 like its
 * NumPy. A dad3d_uvmap holds, in HBM, the vertex -> face lists of the mesh's normals and the texel -> candidate table of a
 * texture atlas. Candidate i (the atlas' valid pixel i) has three vertex ids, three float64 barycentrics and its texel
 * y * S + x (wrapped into [0, S*S) by the caller, as NumPy's negative indices wrap).
 *   dad3d_uvmap_create          HOST arrays: faces [ntri,3], cand_texel [n], cand_verts [n,3], cand_bary [n,3]. An index
 *                               outside [0,nver), a texel outside [0,S*S) or S <= 0 -> DAD3D_E_INVALID.
 *   dad3d_uvmap_vertex_normals  psbody-mesh's `Mesh.estimate_vertex_normals` of fp32 vertices widened to float64: the
 *                               unnormalised face normals cross(v1 - v0, v2 - v0) summed in ascending face order (a face that
 *                               names a vertex twice counts twice), divided by sqrt((x*x + y*y) + z*z), a zero norm read as 1.
 *                               DEVICE normals [B,nver,3] float64, vertices [B,nver,3] float32.
 *   dad3d_uvmap_bake            for every texel the LAST candidate (the reference loop's last writer) whose interpolated normal
 *                               has -n.z >= 0 (or NaN) and whose interpolated point rounds half to even to 0 < x < w,
 *                               0 < y < h takes images[b, y, x]; texels no candidate reaches are 0. DEVICE texture [B,S,S,3]
 *                               (every byte written), vertices [B,nver,3] float32, normals [B,nver,3] float64 (from
 *                               dad3d_uvmap_vertex_normals), images [B,h,w,3] uint8, hw [B,2] int32 = per-item (height,
 *                               width) bounds inside the padded h x w (clamped to it), or NULL for (h, w).
 * Neither launch allocates; both are stream-ordered and can be captured into a graph. One handle may serve several streams.
 * --------------------------------------------------------------------------------------------- */
typedef struct dad3d_uvmap dad3d_uvmap; /* opaque: face CSR + texel -> candidate CSR (vertex ids, float64 barycentrics) */
DAD3D_EXPORT dad3d_status dad3d_uvmap_create(const int32_t* faces, int ntri, int nver, const int32_t* cand_texel,
                                const int32_t* cand_verts, const double* cand_bary, int n, int img_size, int device,
                                dad3d_uvmap** out);
DAD3D_EXPORT void dad3d_uvmap_destroy(dad3d_uvmap* m);
DAD3D_EXPORT int dad3d_uvmap_size(const dad3d_uvmap* m);
DAD3D_EXPORT dad3d_status dad3d_uvmap_vertex_normals(dad3d_uvmap* m, double* normals, const float* vertices, int batch,
                                        void* stream);
DAD3D_EXPORT dad3d_status dad3d_uvmap_bake(dad3d_uvmap* m, uint8_t* texture, const float* vertices, const double* normals,
                              const uint8_t* images, const int32_t* hw, int batch, int h, int w, void* stream);

/* The bake for heads that name their frames (a tracker's slots over a video): head k reads the frame image_index[k] of the frame
 * table of dad3d_preprocess_boxes and owns texture k, so frames of any sizes and row strides serve several heads each without
 * being gathered into a batch, and no two heads ever write one texture. One launch: a lane owns four consecutive texels of a head.
 *   texture      DEVICE uint8 [n_heads,S,S,3]
 *   score        DEVICE float32 [n_heads,S,S], or NULL (see below)
 *   vertices     DEVICE [n_heads,nver,3] float32 (frame pixel x, pixel y, depth); normals DEVICE [n_heads,nver,3] float64 (from
 *                dad3d_uvmap_vertex_normals)
 *   frames       DEVICE int64 [n_frames][4] {address of the first byte, h, w, row stride in bytes}: uint8 RGB pixels, HWC, unit pixel
 *                stride; neither the address nor the stride need be aligned
 *   frames_host  HOST copy of the same table, checked before any device work: an address, h, w >= 1, stride >= 3 * w, else
 *                DAD3D_E_INVALID. The tile limits of dad3d_mesh_rasterize_frames do not apply.
 *   image_index  DEVICE int32 [n_heads], in any order; never read on the host
 *   flags        DEVICE int32 [n_heads], written: 0, or DAD3D_BAKE_FLAG_INDEX = image_index outside [0, n_frames) -- what a tracker
 *                reports for a lost slot (-1), so an ordinary outcome
 * Per texel the candidate is chosen exactly as dad3d_uvmap_bake chooses it: the LAST candidate with !(n_dot_view < 0) whose
 * interpolated point, rounded half to even, satisfies 0 < x < w, 0 < y < h with the FRAME's own w and h; its pixel is the three
 * bytes at address + y * stride + 3 * x.
 *   score == NULL  plain bake: every byte of texture k is written, the pixel where there is a candidate, zeros elsewhere; a flagged
 *                  head gives zeros. For one head per equal-size frame these are the bytes of dad3d_uvmap_bake.
 *   score != NULL  accumulate, "best view wins": with s = (float) n_dot_view of the chosen candidate (float64 rounded to the nearest
 *                  float32), the texel's three bytes and score[k,t] are replaced iff s > score[k,t]. A NaN s never replaces, a tie
 *                  keeps the older sample, a texel without a candidate keeps its state, and a flagged head changes no byte of its
 *                  texture or score. Start a texture at zeros with score -1.0f: then any first sample (n_dot_view >= 0) enters.
 * Not done: blending of samples, occlusion of a head by another head or an object (a head's occlusion of itself:
 * dad3d_uvmap_bake_frames_occluded below), temporal filtering of the texture.
 * The entry allocates nothing, is stream-ordered and can be captured into a graph. n_heads == 0: DAD3D_OK, nothing to do; n_frames
 * == 0: every head is flagged. At most 65535 heads a call. One handle may serve several streams. */
#define DAD3D_BAKE_FLAG_INDEX 1
#define DAD3D_BAKE_FLAG_DEPTH_WINDOW 2 /* the head's box in its frame is wider or higher than depth_side */
#define DAD3D_BAKE_FLAG_NONFINITE 4    /* a coordinate of one of the head's vertices is NaN or +-inf */
#define DAD3D_BAKE_MAX_DEPTH_SIDE 4096
DAD3D_EXPORT dad3d_status dad3d_uvmap_bake_frames(dad3d_uvmap* m, uint8_t* texture, float* score, const float* vertices,
                                                  const double* normals, const int64_t* frames, const int64_t* frames_host, int n_frames,
                                                  const int32_t* image_index, int n_heads, int32_t* flags, void* stream);

/* Depth maps of heads in frames: for every head the nearest z of its own surface at every pixel of its box in the frame it names --
 * what a depth test against the head itself needs, and a depth output in its own right. Coordinates are the bake's: frame pixel x,
 * pixel y, and z with the viewer at -z (n_dot_view = -n_z), so the nearer surface has the SMALLER z. Depths of different heads do not
 * compare (every head is decoded with translation z := 0).
 *   depth        DEVICE float32 [n_heads, D, D], D = depth_side in 1 .. DAD3D_BAKE_MAX_DEPTH_SIDE
 *   window       DEVICE int32 [n_heads,4] = {x0, y0, ww, wh}, written
 *   vertices     DEVICE [n_heads,nver,3] float32; frames / frames_host / image_index as in dad3d_uvmap_bake_frames, with the same host
 *                checks; only h and w of a frame entry are used, no pixel is read
 *   flags        DEVICE int32 [n_heads], written: DAD3D_BAKE_FLAG_INDEX (the bake's rule) | DAD3D_BAKE_FLAG_NONFINITE (any x, y or z of the
 *                head's vertices is NaN or +-inf) | DAD3D_BAKE_FLAG_DEPTH_WINDOW (ww > D or wh > D). A flagged head gets the window
 *                {0,0,0,0} and no byte of its map is written.
 * Window, in float: x0 = max(floorf(min x), 0), x1 = min(ceilf(max x), w - 1), likewise y; ww = x1 - x0 + 1. x0 > x1 or y0 > y1: the head
 * lies outside its frame, the window is {0,0,0,0} and NO flag is set. For 0 <= j < wh, 0 <= i < ww, depth[k, j, i] (row pitch D) belongs
 * to pixel (x0 + i, y0 + j): the minimum interpolated z over the head's triangles that cover the pixel centre, in exactly the
 * arithmetic of the reference's _rasterize_triangles (rasterize_kernel.cpp:295-353) called on the head with z negated on an h x w canvas
 * initialised to -1e8 and negated back -- the box of lines 321-325, is_point_in_tri, w0 * z0 + w1 * z1 + w2 * z2 with
 * get_point_weight's float32 weights. +inf where no triangle covers the pixel, or only fragments with z >= 1e8 do; NaN never enters;
 * -0 is stored as +0. Entries outside ww x wh are not written.
 * Three launches (window, clear, one lane per head and triangle with a 32-bit atomic minimum); nothing is allocated; stream-ordered
 * and capturable. Every store is bounded by the head's own ww, wh <= D, whatever the device frame table says. */
DAD3D_EXPORT dad3d_status dad3d_uvmap_depth_frames(dad3d_uvmap* m, float* depth, int32_t* window, const float* vertices,
                                                   const int64_t* frames, const int64_t* frames_host, int n_frames,
                                                   const int32_t* image_index, int n_heads, int depth_side, int32_t* flags, void* stream);

/* dad3d_uvmap_bake_frames with a depth test against the head itself: a texel on the far cheek that faces the camera from behind the
 * nose no longer takes the nose's pixel. depth / window / depth_flags / depth_side: what dad3d_uvmap_depth_frames wrote for the SAME
 * vertices, frames and image_index (read only). Everything is dad3d_uvmap_bake_frames except:
 *   third test   a candidate that passes the two tests, with rounded pixel (rx, ry), is HIDDEN iff
 *                    pz > (double) d + (depth_bias + slope_bias * ((fabs(nx) + fabs(ny)) / n_dot_view))
 *                d = the head's depth at (rx, ry), +inf for a pixel outside the window; pz, nx, ny = the float64 sums of products of the
 *                candidate's z and its normal's x and y, in the order of the point's x and the normal's z; every operation rounds on its
 *                own. The comparison is false on NaN: an uncovered pixel, n_dot_view == +0 (a slope of inf or NaN) and a NaN leave the
 *                candidate visible (n_dot_view == -0 divides to -inf where the normal has an x or y, and hides it). A hidden candidate is skipped like a back-facing one: the texel's next candidate is tried.
 *   flags        flags[k] = depth_flags[k] | DAD3D_BAKE_FLAG_INDEX where the index names no frame. A head with any flag changes no
 *                byte of texture or score (score != NULL) or gives zeros (score == NULL).
 *   biases       in pixels of depth, both finite and >= 0, else DAD3D_E_INVALID before any device work. depth_bias covers the rounding of
 *                the map against the point; the slope term covers the up to half a pixel in x and in y between the point and the pixel
 *                centre, 0.5 * (|nx| + |ny|) / |nz| of depth on a plane with normal n, at slope_bias = 0.5; 1.0 and 1.0 are what the
 *                Python layer passes by default -- UNTUNED design choices: with both at 0 a quarter to a half of the accepted samples
 *                are "hidden" by their own surface (shadow acne).
 * Not done: occlusion of a head by another head or by an object -- depths of different heads do not compare.
 * One launch; nothing is allocated; stream-ordered and capturable. */
DAD3D_EXPORT dad3d_status dad3d_uvmap_bake_frames_occluded(dad3d_uvmap* m, uint8_t* texture, float* score, const float* vertices,
                                                           const double* normals, const int64_t* frames, const int64_t* frames_host,
                                                           int n_frames, const int32_t* image_index, int n_heads, const float* depth,
                                                           const int32_t* window, const int32_t* depth_flags, int depth_side,
                                                           double depth_bias, double slope_bias, int32_t* flags, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The vertex block of the demo's `.obj` files (demo_utils.py:130-144 `MeshSaver.__call__`): for every mesh of a batch the bytes of
 * its N lines `v %.8f %.8f %.8f\n`, exactly what Python's `'%.8f' % float(x)` prints, made on the device with 64-bit integer
 * arithmetic. All DEVICE pointers:
 *   vertices [batch,nver,3] float32, contiguous
 *   text     [batch][text_stride] bytes, 16-byte aligned; text_stride a multiple of 16, at least nver * DAD3D_OBJ_MAX_LINE_BYTES.
 *            Mesh b's lines are text[b * text_stride .. + lengths[b]); bytes behind them are left as they were
 *   lengths  [batch] int64   flags [batch] int32   scratch: dad3d_obj_format_scratch_bytes(batch, nver) bytes, 8-byte aligned
 * Domain: finite values with |x| < 2^37. A mesh that holds any other value gets its DAD3D_OBJ_FLAG_* bits set, a length of 0 and
 * no text: the caller formats that mesh on the host (`nan`, `inf`, up to 39 integer digits). flags[b] == 0 otherwise.
 * Two launches on `stream`, no allocation, no synchronisation: can be captured into a graph. Arguments (NULL, negative sizes, a
 * stride or scratch below what the shape needs, alignment) are validated before any device work -> DAD3D_E_INVALID.
 * dad3d_obj_format_scratch_bytes (demo_utils.py:130-144, host-only) returns 0 for a negative size.
 * --------------------------------------------------------------------------------------------- */
#define DAD3D_OBJ_MAX_LINE_BYTES 71 /* "v" + 3 x (" " "-" 12 digits "." 8 digits) + "\n" */
#define DAD3D_OBJ_FLAG_NONFINITE 0x1
#define DAD3D_OBJ_FLAG_LARGE 0x2
DAD3D_EXPORT size_t dad3d_obj_format_scratch_bytes(int batch, int nver);
DAD3D_EXPORT dad3d_status dad3d_obj_format_vertices(const float* vertices, int batch, int nver, uint8_t* text, size_t text_stride,
                                       int64_t* lengths, int32_t* flags, void* scratch, size_t scratch_bytes, int device,
                                       void* stream);

/* ---------------------------------------------------------------------------------------------
 * JSON text as `json.dump` writes it, made on the device from a layout template: the value of one image in a benchmark submission
 * (`{"68_landmarks_2d": [[x, y], ...], "N_landmarks_3d": [...], "7_landmarks_3d": [...], "rotation_matrix": [...]}`, the submission
 * format of dad_3dheads_benchmark/README.md:78-95) and the demo's flame_params file (demo_utils.py:114-118,147-153: `get_flame_params`
 * through `JsonSaver`). An item is n_slots numbers; the template holds the literal bytes in front of each number and a suffix that
 * closes the item. A number is float.__repr__ of the float32 widened to double: the shortest decimal string that reads back to that
 * double, positional while -4 < decimal point position <= 16, else d[.ddd]e+-XX, at most DAD3D_JSON_MAX_NUMBER_BYTES bytes; made from
 * 64 x 64 -> 128-bit integer products against a table of powers of ten, no floating point.
 *   values          DEVICE [batch,n_slots] float32, contiguous
 *   literals        DEVICE the template image, 4-byte aligned: int32 offsets [n_slots + 2], then the literal bytes. Literal i, in front
 *                   of slot i, is bytes [offsets[i], offsets[i + 1]); the suffix is literal n_slots
 *   literal_offsets HOST   the same n_slots + 2 offsets: ascending from 0, no literal longer than DAD3D_JSON_MAX_LITERAL_BYTES. They
 *                   are what the arguments are validated against without touching the device
 *   text            DEVICE [batch][text_stride] bytes, 16-byte aligned; text_stride a multiple of 16, at least the template's worst
 *                   case offsets[n_slots + 1] + n_slots * DAD3D_JSON_MAX_NUMBER_BYTES. Item b's text is text[b * text_stride ..
 *                   + lengths[b]); bytes behind it are left as they were
 *   lengths         DEVICE [batch] int64   flags DEVICE [batch] int32
 *   scratch         DEVICE dad3d_json_format_scratch_bytes(batch, n_slots) bytes, 8-byte aligned
 * An item that holds NaN or +-inf gets DAD3D_JSON_FLAG_NONFINITE, a length of 0 and no text: the caller formats it on the host
 * (`NaN`, `Infinity`, `-Infinity`). flags[b] == 0 otherwise. Two launches on `stream`, no allocation, no synchronisation: can be
 * captured into a graph. Arguments (NULL, batch <= 0, n_slots <= 0, a literal over the cap, a stride or scratch below what the
 * template needs, alignment) are validated before any device work -> DAD3D_E_INVALID. dad3d_json_format_scratch_bytes (host-only)
 * returns 0 for a size below 1.
 * dad3d_json_number_host runs the same number routine on the CPU, HOST pointers: the text of values[i] goes to
 * out[i * out_stride ..) (out_stride >= DAD3D_JSON_MAX_NUMBER_BYTES), its length to lengths[i]; -1 and no text for NaN / +-inf.
 * --------------------------------------------------------------------------------------------- */
#define DAD3D_JSON_MAX_NUMBER_BYTES 23 /* "-1.1754942106924411e-38", "-0.00010000000474974513" */
#define DAD3D_JSON_MAX_LITERAL_BYTES 64
#define DAD3D_JSON_FLAG_NONFINITE 0x1
DAD3D_EXPORT size_t dad3d_json_format_scratch_bytes(int batch, int n_slots);
DAD3D_EXPORT dad3d_status dad3d_json_format_values(const float* values, int batch, int n_slots, const void* literals,
                                      const int32_t* literal_offsets, uint8_t* text, size_t text_stride, int64_t* lengths,
                                      int32_t* flags, void* scratch, size_t scratch_bytes, int device, void* stream);
DAD3D_EXPORT dad3d_status dad3d_json_number_host(const float* values, size_t n, uint8_t* out, size_t out_stride, int32_t* lengths);

/* ---------------------------------------------------------------------------------------------
 * Images as PNG files, and byte rows as zlib streams, made on the device: what the demo's `ImageSaver` (demo_utils.py:122-127)
 * hands to an image library. Lossless and fixed by the PNG / zlib / deflate specifications (RFC 1950, 1951); the bytes are this
 * encoder's own, not those of any other.
 *   images  DEVICE [batch,h,w,c] uint8, contiguous, c = 1 / 2 / 3 / 4 -> colour type 0 / 4 / 2 / 6, bit depth 8, no interlace; the
 *           array is stored in the order it is given
 *   data    DEVICE [batch,n] uint8, contiguous (dad3d_zlib_compress)
 *   out     DEVICE [batch][out_stride] bytes, 16-byte aligned; out_stride a multiple of 16, at least dad3d_png_max_bytes(h, w, c) /
 *           dad3d_zlib_max_bytes(n). Item b's file is out[b * out_stride .. + lengths[b]); bytes behind it are left as they were
 *   lengths DEVICE [batch] int64   flags DEVICE [batch] int32   scratch DEVICE dad3d_*_scratch_bytes(..) bytes, 16-byte aligned
 * The filtered stream (per row the type byte of the filter with the smallest sum of |signed byte|, lowest type on a tie, then
 * the filtered row; for dad3d_zlib_compress the data itself) is cut into segments of DAD3D_PNG_SEGMENT_BYTES. A segment is one
 * deflate block -- stored, fixed or dynamic Huffman, whichever is shortest; matches at distances 1 and c
 * (DAD3D_ZLIB_SECOND_DISTANCE for a zlib stream), greedy -- and the empty stored block 00 00 FF FF. A PNG holds the zlib header,
 * every segment and the trailer (03 00 + Adler-32) in IDAT chunks of their own; a zlib stream is the same bytes without chunks.
 * flags[b] == 0 unless the encoder's own consistency check failed (DAD3D_PNG_FLAG_INTERNAL: length 0, the caller encodes that
 * item on the host). Three launches (two for a zlib stream) on `stream`, no allocation, no synchronisation: can be captured
 * into a graph. Arguments (NULL, c outside 1..4, h or w < 1, batch outside 1..65535, a filtered stream of 2^31 bytes or more, a
 * stride or scratch below what the shape needs, alignment) are validated before any device work -> DAD3D_E_INVALID. The
 * *_max_bytes / *_scratch_bytes calls are host-only and return 0 for such a shape.
 * dad3d_deflate_tables_host runs the encoder's table routine on the CPU, HOST pointers: histograms ll_hist[286] (end of block
 * counted) and d_hist[30], every count below 2^22 -> code lengths (15 bits at most; 7 for the code-length alphabet cl_*[19]),
 * canonical codes numbered as in RFC 1951 3.2.2, the block header (BFINAL = 0, BTYPE = 10, HLIT, HDIST, HCLEN, the code-length
 * code, the run-length coded lengths) packed low bit first into header[DAD3D_DEFLATE_HEADER_BYTES], its bit count, and the bits
 * of the whole block as a dynamic and as a fixed block.
 * --------------------------------------------------------------------------------------------- */
#define DAD3D_PNG_SEGMENT_BYTES 8192
#define DAD3D_ZLIB_SECOND_DISTANCE 4
#define DAD3D_PNG_FLAG_INTERNAL 0x1
#define DAD3D_DEFLATE_HEADER_BYTES 640
DAD3D_EXPORT size_t dad3d_png_max_bytes(int h, int w, int c);
DAD3D_EXPORT size_t dad3d_png_scratch_bytes(int batch, int h, int w, int c);
DAD3D_EXPORT dad3d_status dad3d_png_encode(const uint8_t* images, int batch, int h, int w, int c, uint8_t* out, size_t out_stride,
                                           int64_t* lengths, int32_t* flags, void* scratch, size_t scratch_bytes, int device, void* stream);
DAD3D_EXPORT size_t dad3d_zlib_max_bytes(int64_t n);
DAD3D_EXPORT size_t dad3d_zlib_scratch_bytes(int batch, int64_t n);
DAD3D_EXPORT dad3d_status dad3d_zlib_compress(const uint8_t* data, int batch, int64_t n, uint8_t* out, size_t out_stride, int64_t* lengths,
                                              int32_t* flags, void* scratch, size_t scratch_bytes, int device, void* stream);
DAD3D_EXPORT dad3d_status dad3d_deflate_tables_host(const uint32_t* ll_hist, const uint32_t* d_hist, uint8_t* ll_len, uint8_t* d_len,
                                                    uint8_t* cl_len, uint16_t* ll_code, uint16_t* d_code, uint16_t* cl_code, uint8_t* header,
                                                    int32_t* header_bits, uint32_t* dynamic_bits, uint32_t* fixed_bits);

/* ---------------------------------------------------------------------------------------------
 * The demo's overlays drawn on the device: the dots of `draw_points` (demo_utils.py:22-29, cv2.circle filled), the mesh edges of
 * `draw_mesh` (demo_utils.py:60-62, cv2.line LINE_AA) and the arrows of `draw_pose` (demo_utils.py:90-92, cv2.arrowedLine) as
 * discs and segments over a point table. All DEVICE pointers:
 *   src, dst  [batch,h,w,3] uint8, contiguous, h and w at most DAD3D_OVERLAY_MAX_COORD; every byte of dst is written; src == dst
 *             draws in place (any other overlap is undefined)
 *   points    [batch,n_points,2] float32 (x, y); a coordinate is truncated toward zero (`astype(int)`)
 *   edges     [n_edges,2] int32 into the point table, one list for the whole batch; index [n_discs] int32 or NULL (the first
 *             n_discs points)
 *   colors    [n_edges,3] uint8 or NULL (`color` for every segment); color = channel 0 | channel 1 << 8 | channel 2 << 16
 *   thickness 0: anti-aliased, one pixel wide; 1 .. 255: solid          radius 1 .. DAD3D_OVERLAY_MAX_COORD
 * The strokes are this library's own rules in exact integer arithmetic, not cv2's bits:
 *   disc      pixel (x, y) takes the colour iff (x - cx)^2 + (y - cy)^2 <= r^2
 *   solid     pixel q takes the colour iff its centre lies within t / 2 of the segment: with d = p1 - p0, u = q - p0,
 *             (d.d > 0 and 0 <= u.d <= d.d and 4 (u x d)^2 <= t^2 d.d) or 4 |q - p0|^2 <= t^2 or 4 |q - p1|^2 <= t^2
 *   AA        for i = 0 .. n = |d_major| the pixel at major coordinate m0 + i sign(d_major) and minor coordinate q >> 8 is blended
 *             with a = 256 - (q & 255), its neighbour at (q >> 8) + 1 with a = q & 255, where
 *             q = 256 minor0 + floor((512 i d_minor + n) / (2 n)) (n = 0: q = 256 minor0); dst = (dst (256 - a) + colour a + 128) >> 8
 * The primitives of a call apply to a pixel in ascending index: the result is that of drawing them one after another. A
 * primitive with a non-finite coordinate, one outside [-DAD3D_OVERLAY_MAX_COORD, DAD3D_OVERLAY_MAX_COORD] after truncation, or an
 * index outside [0, n_points) is skipped whole; pixels outside the image are not written. One launch on `stream`, no allocation,
 * no scratch, no synchronisation: can be captured into a graph. Arguments (NULL, sizes, thickness, radius, batch above 65535) are
 * validated before any device work -> DAD3D_E_INVALID.
 * --------------------------------------------------------------------------------------------- */
#define DAD3D_OVERLAY_MAX_COORD 8192
DAD3D_EXPORT dad3d_status dad3d_overlay_segments(const uint8_t* src, uint8_t* dst, int batch, int h, int w, const float* points, int n_points,
                                                 const int32_t* edges, int n_edges, const uint8_t* colors /* or NULL */, uint32_t color,
                                                 int thickness, int device, void* stream);
DAD3D_EXPORT dad3d_status dad3d_overlay_discs(const uint8_t* src, uint8_t* dst, int batch, int h, int w, const float* points, int n_points,
                                              const int32_t* index /* or NULL */, int n_discs, int radius, uint32_t color, int device,
                                              void* stream);

/* ---------------------------------------------------------------------------------------------
 * Head pose where the params lie: the rotation matrix, (roll, pitch, yaw) and the arrows of `draw_pose`, one lane per row, and the
 * similarity alignment of the scorer, one wave per item. Both rest on one float64 3x3 SVD (one-sided cyclic Jacobi, a fixed number
 * of sweeps; csrc/pose_math.hpp). DESIGN.md 4.29.
 *
 * dad3d_head_pose   row i reads its six rotation floats at params[i * row_stride + rot_offset ..] (strides in floats: a [n,413]
 *   tensor with rot_offset 403, a view of it, or a bare [n,6] with row_stride 6 and rot_offset 0) and writes whichever outputs are
 *   not NULL:
 *     rotation [n,3,3] float32  `rot_mat_from_6dof` (model_training/model/utils.py:92-101), columns b1 b2 b3, row-major; float32
 *                               operation for operation: sqrt of the left-to-right sum of squares, clamped at 1e-12, three
 *                               divisions, the two crosses
 *     rpy      [n,3]   float64  roll, pitch, yaw in degrees (model_training/model/flame.py:254-264): the matrix transposed, its
 *                               orthogonal polar factor, scipy's quaternion and `as_euler("xyz")` route, then limit_angle of
 *                               (a[2], a[0] - 180, a[1])
 *     points   [n,10,2] float32 the point table of the three arrows (demo_utils.py:73-92) for dad3d_overlay_segments: the frame's
 *                               centre, the three ends (truncated), the six tip ends (rounded half to even)
 *     flags    [n]     int32    0 or DAD3D_POSE_FLAG_*
 *   The frame of a row's points: `frames` NULL: h x w for every row; else the DEVICE int64 table [n_frames][4] {address, h, w, row
 *   stride} of dad3d_preprocess_boxes with the DEVICE int32 image_index [n] (only h and w are read; no pixel is).
 *     NONFINITE   one of the six floats is NaN or +-inf
 *     DEGENERATE  the polar factor is undefined: the smallest singular value is below 1e-6 or the determinant is <= 0 (a zero first
 *                 vector, a second one parallel to it): the rows on which scipy raises
 *     GIMBAL      the second Euler angle is within 1e-7 rad of +-90 degrees: the third angle is 0 by convention
 *     INDEX       image_index outside [0, n_frames) or a frame without a size: rotation and rpy are written, points are all zero
 *   A NONFINITE or DEGENERATE row gets NaN angles and all ten points at its frame's centre.
 *   One launch on `stream`, no allocation, no scratch, no synchronisation: can be captured into a graph.
 * dad3d_procrustes  utils.py:183-272 `procrustes(X, Y)` with scaling and reflection="best" per item, float64:
 *     x, y [batch,n_points,3] -> b [batch], t [batch,3,3] row-major, c [batch,3] such that b * y . t + c best fits x; t = V U^T of
 *     the SVD of the normalised covariance with NO determinant fix (it may be a reflection); flags [batch]: DAD3D_POSE_FLAG_DEGENERATE
 *     with NaN results where a centred norm is 0 or not finite (one point, identical points, non-finite input; "0" is anything
 *     within n sqrt(n) eps max|mean|, the rounding error that the mean of n identical points leaves). Where the
 *     covariance is singular (planar or collinear points) t is one of the orthogonal matrices that fit, a proper rotation.
 *     An item's bits do not depend on what else is in the batch.
 * The two `_host` entries run the same routines on the CPU with HOST pointers (the frame table and image_index too) and need no GPU.
 * Arguments (NULL, negative sizes, alignment, points without a frame size) are validated before any work -> DAD3D_E_INVALID; n == 0 or
 * batch == 0: DAD3D_OK, nothing to do.
 * --------------------------------------------------------------------------------------------- */
#define DAD3D_POSE_FLAG_NONFINITE 0x1
#define DAD3D_POSE_FLAG_DEGENERATE 0x2
#define DAD3D_POSE_FLAG_GIMBAL 0x4
#define DAD3D_POSE_FLAG_INDEX 0x8
DAD3D_EXPORT dad3d_status dad3d_head_pose(const float* params, int n, int64_t row_stride, int rot_offset, const int64_t* frames /* or NULL */,
                                          int n_frames, const int32_t* image_index /* with frames */, int h, int w, float* rotation,
                                          double* rpy, float* points, int32_t* flags, int device, void* stream);
DAD3D_EXPORT dad3d_status dad3d_head_pose_host(const float* params, int n, int64_t row_stride, int rot_offset, const int64_t* frames,
                                               int n_frames, const int32_t* image_index, int h, int w, float* rotation, double* rpy,
                                               float* points, int32_t* flags);
DAD3D_EXPORT dad3d_status dad3d_procrustes(const double* x, const double* y, int batch, int n_points, double* b, double* t, double* c,
                                           int32_t* flags, int device, void* stream);
DAD3D_EXPORT dad3d_status dad3d_procrustes_host(const double* x, const double* y, int batch, int n_points, double* b, double* t, double* c,
                                                int32_t* flags);

/* ---------------------------------------------------------------------------------------------
 * PNG files and zlib streams read back on the device, bit-equal to `PIL.Image.open` and `zlib.decompress` (RFC 1950, 1951, the PNG
 * specification): 8-bit grey, grey + alpha, RGB and RGBA files without interlace, of any sizes in one call.
 *   files   DEVICE: the bytes of every file, file b at files[desc[b][0] .. + desc[b][1])
 *   desc    DEVICE [batch][DAD3D_PNG_DECODE_DESC_INTS] int64: file offset, file bytes (below 2^31), height, width and channels as
 *           the file's IHDR states them (the caller has read the signature and IHDR, nothing else, to size the outputs), offset of
 *           the image in `out`, its row stride in bytes (at least width * out channels), out channels 1 .. 4, and four columns
 *           that dad3d_png_decode_scratch_bytes fills: where the item's filtered stream, IDAT range table (and its capacity) and
 *           segment records lie in `scratch`
 *   out     DEVICE: image b is [height][row stride] bytes from out[desc[b][5]], `width * out channels` of each row written; bytes
 *           between and behind the rows, and behind an item, are left as they were
 *   flags   DEVICE [batch] int32: 0, or why the item was not decoded -- DAD3D_PNG_DECODE_FLAG_MALFORMED (signature, a chunk's
 *           CRC-32 or length, chunk order, an unknown critical chunk, IHDR against the row, the zlib stream, its Adler-32, its
 *           length, a filter type above 4, or a row that points outside the buffers) or _UNSUPPORTED (a valid file outside this
 *           decoder: palette, 16-bit, depth below 8, Adam7). The pixels of a flagged item are unspecified; the caller decodes it on
 *           the host. Nothing outside the item's own places is read or written whatever the file holds.
 *   info    DEVICE [batch] int32: DAD3D_PNG_DECODE_INFO_SEGMENTED when the file had the layout dad3d_png_encode writes (an IDAT
 *           with the zlib header, IDATs ending in 00 00 FF FF, an IDAT with 03 00 + Adler-32) and every IDAT inflated by itself:
 *           complete non-final blocks ending on its last byte, no distance more than 4 bytes in front of its own output (those 4
 *           are resolved from the IDAT before, as the encoder's matches need), DAD3D_PNG_SEGMENT_BYTES bytes each and the
 *           rest in the last, the combined Adler-32 equal to the trailer. Any other file, and every file when
 *           `force_general` is nonzero, goes through the serial inflate of the whole stream in the same call.
 * Out channels follow PIL's `convert`: grey is replicated, alpha is dropped or 255, L = (19595 R + 38470 G + 7471 B + 32768) >> 16.
 * dad3d_png_decode_scratch_bytes is host-only: it reads columns 1 .. 4 and 7 of HOST rows, fills columns 8 .. 11, gives the grid
 * width `max_segments` and returns the bytes of scratch (16-byte aligned), 0 for a row outside the limits (a filtered stream of
 * 2^31 bytes or more). Five launches on `stream` (three with force_general), no allocation, no synchronisation: can be captured.
 * dad3d_zlib_decompress is the inverse of dad3d_zlib_compress for any zlib stream: desc DEVICE [batch][DAD3D_ZLIB_DECODE_DESC_INTS]
 * int64 = offset and bytes of the stream in `streams`, offset (a multiple of 16) and capacity of its place in `out` (16-byte
 * aligned). lengths[b] = the bytes written, flags[b] = 0, _MALFORMED or _OVERFLOW (the stream holds more than the capacity; length 0).
 * dad3d_inflate_host runs the same inflate routine on the CPU, HOST pointers: the stream is the concatenation of n_ranges byte
 * ranges (empty ones allowed); *flag as above, *length = the bytes written into out[0, capacity).
 * --------------------------------------------------------------------------------------------- */
#define DAD3D_PNG_DECODE_DESC_INTS 12
#define DAD3D_ZLIB_DECODE_DESC_INTS 4
#define DAD3D_PNG_DECODE_FLAG_MALFORMED 0x1
#define DAD3D_PNG_DECODE_FLAG_UNSUPPORTED 0x2
#define DAD3D_PNG_DECODE_FLAG_OVERFLOW 0x4
#define DAD3D_PNG_DECODE_INFO_SEGMENTED 0x1
DAD3D_EXPORT size_t dad3d_png_decode_scratch_bytes(int64_t* desc, int batch, int32_t* max_segments);
DAD3D_EXPORT dad3d_status dad3d_png_decode(const uint8_t* files, size_t files_bytes, const int64_t* desc, int batch, int max_segments,
                                           uint8_t* out, size_t out_bytes, int32_t* flags, int32_t* info, void* scratch, size_t scratch_bytes,
                                           int force_general, int device, void* stream);
DAD3D_EXPORT dad3d_status dad3d_zlib_decompress(const uint8_t* streams, size_t streams_bytes, const int64_t* desc, int batch, uint8_t* out,
                                                size_t out_bytes, int64_t* lengths, int32_t* flags, int device, void* stream);
DAD3D_EXPORT dad3d_status dad3d_inflate_host(const uint8_t* const* ranges, const int64_t* range_bytes, int n_ranges, uint8_t* out,
                                             int64_t capacity, int64_t* length, int32_t* flag);

/* ---------------------------------------------------------------------------------------------
 * Baseline JPEG files read back on the device, bit-equal to `PIL.Image.open` (libjpeg-turbo: the "islow" integer IDCT, "fancy"
 * upsampling): Huffman-coded sequential files of 8-bit samples with one scan, grey or YCbCr at 4:4:4, 4:2:2 (2x1) or 4:2:0 (2x2),
 * with or without restart markers, of any sizes in one call.
 *   files   DEVICE: the bytes of every file, file b at files[desc[b][0] .. + desc[b][1])
 *   desc    DEVICE [batch][DAD3D_JPEG_DECODE_DESC_INTS] int64: file offset, file bytes (below 2^31), height, width and components
 *           (1 or 3) as the file's SOF0 states them (the caller has walked the markers up to SOF, nothing else, to size the
 *           outputs), offset of the image in `out`, its row stride in bytes (at least width * out channels), out channels 1 or 3,
 *           and four columns that dad3d_jpeg_decode_scratch_bytes fills: where the item's coefficients, planes and segment table
 *           (and its capacity) lie in `scratch`
 *   grid    HOST [DAD3D_JPEG_DECODE_GRID_INTS] int32 from dad3d_jpeg_decode_scratch_bytes: the most segments, blocks and pixels a
 *           file of the batch may have, which size the launches
 *   out     DEVICE: image b is [height][row stride] bytes from out[desc[b][5]], `width * out channels` of each row written; bytes
 *           between and behind the rows, and behind an item, are left as they were
 *   flags   DEVICE [batch] int32: 0, or why the item was not decoded -- DAD3D_JPEG_DECODE_FLAG_MALFORMED (a marker segment's
 *           length, a table's validity, a missing table, SOF0 against the row, the restart markers' number or sequence, a
 *           segment that needs a bit beyond its last byte or leaves a whole byte unread, a code no table assigns, a
 *           coefficient index beyond 63, no EOI, or a row that points outside the buffers) and / or _UNSUPPORTED (a valid file
 *           outside this decoder: progressive, extended, lossless, arithmetic coding, 12-bit samples, 16-bit tables, two or
 *           four components, other sampling factors, several scans, DNL, an Adobe APP14, component ids other than 1 2 3 without
 *           JFIF, fill bytes in front of a marker inside the scan, or values outside the 16 bits in front of and behind the
 *           first IDCT pass, or outside -512 .. 511 behind the second, where libjpeg-turbo's vector code and its C code part).
 *           The pixels of a flagged item are unspecified; the caller decodes it on the host. Nothing outside the item's own
 *           places is read or written whatever the file holds.
 * Out channels follow PIL's `convert`: grey is replicated, L = (19595 R + 38470 G + 7471 B + 32768) >> 16.
 * dad3d_jpeg_decode_scratch_bytes is host-only: it reads columns 1 .. 4 of HOST rows, fills columns 8 .. 11 and `grid`, and returns
 * the bytes of scratch (16-byte aligned), 0 for a row outside the limits. Four launches on `stream`, no allocation, no
 * synchronisation: can be captured.
 * dad3d_jpeg_decode_host runs the same routines on one file on the CPU, HOST pointers: channels 0 keeps the file's own; *h, *w, *c
 * are set whenever the header was accepted; `out` may be NULL to read the header alone, and is otherwise [h][w][c] (DAD3D_E_INVALID
 * where out_bytes is too small). *flag as above.
 * --------------------------------------------------------------------------------------------- */
#define DAD3D_JPEG_DECODE_DESC_INTS 12
#define DAD3D_JPEG_DECODE_GRID_INTS 3
#define DAD3D_JPEG_DECODE_FLAG_MALFORMED 0x1
#define DAD3D_JPEG_DECODE_FLAG_UNSUPPORTED 0x2
DAD3D_EXPORT size_t dad3d_jpeg_decode_scratch_bytes(int64_t* desc, int batch, int32_t* grid);
DAD3D_EXPORT dad3d_status dad3d_jpeg_decode(const uint8_t* files, size_t files_bytes, const int64_t* desc, int batch, const int32_t* grid,
                                            uint8_t* out, size_t out_bytes, int32_t* flags, void* scratch, size_t scratch_bytes, int device,
                                            void* stream);
DAD3D_EXPORT dad3d_status dad3d_jpeg_decode_host(const uint8_t* file, int64_t size, int channels, uint8_t* out, int64_t out_bytes, int32_t* h,
                                                 int32_t* w, int32_t* c, int32_t* flag);

/* ---------------------------------------------------------------------------------------------
 * dad3d_jpeg_decode with a second entropy stage: the same files, pixels and flags, but a file WITHOUT restart markers (DRI 0), which
 * dad3d_jpeg_decode hands to a single lane, is cut into pieces of `piece_bytes` (a power of two, 16 .. 256) that are decoded side by
 * side. Every piece first walks the Huffman codes from a guess; groups of 256 pieces hand their exit states forward until nothing
 * changes (launch A), then once more from the exit of the group in front (launch B). A file is *verified* when every group's exit is
 * the same behind both launches: its chain of states is then the serial walk's, and every piece decodes its own codes with all the
 * checks of the serial walk. A file that is not verified is decoded by one lane inside the same call, so the result never depends on
 * the guesses. A file with restart markers takes one lane per segment as in dad3d_jpeg_decode.
 *   desc    DEVICE [batch * DAD3D_JPEG_DECODE_SYNC_DESC_INTS] int64: the batch's rows of DAD3D_JPEG_DECODE_DESC_INTS columns exactly
 *           as dad3d_jpeg_decode takes them, and behind all of them [batch][4]: where the item's piece table and group table lie in
 *           `scratch` and how many entries each holds. dad3d_jpeg_decode_sync_scratch_bytes fills these four and columns 8 .. 11.
 *   grid    HOST [DAD3D_JPEG_DECODE_SYNC_GRID_INTS] int32: the three of dad3d_jpeg_decode and the most groups a file may have
 *   info    DEVICE [batch][4] int32: mode, pieces, groups, 0. Mode DAD3D_JPEG_DECODE_SYNC_MODE_SEGMENTS (0): one lane per restart
 *           segment; _VERIFIED (1): in pieces; _SERIAL (2): not verified, one lane. All 0 for an item the header scan has flagged.
 *   files, out, flags, scratch as for dad3d_jpeg_decode; the flags are the same for every file whatever `piece_bytes`.
 * A `piece_bytes` outside the rule gives DAD3D_E_INVALID before any device work (0 from dad3d_jpeg_decode_sync_scratch_bytes). Nine
 * launches on `stream`, no allocation, no synchronisation: can be captured. Nothing outside the item's own places is read or written
 * whatever the file holds.
 * dad3d_jpeg_decode_sync_host runs the same routines on one file on the CPU, group after group, as dad3d_jpeg_decode_host does for
 * dad3d_jpeg_decode; info is HOST [4] (all 0 while `out` is NULL or the header is flagged).
 * --------------------------------------------------------------------------------------------- */
#define DAD3D_JPEG_DECODE_SYNC_DESC_INTS 16
#define DAD3D_JPEG_DECODE_SYNC_GRID_INTS 4
#define DAD3D_JPEG_DECODE_SYNC_MODE_SEGMENTS 0
#define DAD3D_JPEG_DECODE_SYNC_MODE_VERIFIED 1
#define DAD3D_JPEG_DECODE_SYNC_MODE_SERIAL 2
DAD3D_EXPORT size_t dad3d_jpeg_decode_sync_scratch_bytes(int64_t* desc, int batch, int32_t* grid, int piece_bytes);
DAD3D_EXPORT dad3d_status dad3d_jpeg_decode_sync(const uint8_t* files, size_t files_bytes, const int64_t* desc, int batch, const int32_t* grid,
                                                 int piece_bytes, uint8_t* out, size_t out_bytes, int32_t* flags, int32_t* info, void* scratch,
                                                 size_t scratch_bytes, int device, void* stream);
DAD3D_EXPORT dad3d_status dad3d_jpeg_decode_sync_host(const uint8_t* file, int64_t size, int channels, int piece_bytes, uint8_t* out,
                                                      int64_t out_bytes, int32_t* h, int32_t* w, int32_t* c, int32_t* flag, int32_t* info);

/* ---------------------------------------------------------------------------------------------
 * Images as baseline JPEG files made on the device, byte-equal to
 *   PIL.Image.fromarray(img).save(buf, "JPEG", quality=q, subsampling=s, restart_marker_rows=r)
 * with libjpeg-turbo behind PIL (mode RGB for c = 3, mode L for c = 1): its 16-bit fixed-point RGB -> YCbCr, edge replication, the
 * h2v1 / h2v2 box filters with their alternating bias, the "islow" integer forward DCT, division by 8 Q rounded half away from zero,
 * the standard Huffman tables, and libjpeg's order of header segments (SOI, JFIF APP0 with units 0 and density 1 x 1, a DQT per
 * table, SOF0, a DHT per table, DRI when there is an interval, SOS).
 *   images   DEVICE [batch,h,w,c] uint8, contiguous, c = 1 (grey) or 3 (RGB); h, w in 1 .. 65535 and at most 2^22 blocks per image
 *   quality  1 .. 100: libjpeg's scaling of the Annex K tables, forced to baseline (1 .. 255)
 *   subsampling  0 / 1 / 2 = 4:4:4 / 4:2:2 / 4:2:0; ignored for c = 1
 *   restart_interval  MCUs between restart markers, 0 .. 65535, 0 for none (libjpeg's restart_in_rows is rows x MCUs per row; the
 *            caller multiplies, and refuses a product above 65535 where libjpeg would clamp it)
 *   out      DEVICE [batch][out_stride] bytes, 16-byte aligned; out_stride a multiple of 16, at least dad3d_jpeg_max_bytes(h, w, c,
 *            subsampling). Item b's file is out[b * out_stride .. + lengths[b]); bytes behind it are left as they were
 *   lengths  DEVICE [batch] int64   flags DEVICE [batch] int32   scratch DEVICE dad3d_jpeg_encode_scratch_bytes(..) bytes, 16-byte aligned
 * dad3d_jpeg_max_bytes is a bound no file passes: the header (at most 629 bytes) + per block of the scan, dummy blocks included, twice
 * 208 bytes -- a block's worst is a DC code of 11 bits with 11 value bits and 63 AC codes of 16 bits with 10 value bits each, 1660
 * bits, rounded up to bytes per block so that the sum covers the padding of every interval, and byte stuffing (FF -> FF 00) at most
 * doubles entropy bytes -- + 4 bytes per MCU (a restart marker behind every interval of the shortest interval, EOI behind the last;
 * twice two bytes because the device checks each chunk against the row as if every byte of it were stuffed) + 16.
 * flags[b] == 0 unless the encoder's own consistency check failed (DAD3D_JPEG_ENCODE_FLAG_INTERNAL: a coefficient outside baseline's
 * categories, or a file that would pass its row; length 0, the caller encodes that item on the host). Two launches on `stream`, no
 * allocation, no synchronisation: can be captured into a graph. Arguments (NULL, c not 1 or 3, h or w outside 1 .. 65535, more than
 * 2^22 blocks, batch outside 1 .. 65535, quality outside 1 .. 100, subsampling outside 0 .. 2, an interval outside 0 .. 65535, a
 * stride or scratch below what the shape needs, alignment) are validated before any device work -> DAD3D_E_INVALID. The *_max_bytes /
 * *_scratch_bytes calls are host-only and return 0 for such a shape.
 * dad3d_jpeg_encode_host runs the same routines on one image on the CPU, HOST pointers: the file goes to out[0 .. *length),
 * capacity >= dad3d_jpeg_max_bytes; *flag as above.
 * --------------------------------------------------------------------------------------------- */
#define DAD3D_JPEG_ENCODE_FLAG_INTERNAL 0x1
DAD3D_EXPORT size_t dad3d_jpeg_max_bytes(int h, int w, int c, int subsampling);
DAD3D_EXPORT size_t dad3d_jpeg_encode_scratch_bytes(int batch, int h, int w, int c, int subsampling);
DAD3D_EXPORT dad3d_status dad3d_jpeg_encode(const uint8_t* images, int batch, int h, int w, int c, int quality, int subsampling,
                                            int restart_interval, uint8_t* out, size_t out_stride, int64_t* lengths, int32_t* flags,
                                            void* scratch, size_t scratch_bytes, int device, void* stream);
DAD3D_EXPORT dad3d_status dad3d_jpeg_encode_host(const uint8_t* image, int h, int w, int c, int quality, int subsampling, int restart_interval,
                                                 uint8_t* out, int64_t capacity, int64_t* length, int32_t* flag);

/* ---------------------------------------------------------------------------------------------
 * Reading JSON back: the large arrays of numbers of a document lifted into float64 on the device, with the doubles `json.load` makes
 * (dad_3dheads_benchmark/benchmark.py:177-180, the two `json.load` calls of `DADEvaluator.__call__`). The device lifts only what it has
 * validated and converted exactly; every other byte stays with the host parser, so a result can never differ from `json.load`.
 * The document is `text`, n_bytes < 2^31 bytes on the DEVICE, 16-byte aligned, worked on in tiles of DAD3D_JSON_PARSE_TILE_BYTES. Every
 * scan is per-tile totals, a scan of the totals, then apply, as separate launches: no workgroup waits on another. Four stream-ordered
 * entries, all DEVICE pointers unless said otherwise; none allocates or synchronises, and each validates its arguments (NULL, sizes,
 * alignment, scratch) before any device work -> DAD3D_E_INVALID:
 *   dad3d_json_parse_index   string state (a quote behind an odd run of backslashes is escaped; parity of the others), the class of
 *                            every byte (one byte each, in `scratch`) and the totals. counts [4] int32 = {number tokens, brackets
 *                            `[` `]` outside strings, non-numeric bytes, final bracket depth}. A token is a maximal run of
 *                            `0-9 + - . e E` outside strings; a non-numeric byte is one inside a string, a quote, or any byte outside
 *                            strings that is not `[ ] ,`, space, tab, LF, CR or a token byte. Four launches.
 *   dad3d_json_parse_lists   after _index on the same scratch: compacts the tokens and brackets in document order. Token i: tok_pos[i]
 *                            = its first byte, tok_brk[i] = brackets in front of it. Bracket j: brk_pos[j], brk_key[j] = the depth
 *                            inside it (a `[` and its `]` share a key), brk_nonnum[j] / brk_tok[j] = non-numeric bytes / tokens in
 *                            front of it. Only the first tok_cap / brk_cap entries are written. One launch.
 *   dad3d_json_parse_check_arrays  for n_arrays candidate spans (bracket indices arr_open[a] < arr_close[a] of a matched pair with no
 *                            non-numeric byte inside), one workgroup each: arr_rows[a] = 0 for shape (n,), r for shape (r, n / r), -1
 *                            when the span is not liftable: brackets deeper than two levels, ragged or empty rows, a token beside a
 *                            row, malformed separators (with whitespace skipped: `[` or `,` in front of every token and inner `[`,
 *                            a token or `]` in front of that `,`, `,` or `]` behind every token and inner `]`, no `,` in front of a
 *                            `]`), or a token the number routine flags. One launch.
 *   dad3d_json_parse_extract for n_records lifted arrays, records [n_records][DAD3D_JSON_PARSE_RECORD_INTS] int32 = {byte of `[`,
 *                            byte behind `]`, first value index, count, rows, first token index}, first value indices ascending from 0:
 *                            one lane per value writes values[v] (float64) and is_int[v] (1: the token has no fraction and no
 *                            exponent part). n_values = the sum of the counts; nothing behind it is written. One launch.
 * dad3d_json_parse_scratch_bytes (host-only): the scratch both of the first two entries take, 0 for n_bytes < 1 or >= 2^31.
 * dad3d_json_parse_number_host runs the number routine on the CPU, HOST pointers: token i is text[starts[i], ends[i]); its double's
 * bits go to bits_out[i], is_int_out[i], and flags_out[i] = 0 or DAD3D_JSON_PARSE_FLAG_* (then bits_out[i] = 0). The routine is exact
 * integer arithmetic (Eisel-Lemire against a 128-bit table of powers of five) and flags what it will not decide.
 * --------------------------------------------------------------------------------------------- */
#define DAD3D_JSON_PARSE_TILE_BYTES 4096 /* 256 lanes x 16 bytes */
#define DAD3D_JSON_PARSE_RECORD_INTS 6
#define DAD3D_JSON_PARSE_FLAG_GRAMMAR 0x1   /* not -?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][+-]?[0-9]+)? */
#define DAD3D_JSON_PARSE_FLAG_DIGITS 0x2    /* more than 19 significant digits */
#define DAD3D_JSON_PARSE_FLAG_BIG_INT 0x4   /* an integer token beyond 2^53 */
#define DAD3D_JSON_PARSE_FLAG_SUBNORMAL 0x8 /* below the smallest normal double */
#define DAD3D_JSON_PARSE_FLAG_OVERFLOW 0x10 /* beyond the largest double */
#define DAD3D_JSON_PARSE_FLAG_AMBIGUOUS 0x20 /* the truncated product cannot decide the rounding */
DAD3D_EXPORT size_t dad3d_json_parse_scratch_bytes(int64_t n_bytes);
DAD3D_EXPORT dad3d_status dad3d_json_parse_index(const uint8_t* text, int64_t n_bytes, void* scratch, size_t scratch_bytes, int32_t* counts,
                                    int device, void* stream);
DAD3D_EXPORT dad3d_status dad3d_json_parse_lists(const uint8_t* text, int64_t n_bytes, const void* scratch, size_t scratch_bytes,
                                    int32_t* tok_pos, int32_t* tok_brk, int64_t tok_cap, int32_t* brk_pos, int32_t* brk_key,
                                    int32_t* brk_nonnum, int32_t* brk_tok, int64_t brk_cap, int device, void* stream);
DAD3D_EXPORT dad3d_status dad3d_json_parse_check_arrays(const uint8_t* text, int64_t n_bytes, const int32_t* tok_pos, const int32_t* tok_brk,
                                           int64_t n_tokens, const int32_t* brk_pos, const int32_t* brk_key, const int32_t* brk_tok,
                                           int64_t n_brackets, const int32_t* arr_open, const int32_t* arr_close, int32_t* arr_rows,
                                           int64_t n_arrays, int device, void* stream);
DAD3D_EXPORT dad3d_status dad3d_json_parse_extract(const uint8_t* text, int64_t n_bytes, const int32_t* tok_pos, int64_t n_tokens,
                                      const int32_t* records, int64_t n_records, int64_t n_values, double* values, uint8_t* is_int,
                                      int64_t values_cap, int device, void* stream);
DAD3D_EXPORT dad3d_status dad3d_json_parse_number_host(const uint8_t* text, const int64_t* starts, const int64_t* ends, size_t n,
                                          uint64_t* bits_out, uint8_t* is_int_out, uint32_t* flags_out);

/* ---------------------------------------------------------------------------------------------
 * DAD-3DHeads annotation files read on the device: what `FlameDataset._load_mesh` (model_training/data/flame_dataset.py:115-127) makes of
 * `json.load` -- np.array(data["vertices"], float32) [n_verts,3], data["model_view_matrix"] and data["projection_matrix"] [4,4] -- for a
 * batch of documents in ONE stream-ordered launch, one workgroup per document. All DEVICE pointers; the entry validates its arguments
 * before any device work (-> DAD3D_E_INVALID), allocates nothing, takes no scratch and never synchronises.
 *   text        n_bytes bytes, 16-byte aligned; document i is text[doc_offsets[i], doc_offsets[i] + doc_sizes[i]), its offset a multiple
 *               of 16, its size < 2^31. A document outside `text` gets DAD3D_ANNOTATION_FLAG_RANGE and is not read.
 *   vertices [B,n_verts,3], model_view [B,16], projection [B,16] float32; status [B] int32.
 * Documents are parsed in isolation: whatever one holds, the outputs and status of the others are those of parsing them alone.
 * status[i] == 0: the device validated every byte of document i and the three outputs are bit-equal to `_load_mesh` (every number token
 * through the routine of dad3d_json_parse_number_host, then a round-to-nearest-even cast to float32; the int token `-0` is 0).
 * status[i] != 0: DAD3D_ANNOTATION_FLAG_* bits; all three outputs of item i are NaN and the host parses the file. Status 0 requires:
 *   - outside strings only space, tab, LF, CR, `{ } [ ] , :` and words (maximal runs of letters, digits, `+ - .`, at most
 *     DAD3D_ANNOTATION_MAX_WORD_BYTES long): a word that starts with a digit or `-` is a number token the number routine does not flag
 *     (else _FLAG_NUMBER), any other word is `true`, `false` or `null`;
 *   - a quote opens or closes a string unless an odd run of backslashes stands in front of it (runs are counted up to
 *     DAD3D_ANNOTATION_MAX_BACKSLASH_RUN; a longer one is flagged). Every string byte is 0x20 .. 0x7E and a backslash escapes one of
 *     `" \ / b f n r t` only (else _FLAG_STRING);
 *   - every significant token (`{ } [ ] , :`, a string, a word) is legal given its kind, the two tokens in front of it and its depth: `{`
 *     is the first token and `}`, at depth 1, the last; no other `{` anywhere; at depth 1 `"key" : value` separated by commas, in arrays
 *     values separated by commas; nothing trailing, doubled or missing; quotes and brackets balance (else _FLAG_GRAMMAR);
 *   - among the keys at depth 1, "vertices", "model_view_matrix" and "projection_matrix" each appear exactly once, spelled plainly, no
 *     depth-1 key holds a backslash, and no key appears twice: keys are compared by a 32-bit FNV-1a hash of their bytes, so two keys
 *     that share a hash count as a repeat; a key is at most DAD3D_ANNOTATION_MAX_KEY_BYTES long and a document has at most
 *     DAD3D_ANNOTATION_MAX_KEYS of them (else _FLAG_KEYS);
 *   - "vertices" is an array of exactly n_verts arrays of exactly 3 number tokens, each matrix an array of 4 arrays of 4 (else
 *     _FLAG_SHAPE). Other keys' values: numbers, true, false, null, strings, and arrays of those nested to any depth. */
#define DAD3D_ANNOTATION_FLAG_GRAMMAR 0x1
#define DAD3D_ANNOTATION_FLAG_KEYS 0x2
#define DAD3D_ANNOTATION_FLAG_SHAPE 0x4
#define DAD3D_ANNOTATION_FLAG_NUMBER 0x8
#define DAD3D_ANNOTATION_FLAG_STRING 0x10
#define DAD3D_ANNOTATION_FLAG_RANGE 0x20
#define DAD3D_ANNOTATION_MAX_BACKSLASH_RUN 64
#define DAD3D_ANNOTATION_MAX_WORD_BYTES 32
#define DAD3D_ANNOTATION_MAX_KEY_BYTES 64
#define DAD3D_ANNOTATION_MAX_KEYS 128
DAD3D_EXPORT dad3d_status dad3d_annotation_parse(const uint8_t* text, int64_t n_bytes, const int64_t* doc_offsets, const int64_t* doc_sizes,
                                    int batch, int n_verts, float* vertices, float* model_view, float* projection, int32_t* status,
                                    int device, void* stream);

/* ---------------------------------------------------------------------------------------------
 * FaceMeshPredictor._transform + _array_to_batch (predictor.py:80-95,195-203) for a batch of uint8 RGB images of ANY sizes
 * in one launch: LongestMaxSize (cv2.resize INTER_LINEAR, 8-bit fixed-point path) -> PadIfNeeded (centred, 0) -> Normalize
 * ((x - 255 mean) * (1 / (255 std)), float32) -> CHW. All DEVICE pointers:
 *   descs [B][8] int64: {address of the image's first byte (HWC, 3 channels), h, w, new_h, new_w, pad_top, pad_left, row
 *                        stride in bytes}; the geometry (py3round, calculate_paddings: predictor.py:117-123) is the caller's
 *   out   [B,3,out_size,out_size] float32
 * mean/std: HOST arrays of 3 floats (the [0,1]-scale constants of A.Normalize). */
DAD3D_EXPORT dad3d_status dad3d_preprocess_images(const int64_t* descs, int batch, int out_size, const float* mean, const float* std,
                                     float* out, int device, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Glue of the DAD-3DNet forward between the framework's convolutions (the network itself stays on PyTorch-ROCm): channels-last
 * (NHWC, dense) DEVICE tensors of fp32 / fp16 / bf16 elements; `channels` a multiple of 16 bytes' worth (4 / 8).
 *   dad3d_nhwc_bias_act    y = act(y + bias[c] (+ z)), in place: the folded BatchNorm's shift, the bottleneck's identity and the
 *                          ReLU behind a convolution in ONE pass (model_training/model/layers.py conv-bn-relu blocks; pytorchcv's
 *                          ResUnit `x = body(x) + identity; x = activ(x)`, built at model_training/model/encoders.py:42-48).
 *                          (y + bias) + z in fp32, ONE rounding to nearest even at the store; the ReLU is F.relu's: a NaN stays a
 *                          NaN, -inf becomes 0
 *   dad3d_nhwc_resize_sum  out = sum_k weights[k] * nearest_resize(x_k -> [oh, ow]), k < n_inputs <= 3: a BiFPN node's weighted
 *                          fusion with its F.interpolate folded in (model_training/model/bifpn.py:98-125) */
#define DAD3D_DTYPE_F32 0
#define DAD3D_DTYPE_F16 1
#define DAD3D_DTYPE_BF16 2
DAD3D_EXPORT dad3d_status dad3d_nhwc_bias_act(void* y, const void* bias, const void* z /* or NULL */, int64_t n_pixels, int channels, int dtype,
                                 int relu, int device, void* stream);
DAD3D_EXPORT dad3d_status dad3d_nhwc_resize_sum(void* out, int n, int oh, int ow, int channels, int dtype, int n_inputs, const void* const* xs,
                                   const int* hs, const int* ws, const float* weights, int device, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The tail of the DAD-3DNet forward (csrc/net_tail.hip): the fusion layer's glue and the three regression heads
 * (model_training/model/flame_regression.py:28-43, 45-59, 96-100). Channels-last (NHWC, dense) DEVICE tensors of dtype
 * DAD3D_DTYPE_*, base pointers 16-byte aligned. Each entry runs on `stream`, allocates nothing, waits for nothing and uses no
 * floating-point atomics: two calls, and a graph replay, give the same bits.
 *
 * dad3d_nhwc_fusion_concat  out[n,y,x,:] = [ x[n,y,x,0:cx] | sigmoid(bilinear(heat)[n,y,x,0:ch]) | level[n,y,x,0:cl] ]
 *   x [n,oh,ow,cx] and level [n,oh,ow,cl] at out's extent, heat [n,hh,hw,ch] at its own; every segment's byte width a multiple of 8
 *   (the 68 heat-map channels of a 2-byte type are 136 bytes). The copied segments are byte copies. The middle one is
 *   F.interpolate(mode="bilinear", align_corners=True) and the sigmoid in fp32, every operation rounded on its own (no fused
 *   multiply-add), ONE rounding to nearest even at the store; per axis
 *     scale = (n_out > 1) ? (float)(n_in - 1) / (float)(n_out - 1) : 0.0f
 *     src = scale * (float)dst;  i0 = (int)src;  i1 = i0 + (i0 < n_in - 1);  l1 = src - (float)i0;  l0 = 1.0f - l1
 *     v   = lh0 * (lw0 * a + lw1 * b) + lh1 * (lw0 * c + lw1 * d)              (a, b from row i0; c, d from row i1)
 *     out = round_to_dtype(1.0f / (1.0f + expf(-v)))
 *   Non-finite values follow the formula (0 * inf = NaN).
 *
 * dad3d_nhwc_bias_mul  y[p][c] = round_to_dtype((y[p][c] + bias[c]) * x[p][c]), in place: the fusion convolution's bias and the
 *   product with its first input in one pass; fp32, two rounded operations (no fused form); `channels` a multiple of 16 bytes' worth.
 *
 * dad3d_regression_heads  top [batch, hw positions, channels] -> for each of n_heads <= DAD3D_HEADS_MAX heads
 *     pooled = (fp32 sum of top over the hw positions) / (float)hw                       (once for all heads)
 *     hidden = relu(pooled . w1^T + b1);  dst[b][col_offset + j] = act(hidden . w2^T + b2)[j]
 *   fp32 accumulation throughout; pooled and hidden are never rounded to the tensors' dtype. w1 [hidden, channels], b1 [hidden],
 *   w2 [out_dim, hidden], b2 [out_dim] row-major in top's dtype (nn.Linear's layout), 16-byte aligned; `channels` and every `hidden`
 *   a multiple of 16 bytes' worth. act: DAD3D_HEAD_ACT_NONE, _RELU (a NaN stays a NaN, as in F.relu) or _TANH (limit * tanhf(v),
 *   one rounded product). dst is float32 with dst_row_stride floats between images, so several heads can share one buffer.
 *     workspace   float32 [batch * (channels + sum of hidden)], 16-byte aligned: pooled, then hidden
 *     pooled_out  float32 [batch, channels] or NULL;  hidden_out  float32 [batch, sum of hidden] or NULL (heads in order): when given,
 *                 the stage is written there instead of into the workspace (for tests; 16-byte aligned)
 *   Three launches: the pool, the first layer of all heads, the second layer of all heads.
 *   DAD3D_E_INVALID before any device work: a null or misaligned tensor, a size <= 0, batch > 65535, an unknown dtype or activation,
 *   a channel or hidden count that is no multiple of 16 bytes' worth, a destination row shorter than its columns. */
#define DAD3D_HEADS_MAX 4
#define DAD3D_HEAD_ACT_NONE 0
#define DAD3D_HEAD_ACT_RELU 1
#define DAD3D_HEAD_ACT_TANH 2
typedef struct dad3d_head_desc {
    const void *w1, *b1, *w2, *b2;
    float* dst;
    int64_t dst_row_stride, dst_col_offset; /* in floats */
    int32_t hidden, out_dim, act;
    float limit; /* DAD3D_HEAD_ACT_TANH only */
} dad3d_head_desc;
DAD3D_EXPORT dad3d_status dad3d_nhwc_fusion_concat(void* out, const void* x, const void* heat, const void* level, int n, int oh, int ow, int hh,
                                      int hw, int cx, int ch, int cl, int dtype, int device, void* stream);
DAD3D_EXPORT dad3d_status dad3d_nhwc_bias_mul(void* y, const void* bias, const void* x, int64_t n_pixels, int channels, int dtype, int device,
                                 void* stream);
DAD3D_EXPORT dad3d_status dad3d_regression_heads(const void* top, int batch, int channels, int hw, int dtype, const dad3d_head_desc* heads,
                                    int n_heads, float* workspace, float* pooled_out /* or NULL */, float* hidden_out /* or NULL */,
                                    int device, void* stream);

/* ---------------------------------------------------------------------------------------------
 * From the network's 2-D outputs to landmark points (csrc/heatmap_points.hip). All tensors are DEVICE pointers.
 *
 * dad3d_heatmap_argmax   `unravel_index` (model_training/model/utils.py:44-52) of a dense [B,C,H,W] heatmap: the argmax of
 *   torch.sigmoid(heatmap) with sigmoid = 1 (predictor.py:108-112) or of the values themselves with sigmoid = 0
 *   (train/flame_lightning_model.py:294-297). Every value is read once. NCHW is one launch; so is a channels-last image of
 *   fewer than 512 pixels, and a larger one is split over workgroups that meet in yx_out (zeroed first, an atomic maximum of
 *   packed pairs: order-free, so deterministic) with a second tiny launch that unpacks it in place.
 *     dtype    DAD3D_DTYPE_F32 / _F16 / _BF16 or DAD3D_HEATMAP_DTYPE_U8 (the target heatmap of `get_2d_visuals`; no sigmoid)
 *     layout   DAD3D_LAYOUT_NCHW: contiguous; DAD3D_LAYOUT_NHWC: channels-last, each pixel's C channels adjacent, pixels row-major
 *     yx_out   int32 [B,C,2] = (k // H, k % H): the reference's own unravel (utils.py:50-51 divides by H, not W), kept for H != W
 *     peak_out float32 [B,C] or NULL: the winning value (the sigmoid's value with sigmoid = 1, the byte's value for uint8)
 *   k is torch.argmax's / np.argmax's flat index in [0, H*W): the smallest k whose value is NaN if there is one, else the smallest
 *   k whose value equals the maximum; -0.0 == +0.0; an all -inf or all-equal plane gives 0. With sigmoid = 1 the values compared
 *   are 1.0f / (1.0f + expf(-x)) in float32, rounded to nearest even to fp16 / bf16 for those inputs and compared there, so the
 *   first saturated position wins (float32: every logit >= 16.636066 is 1.0), not the largest logit.
 *   DAD3D_E_INVALID before any device work: a null heatmap or yx_out, a heatmap not aligned to its element, a size <= 0,
 *   H*W > 2^24, B*C > 2^31 - 1, an unknown dtype or layout, sigmoid with uint8.
 *
 * dad3d_points_readjust  `readjust_landmarks_to_the_input_image` with the clip in front of it (predictor.py:132-133,147-152) for a
 *   batch. src_kind 0: float32 [B,n,2] regressed (x, y); src_kind 1: int32 [B,n,2] (row, col) of dad3d_heatmap_argmax, flipped to
 *   (x, y) here. Per coordinate, every step rounded on its own as numpy does: float32 v = src * mul (256.0 or float(stride));
 *   clip to [0, limit] in float32; widen to float64; subtract the integer pad (pad_left for x, pad_top for y); divide by the
 *   float64 scale (img_size / float(max_side)); truncate toward zero to int32 (saturating). +-inf are made finite by the clip; a NaN
 *   gives INT32_MIN (numpy's cast is undefined there: this library's choice).
 *     geometry   float64 [B,3] (pad_left, pad_top, scale) per image, or NULL: the one triple passed by value holds for the batch
 *     points_out int32 [B,n,2] (x, y)
 *   DAD3D_E_INVALID before any device work: a null src or points_out, a size <= 0, B*n*2 > 2^31 - 1, an unknown src_kind, and
 *   without geometry a scale that is not a positive finite number. */
#define DAD3D_HEATMAP_DTYPE_U8 3
#define DAD3D_LAYOUT_NCHW 0
#define DAD3D_LAYOUT_NHWC 1
#define DAD3D_POINTS_SRC_XY_F32 0
#define DAD3D_POINTS_SRC_YX_I32 1
DAD3D_EXPORT dad3d_status dad3d_heatmap_argmax(const void* heatmap, int dtype, int batch, int channels, int h, int w, int layout, int sigmoid,
                                  int32_t* yx_out, float* peak_out /* or NULL */, int device, void* stream);
DAD3D_EXPORT dad3d_status dad3d_points_readjust(const void* src, int src_kind, int batch, int n_points, float mul, float limit,
                                   const double* geometry /* or NULL */, int pad_left, int pad_top, double scale, int32_t* points_out,
                                   int device, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The heads of a frame from bounding boxes (csrc/preprocess_boxes.hip): DAD-3DNet was trained on crops made by a box widened by
 * about 10 % (model_training/data/flame_dataset.py:96-99), and its results are wanted in the frame's coordinates. No detector is
 * part of this library: the boxes are the caller's.
 *
 * dad3d_preprocess_boxes  ONE launch from frames and boxes to the network's input. DEVICE pointers except `offset`, `mean`, `std`:
 *     images      int64 [M][4]: {address of the frame's first byte (uint8 RGB, HWC, unit pixel stride), h, w, row stride in bytes}
 *     boxes       [N][4] (x, y, w, h) of box_dtype (DAD3D_BOX_DTYPE_*); every value is widened exactly to float64
 *     image_index int32 [N]: the frame of each box
 *     offset      HOST (left, right, top, bottom), the factors of `extend_bbox`, or NULL for none
 *     out         out_format DAD3D_PREPROCESS_OUT_F32_NCHW: float32 [N,3,S,S], the bits of dad3d_preprocess_images on the copied crop;
 *                 _F16_NHWC / _BF16_NHWC: [N,S,S,3] of that dtype, the float32 values rounded to nearest even, i.e. the memory of
 *                 `float32_result.to(dtype).contiguous(memory_format=torch.channels_last)`. 4-byte aligned.
 *     crops       int32 [N][4]: the (x, y, w, h) used
 *     geometry    float64 [N][5]: pad_left, pad_top, scale, x, y
 *     flags       int32 [N]: DAD3D_BOX_FLAG_*
 *   Per box, on the device: with an offset `extend_bbox` (data/utils.py:73-103) in float64 -- x - w*left, y - h*top,
 *   w*((1.0 + right) + left), h*((1.0 + top) + bottom), each truncated toward zero to int32 -- and without one the truncation alone;
 *   `ensure_bbox_boundaries` (data/utils.py:106-115) in integers; then the predictor's geometry on the crop's (h, w)
 *   (predictor.py:117-123): scale = S / float(max(h, w)), new = rint(dim * scale) (half to even: py3round), calculate_paddings;
 *   then LongestMaxSize -> PadIfNeeded -> Normalize -> CHW as dad3d_preprocess_images does them, the crop read in place. The crop's
 *   edges are the resize's borders: no pixel outside the crop is read.
 *     DAD3D_BOX_FLAG_EMPTY      the crop's w or h is <= 0 after the boundary rule
 *     DAD3D_BOX_FLAG_COLLAPSED  new_h or new_w is 0 (a 1 x 1000 crop: py3round(0.256) = 0)
 *     DAD3D_BOX_FLAG_RANGE      a value of the box (before or after extend_bbox) that is not finite or whose magnitude is >= 2^30, an
 *                               image_index outside [0, M), a frame with a null address or a side outside [1, 2^30); crops = 0
 *   A flagged box divides nothing, reads no pixel, gets the all-padding image (normalised zeros) and geometry (0, 0, 1, 0, 0).
 *   DAD3D_E_INVALID before any device work: a null pointer, N or M or S outside 1 .. 65535 (N == 0 returns DAD3D_OK), an unknown
 *   box_dtype or out_format, an offset that is not finite, `out` not 4-byte aligned.
 *
 * dad3d_flame_readjust_params_frame  dad3d_flame_readjust_params on rows of that float64 geometry [B][5] (scale and pads converted
 *   to float32, as torch.tensor(.., dtype=float32) converts them), followed by HeadMesh.adjust_3dmm_to_paddings(params, [y, _, x, _])
 *   (head_mesh.py:48-60): t + (float32([x, y, 0]) * 2) / img_size, each operation rounded once. The decode of these params gives
 *   `projected_vertices` in the frame's pixels. With x = y = 0 the bits of dad3d_flame_readjust_params.
 *
 * dad3d_points_readjust_frame  dad3d_points_readjust with that geometry [B][5]: (x, y) is added as an integer after the reference's
 *   truncation (predictor.py:150-152), saturating. With x = y = 0 the bits of dad3d_points_readjust. */
#define DAD3D_BOX_DTYPE_I32 0
#define DAD3D_BOX_DTYPE_I64 1
#define DAD3D_BOX_DTYPE_F32 2
#define DAD3D_BOX_DTYPE_F64 3
#define DAD3D_PREPROCESS_OUT_F32_NCHW 0
#define DAD3D_PREPROCESS_OUT_F16_NHWC 1
#define DAD3D_PREPROCESS_OUT_BF16_NHWC 2
#define DAD3D_BOX_FLAG_EMPTY 0x1
#define DAD3D_BOX_FLAG_COLLAPSED 0x2
#define DAD3D_BOX_FLAG_RANGE 0x4
DAD3D_EXPORT dad3d_status dad3d_preprocess_boxes(const int64_t* images, int n_images, const void* boxes, int box_dtype,
                                    const int32_t* image_index, int n_boxes, const double* offset /* HOST [4] or NULL */, int out_size,
                                    const float* mean, const float* std, int out_format, void* out, int32_t* crops, double* geometry,
                                    int32_t* flags, int device, void* stream);
DAD3D_EXPORT dad3d_status dad3d_flame_readjust_params_frame(dad3d_flame* h, float* params, int batch, const double* geometry, void* stream);
DAD3D_EXPORT dad3d_status dad3d_points_readjust_frame(const void* src, int src_kind, int batch, int n_points, float mul, float limit,
                                         const double* geometry, int32_t* points_out, int device, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Tracking heads from frame to frame (csrc/track_boxes.hip): the boxes of the next call from the projected vertices of this one,
 * as 3DDFA_V2 tracks (detect once, then each frame's box from the previous frame's fit). Still no detector: the first boxes, and the
 * boxes of a head that was lost, are the caller's.
 *
 * dad3d_boxes_from_heads  ONE launch, one workgroup per head. DEVICE pointers:
 *     proj         float32: head i's vertex v at proj + i*head_stride + v*vertex_stride (strides in floats), x at +0 and y at +1;
 *                  vertex_stride >= 2, so [N,V,2] and [N,V,3] both work
 *     subset       int32 [n_subset]: the vertex indices to bound, duplicates allowed; or NULL / 0 for all n_verts
 *     frames       int64 [n_frames][4], the table of dad3d_preprocess_boxes: {address, h, w, row stride in bytes}; no pixel is read
 *     image_index  int32 [N]: the frame of each head
 *     prev_flags   int32 [N] or NULL: the flags of the call that produced proj (DAD3D_BOX_FLAG_*, or whatever the caller joins to them)
 *     boxes        int32 [N][4] (x, y, w, h), written
 *     flags        int32 [N]: DAD3D_TRACK_FLAG_*, written
 *   Per head, in this order; the first of 1 - 3 that holds is the head's only flag:
 *     1. DAD3D_TRACK_FLAG_PREVIOUS   prev_flags[i] != 0. No vertex of that head is read.
 *     2. DAD3D_TRACK_FLAG_RANGE      image_index[i] outside [0, n_frames); a frame with a null address or a side outside [1, 2^30)
 *                                    (the conditions of DAD3D_BOX_FLAG_RANGE); a subset index outside [0, n_verts)
 *     3. DAD3D_TRACK_FLAG_NONFINITE  a selected x or y is a NaN or +-inf, wherever it stands. Otherwise xmin, xmax, ymin, ymax are
 *                                    float32 values (min and max do not round), and DAD3D_TRACK_FLAG_RANGE again if one of them has a
 *                                    magnitude >= 2^30.
 *     4. x0 = floor(xmin), y0 = floor(ymin), x1 = ceil(xmax), y1 = ceil(ymax); the box is (x0, y0, x1 - x0, y1 - y0). It is NOT
 *        clipped to the frame: `extend_bbox` and `ensure_bbox_boundaries` do that in the next dad3d_preprocess_boxes.
 *     5. DAD3D_TRACK_FLAG_SMALL      min(w, h) < min_side
 *     6. DAD3D_TRACK_FLAG_OUTSIDE    double(inter) < min_visible * double(w * h), with inter the area of the box cut with
 *                                    [0, W) x [0, H), both areas in int64: one product, no division. Not evaluated where w * h == 0.
 *        5 and 6 may both be set.
 *   Any flag zeroes the head's box: (0, 0, 0, 0), which the next dad3d_preprocess_boxes flags DAD3D_BOX_FLAG_EMPTY without reading a
 *   pixel; passed on as prev_flags, that flag keeps the head PREVIOUS in its slot until the caller writes a fresh box there.
 *   (`ensure_bbox_boundaries` alone does not empty a box that lies outside its frame: (-50, -50, 20, 20) becomes the crop
 *   (0, 0, 24, 24) in the frame's corner.)
 *   DAD3D_E_INVALID before any device work: a null proj, frames, image_index, boxes or flags; n_heads, n_verts or n_frames outside
 *   1 .. 65535 (n_heads == 0 returns DAD3D_OK), n_subset outside 1 .. 65535 with a subset, a subset without a count or a count without
 *   a subset; vertex_stride < 2; min_side < 0; min_visible outside [0, 1] or a NaN. */
#define DAD3D_TRACK_FLAG_PREVIOUS 0x1
#define DAD3D_TRACK_FLAG_RANGE 0x2
#define DAD3D_TRACK_FLAG_NONFINITE 0x4
#define DAD3D_TRACK_FLAG_SMALL 0x8
#define DAD3D_TRACK_FLAG_OUTSIDE 0x10
DAD3D_EXPORT dad3d_status dad3d_boxes_from_heads(const float* proj, int n_heads, int n_verts, int64_t head_stride, int vertex_stride,
                                    const int32_t* subset /* or NULL */, int n_subset, const int64_t* frames, int n_frames,
                                    const int32_t* image_index, const int32_t* prev_flags /* or NULL */, int min_side,
                                    double min_visible, int32_t* boxes, int32_t* flags, int device, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Steady tracks (csrc/track_steady.hip): two per-slot rules over state that stays on the device, each ONE launch, each held bit
 * for bit to its numpy statement (steady.one_euro_rows, boxes.suppress_duplicates). The unit is built with -ffp-contract=off.
 *
 * dad3d_one_euro_rows  A One-Euro filter (Casiez, Roussel, Vogel 2012) over the rows of a float32 matrix [n,d]. DEVICE pointers:
 *     x           float32: row i at x + i*x_stride (strides in floats, >= d)
 *     out         float32: row i at out + i*out_stride, written. out may be x itself with x's stride (in place); any other overlap
 *                 is undefined
 *     flags       int32 [n] or NULL: a row whose flag is not 0 is meaningless (DAD3D_BOX_FLAG_*, DAD3D_TRACK_FLAG_*)
 *     min_cutoff, beta   float32 [d]: the filter's two constants per column
 *     state_x, state_dx  float32 [n][d], contiguous: the last output and the last filtered derivative, read and written
 *     age         int32 [n]: the number of samples a row's track has seen, read and written; 0 starts a track
 *   The rule is stated on three float32 scalars that the HOST computes once per call from dt in float64 and rounds once:
 *     rate = 1/dt,  two_pi_dt = 2 pi dt,  alpha_d = r_d / (r_d + 1) with r_d = 2 pi d_cutoff dt
 *   Per row i, in this order:
 *     1. flags != NULL && flags[i] != 0:  out[i,:] = x[i,:], age[i] = 0, the state rows stay as they are. The track restarts.
 *     2. some x[i,c] is a NaN or an infinity:  the same as 1.
 *     3. age[i] <= 0:  out = x, state_x = x, state_dx = +0.0, age = 1.
 *     4. otherwise per element, in float32, every operation rounded once (xp = state_x, dxp = state_dx):
 *            dx  = (x - xp) * rate
 *            dxh = dxp + alpha_d * (dx - dxp)
 *            fc  = min_cutoff[c] + beta[c] * fabsf(dxh)
 *            r   = two_pi_dt * fc
 *            a   = r / (r + 1.0f)              (the correctly rounded quotient, denormals kept)
 *            out = xp + a * (x - xp)
 *        then state_x = out, state_dx = dxh, age = min(age + 1, 2^30).
 *     5. if some out[i,c] or dxh of 4 is not finite (x - xp can overflow; inf / inf is a NaN), the row restarts as in 3 instead.
 *        The state therefore never holds a NaN or an infinity that the kernel wrote.
 *   DAD3D_E_INVALID before any launch, and nothing is written: d < 1; n < 0; a stride below d; rate, two_pi_dt or alpha_d not finite
 *   or not positive; alpha_d > 1; then (n == 0 returns DAD3D_OK with no launch) a null x, out, min_cutoff, beta, state_x, state_dx
 *   or age.
 *
 * dad3d_track_suppress_duplicates  Two slots that converged on one head: the later one is flagged and zeroed. In place on what
 * dad3d_boxes_from_heads left. DEVICE pointers:
 *     boxes        int32 [n][4] (x, y, w, h), read and written
 *     flags        int32 [n]: DAD3D_TRACK_FLAG_*, read and written
 *     image_index  int32 [n]: the frame of each slot; any values, compared for equality only
 *   A slot takes part only if flags == 0 and w > 0 and h > 0. Walk j upward: slot j is a duplicate if some KEPT earlier slot i < j
 *   (one that takes part and is no duplicate itself) has image_index[i] == image_index[j] and
 *       inter > 0  and  double(inter) >= merge_iou * double(union)
 *   with all areas in int64: inter from the int64 minimum and maximum of the corners (x, y, x + w, y + h),
 *   union = w_i*h_i + w_j*h_j - inter (two int32 sides cannot overflow that sum); one product, no division. A duplicate gets
 *   flags = DAD3D_TRACK_FLAG_DUPLICATE and the box (0, 0, 0, 0); no other word is written. The rule is greedy, not "any overlap":
 *   a slot suppressed by i suppresses nobody. The lower slot wins; that choice is arbitrary but fixed (which of two converged slots
 *   is the right one cannot be known without appearance).
 *   n <= DAD3D_TRACK_MAX_SLOTS: one workgroup holds the pair bits in LDS. The allocation is static and sized for the cap whatever
 *   n is -- 1024^2 / 8 bytes of bits plus 20 KiB of staged boxes and frame numbers, 151 552 bytes of the CU's 160 KiB -- so a
 *   launch of 64 slots occupies as much LDS as one of 1024; it is one workgroup either way.
 *   DAD3D_E_INVALID before any launch: merge_iou not finite or outside (0, 1]; n < 0 or n > DAD3D_TRACK_MAX_SLOTS; then (n == 0
 *   returns DAD3D_OK) a null boxes, flags or image_index. */
#define DAD3D_TRACK_MAX_SLOTS 1024
/* Parenthesised on purpose: this bit is set by dad3d_track_suppress_duplicates alone. The five plain DAD3D_TRACK_FLAG_* above are
 * the complete set dad3d_boxes_from_heads writes, and are counted as such. */
#define DAD3D_TRACK_FLAG_DUPLICATE (0x20)
DAD3D_EXPORT dad3d_status dad3d_one_euro_rows(const float* x, int64_t x_stride, float* out, int64_t out_stride, int n, int d,
                                 const int32_t* flags /* or NULL */, const float* min_cutoff, const float* beta, float rate,
                                 float two_pi_dt, float alpha_d, float* state_x, float* state_dx, int32_t* age, int device,
                                 void* stream);
DAD3D_EXPORT dad3d_status dad3d_track_suppress_duplicates(int32_t* boxes, int32_t* flags, const int32_t* image_index, int n,
                                 double merge_iou, int device, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Detections into tracks (csrc/track_assign.hip): what a caller's detector found, as a padded buffer of boxes and a count on the
 * device, against the tracker's slots. ONE launch, no value is read on the host: detections are matched to live slots, unmatched
 * ones get a free slot, live slots the detector has not confirmed for a while are retired, and the assignment is reported. Still no
 * detector and no appearance. Held word for word to its numpy statement (boxes.assign_detections); built with -ffp-contract=off.
 *
 * dad3d_track_assign_detections  DEVICE pointers; all boxes int32 (x, y, w, h); every sum and product of coordinates in int64.
 *   Slot state, read and written in place:
 *     boxes           int32 [n][4]
 *     flags           int32 [n]: DAD3D_TRACK_FLAG_*
 *     image_index     int32 [n]: the frame of each slot
 *     misses          int32 [n] or NULL: the consecutive calls in which a slot was searched for and not confirmed
 *   Detections, read only:
 *     det_boxes       int32 [m][4]
 *     det_index       int32 [m]: the frame of each detection
 *     det_count       one int32 or NULL: count = m if NULL, else *det_count clamped to [0, m]; the rest is padding
 *     frame_searched  int32 [n_frames] or NULL: non-zero where the detector looked; NULL: everywhere
 *   Written in full: assign int32 [m], det_flags int32 [m] (DAD3D_ASSIGN_FLAG_*), spawned int32 [n].
 *   The rule, in this order:
 *     1. A slot is LIVE if flags == 0 and w > 0 and h > 0, as it stands at entry; every other slot is FREE.
 *     2. A detection k >= count is padding: assign -1, DAD3D_ASSIGN_FLAG_PADDING. One with w <= 0, h <= 0 or det_index outside
 *        [0, n_frames) is invalid: assign -1, DAD3D_ASSIGN_FLAG_INVALID.
 *     3. A pair (valid detection d, live slot s) PASSES if both are in the same frame and
 *            inter > 0  and  double(inter) >= match_iou * double(union)
 *        with inter and union as in dad3d_track_suppress_duplicates: one rounded product, no division.
 *     4. One-to-one, greedy, best IoU first: the passing pairs sorted by the exact ratio inter / union, descending (ratios are
 *        compared as the 128-bit products inter_a * union_b and inter_b * union_a), ties by the lower detection, then the lower
 *        slot; walking that list, a pair is taken if neither its detection nor its slot is taken. Best-first, not "the first slot
 *        that passes", which swaps the identities of two neighbouring heads whose boxes overlap.
 *     5. A taken pair: assign[d] = s, det_flags[d] = 0, misses[s] = 0; with refresh the slot's box becomes the detection's.
 *     6. An unmatched valid detection that passes with ANY live slot, matched or not: assign -1, DAD3D_ASSIGN_FLAG_COVERED. It
 *        spawns nothing: its head has a track.
 *     7. The other unmatched valid detections are spawn candidates, in detection order; the r-th takes the r-th slot that was free
 *        at entry, in slot order: the slot gets the detection's box and frame, flags 0, misses 0, spawned 1; the detection
 *        assign = slot and DAD3D_ASSIGN_FLAG_SPAWNED. Candidates beyond the free slots: assign -1, DAD3D_ASSIGN_FLAG_FULL. Two
 *        unmatched detections that overlap each other both spawn: that is the detector's own NMS to prevent, and
 *        dad3d_track_suppress_duplicates takes what is left.
 *     8. A slot that was live at entry, is unmatched, and whose frame was searched (frame_searched is NULL, or image_index is in
 *        [0, n_frames) and its word is non-zero) gets misses = min(misses + 1, 2^30). If max_misses >= 0 and the new count exceeds
 *        it, the slot is retired: flags = DAD3D_TRACK_FLAG_RETIRED, box (0, 0, 0, 0); it is free from the next call on, and until
 *        then an ordinary lost slot. A live unmatched slot whose frame was not searched is untouched. Without misses (NULL) nothing
 *        is counted and nothing retires.
 *     9. spawned[s] = 0 for every slot that did not spawn.
 *   No other word is written. A matched slot is the same head: nothing else of it changes.
 *   n <= DAD3D_TRACK_MAX_SLOTS and m <= DAD3D_TRACK_MAX_DETECTIONS: one workgroup holds the pass bits in LDS. The allocation is
 *   static, 160 072 bytes of the CU's 160 KiB whatever n and m are: 1024^2 / 8 bytes of pass bits, 16 KiB of slot boxes, 4 KiB of
 *   slot frames, two lists of 1024 ints, 64 words of free masks, 16 of scan scratch and 2 round words. The detections are not staged.
 *   DAD3D_E_INVALID before any launch: match_iou not finite or outside (0, 1]; n or m negative or beyond its cap; n_frames < 1;
 *   refresh not 0 or 1; max_misses >= 0 with a null misses and n > 0; a null boxes, flags, image_index or spawned with n > 0; a null
 *   det_boxes, det_index, assign or det_flags with m > 0. n == 0 is valid (every detection ends padding, invalid or FULL), m == 0
 *   is valid (only step 8 runs and spawned is zeroed), both 0 launch nothing. */
#define DAD3D_TRACK_MAX_DETECTIONS 1024
/* Parenthesised as DAD3D_TRACK_FLAG_DUPLICATE is: set by dad3d_track_assign_detections alone. */
#define DAD3D_TRACK_FLAG_RETIRED (0x40)
#define DAD3D_ASSIGN_FLAG_PADDING 0x1
#define DAD3D_ASSIGN_FLAG_INVALID 0x2
#define DAD3D_ASSIGN_FLAG_COVERED 0x4
#define DAD3D_ASSIGN_FLAG_SPAWNED 0x8
#define DAD3D_ASSIGN_FLAG_FULL 0x10
DAD3D_EXPORT dad3d_status dad3d_track_assign_detections(int32_t* boxes, int32_t* flags, int32_t* image_index, int32_t* misses /* or NULL */,
                                 int n, const int32_t* det_boxes, const int32_t* det_index, const int32_t* det_count /* or NULL */, int m,
                                 const int32_t* frame_searched /* or NULL */, int n_frames, double match_iou, int refresh, int max_misses,
                                 int32_t* assign, int32_t* det_flags, int32_t* spawned, int device, void* stream);

/* Single-image HOST entry points with the argument lists of Sim3DR/lib/rasterize.h:84-100 (`bool` spelled
 * `int` for C). libdad3d_hip.so additionally exports the C++-linkage symbols `_get_tri_normal`,
 * `_get_ver_normal`, `_get_normal`, `_rasterize_triangles`, `_rasterize` with the reference's exact
 * prototypes (csrc/sim3dr_compat.cpp), so Sim3DR/lib/rasterize.pyx links against it unchanged (see
 * INTEGRATION.md). They stage through the GPU synchronously on device $DAD3D_DEVICE (default 0); the
 * vertex count the reference API omits is derived from the triangle list. The reference signatures
 * return void: failures are reported through dad3d_last_error() and leave the outputs untouched. */
DAD3D_EXPORT void dad3d_sim3dr_get_tri_normal(float* tri_normal, float* vertices, int* triangles, int ntri, int norm_flg);
DAD3D_EXPORT void dad3d_sim3dr_get_ver_normal(float* ver_normal, float* tri_normal, int* triangles, int nver, int ntri);
DAD3D_EXPORT void dad3d_sim3dr_get_normal(float* ver_normal, float* vertices, int* triangles, int nver, int ntri);
DAD3D_EXPORT void dad3d_sim3dr_rasterize_triangles(float* vertices, int* triangles, float* depth_buffer, int* triangle_buffer,
                                      float* barycentric_weight, int ntri, int h, int w);
DAD3D_EXPORT void dad3d_sim3dr_rasterize(unsigned char* image, float* vertices, int* triangles, float* colors,
                            float* depth_buffer, int ntri, int h, int w, int c, float alpha, int reverse);

#ifdef __cplusplus
}
#endif
#endif /* DAD3D_H_ */
