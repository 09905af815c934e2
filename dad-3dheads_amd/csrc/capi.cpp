// C ABI, core: the error string, version and device queries, and the FLAME handle with its decode dispatch. The rest of include/dad3d.h
// lives in capi_render.cpp (mesh, UV map, overlays), capi_files.cpp (text and codecs), capi_batch.cpp (stateless tensor calls), sim3dr_compat.cpp.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>

#include "capi_checks.hpp"
#include "flame_plan.hpp"

namespace dad3d {

static thread_local std::string g_last_error;

void set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

}  // namespace dad3d

using namespace dad3d;

static_assert(plan::kJoints == kNumJoints && plan::kTileVerts == kTileVerts && plan::kTileCols == kTileCols &&
                  plan::kPipeTileVerts == kPipeTileVerts && plan::kPipeKGroups == kPipeKGroups,
              "flame_plan.hpp: not the tile geometry of common.hpp");

// Read-only model constants on the device, shared by a handle and its forks (dad3d_flame_fork). A landmark sub-model keeps its pipelined
// pack in one of these too (d_bpack_pipe, n_tiles_pipe, split_b_scale and the fp16 planes only).
struct FlameConsts {
    DeviceArray<float> d_bpack, d_jdirs, d_j0, d_w8;
    DeviceArray<float> d_bpack_pipe;  // basis of the 20-vertex tiles + jaw-joint columns (flame_decode_pipe.hip); empty: model not covered
    float split_b_scale = 1.0f;       // DAD3D_KERNEL_SPLIT_F16: the power of two its entries are multiplied by in front of their fp16 split
    DeviceArray<float> d_bpack_f16;   // ... and the pack split into its two fp16 planes, built by the first decode in that form (ensure_basis_f16)
    std::mutex f16_mu;
    int n_tiles_pipe = 0;
    DeviceArray<float> d_gpack;  // basis^T in MFMA fragment order for dad3d_flame_grad_inputs: built by the first training forward
    std::mutex gpack_mutex;
};

// A landmark list on the device. Immutable once built -- dad3d_flame_set_landmarks builds a new one -- except for the sub-model's fp16
// planes (built under their mutex), so a handle and its forks share it until one of them installs another list.
struct LandmarkList {
    int n = 0;
    DeviceArray<int> d_head, d_next;  // [V][2] {first slot of the vertex, the slot after it}, [n] the slot after each slot
    DeviceArray<float4> d_vtab;  // [V] {W, w_jaw, first landmark slot, slot chained after it}: the pipelined kernel's; empty when it does not cover the model
    // Landmark-only launches on the pipelined and split kernels (SURVEY 7.1 "landmark-only fast path"; BASELINE configs[3]'s per-GPU work):
    // the SUB-MODEL of the distinct vertices the list names (445 of 5023: 23 tiles instead of 252). Same per-vertex arithmetic, ~11x less
    // of it. Its slot chains are the list's own (d_next): renumbering the vertices does not change which slot follows which.
    std::unique_ptr<FlameConsts> sub;  // its pipelined pack (plan::landmark_sub); null: no sub-model
    int sub_verts = 0;
    DeviceArray<float4> d_sub_vtab;  // [sub_verts] the rows of d_vtab of its vertices
};

// What a fork copies from its parent: the model's dimensions and parameter layout
struct FlameShape {
    int device = 0;
    int n_verts = 0, n_betas = 0;
    ParamLayout lay{};
    int parents[kNumJoints]{};
    int n_pose_feats = 0, pose_feat_first = 0;
    int kgroups = 0, ksteps = 0;
    int n_tiles = 0, n_tiles_pad8 = 0;
    int max_shape = 300;
    float image_size = 256.f;
};

struct dad3d_flame : FlameShape {
    std::shared_ptr<FlameConsts> c;     // shared with forks
    std::shared_ptr<LandmarkList> lmk;  // shared with forks until either calls dad3d_flame_set_landmarks; never null
    int kernel_choice = -1;    // dad3d_flame_select_kernel; -1 = the process default (DAD3D_DECODE_KERNEL)
    // ---- per handle
    DeviceScratch d_bwd_partials;   // [batch][kBackwardMaxSplit][72] scratch of dad3d_flame_decode_backward
    DeviceScratch d_grad_partials;  // [slices][padded batch][kGradRows] scratch of dad3d_flame_grad_inputs
    DeviceScratch d_imgc;           // [blocks of kBlockImages images][kImgConsts]
    DeviceArray<unsigned> d_sync;   // [0] arrival counter, [1] time-out counter; [4], [5], [last]: device-epoch launches
    unsigned arrive_total = 0;      // host mirror of sync[0] after the last launch
    bool profiling = false;
    unsigned long long* d_trace = nullptr;  // diagnostics (dad3d_flame_debug_trace): the caller's buffer, borrowed
    uint64_t trace_capacity = 0;
    DeviceScratch d_split_a;  // scratch of the split kernels (flame_decode_split.hip): params rows as planes + per-image constants
    std::vector<DeviceArray<char>> split_retired;  // smaller scratches it outgrew: kept until destroy -- a graph captured at a smaller batch still points there
    hipEvent_t ev_first = nullptr, ev_last = nullptr;  // bracket a run of back-to-back launches
    int prof_launches = 0;
    ~dad3d_flame() {
        DeviceGuard guard(device);
        if (ev_first) (void)hipEventDestroy(ev_first);
        if (ev_last) (void)hipEventDestroy(ev_last);
    }
};

// Process-wide default of dad3d_flame_select_kernel: DAD3D_DECODE_KERNEL=v1 forces the two-role kernel of rounds 1-3 (A/B timing).
static int decode_kernel_choice() {
    static const int choice = [] {
        const char* e = getenv("DAD3D_DECODE_KERNEL");
        if (!e) return 0;
        if (e[0] == 'v' && e[1] == '1') return DAD3D_KERNEL_TWO_ROLE;
        if (std::strcmp(e, "split") == 0) return DAD3D_KERNEL_SPLIT_BF16;
        if (std::strcmp(e, "split_f16") == 0) return DAD3D_KERNEL_SPLIT_F16;
        return std::strcmp(e, "force_pipe") == 0 ? DAD3D_KERNEL_PIPELINED : DAD3D_KERNEL_AUTO;  // "pipe" = the default
    }();
    return choice;
}
// DAD3D_DECODE_KERNEL=halfblocks (read once per process, like the choice above): whole-mesh launches of 33..64 rows stay on the pipelined
// kernel's two half-blocks instead of flame_decode_head.hip's 48 + 16 (A/B timing; the bits are the same: tests/test_gpu_decode_head.py).
static bool decode_halfblocks_forced() {
    static const bool forced = [] {
        const char* e = getenv("DAD3D_DECODE_KERNEL");
        return e && std::strcmp(e, "halfblocks") == 0;
    }();
    return forced;
}

static int grad_chunks(const dad3d_flame* h) { return (h->n_verts * 3 + kGradChunk - 1) / kGradChunk; }

// basis^T pack (once per model, shared by forks) and the split-K scratch for `batch` images (per handle)
static dad3d_status grad_inputs_prepare(dad3d_flame* h, int batch, hipStream_t s) {
    const int pad = (batch + kBlockImages - 1) / kBlockImages * kBlockImages;
    const int per_slice = grad_chunks_per_slice(pad);
    const size_t rows = (size_t)((grad_chunks(h) + per_slice - 1) / per_slice) * pad;
    bool need_pack;
    {   // forks share the pack: the pointer is only ever looked at under its mutex
        std::lock_guard<std::mutex> lock(h->c->gpack_mutex);
        need_pack = !h->c->d_gpack;
    }
    const size_t scratch_bytes = rows * kGradRows * sizeof(float);
    const bool need_scratch = scratch_bytes > h->d_grad_partials.capacity();
    if (!need_pack && !need_scratch) return DAD3D_OK;
    DAD3D_REQUIRE(!stream_is_capturing(s),
                  "the first training step of a handle (and the first at a larger batch) allocates: run it once before capturing a graph");
    DAD3D_REQUIRE(h->n_betas + 36 <= kGradRows, "dad3d_flame_grad_inputs: %d inputs exceed %d", h->n_betas + 36, kGradRows);
    if (need_pack) {
        std::lock_guard<std::mutex> lock(h->c->gpack_mutex);
        if (!h->c->d_gpack) {
            DeviceArray<float> pack;
            if (dad3d_status st = pack.allocate(grad_pack_floats(grad_chunks(h)))) return st;
            GradPackArgs pa{h->c->d_bpack.get(), pack.get(), h->kgroups, h->n_betas, h->n_pose_feats, h->pose_feat_first, h->n_betas + 36,
                            h->n_verts * 3, grad_chunks(h)};
            dad3d_status st = launch_grad_pack(pa, nullptr);
            if (st == DAD3D_OK && hipDeviceSynchronize() != hipSuccess) st = DAD3D_E_HIP;
            if (st) {
                set_error("building the basis^T pack failed");
                return st;
            }
            h->c->d_gpack = std::move(pack);
        }
    }
    return h->d_grad_partials.grow(scratch_bytes);
}

static size_t imgc_bytes(int nbb) { return (size_t)nbb * kBlockImages * kImgConsts * sizeof(float); }

static bool landmark_subset_enabled() {
    static const bool on = [] {
        const char* e = getenv("DAD3D_LANDMARK_SUBSET");  // =0: landmark-only launches decode the whole mesh like any other (A/B timing)
        return !(e && e[0] == '0');
    }();
    return on;
}

// A new landmark list for h's model: the per-vertex slot chains, the pipelined kernel's per-vertex table (skinning weights from the model,
// landmark slots from the list) and the sub-model of the vertices the list names (flame_plan.hpp), the last two for models the pipelined
// kernel covers only. The model's tables are read back from the device: the handle keeps no host copy of 27 MB.
static dad3d_status build_landmarks(const dad3d_flame* h, const int64_t* idx, int n, std::shared_ptr<LandmarkList>* out) {
    const int V = h->n_verts;
    std::vector<int> head2, next;
    plan::landmark_chains(idx, n, V, &head2, &next);
    auto L = std::make_shared<LandmarkList>();
    L->n = n;
    dad3d_status st;
    if ((st = L->d_head.upload(head2)) || (st = L->d_next.upload(next))) return st;
    if (h->c->d_bpack_pipe) {
        std::vector<float> w8((size_t)V * 8);
        DAD3D_HIP_TRY(hipMemcpy(w8.data(), h->c->d_w8.get(), w8.size() * sizeof(float), hipMemcpyDeviceToHost));
        const std::vector<plan::Float4> vtab = plan::vertex_table(w8, head2, V);
        if ((st = L->d_vtab.upload(vtab))) return st;
        const std::vector<int> uniq = landmark_subset_enabled() ? plan::landmark_sub_vertices(idx, n, V) : std::vector<int>();
        if (!uniq.empty()) {
            std::vector<float> full(plan::pack_floats(h->c->n_tiles_pipe, kPipeKGroups));
            DAD3D_HIP_TRY(hipMemcpy(full.data(), h->c->d_bpack_pipe.get(), full.size() * sizeof(float), hipMemcpyDeviceToHost));
            const plan::LandmarkSub sub = plan::landmark_sub(uniq, full, vtab);
            L->sub.reset(new FlameConsts);
            L->sub->n_tiles_pipe = sub.n_tiles;
            L->sub->split_b_scale = h->c->split_b_scale;  // a subset of the model's entries: its scale holds
            L->sub_verts = (int)uniq.size();
            if ((st = L->sub->d_bpack_pipe.upload(sub.pack)) || (st = L->d_sub_vtab.upload(sub.vtab))) return st;
        }
    }
    *out = std::move(L);
    return DAD3D_OK;
}

extern "C" {

const char* dad3d_last_error(void) { return g_last_error.c_str(); }
void dad3d_clear_error(void) { g_last_error.clear(); }
int dad3d_version(void) { return DAD3D_VERSION; }
const char* dad3d_build_info(void) {
    static const std::string info = [] {
        int rt = 0, drv = 0;
        (void)hipRuntimeGetVersion(&rt);
        (void)hipDriverGetVersion(&drv);
        char buf[384];
        snprintf(buf, sizeof buf, "built: clang %s, HIP headers %d.%d.%d; running: HIP runtime %d, driver %d", __clang_version__, HIP_VERSION_MAJOR,
                 HIP_VERSION_MINOR, HIP_VERSION_PATCH, rt, drv);
        return std::string(buf);
    }();
    return info.c_str();
}
int dad3d_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

dad3d_status dad3d_flame_create(const dad3d_flame_model* m, const dad3d_flame_consts* c, float image_size, int device,
                                dad3d_flame** out) {
    DAD3D_REQUIRE(m && c && out, "dad3d_flame_create: null argument");
    *out = nullptr;
    DAD3D_REQUIRE(m->v_template && m->shapedirs && m->posedirs && m->j_regressor && m->parents && m->lbs_weights,
                  "dad3d_flame_create: null model array");
    DAD3D_REQUIRE(m->n_joints == kNumJoints, "FLAME has %d joints, got %d", kNumJoints, m->n_joints);
    DAD3D_REQUIRE(m->n_verts > 0 && m->n_betas == 400, "expected n_betas == 400 (MAX_SHAPE+MAX_EXPRESSION), got %d",
                  m->n_betas);
    // `assert v.shape[-1] == 6` (model/utils.py:93); translation/scale widths are fixed by head_mesh.py:39-42
    DAD3D_REQUIRE(c->rotation == 6 && c->translation == 3 && c->scale == 1,
                  "consts: rotation/translation/scale must be 6/3/1");
    DAD3D_REQUIRE(c->shape >= 0 && c->shape <= 300 && c->expression >= 0 && c->expression <= 100,
                  "consts: shape <= 300 and expression <= 100 required");
    DAD3D_REQUIRE((c->jaw == 0 || c->jaw == 3) && (c->neck == 0 || c->neck == 3) && (c->eyeballs == 0 || c->eyeballs == 6),
                  "consts: jaw/neck in {0,3}, eyeballs in {0,6}");
    for (int j = 1; j < kNumJoints; ++j)
        DAD3D_REQUIRE(m->parents[j] >= 0 && m->parents[j] < j, "parents[%d] = %d is not a valid kinematic tree", j,
                      m->parents[j]);
    DAD3D_SELECT_DEVICE(device);

    const plan::FlameDims<ParamLayout> d = plan::flame_dims<ParamLayout>(*m, *c);
    DAD3D_REQUIRE(d.kgroups == 26 || d.kgroups == 28, "unexpected basis depth %d", d.k_used);
    std::unique_ptr<dad3d_flame> h(new dad3d_flame);
    h->device = device;
    h->n_verts = m->n_verts;
    h->n_betas = m->n_betas;
    h->image_size = image_size;
    h->lay = d.lay;
    for (int j = 0; j < kNumJoints; ++j) h->parents[j] = (j == 0) ? -1 : m->parents[j];
    h->n_pose_feats = d.n_pose_feats;
    h->pose_feat_first = d.pose_feat_first;
    h->kgroups = d.kgroups;
    h->ksteps = d.kgroups * 4;
    h->n_tiles = d.n_tiles;
    h->n_tiles_pad8 = (d.n_tiles + 7) / 8 * 8;

    std::vector<float> j0, jdirs;
    plan::joint_regressors(*m, &j0, &jdirs);
    h->c = std::make_shared<FlameConsts>();
    h->c->n_tiles_pipe = d.n_tiles_pipe;
    dad3d_status st;
    if (d.pipe_ok) {
        const std::vector<float> bpack_pipe = plan::basis_pack_pipe(*m, d, j0, jdirs);
        h->c->split_b_scale = split_basis_scale(plan::max_abs(bpack_pipe));
        if ((st = h->c->d_bpack_pipe.upload(bpack_pipe))) return st;
    }
    if ((st = h->c->d_bpack.upload(plan::basis_pack(*m, d))) || (st = h->c->d_jdirs.upload(jdirs)) || (st = h->c->d_j0.upload(j0)) ||
        (st = h->c->d_w8.upload(plan::weights8(*m))) || (st = h->d_sync.upload(std::vector<unsigned>(kSyncWords, 0u))) ||
        (st = h->d_imgc.allocate(imgc_bytes(1))) || (st = build_landmarks(h.get(), nullptr, 0, &h->lmk)))
        return st;
    *out = h.release();
    return DAD3D_OK;
}

void dad3d_flame_destroy(dad3d_flame* h) { delete h; }

dad3d_status dad3d_flame_fork(dad3d_flame* parent, dad3d_flame** out) {
    DAD3D_REQUIRE(parent && out, "dad3d_flame_fork: bad argument");
    *out = nullptr;
    DAD3D_SELECT_DEVICE(parent->device);
    std::unique_ptr<dad3d_flame> h(new dad3d_flame);
    static_cast<FlameShape&>(*h) = *parent;
    h->c = parent->c;
    h->lmk = parent->lmk;
    h->kernel_choice = parent->kernel_choice;
    dad3d_status st;
    if ((st = h->d_sync.upload(std::vector<unsigned>(kSyncWords, 0u))) || (st = h->d_imgc.allocate(imgc_bytes(1)))) return st;
    *out = h.release();
    return DAD3D_OK;
}

int dad3d_flame_num_params(const dad3d_flame* h) { return h ? h->lay.n_params : -1; }
int dad3d_flame_num_verts(const dad3d_flame* h) { return h ? h->n_verts : -1; }
int dad3d_flame_num_landmarks(const dad3d_flame* h) { return h ? h->lmk->n : -1; }
int dad3d_flame_num_landmark_vertices(const dad3d_flame* h) { return h ? h->lmk->sub_verts : 0; }

dad3d_status dad3d_flame_set_landmarks(dad3d_flame* h, const int64_t* idx, int n) {
    DAD3D_REQUIRE(h && n >= 0 && (idx || n == 0), "dad3d_flame_set_landmarks: bad argument");
    for (int s = 0; s < n; ++s)
        DAD3D_REQUIRE(idx[s] >= 0 && idx[s] < h->n_verts, "landmark index %lld out of range [0,%d)", (long long)idx[s], h->n_verts);
    DeviceGuard guard(h->device);
    std::shared_ptr<LandmarkList> list;
    dad3d_status st = build_landmarks(h, idx, n, &list);
    if (st) return st;  // the handle keeps its old list
    DAD3D_HIP_TRY(hipDeviceSynchronize());  // no decode of this handle may still be walking the old list when it is freed
    h->lmk = std::move(list);
    return DAD3D_OK;
}

// entries of a dad3d_flame_debug_trace buffer one launch stamps (the two kernels lay it out differently, include/dad3d.h)
static uint64_t trace_entries_two_role(const dad3d_flame* h, int batch) {
    const uint64_t nbb = (batch + kBlockImages - 1) / kBlockImages, pose_blocks = ((uint64_t)(batch + 3) / 4 + 7) / 8 * 8;
    return ((uint64_t)h->n_tiles_pad8 * nbb * 8 + pose_blocks * 4) * 32;
}
static uint64_t trace_entries_pipe(const dad3d_flame* h) { return (uint64_t)h->c->n_tiles_pipe * 8 * 32; }

// DAD3D_KERNEL_SPLIT_F16: the model's basis pack as two fp16 planes, built on the device by the first decode in that form (26.7 MB for the whole
// mesh: not spent on models that never use the form), shared by forks. The builder waits for its kernel before publishing the pointer: a fork
// on another stream must not read a pack still being written.
static dad3d_status ensure_basis_f16(FlameConsts* c, hipStream_t s) {
    std::lock_guard<std::mutex> lock(c->f16_mu);
    if (c->d_bpack_f16) return DAD3D_OK;
    DAD3D_REQUIRE(!stream_is_capturing(s), "the first fp16-split decode of a model builds its basis planes: run it once before capturing a graph");
    const size_t floats = plan::pack_floats(c->n_tiles_pipe, kPipeKGroups);
    DeviceArray<float> d;
    if (dad3d_status st = d.allocate(floats)) return st;
    dad3d_status st = launch_split_basis_f16(c->d_bpack_pipe.get(), d.get(), c->n_tiles_pipe, c->split_b_scale, s);
    if (st == DAD3D_OK && hipStreamSynchronize(s) != hipSuccess) {
        set_error("ensure_basis_f16: hipStreamSynchronize failed");
        st = DAD3D_E_HIP;
    }
    if (st) return st;
    c->d_bpack_f16 = std::move(d);
    return DAD3D_OK;
}

// Scratch of the split kernels (pre-pass -> tile kernel): n_phase blocks of kSplitBlockBytes, grown on demand -- never inside a capture.
static dad3d_status ensure_split_scratch(dad3d_flame* h, int n_phase, hipStream_t s) {
    const size_t bytes = (size_t)n_phase * kSplitBlockBytes;
    if (bytes <= h->d_split_a.capacity()) return DAD3D_OK;
    DAD3D_REQUIRE(!stream_is_capturing(s),
                  "the first split-kernel decode of a handle (and the first at a larger batch) allocates: run it once before capturing a graph");
    if (h->d_split_a.get()) h->split_retired.push_back(h->d_split_a.retire());  // (2.6 KB per image: never worth a dangling pointer in somebody's graph)
    if (dad3d_status st = h->d_split_a.allocate(bytes)) return st;
    // (the padding is copied into LDS, never read.) On the LAUNCH's stream: hipMemset is ordered on the null stream only, and a
    // non-blocking stream's pre-pass overtook it -- zero planes under the first launch of a fork (found by the two-streams test)
    DAD3D_HIP_TRY(hipMemsetAsync(h->d_split_a.get(), 0, bytes, s));
    return DAD3D_OK;
}

// The kernel a decode launch of h takes: DAD3D_KERNEL_TWO_ROLE, _PIPELINED, _SPLIT_BF16 or _SPLIT_F16; -1 (error set) when the pinned one
// does not cover it. The pipelined single-role kernel (flame_decode_pipe.hip) takes EVERY inference launch it covers (jaw-only model, the
// dad_3dnet.yaml params layout, no DAD3D_ZERO_ROTATION / DAD3D_COMPAT_CROSS_B3, outputs below 2 GB); the two-role kernel of rounds 1-3 keeps
// the rest and the training forward. Round 4 also sent 1..3 and 33..40 images to the two-role kernel for 0.3-0.6 us measured on one box
// (profiles/r04_ab_decode.txt: 6.8 against 7.4 us at B = 1, 11.63 against 11.90 at 33); that crossover table is gone -- inside box-to-box
// spread at 33..40, irrelevant next to a 4 ms network at B = 1, and it made the jaw sine/cosine (flame_math.hpp against OCML) depend on the
// batch size. DAD3D_DECODE_KERNEL=v1 / dad3d_flame_select_kernel remain the escape hatch. The split forms are never chosen automatically.
static int resolve_kernel(const dad3d_flame* h, int pinned, int batch, unsigned flags, bool posed) {
    const bool pipe_covers = h->c->d_bpack_pipe && !posed && !(flags & (DAD3D_COMPAT_CROSS_B3 | DAD3D_ZERO_ROTATION)) &&
                             (size_t)batch * h->n_verts * 12 < ((size_t)1 << 31) && (size_t)batch * std::max(h->lmk->n, 1) * 8 < ((size_t)1 << 31);
    if (pinned == DAD3D_KERNEL_TWO_ROLE || (pinned == DAD3D_KERNEL_AUTO && !pipe_covers)) return DAD3D_KERNEL_TWO_ROLE;
    if (pipe_covers) return pinned == DAD3D_KERNEL_AUTO ? DAD3D_KERNEL_PIPELINED : pinned;
    set_error("dad3d_flame_decode: the %s kernel does not cover this launch (model, flags or output size)",
              pinned == DAD3D_KERNEL_PIPELINED ? "pipelined" : "split");
    return -1;
}

static dad3d_status decode_impl(dad3d_flame* h, float* params, int batch, unsigned flags, float* verts3d, float* proj,
                                float* lmk_xy, int32_t* lmk_px, float* posed, void* stream) {
    DAD3D_REQUIRE(h, "dad3d_flame_decode: null handle");
    DAD3D_REQUIRE(batch >= 0, "dad3d_flame_decode: negative batch");
    if (batch == 0) return DAD3D_OK;
    DAD3D_REQUIRE(params, "dad3d_flame_decode: null params");  // `assert tensor_3dmm.ndim == 2` lives in the binding
    DAD3D_REQUIRE(!((flags & DAD3D_FLIP_Z) && (flags & DAD3D_TO_2D)), "DAD3D_FLIP_Z needs a 3-component projection");
    // the batch-axis cross product exists in the inference forward only: its backward pass (flame_backward.hip) differentiates
    // the per-image Gram-Schmidt rotation, so a training forward with the flag would get gradients of another function
    DAD3D_REQUIRE(!(posed && (flags & DAD3D_COMPAT_CROSS_B3)), "DAD3D_COMPAT_CROSS_B3 is inference-only (dad3d_flame_decode_posed refuses it)");
    DeviceGuard guard(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int pinned = h->kernel_choice >= 0 ? h->kernel_choice : decode_kernel_choice();
    const int kernel = resolve_kernel(h, pinned, batch, flags, posed != nullptr);
    if (kernel < 0) return DAD3D_E_UNSUPPORTED;
    const LandmarkList& L = *h->lmk;
    const int n_lmk = (lmk_xy || lmk_px) ? L.n : 0;

    // Geometry of the pipelined and split kernels. Landmark outputs only (BASELINE configs[3]'s per-GPU work;
    // sharding.ShardedLandmarkDecoder): the sub-model of the listed vertices, 23 column tiles instead of 252 with the batch cut into chunks
    // across workgroups (pipe_chunking / split_chunking) -- same kernel, same bits as the landmark rows of a full-output launch -- unless the
    // caller pinned the pipelined kernel or traces the launch (A/B timing, diagnostics: the whole mesh then). The launch covers no posed
    // output and no DAD3D_COMPAT_CROSS_B3 here: resolve_kernel sent those to the two-role kernel, which always decodes the whole mesh.
    const bool on_sub = L.sub && !verts3d && !proj && n_lmk && !h->d_trace && pinned != DAD3D_KERNEL_PIPELINED;
    FlameConsts* c = on_sub ? L.sub.get() : h->c.get();
    const float4* vtab = on_sub ? L.d_sub_vtab.get() : L.d_vtab.get();
    const int n_verts = on_sub ? L.sub_verts : h->n_verts;

    dad3d_status st;
    if (kernel == DAD3D_KERNEL_SPLIT_BF16 || kernel == DAD3D_KERNEL_SPLIT_F16) {
        // The gated exact-product splits (flame_decode_split.hip; bf16 x 3 planes x 6 products, or fp16 x 2 planes x 3 products): same
        // model coverage, same pack, same epilogue as the pipelined kernel; the contraction differs (and is more accurate than the
        // fp32 MFMA chain in both forms: profiles/r06_split_error.md). Two launches, the handle's own scratch in between.
        DAD3D_REQUIRE(!h->d_trace, "dad3d_flame_decode: the split kernels have no trace stamps");
        const int n_phase = (batch + kSplitRows - 1) / kSplitRows;
        st = ensure_split_scratch(h, n_phase, s);
        if (!st && kernel == DAD3D_KERNEL_SPLIT_F16) st = ensure_basis_f16(c, s);
        // (and the sub-model's, so that a landmark-only launch captured behind a full-output warm-up builds nothing)
        if (!st && kernel == DAD3D_KERNEL_SPLIT_F16 && L.sub) st = ensure_basis_f16(L.sub.get(), s);
        if (st) return st;
        SplitArgs sa{};
        sa.params = params;
        sa.bpack = c->d_bpack_pipe.get();
        sa.bpack_f16 = c->d_bpack_f16.get();
        sa.vtab = vtab;
        sa.lmk_next = L.d_next.get();
        sa.verts3d = verts3d;
        sa.proj = proj;
        sa.lmk_xy = lmk_xy;
        sa.lmk_px = lmk_px;
        sa.aplanes = static_cast<char*>(h->d_split_a.get());
        sa.b_scale = c->split_b_scale;
        sa.n_params = h->lay.n_params;
        sa.batch = batch;
        sa.n_phase = n_phase;
        sa.n_tiles = c->n_tiles_pipe;
        split_chunking(sa.n_tiles, n_phase, &sa.n_chunks, &sa.phases_per_chunk);
        sa.n_verts = n_verts;
        sa.n_lmk = n_lmk;
        sa.image_size = h->image_size;
        sa.flags = flags & 0xFFu;
        st = launch_flame_decode_split(sa, kernel, s);
    } else if (kernel == DAD3D_KERNEL_PIPELINED) {
        DAD3D_REQUIRE(!h->d_trace || h->trace_capacity >= trace_entries_pipe(h), "dad3d_flame_decode: the trace buffer holds %llu entries, "
                      "this launch stamps %llu (dad3d_flame_debug_trace_entries)", (unsigned long long)h->trace_capacity,
                      (unsigned long long)trace_entries_pipe(h));
        PipeArgs pa{};
        pa.params = params;
        pa.bpack = c->d_bpack_pipe.get();
        pa.vtab = vtab;
        pa.lmk_next = L.d_next.get();
        pa.verts3d = verts3d;
        pa.proj = proj;
        pa.lmk_xy = lmk_xy;
        pa.lmk_px = lmk_px;
        pa.trace = h->d_trace;
        pa.n_params = h->lay.n_params;
        pa.batch = batch;
        pa.n_half = (batch + kPipeHalf - 1) / kPipeHalf;
        pa.n_tiles = c->n_tiles_pipe;
        pa.n_verts = n_verts;
        pa.n_lmk = n_lmk;
        pa.image_size = h->image_size;
        pa.flags = flags & 0xFFu;
        pa.n_chunks = 1;
        if (!h->d_trace && (!proj || (flags & DAD3D_TO_2D))) pipe_chunking(pa.n_tiles, pa.n_half, &pa.chunk_half, &pa.n_chunks, &pa.wg_per_xcd);
        // 33..64 rows of the whole mesh with a vertex output: 48 rows under the basis stream, 16 behind it (flame_decode_head.hip; same bits)
        const bool head = pa.chunk_half == 0 && batch > kPipeHalf && batch <= 2 * kPipeHalf && (verts3d || proj) && !decode_halfblocks_forced();
        st = head ? launch_flame_decode_head(pa, s) : launch_flame_decode_pipe(pa, s);
    } else {
        DAD3D_REQUIRE(!h->d_trace || h->trace_capacity >= trace_entries_two_role(h, batch), "dad3d_flame_decode: the trace buffer holds %llu "
                      "entries, this launch stamps %llu (dad3d_flame_debug_trace_entries)", (unsigned long long)h->trace_capacity,
                      (unsigned long long)trace_entries_two_role(h, batch));
        // A training forward: what its backward pass needs exists before any of it can be captured into a graph -- for the batches
        // the host mirror sends to dad3d_flame_grad_inputs (up to DAD3D_GRAD_INPUTS_MAX_BATCH; above it takes the library GEMM and
        // the split-K scratch, tens to hundreds of MB, would never be used) and for models the kernel covers (otherwise the
        // forward must not fail for a backward path that will not be taken: dad3d_flame_grad_inputs reports it when called).
        if (posed && batch <= DAD3D_GRAD_INPUTS_MAX_BATCH && h->n_betas + 36 <= kGradRows && (st = grad_inputs_prepare(h, batch, s))) return st;
        const int nbb = (batch + kBlockImages - 1) / kBlockImages;
        if ((st = h->d_imgc.grow(imgc_bytes(nbb)))) return st;
        DecodeArgs da{};
        da.params = params;
        da.bpack = h->c->d_bpack.get();
        da.jdirs = h->c->d_jdirs.get();
        da.j0 = h->c->d_j0.get();
        da.weights8 = h->c->d_w8.get();
        da.lmk_head = L.d_head.get();
        da.lmk_next = L.d_next.get();
        da.imgc = static_cast<float*>(h->d_imgc.get());
        da.sync = h->d_sync.get();
        da.verts3d = verts3d;
        da.proj = proj;
        da.lmk_xy = lmk_xy;
        da.lmk_px = lmk_px;
        da.posed = posed;
        da.trace = h->d_trace;
        da.lay = h->lay;
        std::copy(h->parents, h->parents + kNumJoints, da.parents);
        da.batch = batch;
        da.nbb = nbb;
        da.n_tiles = h->n_tiles;
        da.n_tiles_pad8 = h->n_tiles_pad8;
        da.n_verts = h->n_verts;
        da.n_lmk = n_lmk;
        da.n_pose_blocks = (batch + 3) / 4;  // one wave per image, four per workgroup
        da.n_pose_blocks_pad8 = (da.n_pose_blocks + 7) / 8 * 8;
        da.n_betas = h->n_betas;
        da.max_shape = h->max_shape;
        da.betas_contiguous = (h->lay.shape_n == 300 && h->lay.expr_n == 100 && h->lay.shape_off == 0 && h->lay.expr_off == 300);
        da.kgroups = h->kgroups;
        // a launch that is being captured into a graph cannot carry a per-launch target: the epoch then lives on the device
        const bool device_epoch = stream_is_capturing(s);
        da.arrive_target = h->arrive_total + (unsigned)da.n_pose_blocks;  // every pose workgroup arrives once per launch
        da.spin_limit = 1u << 20;
#ifdef DAD3D_DIAG_SPIN_ENV  // diagnostics builds only (tools/build_variant.sh): hand-off spin limit from the environment
        if (const char* e = getenv("DAD3D_SPIN_LIMIT")) da.spin_limit = (unsigned)atoi(e);
#endif
        da.image_size = h->image_size;
        da.flags = (flags & 0xFFu) | (device_epoch ? kDeviceEpoch : 0u);
        st = launch_flame_decode(da, s);
        if (!st && !device_epoch) h->arrive_total = da.arrive_target;  // committed only once the launch was accepted
    }
    if (!st && h->profiling) ++h->prof_launches;
    return st;
}

dad3d_status dad3d_flame_decode(dad3d_flame* h, float* params, int batch, unsigned flags, float* verts3d, float* proj,
                                float* lmk_xy, int32_t* lmk_px, void* stream) {
    return decode_impl(h, params, batch, flags, verts3d, proj, lmk_xy, lmk_px, nullptr, stream);
}

dad3d_status dad3d_flame_decode_posed(dad3d_flame* h, float* params, int batch, unsigned flags, float* verts3d, float* proj,
                                      float* posed, void* stream) {
    return decode_impl(h, params, batch, flags, verts3d, proj, nullptr, nullptr, posed, stream);
}

dad3d_status dad3d_flame_decode_host(dad3d_flame* h, float* params, int batch, unsigned flags, float* verts3d,
                                     float* proj, float* lmk_xy, int32_t* lmk_px) {
    DAD3D_REQUIRE(h, "dad3d_flame_decode_host: null handle");
    DAD3D_REQUIRE(batch >= 0, "dad3d_flame_decode_host: negative batch");
    if (batch == 0) return DAD3D_OK;
    DAD3D_REQUIRE(params, "dad3d_flame_decode_host: null params");
    DeviceGuard guard(h->device);
    const size_t B = batch, V = h->n_verts, P = h->lay.n_params, NL = h->lmk->n;
    const size_t pc = (flags & DAD3D_TO_2D) ? 2 : 3;
    const size_t n_par = B * P, n_v = verts3d ? B * V * 3 : 0, n_p = proj ? B * V * pc : 0;
    const size_t n_lx = lmk_xy ? B * NL * 2 : 0, n_lp = lmk_px ? B * NL * 2 : 0;
    DeviceArray<float> d;
    if (dad3d_status st = d.allocate(n_par + n_v + n_p + n_lx + n_lp + 4)) return st;
    float* d_par = d.get();
    float* d_v = n_v ? d_par + n_par : nullptr;
    float* d_p = n_p ? d_par + n_par + n_v : nullptr;
    float* d_lx = n_lx ? d_par + n_par + n_v + n_p : nullptr;
    int32_t* d_lp = n_lp ? reinterpret_cast<int32_t*>(d_par + n_par + n_v + n_p + n_lx) : nullptr;
    dad3d_status st = DAD3D_OK;
    auto fail = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && st == DAD3D_OK) {
            set_error("%s failed: %s", what, hipGetErrorString(e));
            st = DAD3D_E_HIP;
        }
    };
    fail(hipMemcpy(d_par, params, n_par * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy(params)");
    if (!st) st = dad3d_flame_decode(h, d_par, batch, flags, d_v, d_p, d_lx, d_lp, nullptr);
    if (!st) fail(hipDeviceSynchronize(), "hipDeviceSynchronize");
    if (!st && (flags & DAD3D_MUTATE_PARAMS)) fail(hipMemcpy(params, d_par, n_par * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy");
    if (!st && n_v) fail(hipMemcpy(verts3d, d_v, n_v * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy");
    if (!st && n_p) fail(hipMemcpy(proj, d_p, n_p * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy");
    if (!st && n_lx) fail(hipMemcpy(lmk_xy, d_lx, n_lx * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy");
    if (!st && n_lp) fail(hipMemcpy(lmk_px, d_lp, n_lp * sizeof(int32_t), hipMemcpyDeviceToHost), "hipMemcpy");
    return st;
}

dad3d_status dad3d_flame_readjust_params(dad3d_flame* h, float* params, int batch, const float* pads_scale,
                                         float pad_left, float pad_top, float scale, void* stream) {
    DAD3D_REQUIRE(h && batch >= 0, "dad3d_flame_readjust_params: bad argument");
    if (batch == 0) return DAD3D_OK;
    DAD3D_REQUIRE(params, "dad3d_flame_readjust_params: null params");
    DeviceGuard guard(h->device);
    return launch_readjust(params, batch, h->lay, pads_scale, pad_left, pad_top, scale, h->image_size,
                           static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_flame_readjust_params_frame(dad3d_flame* h, float* params, int batch, const double* geometry, void* stream) {
    DAD3D_REQUIRE(h && batch >= 0, "dad3d_flame_readjust_params_frame: bad argument");
    if (batch == 0) return DAD3D_OK;
    DAD3D_REQUIRE(params && geometry, "dad3d_flame_readjust_params_frame: null argument");
    DeviceGuard guard(h->device);
    return launch_readjust_frame(params, batch, h->lay, geometry, h->image_size, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_flame_select_kernel(dad3d_flame* h, int which) {
    DAD3D_REQUIRE(h && which >= DAD3D_KERNEL_AUTO && which <= DAD3D_KERNEL_SPLIT_F16, "dad3d_flame_select_kernel: bad argument");
    h->kernel_choice = which;
    return DAD3D_OK;
}

dad3d_status dad3d_flame_handoff_timeouts(dad3d_flame* h, unsigned* count) {
    DAD3D_REQUIRE(h && count, "null argument");
    DeviceGuard guard(h->device);
    DAD3D_HIP_TRY(hipDeviceSynchronize());
    DAD3D_HIP_TRY(hipMemcpy(count, h->d_sync.get() + 1, sizeof(unsigned), hipMemcpyDeviceToHost));
    return DAD3D_OK;
}

uint64_t dad3d_flame_debug_trace_entries(const dad3d_flame* h, int batch) {
    if (!h || batch <= 0) return 0;
    return std::max(trace_entries_two_role(h, batch), trace_entries_pipe(h));
}

dad3d_status dad3d_flame_debug_trace(dad3d_flame* h, unsigned long long* device_buffer, uint64_t capacity) {
    DAD3D_REQUIRE(h, "null handle");
    h->d_trace = device_buffer;
    h->trace_capacity = device_buffer ? capacity : 0;
    return DAD3D_OK;
}

dad3d_status dad3d_flame_decode_backward(dad3d_flame* h, int batch, unsigned flags, const float* consts, const float* posed,
                                         const float* grad_verts3d, const float* grad_proj, float* grad_posed,
                                         float* grad_consts, void* stream) {
    DAD3D_REQUIRE(h, "dad3d_flame_decode_backward: null handle");
    DAD3D_REQUIRE(batch >= 0, "dad3d_flame_decode_backward: negative batch");
    if (batch == 0) return DAD3D_OK;
    DAD3D_REQUIRE(consts && posed && grad_posed && grad_consts, "dad3d_flame_decode_backward: null argument");
    DAD3D_REQUIRE(grad_verts3d || grad_proj, "dad3d_flame_decode_backward: no upstream gradient");
    DAD3D_REQUIRE(!((flags & DAD3D_FLIP_Z) && (flags & DAD3D_TO_2D)), "DAD3D_FLIP_Z needs a 3-component projection");
    // the batch-axis cross product exists in the inference forward only: its backward pass (flame_backward.hip) differentiates
    // the per-image Gram-Schmidt rotation, so a training forward with the flag would get gradients of another function
    DAD3D_REQUIRE(!(posed && (flags & DAD3D_COMPAT_CROSS_B3)), "DAD3D_COMPAT_CROSS_B3 is inference-only (dad3d_flame_decode_posed refuses it)");
    DeviceGuard guard(h->device);
    BackwardArgs ba{};
    ba.weights8 = h->c->d_w8.get();
    ba.consts = consts;
    ba.posed = posed;
    ba.g_verts3d = grad_verts3d;
    ba.g_proj = grad_proj;
    ba.g_posed = grad_posed;
    ba.g_consts = grad_consts;
    ba.batch = batch;
    ba.n_verts = h->n_verts;
    ba.image_size = h->image_size;
    ba.flags = flags;
    // small batches: split every image over several workgroups (about one per CU), partial sums added in fixed order
    ba.nsplit = std::max(1, std::min(kBackwardMaxSplit, 256 / batch));
    if (ba.nsplit > 1) {
        if (dad3d_status st = h->d_bwd_partials.grow((size_t)batch * kBackwardMaxSplit * kBackwardConsts * sizeof(float))) return st;
        ba.partials = static_cast<float*>(h->d_bwd_partials.get());
    }
    return launch_flame_backward(ba, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_flame_grad_inputs(dad3d_flame* h, const float* grad_posed, int batch, float* grad_inputs, void* stream) {
    DAD3D_REQUIRE(h && batch >= 0, "dad3d_flame_grad_inputs: bad argument");
    if (batch == 0) return DAD3D_OK;
    DAD3D_REQUIRE(grad_posed && grad_inputs, "dad3d_flame_grad_inputs: null argument");
    DeviceGuard guard(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    // a no-op after the training forward of the same batch size (up to DAD3D_GRAD_INPUTS_MAX_BATCH; larger batches allocate here)
    dad3d_status st = grad_inputs_prepare(h, batch, s);
    if (st) return st;
    const int pad = (batch + kBlockImages - 1) / kBlockImages * kBlockImages;
    const int per_slice = grad_chunks_per_slice(pad);
    GradInputsArgs ga{grad_posed, h->c->d_gpack.get(), static_cast<float*>(h->d_grad_partials.get()), grad_inputs, batch, pad, h->n_verts * 3, grad_chunks(h),
                      h->n_betas + 36, per_slice, (grad_chunks(h) + per_slice - 1) / per_slice};
    return launch_grad_inputs(ga, s);
}

static ChainArgs chain_args(const dad3d_flame* h, const float* params, int batch) {
    ChainArgs ca{};
    ca.params = params;
    ca.jdirs = h->c->d_jdirs.get();
    ca.j0 = h->c->d_j0.get();
    ca.lay = h->lay;
    std::copy(h->parents, h->parents + kNumJoints, ca.parents);
    ca.batch = batch;
    ca.n_betas = h->n_betas;
    ca.max_shape = h->max_shape;
    return ca;
}

dad3d_status dad3d_flame_pose_chain(dad3d_flame* h, const float* params, int batch, float* inputs, float* consts, void* stream) {
    DAD3D_REQUIRE(h && batch >= 0, "dad3d_flame_pose_chain: bad argument");
    if (batch == 0) return DAD3D_OK;
    DAD3D_REQUIRE(params && inputs && consts, "dad3d_flame_pose_chain: null argument");
    DeviceGuard guard(h->device);
    ChainArgs ca = chain_args(h, params, batch);
    ca.inputs = inputs;
    ca.consts = consts;
    return launch_pose_chain(ca, false, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_flame_pose_chain_backward(dad3d_flame* h, const float* params, int batch, const float* grad_inputs,
                                             const float* grad_consts, float* grad_params, void* stream) {
    DAD3D_REQUIRE(h && batch >= 0, "dad3d_flame_pose_chain_backward: bad argument");
    if (batch == 0) return DAD3D_OK;
    DAD3D_REQUIRE(params && grad_inputs && grad_consts && grad_params, "dad3d_flame_pose_chain_backward: null argument");
    DeviceGuard guard(h->device);
    ChainArgs ca = chain_args(h, params, batch);
    ca.g_inputs = grad_inputs;
    ca.g_consts = grad_consts;
    ca.g_params = grad_params;
    return launch_pose_chain(ca, true, static_cast<hipStream_t>(stream));
}

int dad3d_flame_num_chain_inputs(const dad3d_flame* h) { return h ? h->n_betas + 36 : -1; }

dad3d_status dad3d_flame_profile_begin(dad3d_flame* h, void* stream) {
    DAD3D_REQUIRE(h, "null handle");
    DeviceGuard guard(h->device);
    if (!h->ev_first) {
        DAD3D_HIP_TRY(hipEventCreate(&h->ev_first));
        DAD3D_HIP_TRY(hipEventCreate(&h->ev_last));
    }
    h->profiling = true;
    h->prof_launches = 0;
    DAD3D_HIP_TRY(hipEventRecord(h->ev_first, static_cast<hipStream_t>(stream)));
    return DAD3D_OK;
}

dad3d_status dad3d_flame_profile_end(dad3d_flame* h, void* stream, double* total_ms, int* launches) {
    DAD3D_REQUIRE(h && total_ms && launches, "null argument");
    DAD3D_REQUIRE(h->profiling, "dad3d_flame_profile_end without dad3d_flame_profile_begin");
    DeviceGuard guard(h->device);
    DAD3D_HIP_TRY(hipEventRecord(h->ev_last, static_cast<hipStream_t>(stream)));
    DAD3D_HIP_TRY(hipEventSynchronize(h->ev_last));
    float ms = 0.f;
    DAD3D_HIP_TRY(hipEventElapsedTime(&ms, h->ev_first, h->ev_last));
    *total_ms = ms;
    *launches = h->prof_launches;
    h->profiling = false;
    return DAD3D_OK;
}

}  // extern "C"
