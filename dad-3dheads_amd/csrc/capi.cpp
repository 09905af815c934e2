// C ABI of libdad3d_hip.so (include/dad3d.h): handle management, host-side operand packing, launches.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>

#include "common.hpp"

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

template <typename T>
static dad3d_status upload(T** dst, const std::vector<T>& src) {
    *dst = nullptr;
    const size_t bytes = std::max<size_t>(src.size(), 1) * sizeof(T);
    DAD3D_HIP_TRY(hipMalloc(reinterpret_cast<void**>(dst), bytes));
    if (!src.empty()) DAD3D_HIP_TRY(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return DAD3D_OK;
}

}  // namespace dad3d

using namespace dad3d;

// =================================================================================================
// FLAME
// =================================================================================================
static void free_device(int device, std::initializer_list<void*> ptrs) {
    DeviceGuard guard(device);
    for (void* p : ptrs) (void)hipFree(p);
}

// Read-only model constants on the device, shared by a handle and its forks (dad3d_flame_fork). A landmark sub-model keeps its pipelined
// pack in one of these too (d_bpack_pipe, n_tiles_pipe, split_b_scale and the fp16 planes only).
struct FlameConsts {
    int device = 0;
    float *d_bpack = nullptr, *d_jdirs = nullptr, *d_j0 = nullptr, *d_w8 = nullptr;
    float* d_bpack_pipe = nullptr;  // basis of the 20-vertex tiles + jaw-joint columns (flame_decode_pipe.hip); null: model not covered
    float split_b_scale = 1.0f;     // DAD3D_KERNEL_SPLIT_F16: the power of two its entries are multiplied by in front of their fp16 split
    float* d_bpack_f16 = nullptr;   // ... and the pack split into its two fp16 planes, built by the first decode in that form (ensure_basis_f16)
    std::mutex f16_mu;
    int n_tiles_pipe = 0;
    float* d_gpack = nullptr;  // basis^T in MFMA fragment order for dad3d_flame_grad_inputs: built by the first training forward
    std::mutex gpack_mutex;
    ~FlameConsts() { free_device(device, {d_bpack, d_jdirs, d_j0, d_w8, d_gpack, d_bpack_pipe, d_bpack_f16}); }
};

// A landmark list on the device. Immutable once built -- dad3d_flame_set_landmarks builds a new one -- except for the sub-model's fp16
// planes (built under their mutex), so a handle and its forks share it until one of them installs another list.
struct LandmarkList {
    int device = 0;
    int n = 0;
    int *d_head = nullptr, *d_next = nullptr;  // [V][2] {first slot of the vertex, the slot after it}, [n] the slot after each slot
    float4* d_vtab = nullptr;  // [V] {W, w_jaw, first landmark slot, slot chained after it}: the pipelined kernel's; null when it does not cover the model
    // Landmark-only launches on the pipelined and split kernels (SURVEY 7.1 "landmark-only fast path"; BASELINE configs[3]'s per-GPU work):
    // the SUB-MODEL of the distinct vertices the list names (445 of 5023: 23 tiles instead of 252). Same per-vertex arithmetic, ~11x less
    // of it. Its slot chains are the list's own (d_next): renumbering the vertices does not change which slot follows which.
    std::unique_ptr<FlameConsts> sub;  // its pipelined pack (build_landmark_sub); null: no sub-model
    int sub_verts = 0;
    float4* d_sub_vtab = nullptr;  // [sub_verts] the rows of d_vtab of its vertices
    ~LandmarkList() { free_device(device, {d_head, d_next, d_vtab, d_sub_vtab}); }
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
    // ---- per handle, freed by the destructor
    float* d_bwd_partials = nullptr;  // [cap][kBackwardMaxSplit][72] scratch of dad3d_flame_decode_backward
    int bwd_cap = 0;
    float* d_grad_partials = nullptr;  // [slices][padded batch][kGradRows] scratch of dad3d_flame_grad_inputs
    size_t grad_cap = 0;               // its capacity in rows of kGradRows floats
    float* d_imgc = nullptr;
    unsigned* d_sync = nullptr;   // [0] arrival counter, [1] time-out counter; [4], [5], [last]: device-epoch launches
    unsigned arrive_total = 0;    // host mirror of sync[0] after the last launch
    int cap_nbb = 0;
    bool profiling = false;
    unsigned long long* d_trace = nullptr;  // diagnostics (dad3d_flame_debug_trace)
    uint64_t trace_capacity = 0;
    char* d_split_a = nullptr;    // scratch of the split kernels (flame_decode_split.hip): params rows as planes + per-image
    int split_cap = 0;            // constants; split_cap phases of 16 images
    std::vector<char*> split_retired;  // smaller scratches it outgrew: kept until destroy -- a graph captured at a smaller batch still points there
    hipEvent_t ev_first = nullptr, ev_last = nullptr;  // bracket a run of back-to-back launches
    int prof_launches = 0;
    ~dad3d_flame() {
        DeviceGuard guard(device);
        for (void* p : {(void*)d_sync, (void*)d_imgc, (void*)d_bwd_partials, (void*)d_grad_partials, (void*)d_split_a}) (void)hipFree(p);
        for (char* p : split_retired) (void)hipFree(p);
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

// Every fragment of a basis pack in MFMA B-fragment order, [tile][group of 16 k][wave][lane][4 MFMA steps]: MFMA step s of group g has
// lane (q = lane >> 4, n = lane & 15) of wave w supply basis row k = 16 g + 4 q + s of column 16 w + n (the k order inside a group is
// permuted so the A operand can be read row-major with one 16-byte LDS load). frag_offset places the four floats of (tile, g, col, q).
static size_t frag_offset(int tile, int kgroups, int g, int col, int q) {
    return ((((size_t)tile * kgroups + g) * 4 + col / 16) * 64 + (col % 16) + 16 * q) * 4;
}
template <typename F>
static void for_each_fragment(std::vector<float>& pack, int n_tiles, int kgroups, F&& f) {  // f(tile, g, col, q, float* four)
    for (int t = 0; t < n_tiles; ++t)
        for (int g = 0; g < kgroups; ++g)
            for (int col = 0; col < kTileCols; ++col)
                for (int q = 0; q < 4; ++q) f(t, g, col, q, &pack[frag_offset(t, kgroups, g, col, q)]);
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
        need_pack = h->c->d_gpack == nullptr;
    }
    const bool need_scratch = rows > h->grad_cap;
    if (!need_pack && !need_scratch) return DAD3D_OK;
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    if (s != nullptr) (void)hipStreamIsCapturing(s, &capture);
    DAD3D_REQUIRE(capture == hipStreamCaptureStatusNone,
                  "the first training step of a handle (and the first at a larger batch) allocates: run it once before capturing a graph");
    DAD3D_REQUIRE(h->n_betas + 36 <= kGradRows, "dad3d_flame_grad_inputs: %d inputs exceed %d", h->n_betas + 36, kGradRows);
    if (need_pack) {
        std::lock_guard<std::mutex> lock(h->c->gpack_mutex);
        if (!h->c->d_gpack) {
            float* pack = nullptr;
            DAD3D_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&pack), grad_pack_floats(grad_chunks(h)) * sizeof(float)));
            GradPackArgs pa{h->c->d_bpack, pack, h->kgroups, h->n_betas, h->n_pose_feats, h->pose_feat_first, h->n_betas + 36,
                            h->n_verts * 3, grad_chunks(h)};
            dad3d_status st = launch_grad_pack(pa, nullptr);
            if (st == DAD3D_OK && hipDeviceSynchronize() != hipSuccess) st = DAD3D_E_HIP;
            if (st) {
                (void)hipFree(pack);
                set_error("building the basis^T pack failed");
                return st;
            }
            h->c->d_gpack = pack;
        }
    }
    if (need_scratch) {
        DAD3D_HIP_TRY(hipDeviceSynchronize());
        (void)hipFree(h->d_grad_partials);
        h->d_grad_partials = nullptr;
        h->grad_cap = 0;
        DAD3D_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&h->d_grad_partials), rows * kGradRows * sizeof(float)));
        h->grad_cap = rows;
    }
    return DAD3D_OK;
}

static dad3d_status flame_reserve(dad3d_flame* h, int nbb) {
    if (nbb <= h->cap_nbb) return DAD3D_OK;
    if (h->d_imgc) (void)hipFree(h->d_imgc);
    h->d_imgc = nullptr;
    h->cap_nbb = 0;
    DAD3D_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&h->d_imgc), (size_t)nbb * kBlockImages * kImgConsts * sizeof(float)));
    h->cap_nbb = nbb;
    return DAD3D_OK;
}

static bool landmark_subset_enabled() {
    static const bool on = [] {
        const char* e = getenv("DAD3D_LANDMARK_SUBSET");  // =0: landmark-only launches decode the whole mesh like any other (A/B timing)
        return !(e && e[0] == '0');
    }();
    return on;
}

// The sub-model of list L (idx[0..n)): the model's pipelined pack restricted to the distinct vertices the list names, in ascending vertex
// order, copied out fragment by fragment. A column's 416 values do not depend on which tile holds it (the jaw-joint columns are the same in
// every tile), so the sub-model multiplies the same numbers in the same order: a landmark-only launch returns the bits a full-output launch
// of the same handle returns for those vertices (tests/test_gpu_landmark_subset.py). None when the list names more than a third of the mesh.
static dad3d_status build_landmark_sub(const dad3d_flame* h, const int64_t* idx, int n, const std::vector<float4>& vtab, LandmarkList* L) {
    std::vector<char> named(h->n_verts, 0);
    for (int s = 0; s < n; ++s) named[idx[s]] = 1;
    std::vector<int> uniq;
    for (int v = 0; v < h->n_verts; ++v)
        if (named[v]) uniq.push_back(v);
    const int nu = (int)uniq.size(), nt = (nu + kPipeTileVerts - 1) / kPipeTileVerts;
    if ((size_t)nu * 3 > (size_t)h->n_verts) return DAD3D_OK;
    std::vector<float> full((size_t)h->c->n_tiles_pipe * kPipeKGroups * 4 * 64 * 4), pack((size_t)nt * kPipeKGroups * 4 * 64 * 4, 0.0f);
    DAD3D_HIP_TRY(hipMemcpy(full.data(), h->c->d_bpack_pipe, full.size() * sizeof(float), hipMemcpyDeviceToHost));
    for_each_fragment(pack, nt, kPipeKGroups, [&](int t, int g, int col, int q, float* dst) {
        int src_tile = 0, src_col = col;  // the jaw-joint columns (and the zero pad) are the same in every tile
        if (col < 3 * kPipeTileVerts) {
            const int u = t * kPipeTileVerts + col / 3;
            if (u >= nu) return;
            src_tile = uniq[u] / kPipeTileVerts, src_col = (uniq[u] % kPipeTileVerts) * 3 + col % 3;
        }
        std::copy_n(&full[frag_offset(src_tile, kPipeKGroups, g, src_col, q)], 4, dst);
    });
    std::vector<float4> sub_vtab(nu);
    for (int u = 0; u < nu; ++u) sub_vtab[u] = vtab[uniq[u]];
    L->sub.reset(new FlameConsts);
    L->sub->device = h->device;
    L->sub->n_tiles_pipe = nt;
    L->sub->split_b_scale = h->c->split_b_scale;  // a subset of the model's entries: its scale holds
    L->sub_verts = nu;
    const dad3d_status st = upload(&L->sub->d_bpack_pipe, pack);
    return st ? st : upload(&L->d_sub_vtab, sub_vtab);
}

// A new landmark list for h's model: the per-vertex slot chains, the pipelined kernel's per-vertex table (skinning weights from the model,
// landmark slots from the list) and the sub-model, the last two for models the pipelined kernel covers only.
static dad3d_status build_landmarks(const dad3d_flame* h, const int64_t* idx, int n, std::shared_ptr<LandmarkList>* out) {
    const int V = h->n_verts;
    std::vector<int> head(V, -1), next(n, -1);
    for (int s = n - 1; s >= 0; --s) {  // reverse walk: each vertex's chain comes out in ascending slot order
        next[s] = head[idx[s]];
        head[idx[s]] = s;
    }
    std::vector<int> head2((size_t)V * 2, -1);  // what the kernels stage per tile: {head, next[head]}
    for (int v = 0; v < V; ++v)
        if (head[v] >= 0) head2[(size_t)v * 2] = head[v], head2[(size_t)v * 2 + 1] = next[head[v]];
    auto L = std::make_shared<LandmarkList>();
    L->device = h->device;
    L->n = n;
    dad3d_status st;
    if ((st = upload(&L->d_head, head2)) || (st = upload(&L->d_next, next))) return st;
    if (h->c->d_bpack_pipe) {
        std::vector<float> w8((size_t)V * 8);
        DAD3D_HIP_TRY(hipMemcpy(w8.data(), h->c->d_w8, w8.size() * sizeof(float), hipMemcpyDeviceToHost));
        std::vector<float4> vtab(V);
        for (int v = 0; v < V; ++v) {
            const float* w = &w8[(size_t)v * 8];
            float fh, fn;
            memcpy(&fh, &head2[(size_t)v * 2], 4), memcpy(&fn, &head2[(size_t)v * 2 + 1], 4);
            vtab[v] = float4{w[5] + w[2], w[2], fh, fn};  // W = (w0 + w1 + w3 + w4) + w_jaw
        }
        if ((st = upload(&L->d_vtab, vtab))) return st;
        if (landmark_subset_enabled() && n > 0 && (st = build_landmark_sub(h, idx, n, vtab, L.get()))) return st;
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
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);

    std::unique_ptr<dad3d_flame> h(new dad3d_flame);
    h->device = device;
    h->n_verts = m->n_verts;
    h->n_betas = m->n_betas;
    h->image_size = image_size;
    ParamLayout& L = h->lay;
    int cur = 0;
    L.shape_off = cur, L.shape_n = c->shape, cur += c->shape;
    L.expr_off = cur, L.expr_n = c->expression, cur += c->expression;
    L.jaw_off = cur, L.jaw_n = c->jaw, cur += c->jaw;
    L.rot_off = cur, cur += c->rotation;
    L.eye_off = cur, L.eye_n = c->eyeballs, cur += c->eyeballs;
    L.neck_off = cur, L.neck_n = c->neck, cur += c->neck;
    L.trans_off = cur, cur += c->translation;
    L.scale_off = cur, cur += c->scale;
    L.n_params = cur;
    for (int j = 0; j < kNumJoints; ++j) h->parents[j] = (j == 0) ? -1 : m->parents[j];

    // Only the jaw can rotate when neck and eyeballs are size-0 inputs: their Rodrigues matrix is exactly
    // I, so 27 of the 36 pose features are exactly 0 and their basis rows can be skipped (same result).
    // ... and the jaw-only epilogue (S = w0+w1+w3+w4 for "the joints that cannot rotate") also needs no joint to hang
    // off the jaw: a kinematic tree with a child of joint 2 takes the generic 36-feature path.
    bool jaw_is_leaf = true;
    for (int j = 1; j < kNumJoints; ++j) jaw_is_leaf = jaw_is_leaf && m->parents[j] != 2;
    const bool jaw_only = (c->neck == 0 && c->eyeballs == 0 && jaw_is_leaf);
    h->n_pose_feats = jaw_only ? 9 : 36;
    h->pose_feat_first = jaw_only ? 9 : 0;
    const int k_used = h->n_betas + h->n_pose_feats + 1;  // [betas | pose feature | template]
    h->kgroups = (k_used + 15) / 16;
    h->ksteps = h->kgroups * 4;
    DAD3D_REQUIRE(h->kgroups == 26 || h->kgroups == 28, "unexpected basis depth %d", k_used);
    const int V = m->n_verts, NB = m->n_betas;
    h->n_tiles = (V + kTileVerts - 1) / kTileVerts;
    h->n_tiles_pad8 = (h->n_tiles + 7) / 8 * 8;

    // ---- pack the basis in MFMA B-fragment order (for_each_fragment), 21 vertices = 63 columns per tile -------
    auto basis = [&](int k, int v, int comp) -> float {
        if (k < NB) return m->shapedirs[((size_t)v * 3 + comp) * NB + k];
        if (k < NB + h->n_pose_feats) {
            const int f = h->pose_feat_first + (k - NB);
            return m->posedirs[(size_t)f * 3 * V + (size_t)v * 3 + comp];
        }
        return m->v_template[(size_t)v * 3 + comp];  // k == NB + n_pose_feats: the row multiplied by 1
    };
    std::vector<float> bpack((size_t)h->n_tiles * h->kgroups * 4 * 64 * 4, 0.0f);
    for_each_fragment(bpack, h->n_tiles, h->kgroups, [&](int t, int g, int col, int q, float* dst) {
        const int v = t * kTileVerts + col / 3;
        if (col >= kTileVerts * 3 || v >= V) return;
        for (int i = 0; i < 4; ++i) {
            const int k = 16 * g + 4 * q + i;
            if (k < k_used) dst[i] = basis(k, v, col % 3);
        }
    });

    // ---- joints are linear in betas: J = J_regressor.v_template + (J_regressor.shapedirs).betas ----
    std::vector<float> j0(3 * kNumJoints), jdirs((size_t)3 * kNumJoints * NB);
    {
        std::vector<double> acc((size_t)3 * kNumJoints * (NB + 1), 0.0);
        for (int j = 0; j < kNumJoints; ++j)
            for (int v = 0; v < V; ++v) {
                const double r = m->j_regressor[(size_t)j * V + v];
                if (r == 0.0) continue;
                for (int comp = 0; comp < 3; ++comp) {
                    double* a = &acc[((size_t)j * 3 + comp) * (NB + 1)];
                    a[NB] += r * m->v_template[(size_t)v * 3 + comp];
                    const float* sd = &m->shapedirs[((size_t)v * 3 + comp) * NB];
                    for (int l = 0; l < NB; ++l) a[l] += r * sd[l];
                }
            }
        for (int o = 0; o < 3 * kNumJoints; ++o) {
            j0[o] = (float)acc[(size_t)o * (NB + 1) + NB];
            for (int l = 0; l < NB; ++l) jdirs[(size_t)o * NB + l] = (float)acc[(size_t)o * (NB + 1) + l];
        }
    }
    std::vector<float> w8((size_t)V * 8, 0.0f);
    for (int v = 0; v < V; ++v) {
        const float* w = &m->lbs_weights[(size_t)v * kNumJoints];
        for (int j = 0; j < kNumJoints; ++j) w8[(size_t)v * 8 + j] = w[j];
        w8[(size_t)v * 8 + 5] = ((w[0] + w[1]) + w[3]) + w[4];  // weight of the joints that cannot rotate (jaw-only mode)
    }
    // ---- the pipelined single-role kernel (flame_decode_pipe.hip): jaw-only models with the dad_3dnet.yaml params layout.
    // Tiles of 20 vertices; columns 60..62 of every tile carry the jaw joint J_jaw = J0_jaw + Jdirs_jaw . betas (rows of the pose
    // feature contribute nothing to a joint: smplx regresses the joints from v_shaped), column 63 is zero.
    const bool pipe_ok = jaw_only && c->jaw == 3 && c->shape == 300 && c->expression == 100 && L.jaw_off == 400 && L.rot_off == 403 &&
                         L.trans_off == 409 && L.scale_off == 412 && L.n_params == 413 && h->kgroups == kPipeKGroups;
    std::vector<float> bpack_pipe;
    const int n_tiles_pipe = (V + kPipeTileVerts - 1) / kPipeTileVerts;
    if (pipe_ok) {
        bpack_pipe.assign((size_t)n_tiles_pipe * kPipeKGroups * 4 * 64 * 4, 0.0f);
        for_each_fragment(bpack_pipe, n_tiles_pipe, kPipeKGroups, [&](int t, int g, int col, int q, float* dst) {
            for (int i = 0; i < 4; ++i) {
                const int k = 16 * g + 4 * q + i;
                if (k >= k_used) continue;
                if (col < 3 * kPipeTileVerts) {
                    const int v = t * kPipeTileVerts + col / 3;
                    if (v < V) dst[i] = basis(k, v, col % 3);
                } else if (col < 3 * kPipeTileVerts + 3) {
                    const int o = 2 * 3 + (col - 3 * kPipeTileVerts);  // joint 2 = jaw
                    dst[i] = k < NB ? jdirs[(size_t)o * NB + k] : (k == NB + h->n_pose_feats ? j0[o] : 0.0f);
                }
            }
        });
    }

    h->c = std::make_shared<FlameConsts>();
    h->c->device = device;
    h->c->n_tiles_pipe = n_tiles_pipe;
    if (pipe_ok) {
        float max_abs = 0.0f;
        for (float v : bpack_pipe) max_abs = std::max(max_abs, std::fabs(v));
        h->c->split_b_scale = split_basis_scale(max_abs);
    }
    dad3d_status st;
    if ((pipe_ok && (st = upload(&h->c->d_bpack_pipe, bpack_pipe))) || (st = upload(&h->c->d_bpack, bpack)) ||
        (st = upload(&h->c->d_jdirs, jdirs)) || (st = upload(&h->c->d_j0, j0)) || (st = upload(&h->c->d_w8, w8)) ||
        (st = upload(&h->d_sync, std::vector<unsigned>(kSyncWords, 0u))) || (st = flame_reserve(h.get(), 1)) ||
        (st = build_landmarks(h.get(), nullptr, 0, &h->lmk)))
        return st;
    *out = h.release();
    return DAD3D_OK;
}

void dad3d_flame_destroy(dad3d_flame* h) { delete h; }

dad3d_status dad3d_flame_fork(dad3d_flame* parent, dad3d_flame** out) {
    DAD3D_REQUIRE(parent && out, "dad3d_flame_fork: bad argument");
    *out = nullptr;
    DeviceGuard guard(parent->device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", parent->device);
    std::unique_ptr<dad3d_flame> h(new dad3d_flame);
    static_cast<FlameShape&>(*h) = *parent;
    h->c = parent->c;
    h->lmk = parent->lmk;
    h->kernel_choice = parent->kernel_choice;
    dad3d_status st;
    if ((st = upload(&h->d_sync, std::vector<unsigned>(kSyncWords, 0u))) || (st = flame_reserve(h.get(), 1))) return st;
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
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    if (s != nullptr) (void)hipStreamIsCapturing(s, &capture);
    DAD3D_REQUIRE(capture == hipStreamCaptureStatusNone, "the first fp16-split decode of a model builds its basis planes: run it once before capturing a graph");
    const size_t bytes = (size_t)c->n_tiles_pipe * kPipeKGroups * 4 * 64 * 4 * sizeof(float);
    float* d = nullptr;
    DAD3D_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d), bytes));
    dad3d_status st = launch_split_basis_f16(c->d_bpack_pipe, d, c->n_tiles_pipe, c->split_b_scale, s);
    if (st == DAD3D_OK && hipStreamSynchronize(s) != hipSuccess) {
        set_error("ensure_basis_f16: hipStreamSynchronize failed");
        st = DAD3D_E_HIP;
    }
    if (st) {
        (void)hipFree(d);
        return st;
    }
    c->d_bpack_f16 = d;
    return DAD3D_OK;
}

// Scratch of the split kernels (pre-pass -> tile kernel): n_phase blocks of kSplitBlockBytes, grown on demand -- never inside a capture.
static dad3d_status ensure_split_scratch(dad3d_flame* h, int n_phase, hipStream_t s) {
    if (n_phase <= h->split_cap) return DAD3D_OK;
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    if (s != nullptr) (void)hipStreamIsCapturing(s, &capture);
    DAD3D_REQUIRE(capture == hipStreamCaptureStatusNone,
                  "the first split-kernel decode of a handle (and the first at a larger batch) allocates: run it once before capturing a graph");
    if (h->d_split_a) h->split_retired.push_back(h->d_split_a);  // (2.6 KB per image: never worth a dangling pointer in somebody's graph)
    h->d_split_a = nullptr, h->split_cap = 0;
    DAD3D_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&h->d_split_a), (size_t)n_phase * kSplitBlockBytes));
    // (the padding is copied into LDS, never read.) On the LAUNCH's stream: hipMemset is ordered on the null stream only, and a
    // non-blocking stream's pre-pass overtook it -- zero planes under the first launch of a fork (found by the two-streams test)
    DAD3D_HIP_TRY(hipMemsetAsync(h->d_split_a, 0, (size_t)n_phase * kSplitBlockBytes, s));
    h->split_cap = n_phase;
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
    const float4* vtab = on_sub ? L.d_sub_vtab : L.d_vtab;
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
        sa.bpack = c->d_bpack_pipe;
        sa.bpack_f16 = c->d_bpack_f16;
        sa.vtab = vtab;
        sa.lmk_next = L.d_next;
        sa.verts3d = verts3d;
        sa.proj = proj;
        sa.lmk_xy = lmk_xy;
        sa.lmk_px = lmk_px;
        sa.aplanes = h->d_split_a;
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
        pa.bpack = c->d_bpack_pipe;
        pa.vtab = vtab;
        pa.lmk_next = L.d_next;
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
        if (nbb > h->cap_nbb) {
            DAD3D_HIP_TRY(hipDeviceSynchronize());
            if ((st = flame_reserve(h, nbb))) return st;
        }
        DecodeArgs da{};
        da.params = params;
        da.bpack = h->c->d_bpack;
        da.jdirs = h->c->d_jdirs;
        da.j0 = h->c->d_j0;
        da.weights8 = h->c->d_w8;
        da.lmk_head = L.d_head;
        da.lmk_next = L.d_next;
        da.imgc = h->d_imgc;
        da.sync = h->d_sync;
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
        hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
        if (s != nullptr) (void)hipStreamIsCapturing(s, &capture);
        const bool device_epoch = capture != hipStreamCaptureStatusNone;
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
    float* d = nullptr;
    DAD3D_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d), (n_par + n_v + n_p + n_lx + n_lp + 4) * sizeof(float)));
    float* d_par = d;
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
    (void)hipFree(d);
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

dad3d_status dad3d_flame_select_kernel(dad3d_flame* h, int which) {
    DAD3D_REQUIRE(h && which >= DAD3D_KERNEL_AUTO && which <= DAD3D_KERNEL_SPLIT_F16, "dad3d_flame_select_kernel: bad argument");
    h->kernel_choice = which;
    return DAD3D_OK;
}

dad3d_status dad3d_flame_handoff_timeouts(dad3d_flame* h, unsigned* count) {
    DAD3D_REQUIRE(h && count, "null argument");
    DeviceGuard guard(h->device);
    DAD3D_HIP_TRY(hipDeviceSynchronize());
    DAD3D_HIP_TRY(hipMemcpy(count, h->d_sync + 1, sizeof(unsigned), hipMemcpyDeviceToHost));
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
    ba.weights8 = h->c->d_w8;
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
        if (batch > h->bwd_cap) {
            DAD3D_HIP_TRY(hipDeviceSynchronize());
            (void)hipFree(h->d_bwd_partials);
            h->d_bwd_partials = nullptr;
            h->bwd_cap = 0;
            DAD3D_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&h->d_bwd_partials),
                                    (size_t)batch * kBackwardMaxSplit * kBackwardConsts * sizeof(float)));
            h->bwd_cap = batch;
        }
        ba.partials = h->d_bwd_partials;
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
    GradInputsArgs ga{grad_posed, h->c->d_gpack, h->d_grad_partials, grad_inputs, batch, pad, h->n_verts * 3, grad_chunks(h),
                      h->n_betas + 36, per_slice, (grad_chunks(h) + per_slice - 1) / per_slice};
    return launch_grad_inputs(ga, s);
}

static ChainArgs chain_args(const dad3d_flame* h, const float* params, int batch) {
    ChainArgs ca{};
    ca.params = params;
    ca.jdirs = h->c->d_jdirs;
    ca.j0 = h->c->d_j0;
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

// =================================================================================================
// Sim3DR
// =================================================================================================
struct dad3d_mesh {
    int device = 0;
    int ntri = 0, nver = 0;
    int *d_tri = nullptr, *d_adj_ptr = nullptr, *d_adj_face = nullptr;
    int4* d_adj_tri = nullptr;
    std::vector<int> h_tri;  // the triangle list on the host (dad3d_mesh_set_texcoords reads it)
    uint2* d_nc_faces[kNormalChunkings] = {};  // chunk face lists of the normals kernels (NormalChunksDev)
    unsigned short* d_nc_slot[kNormalChunkings] = {};
    uint4* d_nc_row8[kNormalChunkings] = {};
    NormalChunksDev nc[kNormalChunkings] = {};
    unsigned long long* d_trace = nullptr;  // diagnostics (dad3d_mesh_debug_trace)
    float4* d_tex_tri[2] = {};  // texel coordinates per triangle corner, [ntri][2] (dad3d_mesh_set_texcoords): corner / reference indexing
    void* d_raster = nullptr;  // per-image triangle boxes + corner planes, grown on demand (one stream at a time)
    size_t raster_bytes = 0;
    int raster_batch = 0, raster_h = 0, raster_w = 0;
    // The scratch layout depends on (batch, h, w): a change of shape re-zeroes the tile counters in stream order.
    dad3d_status raster_scratch(int batch, int h, int w, hipStream_t s) {
        if (batch == raster_batch && h == raster_h && w == raster_w) return DAD3D_OK;
        const size_t need = raster_scratch_bytes(dev(), batch, h, w);
        if (need > raster_bytes) {
            DAD3D_HIP_TRY(hipDeviceSynchronize());
            if (d_raster) (void)hipFree(d_raster);
            d_raster = nullptr;
            raster_bytes = 0;
            raster_batch = 0;
            DAD3D_HIP_TRY(hipMalloc(&d_raster, need));
            raster_bytes = need;
        }
        if (dad3d_status st = raster_scratch_init(dev(), d_raster, batch, h, w, s)) return st;
        raster_batch = batch, raster_h = h, raster_w = w;
        return DAD3D_OK;
    }
    void* d_frames = nullptr;  // scratch of the frames chain (sim3dr_frames.hip), grown on demand like d_raster; needs no initialisation
    size_t frames_bytes = 0;
    dad3d_status frames_scratch(int n_frames, int n_heads, int total_tiles) {
        const size_t need = frames_scratch_bytes(ntri, n_frames, n_heads, total_tiles);
        if (need <= frames_bytes) return DAD3D_OK;
        DAD3D_HIP_TRY(hipDeviceSynchronize());
        if (d_frames) (void)hipFree(d_frames);
        d_frames = nullptr;
        frames_bytes = 0;
        DAD3D_HIP_TRY(hipMalloc(&d_frames, need));
        frames_bytes = need;
        return DAD3D_OK;
    }
    MeshDev dev() const { return MeshDev{d_tri, d_adj_ptr, d_adj_face, d_adj_tri, ntri, nver}; }
};

// the checks the two frames entries share, all on the host; *total_tiles = 0: nothing to do
static dad3d_status frames_arguments(const char* who, dad3d_mesh* m, const int64_t* frames, const int64_t* frames_host, int n_frames,
                                     const float* vertices, const float* colors, const int32_t* image_index, int n_heads, int32_t* flags,
                                     int* total_tiles) {
    *total_tiles = 0;
    DAD3D_REQUIRE(m && n_frames >= 0 && n_heads >= 0, "%s: bad argument", who);
    DAD3D_REQUIRE(n_frames <= DAD3D_FRAME_MAX_COUNT && n_heads <= DAD3D_FRAME_MAX_COUNT, "%s: %d frames and %d heads, at most %d each", who,
                  n_frames, n_heads, DAD3D_FRAME_MAX_COUNT);
    if (n_heads == 0) return DAD3D_OK;
    DAD3D_REQUIRE(image_index && flags, "%s: null buffer", who);
    if (n_frames == 0) return DAD3D_OK;
    DAD3D_REQUIRE(frames && frames_host && (m->ntri == 0 || (vertices && colors)), "%s: null buffer", who);
    DAD3D_REQUIRE(m->ntri <= 65535 && 4ll * m->ntri * n_heads < (1ll << 31), "%s: %d triangles and %d heads exceed 65535 triangles or 2^31 list entries",
                  who, m->ntri, n_heads);
    return frames_check_shapes(who, frames_host, n_frames, total_tiles);
}

extern "C" {

dad3d_status dad3d_mesh_create(const int32_t* tri, int ntri, int nver, int device, dad3d_mesh** out) {
    DAD3D_REQUIRE(out && ntri >= 0 && nver >= 0 && (tri || ntri == 0), "dad3d_mesh_create: bad argument");
    *out = nullptr;
    for (int i = 0; i < 3 * ntri; ++i)
        DAD3D_REQUIRE(tri[i] >= 0 && tri[i] < nver, "triangle index %d out of range [0,%d)", tri[i], nver);
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    // vertex -> incident (face, corner) list; faces ascending, so a gather reproduces the serial
    // scatter-add order of rasterize_kernel.cpp:188-198
    std::vector<int> ptr(nver + 1, 0), face(3 * (size_t)ntri);
    for (int i = 0; i < 3 * ntri; ++i) ++ptr[tri[i] + 1];
    for (int v = 0; v < nver; ++v) ptr[v + 1] += ptr[v];
    std::vector<int> fill(ptr.begin(), ptr.end() - 1);
    for (int f = 0; f < ntri; ++f)
        for (int c = 0; c < 3; ++c) face[fill[tri[3 * f + c]]++] = f;
    std::unique_ptr<dad3d_mesh> m(new dad3d_mesh);
    m->device = device;
    m->ntri = ntri;
    m->nver = nver;
    std::vector<int> tri_v(tri, tri + 3 * (size_t)ntri);
    m->h_tri = tri_v;
    std::vector<int4> adj_tri(face.size());
    for (size_t e = 0; e < face.size(); ++e) {
        const int f = face[e];
        adj_tri[e] = make_int4(tri[3 * f], tri[3 * f + 1], tri[3 * f + 2], f);
    }
    dad3d_status st;
    if ((st = upload(&m->d_tri, tri_v)) || (st = upload(&m->d_adj_ptr, ptr)) || (st = upload(&m->d_adj_face, face)) ||
        (st = upload(&m->d_adj_tri, adj_tri))) {
        dad3d_mesh_destroy(m.release());
        return st;
    }
    // chunk face lists for 1, 2, 4 and 8 vertex chunks per image (only where table + staged vertices fit the LDS)
    for (int k = 0; k < kNormalChunkings && nver > 0 && ntri > 0 && nver <= 65535; ++k) {
        const int chunks = 1 << k, vpb = (nver + chunks - 1) / chunks;
        std::vector<int> fptr(chunks + 1, 0), slot(face.size(), 0);
        std::vector<std::vector<int4>> lists(chunks);
        std::vector<int> pos_of(3 * (size_t)ntri);  // (face, corner) -> position of the face in the list of the corner's chunk
        for (int f = 0; f < ntri; ++f) {
            int seen_chunk[3], seen_pos[3], n_seen = 0;
            for (int c = 0; c < 3; ++c) {
                const int ch = tri[3 * f + c] / vpb;
                int p = -1;
                for (int j = 0; j < n_seen; ++j)
                    if (seen_chunk[j] == ch) p = seen_pos[j];
                if (p < 0) {
                    p = (int)lists[ch].size();
                    lists[ch].push_back(make_int4(tri[3 * f], tri[3 * f + 1], tri[3 * f + 2], f));
                    seen_chunk[n_seen] = ch, seen_pos[n_seen] = p, ++n_seen;
                }
                pos_of[3 * (size_t)f + c] = p;
            }
        }
        {   // slot[e] for the CSR entries, filled in the same (face-ascending) order as `face`
            std::vector<int> cursor(ptr.begin(), ptr.end() - 1);
            for (int f = 0; f < ntri; ++f)
                for (int c = 0; c < 3; ++c) slot[cursor[tri[3 * f + c]]++] = pos_of[3 * (size_t)f + c];
        }
        // The table position of a face is free (a vertex's summation order is the order of its slot row, not of the table):
        // order every chunk list so that the 32 faces a half-wave crosses together read 32 different LDS banks for each of
        // their three corners (bank = 3 * index + component mod 32, 3 is invertible mod 32: corner indices distinct mod 32).
        // First fit over the open groups; what does not fit anywhere goes to the end with its conflicts.
        for (int ch = 0; ch < chunks; ++ch) {
            std::vector<int4>& L = lists[ch];
            const int n = (int)L.size(), ngroups = (n + 31) / 32;
            std::vector<unsigned> used(3 * (size_t)ngroups, 0u);
            std::vector<int> fill(ngroups, 0), where(n, -1), spill;
            int first_open = 0;
            for (int i = 0; i < n; ++i) {
                const unsigned b0 = 1u << (L[i].x & 31), b1 = 1u << (L[i].y & 31), b2 = 1u << (L[i].z & 31);
                int g = first_open, tried = 0;
                for (; g < ngroups && tried < 64; ++g) {
                    if (fill[g] >= 32) continue;
                    ++tried;
                    if (!(used[3 * g] & b0) && !(used[3 * g + 1] & b1) && !(used[3 * g + 2] & b2)) break;
                }
                if (g >= ngroups || tried >= 64) {
                    spill.push_back(i);
                    continue;
                }
                used[3 * g] |= b0, used[3 * g + 1] |= b1, used[3 * g + 2] |= b2;
                where[i] = g * 32 + fill[g]++;
                while (first_open < ngroups && fill[first_open] >= 32) ++first_open;
            }
            // full groups first (each lands on a half-wave boundary), then the members of the unfilled groups and the spill
            std::vector<int> order;  // new position -> old position
            order.reserve(n);
            std::vector<std::vector<int>> members(ngroups);
            for (int i = 0; i < n; ++i)
                if (where[i] >= 0) members[where[i] / 32].push_back(i);
            for (int g = 0; g < ngroups; ++g)
                if (members[g].size() == 32) order.insert(order.end(), members[g].begin(), members[g].end());
            for (int g = 0; g < ngroups; ++g)
                if (members[g].size() != 32) order.insert(order.end(), members[g].begin(), members[g].end());
            order.insert(order.end(), spill.begin(), spill.end());
            std::vector<int> new_of(n);
            std::vector<int4> R(n);
            for (int np = 0; np < n; ++np) new_of[order[np]] = np, R[np] = L[order[np]];
            L.swap(R);
            const int lo = ch * vpb, hi = std::min(nver, lo + vpb);
            for (int v = lo; v < hi; ++v)
                for (int e = ptr[v]; e < ptr[v + 1]; ++e) slot[e] = new_of[slot[e]];
        }
        int max_faces = 0;
        std::vector<uint2> flat;
        for (int ch = 0; ch < chunks; ++ch) {
            fptr[ch] = (int)flat.size();
            for (const int4& f : lists[ch]) flat.push_back(make_uint2((unsigned)f.x | ((unsigned)f.y << 16), (unsigned)f.z));
            max_faces = std::max(max_faces, (int)lists[ch].size());
        }
        fptr[chunks] = (int)flat.size();
        if (max_faces > 65535 || normal_table_lds_bytes(nver, max_faces) > 160 * 1024 - 1024) continue;
        std::vector<unsigned short> slot16(slot.begin(), slot.end());
        std::vector<uint4> row8(nver);
        for (int v = 0; v < nver; ++v) {
            unsigned short r[8];
            const int deg = ptr[v + 1] - ptr[v];
            for (int j = 0; j < 8; ++j) r[j] = j < deg ? slot16[ptr[v] + j] : (unsigned short)0xFFFF;
            if (deg > 8) r[7] = 0xFFFE;
            row8[v] = make_uint4(r[0] | ((unsigned)r[1] << 16), r[2] | ((unsigned)r[3] << 16), r[4] | ((unsigned)r[5] << 16), r[6] | ((unsigned)r[7] << 16));
        }
        if (max_faces >= 0xFFFE) continue;
        if ((st = upload(&m->d_nc_faces[k], flat)) || (st = upload(&m->d_nc_slot[k], slot16)) || (st = upload(&m->d_nc_row8[k], row8))) {
            dad3d_mesh_destroy(m.release());
            return st;
        }
        m->nc[k] = NormalChunksDev{m->d_nc_faces[k], {}, m->d_nc_slot[k], m->d_nc_row8[k], chunks, vpb, max_faces};
        for (int ch = 0; ch <= chunks; ++ch) m->nc[k].face_ptr[ch] = fptr[ch];
    }
    *out = m.release();
    return DAD3D_OK;
}

void dad3d_mesh_destroy(dad3d_mesh* m) {
    if (!m) return;
    DeviceGuard guard(m->device);
    for (void* p : {(void*)m->d_tri, (void*)m->d_adj_ptr, (void*)m->d_adj_face, (void*)m->d_adj_tri, m->d_raster, m->d_frames, (void*)m->d_tex_tri[0],
                    (void*)m->d_tex_tri[1]})
        if (p) (void)hipFree(p);
    for (int k = 0; k < kNormalChunkings; ++k)
        for (void* p : {(void*)m->d_nc_faces[k], (void*)m->d_nc_slot[k], (void*)m->d_nc_row8[k]})
            if (p) (void)hipFree(p);
    delete m;
}

dad3d_status dad3d_mesh_get_normal(dad3d_mesh* m, float* ver_normal, const float* vertices, int batch, unsigned flags,
                                   void* stream) {
    DAD3D_REQUIRE(m && batch >= 0, "dad3d_mesh_get_normal: bad argument");
    if (batch == 0 || m->nver == 0) return DAD3D_OK;
    DAD3D_REQUIRE(ver_normal && vertices, "dad3d_mesh_get_normal: null buffer");
    DeviceGuard guard(m->device);
    return launch_get_normal(m->dev(), m->nc, ver_normal, vertices, batch, flags, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_mesh_get_tri_normal(dad3d_mesh* m, float* tri_normal, const float* vertices, int batch,
                                       int norm_flg, void* stream) {
    DAD3D_REQUIRE(m && batch >= 0, "dad3d_mesh_get_tri_normal: bad argument");
    if (batch == 0 || m->ntri == 0) return DAD3D_OK;
    DAD3D_REQUIRE(tri_normal && vertices, "dad3d_mesh_get_tri_normal: null buffer");
    DeviceGuard guard(m->device);
    return launch_tri_normal(m->dev(), tri_normal, vertices, batch, norm_flg, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_mesh_get_ver_normal(dad3d_mesh* m, float* ver_normal, const float* tri_normal, int batch,
                                       unsigned flags, void* stream) {
    DAD3D_REQUIRE(m && batch >= 0, "dad3d_mesh_get_ver_normal: bad argument");
    if (batch == 0 || m->nver == 0) return DAD3D_OK;
    DAD3D_REQUIRE(ver_normal && (tri_normal || m->ntri == 0), "dad3d_mesh_get_ver_normal: null buffer");
    DeviceGuard guard(m->device);
    return launch_ver_normal(m->dev(), ver_normal, tri_normal, batch, flags, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_mesh_rasterize(dad3d_mesh* m, uint8_t* image, const float* vertices, const float* colors,
                                  float* depth, int batch, int h, int w, int c, float alpha, int reverse,
                                  void* stream) {
    DAD3D_REQUIRE(m && batch >= 0 && h >= 0 && w >= 0 && c >= 0, "dad3d_mesh_rasterize: bad argument");
    DAD3D_REQUIRE(alpha == alpha, "dad3d_mesh_rasterize: alpha is NaN");
    if (batch == 0 || h == 0 || w == 0) return DAD3D_OK;
    DAD3D_REQUIRE(image && (vertices || m->ntri == 0) && (colors || m->ntri == 0 || c == 0),
                  "dad3d_mesh_rasterize: null buffer");
    DeviceGuard guard(m->device);
    if (dad3d_status st = m->raster_scratch(batch, h, w, static_cast<hipStream_t>(stream))) return st;
    // alpha != 1: the blends of rasterize_kernel.cpp:268-284 replayed in triangle order (mode 2)
    return launch_rasterize(m->dev(), m->nc, m->d_raster, m->d_trace, image, vertices, colors, depth, nullptr, nullptr, batch, h, w, c, reverse,
                            alpha == 1.0f ? 0 : 2, nullptr, static_cast<hipStream_t>(stream), alpha);
}

dad3d_status dad3d_mesh_render(dad3d_mesh* m, uint8_t* image, const float* vertices, float* light, float* depth, int batch,
                               int h, int w, const dad3d_light* cfg, int flags, void* stream) {
    DAD3D_REQUIRE(m && cfg && batch >= 0 && h >= 0 && w >= 0, "dad3d_mesh_render: bad argument");
    if (batch == 0 || h == 0 || w == 0) return DAD3D_OK;
    DAD3D_REQUIRE(image, "dad3d_mesh_render: null buffer");
    DeviceGuard guard(m->device);
    if (m->ntri == 0) {  // nothing to draw: only the background
        if (flags & DAD3D_RENDER_CLEAR) DAD3D_HIP_TRY(hipMemsetAsync(image, 0, (size_t)batch * h * w * 3, static_cast<hipStream_t>(stream)));
        return DAD3D_OK;
    }
    DAD3D_REQUIRE(vertices && light, "dad3d_mesh_render: null buffer");
    if (dad3d_status st = m->raster_scratch(batch, h, w, static_cast<hipStream_t>(stream))) return st;
    return launch_rasterize(m->dev(), m->nc, m->d_raster, m->d_trace, image, vertices, light, depth, nullptr, nullptr, batch, h, w, 3,
                            flags, 0, cfg, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_mesh_rasterize_frames(dad3d_mesh* m, const int64_t* frames, const int64_t* frames_host, int n_frames, const float* vertices,
                                         const float* colors, const int32_t* image_index, int n_heads, int reverse, int32_t* flags, void* stream) {
    int total_tiles = 0;
    if (dad3d_status st = frames_arguments("dad3d_mesh_rasterize_frames", m, frames, frames_host, n_frames, vertices, colors, image_index, n_heads,
                                           flags, &total_tiles))
        return st;
    if (total_tiles == 0) return DAD3D_OK;  // no frames or no heads
    DeviceGuard guard(m->device);
    if (dad3d_status st = m->frames_scratch(n_frames, n_heads, total_tiles)) return st;
    return launch_rasterize_frames(m->dev(), m->d_frames, frames, n_frames, total_tiles, vertices, colors, image_index, n_heads, reverse ? 1 : 0,
                                   flags, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_mesh_render_frames(dad3d_mesh* m, const int64_t* frames, const int64_t* frames_host, int n_frames, const float* vertices,
                                      float* light, const int32_t* image_index, int n_heads, const dad3d_light* cfg, int render_flags,
                                      int32_t* flags, void* stream) {
    DAD3D_REQUIRE(cfg, "dad3d_mesh_render_frames: bad argument");
    DAD3D_REQUIRE(!(render_flags & ~DAD3D_RENDER_REVERSE),
                  "dad3d_mesh_render_frames: render flags %d: only DAD3D_RENDER_REVERSE (a frame is the caller's picture: no DAD3D_RENDER_CLEAR)", render_flags);
    int total_tiles = 0;
    if (dad3d_status st = frames_arguments("dad3d_mesh_render_frames", m, frames, frames_host, n_frames, vertices, light, image_index, n_heads, flags,
                                           &total_tiles))
        return st;
    if (total_tiles == 0) return DAD3D_OK;
    DeviceGuard guard(m->device);
    if (dad3d_status st = m->frames_scratch(n_frames, n_heads, total_tiles)) return st;
    // the light of every head, flagged or not, as dad3d_mesh_normal_phong_light computes it; then it is the colours
    if (dad3d_status st = launch_phong(m->dev(), m->nc, light, vertices, nullptr, nullptr, n_heads, *cfg, static_cast<hipStream_t>(stream))) return st;
    return launch_rasterize_frames(m->dev(), m->d_frames, frames, n_frames, total_tiles, vertices, light, image_index, n_heads,
                                   render_flags & DAD3D_RENDER_REVERSE, flags, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_mesh_render_texture_frames(dad3d_mesh* m, const int64_t* frames, const int64_t* frames_host, int n_frames, const float* vertices,
                                              const void* texture, int texture_dtype, int texture_batched, int tex_h, int tex_w, int tex_c,
                                              int mapping_type, int indexing, const int32_t* image_index, int n_heads, int32_t* flags, void* stream) {
    const char* who = "dad3d_mesh_render_texture_frames";
    // the scalar arguments and the host table first: a bad one is refused before the handle is looked at or any device work starts
    DAD3D_REQUIRE(texture_dtype == DAD3D_DTYPE_F32 || texture_dtype == DAD3D_DTYPE_U8, "%s: the texture is float32 (DAD3D_DTYPE_F32) or uint8 (DAD3D_DTYPE_U8)", who);
    DAD3D_REQUIRE(tex_h >= 1 && tex_w >= 1 && tex_c >= 1 && (size_t)tex_h * tex_w * tex_c < (1ull << 31), "%s: texture of %d x %d x %d", who, tex_h, tex_w, tex_c);
    DAD3D_REQUIRE(tex_c >= 3, "%s: a frame has three channels, tex_c = %d", who, tex_c);
    DAD3D_REQUIRE(indexing == DAD3D_TEX_INDEX_CORNER || indexing == DAD3D_TEX_INDEX_REFERENCE, "%s: unknown indexing mode %d", who, indexing);
    DAD3D_REQUIRE(n_frames >= 0 && n_heads >= 0, "%s: bad argument", who);
    DAD3D_REQUIRE(n_frames <= DAD3D_FRAME_MAX_COUNT && n_heads <= DAD3D_FRAME_MAX_COUNT, "%s: %d frames and %d heads, at most %d each", who,
                  n_frames, n_heads, DAD3D_FRAME_MAX_COUNT);
    int total_tiles = 0;
    if (n_frames > 0 && n_heads > 0 && frames_host)
        if (dad3d_status st = frames_check_shapes(who, frames_host, n_frames, &total_tiles)) return st;
    DAD3D_REQUIRE(m, "%s: null handle", who);
    if (dad3d_status st = frames_arguments(who, m, frames, frames_host, n_frames, vertices, vertices, image_index, n_heads, flags, &total_tiles)) return st;
    if (total_tiles == 0) return DAD3D_OK;  // no frames or no heads
    if (m->ntri > 0) {
        DAD3D_REQUIRE(texture, "%s: null buffer", who);
        DAD3D_REQUIRE(m->d_tex_tri[DAD3D_TEX_INDEX_CORNER], "%s: no texture coordinates attached (dad3d_mesh_set_texcoords)", who);
        DAD3D_REQUIRE(m->d_tex_tri[indexing], "%s: reference indexing needs tex_coords rows of 3 floats, one for every vertex a triangle names", who);
    }
    DeviceGuard guard(m->device);
    if (dad3d_status st = m->frames_scratch(n_frames, n_heads, total_tiles)) return st;
    return launch_render_texture_frames(m->dev(), m->d_frames, frames, n_frames, total_tiles, vertices, m->d_tex_tri[indexing], texture,
                                        texture_dtype == DAD3D_DTYPE_U8, texture_batched ? (size_t)tex_h * tex_w * tex_c : 0, tex_h, tex_w, tex_c,
                                        mapping_type == 0, image_index, n_heads, flags, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_mesh_frames_scratch_bytes(dad3d_mesh* m, size_t* bytes) {
    DAD3D_REQUIRE(m && bytes, "dad3d_mesh_frames_scratch_bytes: bad argument");
    *bytes = m->frames_bytes;
    return DAD3D_OK;
}

dad3d_status dad3d_mesh_rasterize_triangles(dad3d_mesh* m, const float* vertices, float* depth, int32_t* tri_buf,
                                            float* bary, int batch, int h, int w, void* stream) {
    DAD3D_REQUIRE(m && batch >= 0 && h >= 0 && w >= 0, "dad3d_mesh_rasterize_triangles: bad argument");
    if (batch == 0 || h == 0 || w == 0) return DAD3D_OK;
    DAD3D_REQUIRE(depth && tri_buf && bary && (vertices || m->ntri == 0), "dad3d_mesh_rasterize_triangles: null buffer");
    DeviceGuard guard(m->device);
    if (dad3d_status st = m->raster_scratch(batch, h, w, static_cast<hipStream_t>(stream))) return st;
    return launch_rasterize(m->dev(), m->nc, m->d_raster, m->d_trace, nullptr, vertices, nullptr, depth, tri_buf, bary, batch, h, w, 3, 0, 1,
                            nullptr, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_mesh_set_texcoords(dad3d_mesh* m, const float* tex_coords, int n_tex, int stride, const int32_t* tex_triangles) {
    DAD3D_REQUIRE(m, "dad3d_mesh_set_texcoords: null handle");
    DAD3D_REQUIRE(stride == 2 || stride == 3, "dad3d_mesh_set_texcoords: tex_coords rows of 2 or 3 floats, got %d", stride);
    DAD3D_REQUIRE(n_tex >= 0 && (tex_coords || n_tex == 0) && (tex_triangles || m->ntri == 0), "dad3d_mesh_set_texcoords: bad argument");
    const size_t nt = (size_t)m->ntri;
    for (size_t i = 0; i < 3 * nt; ++i)
        DAD3D_REQUIRE(tex_triangles[i] >= 0 && tex_triangles[i] < n_tex, "texture triangle index %d out of range [0,%d)", tex_triangles[i], n_tex);
    // reference indexing (rasterize_kernel.cpp:398-403) reads row tri[i] of tex_coords for y: possible when every mesh index is a row
    bool ref_ok = stride == 3;
    for (size_t i = 0; i < 3 * nt && ref_ok; ++i) ref_ok = m->h_tri[i] < n_tex;
    std::vector<float4> corner(2 * nt), ref(ref_ok ? 2 * nt : 0);
    for (size_t f = 0; f < nt; ++f) {
        float cx[3], cy[3], ry[3];
        for (int k = 0; k < 3; ++k) {
            const size_t t = (size_t)tex_triangles[3 * f + k];
            cx[k] = tex_coords[stride * t], cy[k] = tex_coords[stride * t + 1];
            ry[k] = ref_ok ? tex_coords[stride * (size_t)m->h_tri[3 * f + k] + 1] : 0.0f;
        }
        corner[2 * f] = make_float4(cx[0], cy[0], cx[1], cy[1]);
        corner[2 * f + 1] = make_float4(cx[2], cy[2], 0.0f, 0.0f);
        if (ref_ok) {
            ref[2 * f] = make_float4(cx[0], ry[0], cx[1], ry[1]);
            ref[2 * f + 1] = make_float4(cx[2], ry[2], 0.0f, 0.0f);
        }
    }
    DeviceGuard guard(m->device);
    DAD3D_HIP_TRY(hipDeviceSynchronize());  // a launch in flight may still read the tables being replaced
    for (float4*& p : m->d_tex_tri) {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
    if (nt == 0) return DAD3D_OK;
    if (dad3d_status st = upload(&m->d_tex_tri[DAD3D_TEX_INDEX_CORNER], corner)) return st;
    return ref_ok ? upload(&m->d_tex_tri[DAD3D_TEX_INDEX_REFERENCE], ref) : DAD3D_OK;
}

dad3d_status dad3d_mesh_render_texture(dad3d_mesh* m, void* image, int image_dtype, const float* vertices, const void* texture,
                                       int texture_dtype, int texture_batched, float* depth, int batch, int h, int w, int c, int tex_h,
                                       int tex_w, int tex_c, int mapping_type, int indexing, void* stream) {
    // the scalar arguments first: a bad one is refused before the handle is looked at or any device work starts
    DAD3D_REQUIRE(batch >= 0 && h >= 0 && w >= 0, "dad3d_mesh_render_texture: negative batch or image size");
    DAD3D_REQUIRE((image_dtype == DAD3D_DTYPE_F32 || image_dtype == DAD3D_DTYPE_U8) && (texture_dtype == DAD3D_DTYPE_F32 || texture_dtype == DAD3D_DTYPE_U8),
                  "dad3d_mesh_render_texture: image and texture are float32 (DAD3D_DTYPE_F32) or uint8 (DAD3D_DTYPE_U8)");
    DAD3D_REQUIRE(tex_h >= 1 && tex_w >= 1 && tex_c >= 1 && (size_t)tex_h * tex_w * tex_c < (1ull << 31), "dad3d_mesh_render_texture: texture of %d x %d x %d", tex_h, tex_w, tex_c);
    DAD3D_REQUIRE(c >= 1 && c <= 4 && c <= tex_c, "dad3d_mesh_render_texture: c = %d channels, need 1..4 and at most tex_c = %d", c, tex_c);
    DAD3D_REQUIRE(indexing == DAD3D_TEX_INDEX_CORNER || indexing == DAD3D_TEX_INDEX_REFERENCE, "dad3d_mesh_render_texture: unknown indexing mode %d", indexing);
    DAD3D_REQUIRE(m, "dad3d_mesh_render_texture: null handle");
    if (batch == 0 || h == 0 || w == 0 || m->ntri == 0) return DAD3D_OK;
    DAD3D_REQUIRE(image && vertices && texture, "dad3d_mesh_render_texture: null buffer");
    DAD3D_REQUIRE(m->d_tex_tri[DAD3D_TEX_INDEX_CORNER], "dad3d_mesh_render_texture: no texture coordinates attached (dad3d_mesh_set_texcoords)");
    DAD3D_REQUIRE(m->d_tex_tri[indexing], "dad3d_mesh_render_texture: reference indexing needs tex_coords rows of 3 floats, one for every vertex a triangle names");
    DeviceGuard guard(m->device);
    if (dad3d_status st = m->raster_scratch(batch, h, w, static_cast<hipStream_t>(stream))) return st;
    return launch_render_texture(m->dev(), m->d_raster, image, image_dtype == DAD3D_DTYPE_U8, vertices, m->d_tex_tri[indexing], texture,
                                 texture_dtype == DAD3D_DTYPE_U8, texture_batched ? (size_t)tex_h * tex_w * tex_c : 0, depth, batch, h, w, c, tex_h,
                                 tex_w, tex_c, mapping_type == 0, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_project_vertices(const float* vertices, const float* model_view, const float* projection,
                                    const float* frame, int batch, int nver, float* world_homo, float* xy,
                                    int32_t* xy_int, int device, void* stream) {
    DAD3D_REQUIRE(batch >= 0 && nver >= 0, "dad3d_project_vertices: bad argument");
    DAD3D_REQUIRE(batch <= 65535, "dad3d_project_vertices: batch %d beyond the launch grid", batch);
    if (batch == 0 || nver == 0) return DAD3D_OK;
    DAD3D_REQUIRE(vertices && model_view && projection && frame, "dad3d_project_vertices: null input");
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    return launch_project_vertices(vertices, model_view, projection, frame, batch, nver, world_homo, xy, xy_int,
                                   static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_gt_keypoints(const float* vertices, const float* model_view, const float* projection,
                                const int32_t* frames, int batch, int nver, const int32_t* index, const int32_t* corners,
                                const float* weights, int n_subset, int out_size, int resize_mode, float* full, float* subset_px,
                                float* subset_norm, uint8_t* presence, int device, void* stream) {
    DAD3D_REQUIRE(batch >= 0 && nver >= 0 && n_subset >= 0 && out_size > 0, "dad3d_gt_keypoints: bad argument");
    DAD3D_REQUIRE(resize_mode == DAD3D_RESIZE_LONGEST_MAX_SIZE || resize_mode == DAD3D_RESIZE_RESIZE,
                  "dad3d_gt_keypoints: unknown resize mode %d", resize_mode);
    DAD3D_REQUIRE(batch <= 65535, "dad3d_gt_keypoints: batch %d beyond the launch grid", batch);
    DAD3D_REQUIRE((long long)nver + n_subset <= 0x7fffff00LL, "dad3d_gt_keypoints: %d + %d points beyond the launch grid", nver,
                  n_subset);
    DAD3D_REQUIRE(n_subset == 0 || ((index != nullptr) != (corners != nullptr) && (corners == nullptr) == (weights == nullptr)),
                  "dad3d_gt_keypoints: give either index or corners + weights for the subset");
    if (batch == 0 || nver + n_subset == 0) return DAD3D_OK;
    DAD3D_REQUIRE(vertices && model_view && projection && frames, "dad3d_gt_keypoints: null input");
    DAD3D_REQUIRE((nver == 0 || full) && (n_subset == 0 || (subset_px && subset_norm && presence)), "dad3d_gt_keypoints: null output");
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    GtKeypointsArgs a{vertices, model_view, projection, frames, index, corners, weights, full, subset_px, subset_norm, presence,
                      nver, n_subset, out_size, resize_mode};
    return launch_gt_keypoints(a, batch, static_cast<hipStream_t>(stream));
}

size_t dad3d_obj_format_scratch_bytes(int batch, int nver) {
    return batch < 0 || nver < 0 ? 0 : obj_format_scratch_bytes(batch, nver);
}

dad3d_status dad3d_obj_format_vertices(const float* vertices, int batch, int nver, uint8_t* text, size_t text_stride, int64_t* lengths,
                                       int32_t* flags, void* scratch, size_t scratch_bytes, int device, void* stream) {
    DAD3D_REQUIRE(batch >= 0 && nver >= 0, "dad3d_obj_format_vertices: bad argument");
    DAD3D_REQUIRE(batch <= 65535 && nver <= 0x7fffffff / DAD3D_OBJ_MAX_LINE_BYTES, "dad3d_obj_format_vertices: batch %d / %d vertices beyond the launch grid",
                  batch, nver);
    if (batch == 0) return DAD3D_OK;
    DAD3D_REQUIRE((vertices || nver == 0) && text && lengths && flags && scratch, "dad3d_obj_format_vertices: null argument");
    DAD3D_REQUIRE(text_stride >= (size_t)nver * DAD3D_OBJ_MAX_LINE_BYTES, "dad3d_obj_format_vertices: text_stride %zu is below the worst case of %d vertices (%zu bytes)",
                  text_stride, nver, (size_t)nver * DAD3D_OBJ_MAX_LINE_BYTES);
    DAD3D_REQUIRE(text_stride % 16 == 0 && (reinterpret_cast<uintptr_t>(text) & 15) == 0, "dad3d_obj_format_vertices: text and text_stride must be 16-byte aligned");
    DAD3D_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7) == 0 && (reinterpret_cast<uintptr_t>(lengths) & 7) == 0 && (reinterpret_cast<uintptr_t>(flags) & 3) == 0,
                  "dad3d_obj_format_vertices: lengths / flags / scratch are misaligned");
    DAD3D_REQUIRE(scratch_bytes >= obj_format_scratch_bytes(batch, nver), "dad3d_obj_format_vertices: %zu bytes of scratch, %zu needed", scratch_bytes,
                  obj_format_scratch_bytes(batch, nver));
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    ObjFormatArgs a{vertices, text, text_stride, lengths, flags, scratch, batch, nver};
    return launch_obj_format(a, static_cast<hipStream_t>(stream));
}

size_t dad3d_json_format_scratch_bytes(int batch, int n_slots) {
    return batch < 1 || n_slots < 1 ? 0 : json_format_scratch_bytes(batch, n_slots);
}

dad3d_status dad3d_json_format_values(const float* values, int batch, int n_slots, const void* literals, const int32_t* literal_offsets,
                                      uint8_t* text, size_t text_stride, int64_t* lengths, int32_t* flags, void* scratch,
                                      size_t scratch_bytes, int device, void* stream) {
    DAD3D_REQUIRE(batch > 0 && n_slots > 0, "dad3d_json_format_values: batch %d and n_slots %d must be positive", batch, n_slots);
    DAD3D_REQUIRE(batch <= 65535 && n_slots <= 0x7fffffff / (DAD3D_JSON_MAX_LITERAL_BYTES + DAD3D_JSON_MAX_NUMBER_BYTES) - 1,
                  "dad3d_json_format_values: batch %d / %d slots beyond the launch grid", batch, n_slots);
    DAD3D_REQUIRE(values && literals && literal_offsets && text && lengths && flags && scratch, "dad3d_json_format_values: null argument");
    DAD3D_REQUIRE(literal_offsets[0] == 0, "dad3d_json_format_values: literal_offsets must start at 0");
    for (int i = 0; i <= n_slots; ++i) {
        const long long len = (long long)literal_offsets[i + 1] - literal_offsets[i];
        DAD3D_REQUIRE(len >= 0 && len <= DAD3D_JSON_MAX_LITERAL_BYTES, "dad3d_json_format_values: literal %d is %lld bytes long (0 .. %d allowed)", i,
                      len, DAD3D_JSON_MAX_LITERAL_BYTES);
    }
    const size_t worst = (size_t)literal_offsets[n_slots + 1] + (size_t)n_slots * DAD3D_JSON_MAX_NUMBER_BYTES;
    DAD3D_REQUIRE(text_stride >= worst, "dad3d_json_format_values: text_stride %zu is below the worst case of the template (%zu bytes)", text_stride,
                  worst);
    DAD3D_REQUIRE(text_stride % 16 == 0 && (reinterpret_cast<uintptr_t>(text) & 15) == 0, "dad3d_json_format_values: text and text_stride must be 16-byte aligned");
    DAD3D_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7) == 0 && (reinterpret_cast<uintptr_t>(lengths) & 7) == 0 &&
                      (reinterpret_cast<uintptr_t>(flags) & 3) == 0 && (reinterpret_cast<uintptr_t>(literals) & 3) == 0 &&
                      (reinterpret_cast<uintptr_t>(values) & 3) == 0,
                  "dad3d_json_format_values: values / literals / lengths / flags / scratch are misaligned");
    DAD3D_REQUIRE(scratch_bytes >= json_format_scratch_bytes(batch, n_slots), "dad3d_json_format_values: %zu bytes of scratch, %zu needed", scratch_bytes,
                  json_format_scratch_bytes(batch, n_slots));
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    JsonFormatArgs a{values, literals, text, text_stride, lengths, flags, scratch, batch, n_slots};
    return launch_json_format(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_json_number_host(const float* values, size_t n, uint8_t* out, size_t out_stride, int32_t* lengths) {
    if (n == 0) return DAD3D_OK;
    DAD3D_REQUIRE(values && out && lengths, "dad3d_json_number_host: null argument");
    DAD3D_REQUIRE(out_stride >= DAD3D_JSON_MAX_NUMBER_BYTES, "dad3d_json_number_host: out_stride %zu is below the longest number (%d bytes)", out_stride,
                  DAD3D_JSON_MAX_NUMBER_BYTES);
    json_number_host(values, n, out, out_stride, lengths);
    return DAD3D_OK;
}

static bool png_shape_ok(int h, int w, int c) {
    return h >= 1 && w >= 1 && c >= 1 && c <= 4 && (long long)w * c < 0x7fffffffll && png_stream_bytes(h, w, c) < 0x80000000ll;
}

size_t dad3d_png_max_bytes(int h, int w, int c) { return png_shape_ok(h, w, c) ? png_max_bytes(h, w, c) : 0; }

size_t dad3d_png_scratch_bytes(int batch, int h, int w, int c) {
    return batch >= 1 && batch <= 65535 && png_shape_ok(h, w, c) ? png_scratch_bytes(batch, h, w, c) : 0;
}

size_t dad3d_zlib_max_bytes(int64_t n) { return n >= 1 && n < 0x80000000ll ? zlib_max_bytes(n) : 0; }

size_t dad3d_zlib_scratch_bytes(int batch, int64_t n) {
    return batch >= 1 && batch <= 65535 && n >= 1 && n < 0x80000000ll ? zlib_scratch_bytes(batch, n) : 0;
}

static dad3d_status deflate_checked(const char* who, DeflateArgs& a, size_t max_bytes, size_t need_scratch, size_t scratch_bytes, int device,
                                    void* stream) {
    DAD3D_REQUIRE(a.batch >= 1 && a.batch <= 65535, "%s: batch %d outside 1 .. 65535", who, a.batch);
    DAD3D_REQUIRE(a.data && a.out && a.lengths && a.flags && a.scratch, "%s: null argument", who);
    DAD3D_REQUIRE(a.out_stride >= max_bytes, "%s: out_stride %zu is below the worst case of the shape (%zu bytes)", who, a.out_stride, max_bytes);
    DAD3D_REQUIRE(a.out_stride % 16 == 0 && (reinterpret_cast<uintptr_t>(a.out) & 15) == 0, "%s: out and out_stride must be 16-byte aligned", who);
    DAD3D_REQUIRE((reinterpret_cast<uintptr_t>(a.scratch) & 15) == 0 && (reinterpret_cast<uintptr_t>(a.lengths) & 7) == 0 &&
                      (reinterpret_cast<uintptr_t>(a.flags) & 3) == 0,
                  "%s: lengths / flags / scratch are misaligned", who);
    DAD3D_REQUIRE(scratch_bytes >= need_scratch, "%s: %zu bytes of scratch, %zu needed", who, scratch_bytes, need_scratch);
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    return launch_deflate(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_png_encode(const uint8_t* images, int batch, int h, int w, int c, uint8_t* out, size_t out_stride, int64_t* lengths,
                              int32_t* flags, void* scratch, size_t scratch_bytes, int device, void* stream) {
    DAD3D_REQUIRE(c >= 1 && c <= 4, "dad3d_png_encode: %d channels (1 .. 4: grey, grey + alpha, RGB, RGBA)", c);
    DAD3D_REQUIRE(h >= 1 && w >= 1, "dad3d_png_encode: an image of %d x %d", h, w);
    DAD3D_REQUIRE(png_shape_ok(h, w, c), "dad3d_png_encode: the filtered stream of a %d x %d x %d image passes 2^31 bytes", h, w, c);
    DAD3D_REQUIRE(batch >= 1 && batch <= 65535, "dad3d_png_encode: batch %d outside 1 .. 65535", batch);
    DeflateArgs a{images, out, out_stride, lengths, flags, scratch, 0, batch, 1, h, w, c};
    return deflate_checked("dad3d_png_encode", a, png_max_bytes(h, w, c), png_scratch_bytes(batch, h, w, c), scratch_bytes, device, stream);
}

dad3d_status dad3d_zlib_compress(const uint8_t* data, int batch, int64_t n, uint8_t* out, size_t out_stride, int64_t* lengths, int32_t* flags,
                                 void* scratch, size_t scratch_bytes, int device, void* stream) {
    DAD3D_REQUIRE(n >= 1 && n < 0x80000000ll, "dad3d_zlib_compress: a stream of %lld bytes (1 .. 2^31 - 1)", (long long)n);
    DAD3D_REQUIRE(batch >= 1 && batch <= 65535, "dad3d_zlib_compress: batch %d outside 1 .. 65535", batch);
    DeflateArgs a{data, out, out_stride, lengths, flags, scratch, n, batch, 0, 0, 0, 0};
    return deflate_checked("dad3d_zlib_compress", a, zlib_max_bytes(n), zlib_scratch_bytes(batch, n), scratch_bytes, device, stream);
}

dad3d_status dad3d_deflate_tables_host(const uint32_t* ll_hist, const uint32_t* d_hist, uint8_t* ll_len, uint8_t* d_len, uint8_t* cl_len,
                                       uint16_t* ll_code, uint16_t* d_code, uint16_t* cl_code, uint8_t* header, int32_t* header_bits,
                                       uint32_t* dynamic_bits, uint32_t* fixed_bits) {
    DAD3D_REQUIRE(ll_hist && d_hist && ll_len && d_len && cl_len && ll_code && d_code && cl_code && header && header_bits && dynamic_bits && fixed_bits,
                  "dad3d_deflate_tables_host: null argument");
    unsigned long long total = 0;
    for (int i = 0; i < 286 + 30; ++i) {
        const uint32_t v = i < 286 ? ll_hist[i] : d_hist[i - 286];
        DAD3D_REQUIRE(v < (1u << 22), "dad3d_deflate_tables_host: a count of %u (below 2^22)", v);
        total += v;
    }
    DAD3D_REQUIRE(total < (1ull << 26), "dad3d_deflate_tables_host: %llu symbols in one block (below 2^26)", total);
    return deflate_tables_host(ll_hist, d_hist, ll_len, d_len, cl_len, ll_code, d_code, cl_code, header, header_bits, dynamic_bits, fixed_bits);
}

size_t dad3d_png_decode_scratch_bytes(int64_t* desc, int batch, int32_t* max_segments) {
    if (!desc || !max_segments || batch < 1 || batch > 65535) return 0;
    static_assert(sizeof(long long) == sizeof(int64_t), "descriptor rows");
    int most = 0;
    const size_t bytes = png_decode_layout(reinterpret_cast<long long*>(desc), batch, &most);
    *max_segments = most;
    return bytes;
}

dad3d_status dad3d_png_decode(const uint8_t* files, size_t files_bytes, const int64_t* desc, int batch, int max_segments, uint8_t* out,
                              size_t out_bytes, int32_t* flags, int32_t* info, void* scratch, size_t scratch_bytes, int force_general, int device,
                              void* stream) {
    DAD3D_REQUIRE(batch >= 1 && batch <= 65535, "dad3d_png_decode: batch %d outside 1 .. 65535", batch);
    DAD3D_REQUIRE(files && desc && out && flags && info && scratch, "dad3d_png_decode: null argument");
    DAD3D_REQUIRE(max_segments >= 1 && max_segments <= (1 << 18), "dad3d_png_decode: max_segments %d outside 1 .. 2^18", max_segments);
    DAD3D_REQUIRE(reinterpret_cast<uintptr_t>(scratch) % 16 == 0 && reinterpret_cast<uintptr_t>(desc) % 8 == 0,
                  "dad3d_png_decode: scratch must be 16-byte aligned, desc 8-byte aligned");
    DAD3D_REQUIRE(scratch_bytes >= (size_t)batch * 16, "dad3d_png_decode: %zu bytes of scratch for a batch of %d", scratch_bytes, batch);
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    PngDecodeArgs a{files, files_bytes, reinterpret_cast<const long long*>(desc), batch, max_segments, force_general ? 1 : 0, out, out_bytes,
                    flags, info, static_cast<unsigned char*>(scratch), scratch_bytes};
    return launch_png_decode(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_zlib_decompress(const uint8_t* streams, size_t streams_bytes, const int64_t* desc, int batch, uint8_t* out, size_t out_bytes,
                                   int64_t* lengths, int32_t* flags, int device, void* stream) {
    DAD3D_REQUIRE(batch >= 1 && batch <= 65535, "dad3d_zlib_decompress: batch %d outside 1 .. 65535", batch);
    DAD3D_REQUIRE(streams && desc && out && lengths && flags, "dad3d_zlib_decompress: null argument");
    DAD3D_REQUIRE(reinterpret_cast<uintptr_t>(out) % 16 == 0 && reinterpret_cast<uintptr_t>(desc) % 8 == 0,
                  "dad3d_zlib_decompress: out must be 16-byte aligned, desc 8-byte aligned");
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    ZlibDecompressArgs a{streams, streams_bytes, reinterpret_cast<const long long*>(desc), batch, out, out_bytes, lengths, flags};
    return launch_zlib_decompress(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_inflate_host(const uint8_t* const* ranges, const int64_t* range_bytes, int n_ranges, uint8_t* out, int64_t capacity,
                                int64_t* length, int32_t* flag) {
    DAD3D_REQUIRE(n_ranges >= 0 && (n_ranges == 0 || (ranges && range_bytes)) && length && flag && capacity >= 0 && (out || capacity == 0),
                  "dad3d_inflate_host: null or negative argument");
    for (int i = 0; i < n_ranges; ++i)
        DAD3D_REQUIRE(range_bytes[i] >= 0 && (ranges[i] || range_bytes[i] == 0), "dad3d_inflate_host: range %d of %lld bytes", i, (long long)range_bytes[i]);
    long long n = 0;
    *flag = inflate_host(ranges, reinterpret_cast<const long long*>(range_bytes), n_ranges, out, capacity, &n);
    *length = n;
    return DAD3D_OK;
}

size_t dad3d_jpeg_decode_scratch_bytes(int64_t* desc, int batch, int32_t* grid) {
    if (!desc || !grid || batch < 1 || batch > 65535) return 0;
    int dims[DAD3D_JPEG_DECODE_GRID_INTS] = {0, 0, 0};
    const size_t bytes = jpeg_decode_layout(reinterpret_cast<long long*>(desc), batch, dims);
    for (int i = 0; i < DAD3D_JPEG_DECODE_GRID_INTS; ++i) grid[i] = dims[i];
    return bytes;
}

dad3d_status dad3d_jpeg_decode(const uint8_t* files, size_t files_bytes, const int64_t* desc, int batch, const int32_t* grid, uint8_t* out,
                               size_t out_bytes, int32_t* flags, void* scratch, size_t scratch_bytes, int device, void* stream) {
    DAD3D_REQUIRE(batch >= 1 && batch <= 65535, "dad3d_jpeg_decode: batch %d outside 1 .. 65535", batch);
    DAD3D_REQUIRE(files && desc && grid && out && flags && scratch, "dad3d_jpeg_decode: null argument");
    DAD3D_REQUIRE(grid[0] >= 1 && grid[0] <= (1 << 22) && grid[1] >= 1 && grid[1] <= (1 << 22) && grid[2] >= 1 && grid[2] <= (1 << 28),
                  "dad3d_jpeg_decode: a grid of %d segments, %d blocks, %d pixels (dad3d_jpeg_decode_scratch_bytes gives it)", grid[0], grid[1], grid[2]);
    DAD3D_REQUIRE((long long)batch * ((grid[0] + 62) / 64) + (batch + 63) / 64 <= 0x7fffffffll, "dad3d_jpeg_decode: %d files of up to %d segments pass the grid",
                  batch, grid[0]);
    DAD3D_REQUIRE(reinterpret_cast<uintptr_t>(scratch) % 16 == 0 && reinterpret_cast<uintptr_t>(desc) % 8 == 0,
                  "dad3d_jpeg_decode: scratch must be 16-byte aligned, desc 8-byte aligned");
    DAD3D_REQUIRE(scratch_bytes >= (size_t)batch * jpeg_decode_state_bytes(), "dad3d_jpeg_decode: %zu bytes of scratch for a batch of %d", scratch_bytes,
                  batch);
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    JpegDecodeArgs a{files, files_bytes, reinterpret_cast<const long long*>(desc), batch, grid[0], grid[1], grid[2], out, out_bytes,
                     flags, static_cast<unsigned char*>(scratch), scratch_bytes};
    return launch_jpeg_decode(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_jpeg_decode_host(const uint8_t* file, int64_t size, int channels, uint8_t* out, int64_t out_bytes, int32_t* h, int32_t* w,
                                    int32_t* c, int32_t* flag) {
    DAD3D_REQUIRE(size >= 0 && (file || size == 0) && h && w && c && flag && out_bytes >= 0, "dad3d_jpeg_decode_host: null or negative argument");
    DAD3D_REQUIRE(channels == 0 || channels == 1 || channels == 3, "dad3d_jpeg_decode_host: %d channels (0 the file's own, 1, 3)", channels);
    int hh = 0, ww = 0, cc = 0;
    bool fits = true;
    *flag = jpeg_decode_host(file, size, channels, out, out_bytes, &hh, &ww, &cc, &fits);
    *h = hh, *w = ww, *c = cc;
    DAD3D_REQUIRE(fits, "dad3d_jpeg_decode_host: a %d x %d x %d image does not fit %lld bytes", hh, ww, cc, (long long)out_bytes);
    return DAD3D_OK;
}

size_t dad3d_jpeg_decode_sync_scratch_bytes(int64_t* desc, int batch, int32_t* grid, int piece_bytes) {
    if (!desc || !grid || batch < 1 || batch > 65535) return 0;
    int dims[DAD3D_JPEG_DECODE_SYNC_GRID_INTS] = {0, 0, 0, 0};
    const size_t bytes = jpeg_decode_sync_layout(reinterpret_cast<long long*>(desc), batch, dims, piece_bytes);
    for (int i = 0; i < DAD3D_JPEG_DECODE_SYNC_GRID_INTS; ++i) grid[i] = dims[i];
    return bytes;
}

dad3d_status dad3d_jpeg_decode_sync(const uint8_t* files, size_t files_bytes, const int64_t* desc, int batch, const int32_t* grid, int piece_bytes,
                                    uint8_t* out, size_t out_bytes, int32_t* flags, int32_t* info, void* scratch, size_t scratch_bytes, int device,
                                    void* stream) {
    DAD3D_REQUIRE(piece_bytes >= 16 && piece_bytes <= 256 && (piece_bytes & (piece_bytes - 1)) == 0,
                  "dad3d_jpeg_decode_sync: pieces of %d bytes (a power of two, 16 .. 256)", piece_bytes);
    DAD3D_REQUIRE(batch >= 1 && batch <= 65535, "dad3d_jpeg_decode_sync: batch %d outside 1 .. 65535", batch);
    DAD3D_REQUIRE(files && desc && grid && out && flags && info && scratch, "dad3d_jpeg_decode_sync: null argument");
    DAD3D_REQUIRE(grid[0] >= 1 && grid[0] <= (1 << 22) && grid[1] >= 1 && grid[1] <= (1 << 22) && grid[2] >= 1 && grid[2] <= (1 << 28) && grid[3] >= 1 &&
                      grid[3] <= (1 << 19),
                  "dad3d_jpeg_decode_sync: a grid of %d segments, %d blocks, %d pixels, %d groups (dad3d_jpeg_decode_sync_scratch_bytes gives it)", grid[0],
                  grid[1], grid[2], grid[3]);
    DAD3D_REQUIRE((long long)batch * grid[0] <= 64ll * 0x7fffffffll, "dad3d_jpeg_decode_sync: %d files of up to %d segments pass the grid", batch,
                  grid[0]);
    DAD3D_REQUIRE(reinterpret_cast<uintptr_t>(scratch) % 16 == 0 && reinterpret_cast<uintptr_t>(desc) % 8 == 0,
                  "dad3d_jpeg_decode_sync: scratch must be 16-byte aligned, desc 8-byte aligned");
    DAD3D_REQUIRE(scratch_bytes >= (size_t)batch * jpeg_decode_state_bytes(), "dad3d_jpeg_decode_sync: %zu bytes of scratch for a batch of %d",
                  scratch_bytes, batch);
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    JpegDecodeSyncArgs a{{files, files_bytes, reinterpret_cast<const long long*>(desc), batch, grid[0], grid[1], grid[2], out, out_bytes, flags,
                          static_cast<unsigned char*>(scratch), scratch_bytes},
                         piece_bytes, grid[3], info};
    return launch_jpeg_decode_sync(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_jpeg_decode_sync_host(const uint8_t* file, int64_t size, int channels, int piece_bytes, uint8_t* out, int64_t out_bytes, int32_t* h,
                                         int32_t* w, int32_t* c, int32_t* flag, int32_t* info) {
    DAD3D_REQUIRE(size >= 0 && (file || size == 0) && h && w && c && flag && info && out_bytes >= 0,
                  "dad3d_jpeg_decode_sync_host: null or negative argument");
    DAD3D_REQUIRE(channels == 0 || channels == 1 || channels == 3, "dad3d_jpeg_decode_sync_host: %d channels (0 the file's own, 1, 3)", channels);
    DAD3D_REQUIRE(piece_bytes >= 16 && piece_bytes <= 256 && (piece_bytes & (piece_bytes - 1)) == 0,
                  "dad3d_jpeg_decode_sync_host: pieces of %d bytes (a power of two, 16 .. 256)", piece_bytes);
    int hh = 0, ww = 0, cc = 0, what[4] = {0, 0, 0, 0};
    bool fits = true;
    *flag = jpeg_decode_host(file, size, channels, out, out_bytes, &hh, &ww, &cc, &fits, piece_bytes, what);
    *h = hh, *w = ww, *c = cc;
    for (int i = 0; i < 4; ++i) info[i] = what[i];
    DAD3D_REQUIRE(fits, "dad3d_jpeg_decode_sync_host: a %d x %d x %d image does not fit %lld bytes", hh, ww, cc, (long long)out_bytes);
    return DAD3D_OK;
}

size_t dad3d_jpeg_max_bytes(int h, int w, int c, int subsampling) { return jpeg_encode_max_bytes(h, w, c, subsampling); }

size_t dad3d_jpeg_encode_scratch_bytes(int batch, int h, int w, int c, int subsampling) {
    return jpeg_encode_scratch_bytes(batch, h, w, c, subsampling);
}

static dad3d_status jpeg_encode_options_ok(const char* who, int h, int w, int c, int quality, int subsampling, int restart_interval) {
    DAD3D_REQUIRE(c == 1 || c == 3, "%s: %d channels (1 grey, 3 RGB)", who, c);
    DAD3D_REQUIRE(h >= 1 && w >= 1 && h <= 65535 && w <= 65535, "%s: an image of %d x %d (1 .. 65535)", who, h, w);
    DAD3D_REQUIRE(quality >= 1 && quality <= 100, "%s: quality %d outside 1 .. 100", who, quality);
    DAD3D_REQUIRE(subsampling >= 0 && subsampling <= 2, "%s: subsampling %d (0 4:4:4, 1 4:2:2, 2 4:2:0)", who, subsampling);
    DAD3D_REQUIRE(restart_interval >= 0 && restart_interval <= 65535, "%s: a restart interval of %d MCUs (0 .. 65535)", who, restart_interval);
    DAD3D_REQUIRE(jpeg_encode_max_bytes(h, w, c, subsampling) != 0, "%s: an image of %d x %d x %d has more than 2^22 blocks", who, h, w, c);
    return DAD3D_OK;
}

dad3d_status dad3d_jpeg_encode(const uint8_t* images, int batch, int h, int w, int c, int quality, int subsampling, int restart_interval,
                               uint8_t* out, size_t out_stride, int64_t* lengths, int32_t* flags, void* scratch, size_t scratch_bytes,
                               int device, void* stream) {
    const char* who = "dad3d_jpeg_encode";
    DAD3D_REQUIRE(images && out && lengths && flags && scratch, "%s: null argument", who);
    DAD3D_REQUIRE(batch >= 1 && batch <= 65535, "%s: batch %d outside 1 .. 65535", who, batch);
    if (const dad3d_status st = jpeg_encode_options_ok(who, h, w, c, quality, subsampling, restart_interval)) return st;
    const size_t worst = jpeg_encode_max_bytes(h, w, c, subsampling), need = jpeg_encode_scratch_bytes(batch, h, w, c, subsampling);
    DAD3D_REQUIRE(out_stride >= worst, "%s: out_stride %zu is below the worst case of the shape (%zu bytes)", who, out_stride, worst);
    DAD3D_REQUIRE(out_stride % 16 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0, "%s: out and out_stride must be 16-byte aligned", who);
    DAD3D_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 15) == 0 && (reinterpret_cast<uintptr_t>(lengths) & 7) == 0 &&
                      (reinterpret_cast<uintptr_t>(flags) & 3) == 0,
                  "%s: lengths / flags / scratch are misaligned", who);
    DAD3D_REQUIRE(scratch_bytes >= need, "%s: %zu bytes of scratch, %zu needed", who, scratch_bytes, need);
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    JpegEncodeArgs a{images, batch, h, w, c, quality, subsampling, restart_interval, out, out_stride, lengths, flags, scratch};
    return launch_jpeg_encode(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_jpeg_encode_host(const uint8_t* image, int h, int w, int c, int quality, int subsampling, int restart_interval, uint8_t* out,
                                    int64_t capacity, int64_t* length, int32_t* flag) {
    const char* who = "dad3d_jpeg_encode_host";
    DAD3D_REQUIRE(image && out && length && flag, "%s: null argument", who);
    if (const dad3d_status st = jpeg_encode_options_ok(who, h, w, c, quality, subsampling, restart_interval)) return st;
    DAD3D_REQUIRE(capacity >= (int64_t)jpeg_encode_max_bytes(h, w, c, subsampling), "%s: %lld bytes for a file of up to %zu", who,
                  (long long)capacity, jpeg_encode_max_bytes(h, w, c, subsampling));
    long long n = 0;
    *flag = jpeg_encode_host(image, h, w, c, quality, subsampling, restart_interval, out, capacity, &n);
    *length = n;
    return DAD3D_OK;
}

size_t dad3d_json_parse_scratch_bytes(int64_t n_bytes) {
    return n_bytes < 1 || n_bytes > 0x7fffffffLL ? 0 : json_parse_scratch_bytes(n_bytes);
}

namespace {
inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
}  // namespace

dad3d_status dad3d_json_parse_index(const uint8_t* text, int64_t n_bytes, void* scratch, size_t scratch_bytes, int32_t* counts, int device,
                                    void* stream) {
    DAD3D_REQUIRE(n_bytes > 0 && n_bytes <= 0x7fffffffLL, "dad3d_json_parse_index: n_bytes %lld must be in 1 .. 2^31 - 1", (long long)n_bytes);
    DAD3D_REQUIRE(text && scratch && counts, "dad3d_json_parse_index: null argument");
    DAD3D_REQUIRE(aligned_to(text, 16) && aligned_to(scratch, 16) && aligned_to(counts, 4), "dad3d_json_parse_index: text / scratch / counts are misaligned");
    DAD3D_REQUIRE(scratch_bytes >= json_parse_scratch_bytes(n_bytes), "dad3d_json_parse_index: %zu bytes of scratch, %zu needed", scratch_bytes,
                  json_parse_scratch_bytes(n_bytes));
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    return launch_json_parse_index(text, n_bytes, scratch, counts, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_json_parse_lists(const uint8_t* text, int64_t n_bytes, const void* scratch, size_t scratch_bytes, int32_t* tok_pos,
                                    int32_t* tok_brk, int64_t tok_cap, int32_t* brk_pos, int32_t* brk_key, int32_t* brk_nonnum, int32_t* brk_tok,
                                    int64_t brk_cap, int device, void* stream) {
    DAD3D_REQUIRE(n_bytes > 0 && n_bytes <= 0x7fffffffLL, "dad3d_json_parse_lists: n_bytes %lld must be in 1 .. 2^31 - 1", (long long)n_bytes);
    DAD3D_REQUIRE(tok_cap >= 0 && brk_cap >= 0, "dad3d_json_parse_lists: negative capacity");
    DAD3D_REQUIRE(text && scratch && (tok_cap == 0 || (tok_pos && tok_brk)) && (brk_cap == 0 || (brk_pos && brk_key && brk_nonnum && brk_tok)),
                  "dad3d_json_parse_lists: null argument");
    DAD3D_REQUIRE(aligned_to(scratch, 16) && aligned_to(tok_pos, 4) && aligned_to(tok_brk, 4) && aligned_to(brk_pos, 4) && aligned_to(brk_key, 4) &&
                      aligned_to(brk_nonnum, 4) && aligned_to(brk_tok, 4),
                  "dad3d_json_parse_lists: scratch / lists are misaligned");
    DAD3D_REQUIRE(scratch_bytes >= json_parse_scratch_bytes(n_bytes), "dad3d_json_parse_lists: %zu bytes of scratch, %zu needed", scratch_bytes,
                  json_parse_scratch_bytes(n_bytes));
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    JsonParseListsArgs a{scratch, tok_pos, tok_brk, brk_pos, brk_key, brk_nonnum, brk_tok, n_bytes, tok_cap, brk_cap};
    return launch_json_parse_lists(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_json_parse_check_arrays(const uint8_t* text, int64_t n_bytes, const int32_t* tok_pos, const int32_t* tok_brk, int64_t n_tokens,
                                           const int32_t* brk_pos, const int32_t* brk_key, const int32_t* brk_tok, int64_t n_brackets,
                                           const int32_t* arr_open, const int32_t* arr_close, int32_t* arr_rows, int64_t n_arrays, int device,
                                           void* stream) {
    DAD3D_REQUIRE(n_bytes > 0 && n_bytes <= 0x7fffffffLL, "dad3d_json_parse_check_arrays: n_bytes %lld must be in 1 .. 2^31 - 1", (long long)n_bytes);
    DAD3D_REQUIRE(n_tokens >= 0 && n_brackets >= 0 && n_arrays >= 0 && n_tokens <= n_bytes && n_brackets <= n_bytes && n_arrays <= n_brackets,
                  "dad3d_json_parse_check_arrays: %lld tokens / %lld brackets / %lld arrays do not fit a document of %lld bytes", (long long)n_tokens,
                  (long long)n_brackets, (long long)n_arrays, (long long)n_bytes);
    if (n_arrays == 0) return DAD3D_OK;
    DAD3D_REQUIRE(text && (n_tokens == 0 || (tok_pos && tok_brk)) && brk_pos && brk_key && brk_tok && arr_open && arr_close && arr_rows,
                  "dad3d_json_parse_check_arrays: null argument");
    DAD3D_REQUIRE(aligned_to(tok_pos, 4) && aligned_to(tok_brk, 4) && aligned_to(brk_pos, 4) && aligned_to(brk_key, 4) && aligned_to(brk_tok, 4) &&
                      aligned_to(arr_open, 4) && aligned_to(arr_close, 4) && aligned_to(arr_rows, 4),
                  "dad3d_json_parse_check_arrays: lists are misaligned");
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    JsonParseCheckArgs a{text, tok_pos, tok_brk, brk_pos, brk_key, brk_tok, arr_open, arr_close, arr_rows, n_bytes, n_tokens, n_brackets, n_arrays};
    return launch_json_parse_check_arrays(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_json_parse_extract(const uint8_t* text, int64_t n_bytes, const int32_t* tok_pos, int64_t n_tokens, const int32_t* records,
                                      int64_t n_records, int64_t n_values, double* values, uint8_t* is_int, int64_t values_cap, int device,
                                      void* stream) {
    DAD3D_REQUIRE(n_bytes > 0 && n_bytes <= 0x7fffffffLL, "dad3d_json_parse_extract: n_bytes %lld must be in 1 .. 2^31 - 1", (long long)n_bytes);
    DAD3D_REQUIRE(n_tokens >= 0 && n_records >= 0 && n_values >= 0 && n_tokens <= n_bytes && n_values <= n_tokens && n_records <= n_values,
                  "dad3d_json_parse_extract: %lld records / %lld values do not fit %lld tokens", (long long)n_records, (long long)n_values,
                  (long long)n_tokens);
    DAD3D_REQUIRE(values_cap >= n_values, "dad3d_json_parse_extract: room for %lld values, %lld needed", (long long)values_cap, (long long)n_values);
    if (n_values == 0) return DAD3D_OK;
    DAD3D_REQUIRE(n_records > 0, "dad3d_json_parse_extract: %lld values but no record", (long long)n_values);
    DAD3D_REQUIRE(text && tok_pos && records && values && is_int, "dad3d_json_parse_extract: null argument");
    DAD3D_REQUIRE(aligned_to(tok_pos, 4) && aligned_to(records, 4) && aligned_to(values, 8), "dad3d_json_parse_extract: lists / values are misaligned");
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    JsonParseExtractArgs a{text, tok_pos, records, values, is_int, n_bytes, n_tokens, n_records, n_values};
    return launch_json_parse_extract(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_json_parse_number_host(const uint8_t* text, const int64_t* starts, const int64_t* ends, size_t n, uint64_t* bits_out,
                                          uint8_t* is_int_out, uint32_t* flags_out) {
    if (n == 0) return DAD3D_OK;
    DAD3D_REQUIRE(text && starts && ends && bits_out && is_int_out && flags_out, "dad3d_json_parse_number_host: null argument");
    json_parse_number_host(text, reinterpret_cast<const long long*>(starts), reinterpret_cast<const long long*>(ends), n,
                           reinterpret_cast<unsigned long long*>(bits_out), is_int_out, flags_out);
    return DAD3D_OK;
}

dad3d_status dad3d_annotation_parse(const uint8_t* text, int64_t n_bytes, const int64_t* doc_offsets, const int64_t* doc_sizes, int batch, int n_verts,
                                    float* vertices, float* model_view, float* projection, int32_t* status, int device, void* stream) {
    DAD3D_REQUIRE(batch >= 0 && batch <= 65535, "dad3d_annotation_parse: batch %d outside 0 .. 65535", batch);
    DAD3D_REQUIRE(n_verts >= 1 && n_verts <= (1 << 24), "dad3d_annotation_parse: n_verts %d outside 1 .. 2^24", n_verts);
    DAD3D_REQUIRE(n_bytes >= 0 && n_bytes <= 0x7fffffffLL * 65535, "dad3d_annotation_parse: n_bytes %lld is negative or too large", (long long)n_bytes);
    if (batch == 0) return DAD3D_OK;
    DAD3D_REQUIRE(text && doc_offsets && doc_sizes && vertices && model_view && projection && status, "dad3d_annotation_parse: null argument");
    DAD3D_REQUIRE(aligned_to(text, 16) && aligned_to(doc_offsets, 8) && aligned_to(doc_sizes, 8) && aligned_to(vertices, 4) &&
                      aligned_to(model_view, 4) && aligned_to(projection, 4) && aligned_to(status, 4),
                  "dad3d_annotation_parse: text must be 16-byte aligned, the tables 8-byte, the outputs 4-byte aligned");
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    AnnotationParseArgs a{text, n_bytes, reinterpret_cast<const long long*>(doc_offsets), reinterpret_cast<const long long*>(doc_sizes), batch, n_verts,
                          vertices, model_view, projection, status};
    return launch_annotation_parse(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_preprocess_images(const int64_t* descs, int batch, int out_size, const float* mean, const float* std,
                                     float* out, int device, void* stream) {
    DAD3D_REQUIRE(batch >= 0 && out_size > 0, "dad3d_preprocess_images: bad argument");
    if (batch == 0) return DAD3D_OK;
    DAD3D_REQUIRE(descs && mean && std && out, "dad3d_preprocess_images: null argument");
    DAD3D_REQUIRE(batch <= 65535 && out_size <= 65535, "dad3d_preprocess_images: batch / size beyond the launch grid");
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    return launch_preprocess(reinterpret_cast<const long long*>(descs), batch, out_size, mean, std, out,
                             static_cast<hipStream_t>(stream));
}

static int dtype_vec(int dtype) { return dtype == DAD3D_DTYPE_F32 ? 4 : (dtype == DAD3D_DTYPE_F16 || dtype == DAD3D_DTYPE_BF16) ? 8 : 0; }

dad3d_status dad3d_nhwc_bias_act(void* y, const void* bias, const void* z, int64_t n_pixels, int channels, int dtype, int relu,
                                 int device, void* stream) {
    DAD3D_REQUIRE(n_pixels >= 0 && channels > 0 && dtype_vec(dtype), "dad3d_nhwc_bias_act: bad argument");
    if (n_pixels == 0) return DAD3D_OK;
    DAD3D_REQUIRE(y && bias, "dad3d_nhwc_bias_act: null tensor");
    DAD3D_REQUIRE(channels % dtype_vec(dtype) == 0, "dad3d_nhwc_bias_act: %d channels are not a multiple of %d (16 bytes)", channels, dtype_vec(dtype));
    DAD3D_REQUIRE((reinterpret_cast<uintptr_t>(y) & 15) == 0 && (reinterpret_cast<uintptr_t>(bias) & 15) == 0 &&
                      (reinterpret_cast<uintptr_t>(z) & 15) == 0, "dad3d_nhwc_bias_act: tensors must be 16-byte aligned");
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    return launch_nhwc_bias_act(y, bias, z, (size_t)n_pixels, channels, dtype, relu, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_nhwc_resize_sum(void* out, int n, int oh, int ow, int channels, int dtype, int n_inputs, const void* const* xs,
                                   const int* hs, const int* ws, const float* weights, int device, void* stream) {
    DAD3D_REQUIRE(n >= 0 && oh >= 0 && ow >= 0 && channels > 0 && dtype_vec(dtype) && n_inputs >= 1 && n_inputs <= 3,
                  "dad3d_nhwc_resize_sum: bad argument");
    if (n == 0 || oh == 0 || ow == 0) return DAD3D_OK;
    DAD3D_REQUIRE(out && xs && hs && ws && weights, "dad3d_nhwc_resize_sum: null argument");
    DAD3D_REQUIRE(channels % dtype_vec(dtype) == 0, "dad3d_nhwc_resize_sum: %d channels are not a multiple of %d (16 bytes)", channels, dtype_vec(dtype));
    DAD3D_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, "dad3d_nhwc_resize_sum: tensors must be 16-byte aligned");
    for (int j = 0; j < n_inputs; ++j)
        DAD3D_REQUIRE(xs[j] && hs[j] > 0 && ws[j] > 0 && (reinterpret_cast<uintptr_t>(xs[j]) & 15) == 0,
                      "dad3d_nhwc_resize_sum: input %d is null, empty or not 16-byte aligned", j);
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    return launch_nhwc_resize_sum(out, n, oh, ow, channels, dtype, n_inputs, xs, hs, ws, weights, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_heatmap_argmax(const void* heatmap, int dtype, int batch, int channels, int h, int w, int layout, int sigmoid,
                                  int32_t* yx_out, float* peak_out, int device, void* stream) {
    const int es = dtype == DAD3D_DTYPE_F32 ? 4 : (dtype == DAD3D_DTYPE_F16 || dtype == DAD3D_DTYPE_BF16) ? 2 : dtype == DAD3D_HEATMAP_DTYPE_U8 ? 1 : 0;
    DAD3D_REQUIRE(es, "dad3d_heatmap_argmax: unknown dtype %d", dtype);
    DAD3D_REQUIRE(layout == DAD3D_LAYOUT_NCHW || layout == DAD3D_LAYOUT_NHWC, "dad3d_heatmap_argmax: unknown layout %d", layout);
    DAD3D_REQUIRE(batch > 0 && channels > 0 && h > 0 && w > 0, "dad3d_heatmap_argmax: bad size (batch %d, channels %d, h %d, w %d)", batch,
                  channels, h, w);
    DAD3D_REQUIRE((int64_t)h * w <= (1 << 24), "dad3d_heatmap_argmax: a plane of %d x %d is beyond 2^24 positions", h, w);
    DAD3D_REQUIRE((int64_t)batch * channels <= 0x7fffffff, "dad3d_heatmap_argmax: %d x %d planes are beyond the launch grid", batch, channels);
    DAD3D_REQUIRE(!(sigmoid && dtype == DAD3D_HEATMAP_DTYPE_U8), "dad3d_heatmap_argmax: no sigmoid of a uint8 heatmap");
    DAD3D_REQUIRE(heatmap && yx_out, "dad3d_heatmap_argmax: null argument");
    DAD3D_REQUIRE(reinterpret_cast<uintptr_t>(heatmap) % es == 0, "dad3d_heatmap_argmax: the heatmap is not aligned to its %d-byte elements", es);
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    HeatmapArgmaxArgs a{heatmap, dtype, batch, channels, h, w, layout, sigmoid != 0, yx_out, peak_out, 1};
    return launch_heatmap_argmax(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_points_readjust(const void* src, int src_kind, int batch, int n_points, float mul, float limit, const double* geometry,
                                   int pad_left, int pad_top, double scale, int32_t* points_out, int device, void* stream) {
    DAD3D_REQUIRE(src_kind == DAD3D_POINTS_SRC_XY_F32 || src_kind == DAD3D_POINTS_SRC_YX_I32, "dad3d_points_readjust: unknown src_kind %d", src_kind);
    DAD3D_REQUIRE(batch > 0 && n_points > 0, "dad3d_points_readjust: bad size (batch %d, n_points %d)", batch, n_points);
    DAD3D_REQUIRE((int64_t)batch * n_points * 2 <= 0x7fffffff, "dad3d_points_readjust: %d x %d points are beyond the launch grid", batch, n_points);
    DAD3D_REQUIRE(src && points_out, "dad3d_points_readjust: null argument");
    DAD3D_REQUIRE(geometry || (scale > 0.0 && scale <= 1.7976931348623157e308), "dad3d_points_readjust: the scale must be a positive finite number");
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    PointsReadjustArgs a{src, src_kind, batch, n_points, mul, limit, geometry, pad_left, pad_top, scale, points_out};
    return launch_points_readjust(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_preprocess_boxes(const int64_t* images, int n_images, const void* boxes, int box_dtype, const int32_t* image_index,
                                    int n_boxes, const double* offset, int out_size, const float* mean, const float* std, int out_format,
                                    void* out, int32_t* crops, double* geometry, int32_t* flags, int device, void* stream) {
    DAD3D_REQUIRE(n_boxes >= 0 && n_boxes <= 65535 && out_size >= 1 && out_size <= 65535,
                  "dad3d_preprocess_boxes: %d boxes / size %d outside the launch grid (65535)", n_boxes, out_size);
    DAD3D_REQUIRE(box_dtype >= DAD3D_BOX_DTYPE_I32 && box_dtype <= DAD3D_BOX_DTYPE_F64, "dad3d_preprocess_boxes: unknown box_dtype %d", box_dtype);
    DAD3D_REQUIRE(out_format >= DAD3D_PREPROCESS_OUT_F32_NCHW && out_format <= DAD3D_PREPROCESS_OUT_BF16_NHWC,
                  "dad3d_preprocess_boxes: unknown out_format %d", out_format);
    if (n_boxes == 0) return DAD3D_OK;
    DAD3D_REQUIRE(n_images >= 1 && n_images <= 65535, "dad3d_preprocess_boxes: %d images outside 1 .. 65535", n_images);
    DAD3D_REQUIRE(images && boxes && image_index && mean && std && out && crops && geometry && flags, "dad3d_preprocess_boxes: null argument");
    DAD3D_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3) == 0, "dad3d_preprocess_boxes: out must be 4-byte aligned");
    PreprocessBoxesArgs a{};
    if (offset) {
        for (int k = 0; k < 4; ++k)
            DAD3D_REQUIRE(offset[k] - offset[k] == 0.0, "dad3d_preprocess_boxes: offset[%d] is not finite", k);
        a.has_offset = 1, a.left = offset[0], a.right = offset[1], a.top = offset[2], a.bottom = offset[3];
    }
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    a.images = reinterpret_cast<const long long*>(images), a.n_images = n_images;
    a.boxes = boxes, a.box_dtype = box_dtype, a.image_index = image_index, a.n_boxes = n_boxes;
    a.out_size = out_size, a.out_format = out_format, a.out = out, a.crops = crops, a.geometry = geometry, a.flags = flags;
    return launch_preprocess_boxes(a, mean, std, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_flame_readjust_params_frame(dad3d_flame* h, float* params, int batch, const double* geometry, void* stream) {
    DAD3D_REQUIRE(h && batch >= 0, "dad3d_flame_readjust_params_frame: bad argument");
    if (batch == 0) return DAD3D_OK;
    DAD3D_REQUIRE(params && geometry, "dad3d_flame_readjust_params_frame: null argument");
    DeviceGuard guard(h->device);
    return launch_readjust_frame(params, batch, h->lay, geometry, h->image_size, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_points_readjust_frame(const void* src, int src_kind, int batch, int n_points, float mul, float limit, const double* geometry,
                                         int32_t* points_out, int device, void* stream) {
    DAD3D_REQUIRE(src_kind == DAD3D_POINTS_SRC_XY_F32 || src_kind == DAD3D_POINTS_SRC_YX_I32, "dad3d_points_readjust_frame: unknown src_kind %d", src_kind);
    DAD3D_REQUIRE(batch > 0 && n_points > 0, "dad3d_points_readjust_frame: bad size (batch %d, n_points %d)", batch, n_points);
    DAD3D_REQUIRE((int64_t)batch * n_points * 2 <= 0x7fffffff, "dad3d_points_readjust_frame: %d x %d points are beyond the launch grid", batch, n_points);
    DAD3D_REQUIRE(src && points_out && geometry, "dad3d_points_readjust_frame: null argument");
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    PointsReadjustArgs a{src, src_kind, batch, n_points, mul, limit, geometry, 0, 0, 1.0, points_out};
    return launch_points_readjust_frame(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_boxes_from_heads(const float* proj, int n_heads, int n_verts, int64_t head_stride, int vertex_stride, const int32_t* subset,
                                    int n_subset, const int64_t* frames, int n_frames, const int32_t* image_index, const int32_t* prev_flags,
                                    int min_side, double min_visible, int32_t* boxes, int32_t* flags, int device, void* stream) {
    DAD3D_REQUIRE(n_heads >= 0 && n_heads <= 65535, "dad3d_boxes_from_heads: %d heads outside the launch grid (65535)", n_heads);
    DAD3D_REQUIRE(n_verts >= 1 && n_verts <= 65535, "dad3d_boxes_from_heads: %d vertices outside 1 .. 65535", n_verts);
    DAD3D_REQUIRE(vertex_stride >= 2, "dad3d_boxes_from_heads: a vertex stride of %d floats holds no (x, y)", vertex_stride);
    DAD3D_REQUIRE((subset == nullptr) == (n_subset == 0), "dad3d_boxes_from_heads: a subset and its count go together (NULL and 0 for all vertices)");
    DAD3D_REQUIRE(n_subset >= 0 && n_subset <= 65535, "dad3d_boxes_from_heads: %d subset indices outside 1 .. 65535", n_subset);
    DAD3D_REQUIRE(min_side >= 0, "dad3d_boxes_from_heads: min_side %d is negative", min_side);
    DAD3D_REQUIRE(min_visible >= 0.0 && min_visible <= 1.0, "dad3d_boxes_from_heads: min_visible %g is outside [0, 1]", min_visible);  // false for a NaN
    if (n_heads == 0) return DAD3D_OK;
    DAD3D_REQUIRE(n_frames >= 1 && n_frames <= 65535, "dad3d_boxes_from_heads: %d frames outside 1 .. 65535", n_frames);
    DAD3D_REQUIRE(proj && frames && image_index && boxes && flags, "dad3d_boxes_from_heads: null argument");
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    TrackBoxesArgs a{proj, n_heads, n_verts, (long long)head_stride, vertex_stride, subset, n_subset, reinterpret_cast<const long long*>(frames),
                     n_frames, image_index, prev_flags, min_side, min_visible, boxes, flags};
    return launch_boxes_from_heads(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_one_euro_rows(const float* x, int64_t x_stride, float* out, int64_t out_stride, int n, int d, const int32_t* flags,
                                 const float* min_cutoff, const float* beta, float rate, float two_pi_dt, float alpha_d, float* state_x,
                                 float* state_dx, int32_t* age, int device, void* stream) {
    DAD3D_REQUIRE(d >= 1 && n >= 0, "dad3d_one_euro_rows: bad size (n %d, d %d)", n, d);
    DAD3D_REQUIRE(x_stride >= d && out_stride >= d, "dad3d_one_euro_rows: a row stride (%lld, %lld) is below d = %d", (long long)x_stride,
                  (long long)out_stride, d);
    for (float v : {rate, two_pi_dt, alpha_d})  // false for a NaN
        DAD3D_REQUIRE(v > 0.0f && v - v == 0.0f, "dad3d_one_euro_rows: the scalar %g is not finite and positive", (double)v);
    DAD3D_REQUIRE(alpha_d <= 1.0f, "dad3d_one_euro_rows: alpha_d %g is above 1", (double)alpha_d);
    if (n == 0) return DAD3D_OK;
    DAD3D_REQUIRE(x && out && min_cutoff && beta && state_x && state_dx && age, "dad3d_one_euro_rows: null argument");
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    OneEuroArgs a{x, (long long)x_stride, out, (long long)out_stride, n, d, flags, min_cutoff, beta, rate, two_pi_dt, alpha_d, state_x, state_dx, age};
    return launch_one_euro_rows(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_track_suppress_duplicates(int32_t* boxes, int32_t* flags, const int32_t* image_index, int n, double merge_iou, int device,
                                             void* stream) {
    DAD3D_REQUIRE(merge_iou > 0.0 && merge_iou <= 1.0, "dad3d_track_suppress_duplicates: merge_iou %g is outside (0, 1]", merge_iou);  // false for a NaN
    DAD3D_REQUIRE(n >= 0 && n <= DAD3D_TRACK_MAX_SLOTS, "dad3d_track_suppress_duplicates: %d slots outside 0 .. %d", n, DAD3D_TRACK_MAX_SLOTS);
    if (n == 0) return DAD3D_OK;
    DAD3D_REQUIRE(boxes && flags && image_index, "dad3d_track_suppress_duplicates: null argument");
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    SuppressDuplicatesArgs a{boxes, flags, image_index, n, merge_iou};
    return launch_suppress_duplicates(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_track_assign_detections(int32_t* boxes, int32_t* flags, int32_t* image_index, int32_t* misses, int n, const int32_t* det_boxes,
                                           const int32_t* det_index, const int32_t* det_count, int m, const int32_t* frame_searched, int n_frames,
                                           double match_iou, int refresh, int max_misses, int32_t* assign, int32_t* det_flags, int32_t* spawned,
                                           int device, void* stream) {
    const char* who = "dad3d_track_assign_detections";
    DAD3D_REQUIRE(match_iou > 0.0 && match_iou <= 1.0, "%s: match_iou %g is outside (0, 1]", who, match_iou);  // false for a NaN
    DAD3D_REQUIRE(n >= 0 && n <= DAD3D_TRACK_MAX_SLOTS, "%s: %d slots outside 0 .. %d", who, n, DAD3D_TRACK_MAX_SLOTS);
    DAD3D_REQUIRE(m >= 0 && m <= DAD3D_TRACK_MAX_DETECTIONS, "%s: %d detections outside 0 .. %d", who, m, DAD3D_TRACK_MAX_DETECTIONS);
    DAD3D_REQUIRE(n_frames >= 1, "%s: %d frames", who, n_frames);
    DAD3D_REQUIRE(refresh == 0 || refresh == 1, "%s: refresh %d is neither 0 nor 1", who, refresh);
    DAD3D_REQUIRE(max_misses < 0 || misses || n == 0, "%s: max_misses %d needs the misses it counts", who, max_misses);
    DAD3D_REQUIRE(n == 0 || (boxes && flags && image_index && spawned), "%s: null slot argument", who);
    DAD3D_REQUIRE(m == 0 || (det_boxes && det_index && assign && det_flags), "%s: null detection argument", who);
    if (n == 0 && m == 0) return DAD3D_OK;
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    AssignDetectionsArgs a{boxes, flags, image_index, misses, n, det_boxes, det_index, det_count, m, frame_searched, n_frames, match_iou,
                           refresh, max_misses, assign, det_flags, spawned};
    return launch_assign_detections(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_cube_region_loss(const float* pred, const float* target, int batch, int n_verts,
                                    const int32_t* region_ptr, const int32_t* region_idx, const float* region_weight,
                                    int n_regions, const int32_t* vert_ptr, const int32_t* vert_region,
                                    const int32_t* vert_pos, int criterion, float* stats, float* loss_terms,
                                    float* grad_pred, int device, void* stream) {
    DAD3D_REQUIRE(batch >= 0 && n_verts >= 0 && n_regions >= 0, "dad3d_cube_region_loss: negative size");
    DAD3D_REQUIRE(criterion >= DAD3D_LOSS_L1 && criterion <= DAD3D_LOSS_SMOOTH_L1, "dad3d_cube_region_loss: unknown criterion %d", criterion);
    if (batch == 0 || n_regions == 0) return DAD3D_OK;
    DAD3D_REQUIRE(pred && target && region_ptr && region_idx && region_weight && stats && loss_terms,
                  "dad3d_cube_region_loss: null argument");
    DAD3D_REQUIRE(!grad_pred || (vert_ptr && vert_region && vert_pos), "dad3d_cube_region_loss: the gradient needs the vertex incidence list");
    DAD3D_REQUIRE(batch <= 65535 && n_regions <= 65535, "dad3d_cube_region_loss: batch / regions beyond the launch grid");
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    CubeLossArgs a{pred, target, region_ptr, region_idx, region_weight, vert_ptr, vert_region, vert_pos, stats, loss_terms,
                   grad_pred, batch, n_verts, n_regions, criterion};
    return launch_cube_loss(a, static_cast<hipStream_t>(stream));
}

int dad3d_point_loss_terms(int n_points) { return point_loss_blocks(n_points); }

dad3d_status dad3d_weighted_point_loss(const float* pred, const float* target, int batch, int n_points, int comps,
                                       const float* point_weight, float scale, int criterion, float* loss_terms,
                                       float* grad_pred, int device, void* stream) {
    DAD3D_REQUIRE(batch >= 0 && n_points >= 0 && comps > 0, "dad3d_weighted_point_loss: bad size");
    DAD3D_REQUIRE(criterion >= DAD3D_LOSS_L1 && criterion <= DAD3D_LOSS_SMOOTH_L1, "dad3d_weighted_point_loss: unknown criterion %d", criterion);
    if (batch == 0 || n_points == 0) return DAD3D_OK;
    DAD3D_REQUIRE(pred && target && point_weight && loss_terms, "dad3d_weighted_point_loss: null argument");
    DAD3D_REQUIRE(batch <= 65535, "dad3d_weighted_point_loss: batch beyond the launch grid");
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    PointLossArgs a{pred, target, point_weight, loss_terms, grad_pred, scale, batch, n_points, comps, criterion};
    return launch_point_loss(a, static_cast<hipStream_t>(stream));
}

// ---- the rest of the training objective (train_objective.hip) ----------------------------------------------------------
static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

dad3d_status dad3d_heatmap_encode(void* out, int form, const float* keypoints, const uint8_t* presence, int batch,
                                  int n_classes, float stride, int size, int radius, const void* table, int32_t* invalid,
                                  int device, void* stream) {
    DAD3D_REQUIRE(form >= DAD3D_HEATMAP_RAW && form <= DAD3D_HEATMAP_FLOAT, "dad3d_heatmap_encode: unknown form %d", form);
    DAD3D_REQUIRE(batch >= 0 && n_classes >= 0 && size >= 0, "dad3d_heatmap_encode: negative size");
    DAD3D_REQUIRE(size <= 46340, "dad3d_heatmap_encode: heatmap size %d beyond 46340", size);
    DAD3D_REQUIRE(radius >= 0 && radius <= 4096, "dad3d_heatmap_encode: radius %d outside 0..4096", radius);
    DAD3D_REQUIRE(std::isfinite(stride) && stride > 0.0f, "dad3d_heatmap_encode: stride must be finite and positive");
    if (batch == 0 || n_classes == 0 || size == 0) return DAD3D_OK;
    DAD3D_REQUIRE(out && keypoints && presence && table, "dad3d_heatmap_encode: null argument");
    DAD3D_REQUIRE(aligned16(out), "dad3d_heatmap_encode: the output must be 16-byte aligned");
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    HeatmapEncodeArgs a{out, keypoints, presence, table, invalid, (size_t)batch * n_classes, stride, size, radius, form};
    return launch_heatmap_encode(a, static_cast<hipStream_t>(stream));
}

static dad3d_status iou_check(const char* who, const float* pred, const void* target, int target_u8, int batch, int channels,
                              int hw) {
    DAD3D_REQUIRE(batch >= 0 && channels >= 0 && hw >= 0, "%s: negative size", who);
    DAD3D_REQUIRE(target_u8 == 0 || target_u8 == 1, "%s: target_u8 must be 0 or 1", who);
    DAD3D_REQUIRE((long long)batch * channels <= 0x7fffffffLL, "%s: %d x %d channels beyond the launch grid", who, batch, channels);
    DAD3D_REQUIRE(batch == 0 || channels == 0 || (pred && target), "%s: null argument", who);
    return DAD3D_OK;
}

static bool iou_vec(const float* pred, const void* target, int target_u8, int hw) {
    return hw % 4 == 0 && aligned16(pred) && (reinterpret_cast<uintptr_t>(target) & (target_u8 ? 3 : 15)) == 0;
}

dad3d_status dad3d_heatmap_iou(const float* pred, const void* target, int target_u8, int batch, int channels, int hw,
                               int sigmoid, double* sums, float* iou, float* loss, float* accum, int device, void* stream) {
    dad3d_status st = iou_check("dad3d_heatmap_iou", pred, target, target_u8, batch, channels, hw);
    if (st) return st;
    DAD3D_REQUIRE(batch > 0 && channels > 0, "dad3d_heatmap_iou: no channels (the reference's mean over none is NaN)");
    DAD3D_REQUIRE(sums, "dad3d_heatmap_iou: null sums");
    DAD3D_REQUIRE(!accum || loss, "dad3d_heatmap_iou: accum needs loss");
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    IouArgs a{pred, target, sums, iou, loss, accum, nullptr, nullptr, (size_t)batch * channels, hw, target_u8 != 0};
    return launch_heatmap_iou(a, sigmoid != 0, iou_vec(pred, target, target_u8, hw), static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_heatmap_iou_grad(const float* pred, const void* target, int target_u8, int batch, int channels, int hw,
                                    const double* sums, const float* grad_out, float* grad, int device, void* stream) {
    dad3d_status st = iou_check("dad3d_heatmap_iou_grad", pred, target, target_u8, batch, channels, hw);
    if (st) return st;
    if (batch == 0 || channels == 0 || hw == 0) return DAD3D_OK;
    DAD3D_REQUIRE(sums && grad_out && grad, "dad3d_heatmap_iou_grad: null argument");
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    IouArgs a{pred, target, const_cast<double*>(sums), nullptr, nullptr, nullptr, grad_out, grad, (size_t)batch * channels, hw,
              target_u8 != 0};
    return launch_heatmap_iou_grad(a, iou_vec(pred, target, target_u8, hw) && aligned16(grad), static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_visibility_point_loss(const float* pred, const float* pred_presence, const float* target,
                                         const float* target_presence, int batch, int n_points, int criterion, float* loss,
                                         float* grad_pred, int device, void* stream) {
    DAD3D_REQUIRE(batch >= 0 && n_points >= 0, "dad3d_visibility_point_loss: negative size");
    DAD3D_REQUIRE(criterion >= DAD3D_LOSS_L1 && criterion <= DAD3D_LOSS_SMOOTH_L1, "dad3d_visibility_point_loss: unknown criterion %d",
                  criterion);
    DAD3D_REQUIRE(batch > 0 && n_points > 0, "dad3d_visibility_point_loss: no points (the reference's mean over none is NaN)");
    DAD3D_REQUIRE(pred && pred_presence && target && target_presence && loss, "dad3d_visibility_point_loss: null argument");
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    VisibilityLossArgs a{pred, pred_presence, target, target_presence, loss, grad_pred, batch, n_points, criterion};
    return launch_visibility_loss(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_keypoint_errors(const float* pred, const float* target, int batch, int n_verts, int dims, const int32_t* index,
                                   int n_points, const float* presence, float pred_scale, float target_scale, int cube,
                                   const int32_t* bbox, const double* thresholds, int n_thresholds, int below, double* err,
                                   float* out, float* accum, int device, void* stream) {
    DAD3D_REQUIRE(batch > 0 && n_verts > 0 && n_points > 0, "dad3d_keypoint_errors: bad size (batch %d, n_verts %d, n_points %d)",
                  batch, n_verts, n_points);
    DAD3D_REQUIRE(batch <= 0x7fffffff && (dims == 2 || dims == 3), "dad3d_keypoint_errors: dims must be 2 or 3, not %d", dims);
    DAD3D_REQUIRE(index || n_points <= n_verts, "dad3d_keypoint_errors: %d points of %d vertices", n_points, n_verts);
    DAD3D_REQUIRE(n_thresholds >= 0 && n_thresholds <= kMaxThresholds, "dad3d_keypoint_errors: %d thresholds (at most %d)", n_thresholds,
                  kMaxThresholds);
    DAD3D_REQUIRE(!cube || dims == 3, "dad3d_keypoint_errors: normalize_to_cube needs 3-D points");
    DAD3D_REQUIRE(pred && target && err && (n_thresholds == 0 || thresholds), "dad3d_keypoint_errors: null argument");
    DAD3D_REQUIRE(!accum || out, "dad3d_keypoint_errors: accum needs out");
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    KeypointErrArgs a{};
    a.pred = pred, a.target = target, a.index = index, a.presence = presence, a.bbox = bbox, a.err = err, a.out = out,
    a.accum = accum;
    a.pred_scale = pred_scale, a.target_scale = target_scale;
    for (int k = 0; k < n_thresholds; ++k) a.thresholds[k] = thresholds[k];  // HOST array
    a.batch = batch, a.n_verts = n_verts, a.n_points = n_points, a.dims = dims, a.n_thresholds = n_thresholds;
    a.cube = cube != 0, a.below = below != 0;
    return launch_keypoint_errors(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_eval_nearest(const float* query, const float* points, const int32_t* counts, const float* similarity,
                                int batch, int n_query, int n_points, int k, int flags, float* min_dist2, int32_t* knn_index,
                                float* knn_dist2, int device, void* stream) {
    DAD3D_REQUIRE(batch > 0 && n_query > 0 && n_points > 0, "dad3d_eval_nearest: sizes must be positive (B %d, Q %d, N %d)", batch,
                  n_query, n_points);
    DAD3D_REQUIRE(k >= 1 && k <= kEvalMaxK, "dad3d_eval_nearest: k = %d outside 1..%d", k, kEvalMaxK);
    DAD3D_REQUIRE((flags & ~DAD3D_EVAL_SELF_EXCLUDE) == 0, "dad3d_eval_nearest: unknown flags 0x%x", flags);
    DAD3D_REQUIRE(query && points && min_dist2, "dad3d_eval_nearest: null argument");
    DAD3D_REQUIRE(batch <= 65535, "dad3d_eval_nearest: batch beyond the launch grid");
    DAD3D_REQUIRE(!(flags & DAD3D_EVAL_SELF_EXCLUDE) || n_query == n_points,
                  "dad3d_eval_nearest: DAD3D_EVAL_SELF_EXCLUDE needs the same set as query and points (Q %d, N %d)", n_query, n_points);
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    EvalNearestArgs a{query, points, counts, similarity, min_dist2, knn_index, knn_dist2, batch, n_query, n_points, k,
                      (flags & DAD3D_EVAL_SELF_EXCLUDE) ? 1 : 0};
    return launch_eval_nearest(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_eval_z5_ranks(const float* gt_head, const float* pred_head, int batch, int n_head, const int32_t* anchors,
                                 int n_anchors, int32_t* counts, int32_t* order, int device, void* stream) {
    DAD3D_REQUIRE(batch > 0 && n_head > 0, "dad3d_eval_z5_ranks: sizes must be positive (B %d, K %d)", batch, n_head);
    DAD3D_REQUIRE(n_head <= kEvalMaxHead, "dad3d_eval_z5_ranks: K = %d head vertices exceed the %d the LDS sort holds", n_head,
                  kEvalMaxHead);
    DAD3D_REQUIRE(n_anchors >= 1 && n_anchors <= kEvalMaxAnchors, "dad3d_eval_z5_ranks: %d anchors outside 1..%d", n_anchors,
                  kEvalMaxAnchors);
    DAD3D_REQUIRE(gt_head && pred_head && anchors && counts, "dad3d_eval_z5_ranks: null argument");
    DAD3D_REQUIRE(batch <= 65535, "dad3d_eval_z5_ranks: batch beyond the launch grid");
    EvalZ5Args a{gt_head, pred_head, counts, order, {}, batch, n_head, 1, n_anchors};
    for (int i = 0; i < n_anchors; ++i) {
        DAD3D_REQUIRE(anchors[i] >= 0 && anchors[i] < n_head, "dad3d_eval_z5_ranks: anchor %d = %d outside 0..%d", i, anchors[i],
                      n_head - 1);
        a.anchors[i] = anchors[i];
    }
    while (a.sort_len < n_head) a.sort_len <<= 1;
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    return launch_eval_z5(a, static_cast<hipStream_t>(stream));
}

}  // extern "C"

// =================================================================================================
// UV-texture bake (uv_texture.hip)
// =================================================================================================
struct dad3d_uvmap {
    int device = 0;
    int nver = 0, size = 0, n_cand = 0;
    int* d_adj_ptr = nullptr;  // vertex -> faces (UvNormalArgs)
    int4* d_adj = nullptr;
    int* d_texel_ptr = nullptr;  // texel -> candidates, descending (UvBakeArgs)
    int* d_cand_verts = nullptr;
    double* d_cand_bary = nullptr;
};

extern "C" {

dad3d_status dad3d_uvmap_create(const int32_t* faces, int ntri, int nver, const int32_t* cand_texel, const int32_t* cand_verts,
                                const double* cand_bary, int n, int img_size, int device, dad3d_uvmap** out) {
    DAD3D_REQUIRE(out, "dad3d_uvmap_create: null output handle");
    *out = nullptr;
    DAD3D_REQUIRE(ntri >= 0 && nver >= 0 && n >= 0, "dad3d_uvmap_create: negative size (ntri %d, nver %d, n %d)", ntri, nver, n);
    DAD3D_REQUIRE(img_size > 0 && img_size <= 46340, "dad3d_uvmap_create: texture size %d outside 1..46340", img_size);
    DAD3D_REQUIRE((faces || ntri == 0) && ((cand_texel && cand_verts && cand_bary) || n == 0), "dad3d_uvmap_create: null argument");
    for (size_t i = 0; i < 3 * (size_t)ntri; ++i)
        DAD3D_REQUIRE(faces[i] >= 0 && faces[i] < nver, "dad3d_uvmap_create: face %zu names vertex %d outside [0,%d)", i / 3,
                      faces[i], nver);
    const int n_tex = img_size * img_size;
    for (int i = 0; i < n; ++i) {
        DAD3D_REQUIRE(cand_texel[i] >= 0 && cand_texel[i] < n_tex, "dad3d_uvmap_create: candidate %d on texel %d outside [0,%d)", i,
                      cand_texel[i], n_tex);
        for (int c = 0; c < 3; ++c)
            DAD3D_REQUIRE(cand_verts[3 * (size_t)i + c] >= 0 && cand_verts[3 * (size_t)i + c] < nver,
                          "dad3d_uvmap_create: candidate %d names vertex %d outside [0,%d)", i, cand_verts[3 * (size_t)i + c], nver);
    }
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    // vertex -> faces in ascending face order, each face once with its multiplicity: the rows of psbody's faces_by_vertex
    // CSR after scipy summed the duplicate (vertex, face) entries
    std::vector<int> ptr(nver + 1, 0);
    std::vector<int4> adj;
    {
        std::vector<std::vector<int4>> rows(nver);
        for (int f = 0; f < ntri; ++f) {
            const int* t = faces + 3 * (size_t)f;
            for (int c = 0; c < 3; ++c) {
                std::vector<int4>& r = rows[t[c]];
                if ((c > 0 && t[c] == t[0]) || (c == 2 && t[c] == t[1])) {
                    ++r.back().w;  // the same face names this vertex again
                    continue;
                }
                r.push_back(make_int4(t[0], t[1], t[2], 1));
            }
        }
        for (int v = 0; v < nver; ++v) ptr[v + 1] = ptr[v] + (int)rows[v].size();
        adj.reserve(ptr[nver]);
        for (int v = 0; v < nver; ++v) adj.insert(adj.end(), rows[v].begin(), rows[v].end());
    }
    // texel -> candidates, descending candidate index: the first that passes is the reference's last writer
    std::vector<int> tptr(n_tex + 1, 0);
    for (int i = 0; i < n; ++i) ++tptr[cand_texel[i] + 1];
    for (int t = 0; t < n_tex; ++t) tptr[t + 1] += tptr[t];
    std::vector<int> fill(tptr.begin(), tptr.end() - 1), verts(3 * (size_t)n);
    std::vector<double> bary(3 * (size_t)n);
    for (int i = n - 1; i >= 0; --i) {
        const int j = fill[cand_texel[i]]++;
        for (int c = 0; c < 3; ++c) verts[3 * (size_t)j + c] = cand_verts[3 * (size_t)i + c], bary[3 * (size_t)j + c] = cand_bary[3 * (size_t)i + c];
    }
    std::unique_ptr<dad3d_uvmap> m(new dad3d_uvmap);
    m->device = device, m->nver = nver, m->size = img_size, m->n_cand = n;
    dad3d_status st;
    if ((st = upload(&m->d_adj_ptr, ptr)) || (st = upload(&m->d_adj, adj)) || (st = upload(&m->d_texel_ptr, tptr)) ||
        (st = upload(&m->d_cand_verts, verts)) || (st = upload(&m->d_cand_bary, bary))) {
        dad3d_uvmap_destroy(m.release());
        return st;
    }
    *out = m.release();
    return DAD3D_OK;
}

void dad3d_uvmap_destroy(dad3d_uvmap* m) {
    if (!m) return;
    DeviceGuard guard(m->device);
    for (void* p : {(void*)m->d_adj_ptr, (void*)m->d_adj, (void*)m->d_texel_ptr, (void*)m->d_cand_verts, (void*)m->d_cand_bary})
        if (p) (void)hipFree(p);
    delete m;
}

int dad3d_uvmap_size(const dad3d_uvmap* m) { return m ? m->size : 0; }

dad3d_status dad3d_uvmap_vertex_normals(dad3d_uvmap* m, double* normals, const float* vertices, int batch, void* stream) {
    DAD3D_REQUIRE(m && batch >= 0, "dad3d_uvmap_vertex_normals: bad argument");
    DAD3D_REQUIRE(batch <= 65535, "dad3d_uvmap_vertex_normals: batch beyond the launch grid");
    if (batch == 0 || m->nver == 0) return DAD3D_OK;
    DAD3D_REQUIRE(normals && vertices, "dad3d_uvmap_vertex_normals: null argument");
    DeviceGuard guard(m->device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", m->device);
    UvNormalArgs a{m->d_adj_ptr, m->d_adj, vertices, normals, batch, m->nver};
    return launch_uv_vertex_normals(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_uvmap_bake(dad3d_uvmap* m, uint8_t* texture, const float* vertices, const double* normals, const uint8_t* images,
                              const int32_t* hw, int batch, int h, int w, void* stream) {
    DAD3D_REQUIRE(m && batch >= 0 && h > 0 && w > 0, "dad3d_uvmap_bake: bad argument (batch %d, h %d, w %d)", batch, h, w);
    DAD3D_REQUIRE(uv_bake_grid_y(batch, kUvBakeChunk) <= 65535, "dad3d_uvmap_bake: batch beyond the launch grid");
    if (batch == 0) return DAD3D_OK;
    DAD3D_REQUIRE(texture && images && ((vertices && normals) || m->n_cand == 0), "dad3d_uvmap_bake: null argument");
    DeviceGuard guard(m->device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", m->device);
    UvBakeArgs a{m->d_texel_ptr, m->d_cand_verts, m->d_cand_bary, vertices, normals, images, hw, texture,
                 batch, m->nver, m->size, h, w, kUvBakeChunk};
    return launch_uv_bake(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_uvmap_bake_frames(dad3d_uvmap* m, uint8_t* texture, float* score, const float* vertices, const double* normals,
                                     const int64_t* frames, const int64_t* frames_host, int n_frames, const int32_t* image_index, int n_heads,
                                     int32_t* flags, void* stream) {
    const char* who = "dad3d_uvmap_bake_frames";
    // the scalars and the host table first: a bad one is refused before the handle is looked at or any device work starts
    DAD3D_REQUIRE(n_frames >= 0 && n_heads >= 0, "%s: negative count (%d frames, %d heads)", who, n_frames, n_heads);
    DAD3D_REQUIRE(n_heads <= 65535, "%s: %d heads, beyond the launch grid of 65535", who, n_heads);
    DAD3D_REQUIRE(n_frames == 0 || frames_host, "%s: null host frame table", who);
    // the shapes as frames_check_shapes reads them, without the raster chain's tile limits: nothing here works in tiles
    for (int f = 0; f < n_frames; ++f) {
        const int64_t addr = frames_host[4 * (size_t)f], h = frames_host[4 * (size_t)f + 1], w = frames_host[4 * (size_t)f + 2],
                      stride = frames_host[4 * (size_t)f + 3];
        DAD3D_REQUIRE(addr != 0, "%s: frame %d has no address", who, f);
        DAD3D_REQUIRE(h >= 1 && w >= 1 && h <= INT32_MAX && w <= INT32_MAX, "%s: frame %d is %lld x %lld pixels", who, f, (long long)h, (long long)w);
        DAD3D_REQUIRE(stride >= 3 * w, "%s: frame %d has a row stride of %lld bytes for %lld pixels of 3 bytes", who, f, (long long)stride,
                      (long long)w);
    }
    DAD3D_REQUIRE(m, "%s: null handle", who);
    if (n_heads == 0) return DAD3D_OK;
    DAD3D_REQUIRE(texture && image_index && flags && ((vertices && normals) || m->n_cand == 0), "%s: null buffer", who);
    DAD3D_REQUIRE(n_frames == 0 || frames, "%s: null device frame table", who);
    DeviceGuard guard(m->device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", m->device);
    UvBakeFramesArgs a{m->d_texel_ptr, m->d_cand_verts, m->d_cand_bary, vertices, normals, reinterpret_cast<const long long*>(frames), image_index,
                       texture, score, flags, n_heads, n_frames, m->nver, m->size};
    return launch_uv_bake_frames(a, static_cast<hipStream_t>(stream));
}

static dad3d_status overlay_checked(const char* who, const uint8_t* src, uint8_t* dst, int batch, int h, int w, const float* points,
                                    int n_points, int n_prims) {
    DAD3D_REQUIRE(batch >= 0 && batch <= 65535, "%s: batch %d outside 0 .. 65535", who, batch);
    DAD3D_REQUIRE(h >= 1 && w >= 1 && h <= DAD3D_OVERLAY_MAX_COORD && w <= DAD3D_OVERLAY_MAX_COORD, "%s: an image of %d x %d (1 .. %d)", who, h,
                  w, DAD3D_OVERLAY_MAX_COORD);
    DAD3D_REQUIRE(n_points >= 0 && n_prims >= 0 && n_points <= 0x3fffffff && n_prims <= 0x3fffffff, "%s: %d points, %d primitives", who,
                  n_points, n_prims);
    if (batch == 0) return DAD3D_OK;
    DAD3D_REQUIRE(src && dst, "%s: null image", who);
    DAD3D_REQUIRE(n_prims == 0 || n_points == 0 || points, "%s: null point table", who);
    return DAD3D_OK;
}

dad3d_status dad3d_overlay_segments(const uint8_t* src, uint8_t* dst, int batch, int h, int w, const float* points, int n_points,
                                    const int32_t* edges, int n_edges, const uint8_t* colors, uint32_t color, int thickness, int device,
                                    void* stream) {
    DAD3D_REQUIRE(thickness >= 0 && thickness <= 255, "dad3d_overlay_segments: thickness %d outside 0 (anti-aliased) .. 255", thickness);
    const dad3d_status st = overlay_checked("dad3d_overlay_segments", src, dst, batch, h, w, points, n_points, n_edges);
    if (st != DAD3D_OK || batch == 0) return st;
    DAD3D_REQUIRE(n_edges == 0 || edges, "dad3d_overlay_segments: null edge list");
    DAD3D_REQUIRE(n_edges == 0 || (reinterpret_cast<uintptr_t>(edges) & 3) == 0, "dad3d_overlay_segments: misaligned edge list");
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    OverlaySegmentsArgs a{src, dst, points, edges, colors, color & 0xffffffu, batch, h, w, n_points, n_edges, thickness};
    return launch_overlay_segments(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_overlay_discs(const uint8_t* src, uint8_t* dst, int batch, int h, int w, const float* points, int n_points,
                                 const int32_t* index, int n_discs, int radius, uint32_t color, int device, void* stream) {
    DAD3D_REQUIRE(radius >= 1 && radius <= DAD3D_OVERLAY_MAX_COORD, "dad3d_overlay_discs: radius %d outside 1 .. %d", radius,
                  DAD3D_OVERLAY_MAX_COORD);
    const dad3d_status st = overlay_checked("dad3d_overlay_discs", src, dst, batch, h, w, points, n_points, n_discs);
    if (st != DAD3D_OK || batch == 0) return st;
    DAD3D_REQUIRE(index || n_discs <= n_points, "dad3d_overlay_discs: %d discs from %d points without an index list", n_discs, n_points);
    DeviceGuard guard(device);
    DAD3D_REQUIRE(guard.ok, "cannot select HIP device %d", device);
    OverlayDiscsArgs a{src, dst, points, index, color & 0xffffffu, batch, h, w, n_points, n_discs, radius};
    return launch_overlay_discs(a, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_mesh_debug_trace(dad3d_mesh* m, unsigned long long* device_buffer) {
    DAD3D_REQUIRE(m, "null handle");
    m->d_trace = device_buffer;
    return DAD3D_OK;
}

dad3d_status dad3d_mesh_normal_plan(dad3d_mesh* m, int entry, int batch, int h, int w, int* form, int* chunks, int* built_mask) {
    DAD3D_REQUIRE(m && form && chunks && built_mask, "dad3d_mesh_normal_plan: null argument");
    DAD3D_REQUIRE(entry == DAD3D_PLAN_GET_NORMAL || entry == DAD3D_PLAN_PHONG || entry == DAD3D_PLAN_RENDER,
                  "dad3d_mesh_normal_plan: unknown entry %d", entry);
    DAD3D_REQUIRE(entry == DAD3D_PLAN_RENDER ? (h >= 1 && w >= 1) : batch >= 1, "dad3d_mesh_normal_plan: batch or image size below 1");
    DAD3D_REQUIRE(m->nver > 0 && (entry != DAD3D_PLAN_RENDER || m->ntri > 0), "dad3d_mesh_normal_plan: an empty mesh launches nothing");
    DeviceGuard guard(m->device);
    const NormalPlan p = entry == DAD3D_PLAN_GET_NORMAL ? plan_get_normal(m->dev(), m->nc, batch)
                         : entry == DAD3D_PLAN_PHONG    ? plan_phong(m->dev(), m->nc, false, batch)
                                                        : plan_render_light(m->dev(), m->nc, h, w);
    *form = p.form;
    *chunks = p.form == DAD3D_FORM_REFUSED ? 0 : p.chunks;
    *built_mask = 0;
    for (int k = 0; k < kNormalChunkings; ++k)
        if (m->nc[k].chunks) *built_mask |= 1 << k;
    return DAD3D_OK;
}

dad3d_status dad3d_mesh_phong_light(dad3d_mesh* m, float* light, const float* vertices, const float* normals,
                                    int batch, const dad3d_light* cfg, void* stream) {
    DAD3D_REQUIRE(m && cfg && batch >= 0, "dad3d_mesh_phong_light: bad argument");
    if (batch == 0 || m->nver == 0) return DAD3D_OK;
    DAD3D_REQUIRE(light && vertices && normals, "dad3d_mesh_phong_light: null buffer");
    DeviceGuard guard(m->device);
    return launch_phong(m->dev(), m->nc, light, vertices, normals, nullptr, batch, *cfg, static_cast<hipStream_t>(stream));
}

dad3d_status dad3d_mesh_normal_phong_light(dad3d_mesh* m, float* light, float* ver_normal, const float* vertices,
                                           int batch, const dad3d_light* cfg, void* stream) {
    DAD3D_REQUIRE(m && cfg && batch >= 0, "dad3d_mesh_normal_phong_light: bad argument");
    if (batch == 0 || m->nver == 0) return DAD3D_OK;
    DAD3D_REQUIRE(light && vertices, "dad3d_mesh_normal_phong_light: null buffer");
    DeviceGuard guard(m->device);
    return launch_phong(m->dev(), m->nc, light, vertices, nullptr, ver_normal, batch, *cfg, static_cast<hipStream_t>(stream));
}

}  // extern "C"

// -------------------------------------------------------------------------------------------------
// Exact-signature single-image host entry points (Sim3DR/lib/rasterize.h:84-100).
// The reference API carries no vertex count for three of the five calls; it is derived from the
// triangle list (max index + 1), which is all the GPU needs to stage.
// -------------------------------------------------------------------------------------------------
namespace {

struct HostMeshCache {
    std::mutex mu;
    dad3d_mesh* mesh = nullptr;
    uint64_t hash = 0;
    int ntri = -1, nver = -1;
    ~HostMeshCache() { /* process teardown: the HIP runtime may already be gone; leak on purpose */ }
};
HostMeshCache g_cache;

int compat_device() {
    const char* e = std::getenv("DAD3D_DEVICE");
    return e ? std::atoi(e) : 0;
}

// Content hash of the triangle list (the reference API re-passes it on every call): 8 bytes per step, four
// independent lanes -- a byte-wise FNV over 120 KB cost more than the kernels it guards.
uint64_t fnv1a(const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    uint64_t h[4] = {1469598103934665603ull, 0x9E3779B97F4A7C15ull, 0xC2B2AE3D27D4EB4Full, 0x165667B19E3779F9ull};
    size_t i = 0;
    for (; i + 32 <= n; i += 32)
        for (int k = 0; k < 4; ++k) {
            uint64_t w;
            std::memcpy(&w, b + i + 8 * k, 8);
            h[k] = (h[k] ^ w) * 1099511628211ull;
            h[k] ^= h[k] >> 29;
        }
    uint64_t t = n;
    for (; i < n; ++i) t = (t ^ b[i]) * 1099511628211ull;
    return ((h[0] * 31 + h[1]) * 31 + h[2]) * 31 + h[3] + t * 0x9E3779B97F4A7C15ull;
}

int max_index_plus_one(const int* tri, int ntri) {
    int mx = -1;
    for (int i = 0; i < 3 * ntri; ++i) mx = std::max(mx, tri[i]);
    return mx + 1;
}

// topology is static across calls in practice (one mesh, many frames): rebuild only when it changes
dad3d_mesh* cached_mesh(const int* tri, int ntri, int nver) {
    const uint64_t hsh = fnv1a(tri, sizeof(int) * 3 * (size_t)ntri);
    if (g_cache.mesh && g_cache.hash == hsh && g_cache.ntri == ntri && g_cache.nver == nver) return g_cache.mesh;
    if (g_cache.mesh) dad3d_mesh_destroy(g_cache.mesh);
    g_cache.mesh = nullptr;
    if (dad3d_mesh_create(tri, ntri, nver, compat_device(), &g_cache.mesh) != DAD3D_OK) return nullptr;
    g_cache.hash = hsh;
    g_cache.ntri = ntri;
    g_cache.nver = nver;
    return g_cache.mesh;
}

// Staging buffers of the single-image host entry points: a few grow-only device buffers kept for the life of the process
// (a hipMalloc + hipFree per call cost more than the kernels; calls are serialised by g_cache.mu). A DevBuf takes the next
// free slot of the arena; the arena is rewound when the call returns.
struct StagingArena {
    static constexpr int kSlots = 4;
    void* buf[kSlots] = {};
    size_t cap[kSlots] = {};
    int next = 0;
    ~StagingArena() { /* process teardown: leak on purpose, see HostMeshCache */ }
};
StagingArena g_arena;

struct DevBuf {
    void* p = nullptr;
    bool alloc(size_t bytes) {
        if (g_arena.next >= StagingArena::kSlots) return false;
        const int s = g_arena.next++;
        bytes = std::max<size_t>(bytes, 4);
        if (g_arena.cap[s] < bytes) {
            if (g_arena.buf[s]) (void)hipFree(g_arena.buf[s]);
            g_arena.buf[s] = nullptr, g_arena.cap[s] = 0;
            if (hipMalloc(&g_arena.buf[s], bytes) != hipSuccess) return false;
            g_arena.cap[s] = bytes;
        }
        p = g_arena.buf[s];
        return true;
    }
};
struct ArenaScope {  // declared after the lock in every entry point
    ArenaScope() { g_arena.next = 0; }
    ~ArenaScope() { g_arena.next = 0; }
};

bool h2d(void* d, const void* h, size_t n) { return n == 0 || hipMemcpy(d, h, n, hipMemcpyHostToDevice) == hipSuccess; }
bool d2h(void* h, const void* d, size_t n) { return n == 0 || hipMemcpy(h, d, n, hipMemcpyDeviceToHost) == hipSuccess; }

}  // namespace

extern "C" {

void dad3d_sim3dr_get_tri_normal(float* tri_normal, float* vertices, int* triangles, int ntri, int norm_flg) {
    if (ntri <= 0) return;
    std::lock_guard<std::mutex> lock(g_cache.mu);
    ArenaScope arena_scope;
    const int nver = max_index_plus_one(triangles, ntri);
    dad3d_mesh* m = cached_mesh(triangles, ntri, nver);
    if (!m) return;
    DeviceGuard guard(m->device);
    DevBuf dv, dn;
    const size_t vb = sizeof(float) * 3 * (size_t)nver, nb = sizeof(float) * 3 * (size_t)ntri;
    if (!dv.alloc(vb) || !dn.alloc(nb) || !h2d(dv.p, vertices, vb)) return set_error("sim3dr compat: staging failed");
    if (dad3d_mesh_get_tri_normal(m, (float*)dn.p, (const float*)dv.p, 1, norm_flg, nullptr)) return;
    if (hipDeviceSynchronize() != hipSuccess || !d2h(tri_normal, dn.p, nb)) set_error("sim3dr compat: readback failed");
}

void dad3d_sim3dr_get_ver_normal(float* ver_normal, float* tri_normal, int* triangles, int nver, int ntri) {
    if (nver <= 0) return;
    std::lock_guard<std::mutex> lock(g_cache.mu);
    ArenaScope arena_scope;
    dad3d_mesh* m = cached_mesh(triangles, std::max(ntri, 0), nver);
    if (!m) return;
    DeviceGuard guard(m->device);
    DevBuf dt, dn;
    const size_t tb = sizeof(float) * 3 * (size_t)std::max(ntri, 0), nb = sizeof(float) * 3 * (size_t)nver;
    if (!dt.alloc(tb) || !dn.alloc(nb) || !h2d(dt.p, tri_normal, tb) || !h2d(dn.p, ver_normal, nb))
        return set_error("sim3dr compat: staging failed");
    if (dad3d_mesh_get_ver_normal(m, (float*)dn.p, (const float*)dt.p, 1, DAD3D_NORMAL_ACCUMULATE, nullptr)) return;
    if (hipDeviceSynchronize() != hipSuccess || !d2h(ver_normal, dn.p, nb)) set_error("sim3dr compat: readback failed");
}

void dad3d_sim3dr_get_normal(float* ver_normal, float* vertices, int* triangles, int nver, int ntri) {
    if (nver <= 0) return;
    std::lock_guard<std::mutex> lock(g_cache.mu);
    ArenaScope arena_scope;
    dad3d_mesh* m = cached_mesh(triangles, std::max(ntri, 0), nver);
    if (!m) return;
    DeviceGuard guard(m->device);
    DevBuf dv, dn;
    const size_t nb = sizeof(float) * 3 * (size_t)nver;
    if (!dv.alloc(nb) || !dn.alloc(nb) || !h2d(dv.p, vertices, nb) || !h2d(dn.p, ver_normal, nb))
        return set_error("sim3dr compat: staging failed");
    if (dad3d_mesh_get_normal(m, (float*)dn.p, (const float*)dv.p, 1, DAD3D_NORMAL_ACCUMULATE, nullptr)) return;
    if (hipDeviceSynchronize() != hipSuccess || !d2h(ver_normal, dn.p, nb)) set_error("sim3dr compat: readback failed");
}

void dad3d_sim3dr_rasterize_triangles(float* vertices, int* triangles, float* depth_buffer, int* triangle_buffer,
                                      float* barycentric_weight, int ntri, int h, int w) {
    if (ntri <= 0 || h <= 0 || w <= 0) return;
    std::lock_guard<std::mutex> lock(g_cache.mu);
    ArenaScope arena_scope;
    const int nver = max_index_plus_one(triangles, ntri);
    dad3d_mesh* m = cached_mesh(triangles, ntri, nver);
    if (!m) return;
    DeviceGuard guard(m->device);
    DevBuf dv, dd, dt, db;
    const size_t vb = sizeof(float) * 3 * (size_t)nver, pb = (size_t)h * w;
    if (!dv.alloc(vb) || !dd.alloc(pb * 4) || !dt.alloc(pb * 4) || !db.alloc(pb * 12) || !h2d(dv.p, vertices, vb) ||
        !h2d(dd.p, depth_buffer, pb * 4) || !h2d(dt.p, triangle_buffer, pb * 4) || !h2d(db.p, barycentric_weight, pb * 12))
        return set_error("sim3dr compat: staging failed");
    if (dad3d_mesh_rasterize_triangles(m, (const float*)dv.p, (float*)dd.p, (int32_t*)dt.p, (float*)db.p, 1, h, w, nullptr))
        return;
    if (hipDeviceSynchronize() != hipSuccess || !d2h(depth_buffer, dd.p, pb * 4) || !d2h(triangle_buffer, dt.p, pb * 4) ||
        !d2h(barycentric_weight, db.p, pb * 12))
        set_error("sim3dr compat: readback failed");
}

void dad3d_sim3dr_rasterize(unsigned char* image, float* vertices, int* triangles, float* colors, float* depth_buffer,
                            int ntri, int h, int w, int c, float alpha, int reverse) {
    if (ntri <= 0 || h <= 0 || w <= 0) return;
    std::lock_guard<std::mutex> lock(g_cache.mu);
    ArenaScope arena_scope;
    const int nver = max_index_plus_one(triangles, ntri);
    dad3d_mesh* m = cached_mesh(triangles, ntri, nver);
    if (!m) return;
    DeviceGuard guard(m->device);
    DevBuf dv, dc, dd, di;
    const size_t vb = sizeof(float) * 3 * (size_t)nver, cb = sizeof(float) * (size_t)c * nver, pb = (size_t)h * w;
    if (!dv.alloc(vb) || !dc.alloc(cb) || !dd.alloc(pb * 4) || !di.alloc(pb * c) || !h2d(dv.p, vertices, vb) ||
        !h2d(dc.p, colors, cb) || !h2d(dd.p, depth_buffer, pb * 4) || !h2d(di.p, image, pb * c))
        return set_error("sim3dr compat: staging failed");
    if (dad3d_mesh_rasterize(m, (uint8_t*)di.p, (const float*)dv.p, (const float*)dc.p, (float*)dd.p, 1, h, w, c, alpha,
                             reverse, nullptr))
        return;
    if (hipDeviceSynchronize() != hipSuccess || !d2h(image, di.p, pb * c) || !d2h(depth_buffer, dd.p, pb * 4))
        set_error("sim3dr compat: readback failed");
}

}  // extern "C"
