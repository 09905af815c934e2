// What dad3d_flame_create and dad3d_flame_set_landmarks work out on the host before they upload anything: the parameter layout, the basis
// packs in MFMA fragment order, the joint regressors, the weight table, the landmark chains and the landmark sub-model. Plain C++ over host
// arrays: no HIP call, no error string, value results -- capi.cpp validates, plans with these, uploads. Compiles without the HIP headers
// (tests/model_plan_main.cpp runs it under the sanitizers); capi.cpp asserts that the constants below are common.hpp's.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/dad3d.h"
#include "plan_pods.hpp"

namespace dad3d {
namespace plan {

constexpr int kJoints = 5;          // kNumJoints
constexpr int kTileVerts = 21;      // the two-role kernel's tile: 63 basis columns + 1 zero pad
constexpr int kTileCols = 64;
constexpr int kPipeTileVerts = 20;  // the pipelined kernel's: 60 basis columns + 3 jaw-joint columns + 1 zero pad
constexpr int kPipeKGroups = 26;

// What follows from the model and the consts alone. Layout: common.hpp's ParamLayout (a template so that this header needs no HIP).
template <typename Layout>
struct FlameDims {
    Layout lay{};
    bool jaw_only = false, pipe_ok = false;
    int n_pose_feats = 0, pose_feat_first = 0;
    int k_used = 0, kgroups = 0;  // [betas | pose feature | template], in groups of 16
    int n_tiles = 0, n_tiles_pipe = 0;
};
template <typename Layout>
FlameDims<Layout> flame_dims(const dad3d_flame_model& m, const dad3d_flame_consts& c) {
    FlameDims<Layout> d;
    Layout& L = d.lay;
    int cur = 0;
    L.shape_off = cur, L.shape_n = c.shape, cur += c.shape;
    L.expr_off = cur, L.expr_n = c.expression, cur += c.expression;
    L.jaw_off = cur, L.jaw_n = c.jaw, cur += c.jaw;
    L.rot_off = cur, cur += c.rotation;
    L.eye_off = cur, L.eye_n = c.eyeballs, cur += c.eyeballs;
    L.neck_off = cur, L.neck_n = c.neck, cur += c.neck;
    L.trans_off = cur, cur += c.translation;
    L.scale_off = cur, cur += c.scale;
    L.n_params = cur;
    // Only the jaw can rotate when neck and eyeballs are size-0 inputs: their Rodrigues matrix is exactly
    // I, so 27 of the 36 pose features are exactly 0 and their basis rows can be skipped (same result).
    // ... and the jaw-only epilogue (S = w0+w1+w3+w4 for "the joints that cannot rotate") also needs no joint to hang
    // off the jaw: a kinematic tree with a child of joint 2 takes the generic 36-feature path.
    bool jaw_is_leaf = true;
    for (int j = 1; j < kJoints; ++j) jaw_is_leaf = jaw_is_leaf && m.parents[j] != 2;
    d.jaw_only = (c.neck == 0 && c.eyeballs == 0 && jaw_is_leaf);
    d.n_pose_feats = d.jaw_only ? 9 : 36;
    d.pose_feat_first = d.jaw_only ? 9 : 0;
    d.k_used = m.n_betas + d.n_pose_feats + 1;
    d.kgroups = (d.k_used + 15) / 16;
    d.n_tiles = (m.n_verts + kTileVerts - 1) / kTileVerts;
    d.n_tiles_pipe = (m.n_verts + kPipeTileVerts - 1) / kPipeTileVerts;
    // the pipelined single-role kernel (flame_decode_pipe.hip): jaw-only models with the dad_3dnet.yaml params layout
    d.pipe_ok = d.jaw_only && c.jaw == 3 && c.shape == 300 && c.expression == 100 && L.jaw_off == 400 && L.rot_off == 403 &&
                L.trans_off == 409 && L.scale_off == 412 && L.n_params == 413 && d.kgroups == kPipeKGroups;
    return d;
}

// Every fragment of a basis pack in MFMA B-fragment order, [tile][group of 16 k][wave][lane][4 MFMA steps]: MFMA step s of group g has
// lane (q = lane >> 4, n = lane & 15) of wave w supply basis row k = 16 g + 4 q + s of column 16 w + n (the k order inside a group is
// permuted so the A operand can be read row-major with one 16-byte LDS load). frag_offset places the four floats of (tile, g, col, q).
inline size_t frag_offset(int tile, int kgroups, int g, int col, int q) {
    return ((((size_t)tile * kgroups + g) * 4 + col / 16) * 64 + (col % 16) + 16 * q) * 4;
}
inline size_t pack_floats(int n_tiles, int kgroups) { return (size_t)n_tiles * kgroups * 4 * 64 * 4; }
template <typename F>
void for_each_fragment(std::vector<float>& pack, int n_tiles, int kgroups, F&& f) {  // f(tile, g, col, q, float* four)
    for (int t = 0; t < n_tiles; ++t)
        for (int g = 0; g < kgroups; ++g)
            for (int col = 0; col < kTileCols; ++col)
                for (int q = 0; q < 4; ++q) f(t, g, col, q, &pack[frag_offset(t, kgroups, g, col, q)]);
}

// basis row k of vertex v's component: [shapedirs | the pose features in use | the template, the row multiplied by 1]
template <typename Layout>
float basis_entry(const dad3d_flame_model& m, const FlameDims<Layout>& d, int k, int v, int comp) {
    const int NB = m.n_betas, V = m.n_verts;
    if (k < NB) return m.shapedirs[((size_t)v * 3 + comp) * NB + k];
    if (k < NB + d.n_pose_feats) {
        const int f = d.pose_feat_first + (k - NB);
        return m.posedirs[(size_t)f * 3 * V + (size_t)v * 3 + comp];
    }
    return m.v_template[(size_t)v * 3 + comp];  // k == NB + n_pose_feats
}

// the two-role kernel's pack: 21 vertices = 63 columns per tile
template <typename Layout>
std::vector<float> basis_pack(const dad3d_flame_model& m, const FlameDims<Layout>& d) {
    std::vector<float> bpack(pack_floats(d.n_tiles, d.kgroups), 0.0f);
    for_each_fragment(bpack, d.n_tiles, d.kgroups, [&](int t, int g, int col, int q, float* dst) {
        const int v = t * kTileVerts + col / 3;
        if (col >= kTileVerts * 3 || v >= m.n_verts) return;
        for (int i = 0; i < 4; ++i) {
            const int k = 16 * g + 4 * q + i;
            if (k < d.k_used) dst[i] = basis_entry(m, d, k, v, col % 3);
        }
    });
    return bpack;
}

// joints are linear in betas: J = J_regressor.v_template + (J_regressor.shapedirs).betas; j0 [15], jdirs [15][n_betas]
inline void joint_regressors(const dad3d_flame_model& m, std::vector<float>* j0_out, std::vector<float>* jdirs_out) {
    const int V = m.n_verts, NB = m.n_betas;
    std::vector<float> j0(3 * kJoints), jdirs((size_t)3 * kJoints * NB);
    std::vector<double> acc((size_t)3 * kJoints * (NB + 1), 0.0);
    for (int j = 0; j < kJoints; ++j)
        for (int v = 0; v < V; ++v) {
            const double r = m.j_regressor[(size_t)j * V + v];
            if (r == 0.0) continue;
            for (int comp = 0; comp < 3; ++comp) {
                double* a = &acc[((size_t)j * 3 + comp) * (NB + 1)];
                a[NB] += r * m.v_template[(size_t)v * 3 + comp];
                const float* sd = &m.shapedirs[((size_t)v * 3 + comp) * NB];
                for (int l = 0; l < NB; ++l) a[l] += r * sd[l];
            }
        }
    for (int o = 0; o < 3 * kJoints; ++o) {
        j0[o] = (float)acc[(size_t)o * (NB + 1) + NB];
        for (int l = 0; l < NB; ++l) jdirs[(size_t)o * NB + l] = (float)acc[(size_t)o * (NB + 1) + l];
    }
    j0_out->swap(j0), jdirs_out->swap(jdirs);
}

// [V][8] skinning weights w0..w4, S = w0+w1+w3+w4, 0, 0
inline std::vector<float> weights8(const dad3d_flame_model& m) {
    std::vector<float> w8((size_t)m.n_verts * 8, 0.0f);
    for (int v = 0; v < m.n_verts; ++v) {
        const float* w = &m.lbs_weights[(size_t)v * kJoints];
        for (int j = 0; j < kJoints; ++j) w8[(size_t)v * 8 + j] = w[j];
        w8[(size_t)v * 8 + 5] = ((w[0] + w[1]) + w[3]) + w[4];  // weight of the joints that cannot rotate (jaw-only mode)
    }
    return w8;
}

// The pipelined kernel's pack. Tiles of 20 vertices; columns 60..62 of every tile carry the jaw joint J_jaw = J0_jaw + Jdirs_jaw . betas
// (rows of the pose feature contribute nothing to a joint: smplx regresses the joints from v_shaped), column 63 is zero.
template <typename Layout>
std::vector<float> basis_pack_pipe(const dad3d_flame_model& m, const FlameDims<Layout>& d, const std::vector<float>& j0,
                                   const std::vector<float>& jdirs) {
    const int V = m.n_verts, NB = m.n_betas;
    std::vector<float> bpack_pipe(pack_floats(d.n_tiles_pipe, kPipeKGroups), 0.0f);
    for_each_fragment(bpack_pipe, d.n_tiles_pipe, kPipeKGroups, [&](int t, int g, int col, int q, float* dst) {
        for (int i = 0; i < 4; ++i) {
            const int k = 16 * g + 4 * q + i;
            if (k >= d.k_used) continue;
            if (col < 3 * kPipeTileVerts) {
                const int v = t * kPipeTileVerts + col / 3;
                if (v < V) dst[i] = basis_entry(m, d, k, v, col % 3);
            } else if (col < 3 * kPipeTileVerts + 3) {
                const int o = 2 * 3 + (col - 3 * kPipeTileVerts);  // joint 2 = jaw
                dst[i] = k < NB ? jdirs[(size_t)o * NB + k] : (k == NB + d.n_pose_feats ? j0[o] : 0.0f);
            }
        }
    });
    return bpack_pipe;
}

inline float max_abs(const std::vector<float>& pack) {  // what split_basis_scale turns into the fp16 split's power of two
    float mx = 0.0f;
    for (float v : pack) mx = std::max(mx, std::fabs(v));
    return mx;
}

// The per-vertex slot chains of a landmark list: head2 [V][2] {first slot of the vertex, the slot after it} (what the kernels stage per
// tile), next [n] the slot after each slot; -1 = none
inline void landmark_chains(const int64_t* idx, int n, int V, std::vector<int>* head2_out, std::vector<int>* next_out) {
    std::vector<int> head(V, -1), next(n, -1);
    for (int s = n - 1; s >= 0; --s) {  // reverse walk: each vertex's chain comes out in ascending slot order
        next[s] = head[idx[s]];
        head[idx[s]] = s;
    }
    std::vector<int> head2((size_t)V * 2, -1);
    for (int v = 0; v < V; ++v)
        if (head[v] >= 0) head2[(size_t)v * 2] = head[v], head2[(size_t)v * 2 + 1] = next[head[v]];
    head2_out->swap(head2), next_out->swap(next);
}

// the pipelined kernel's per-vertex table: skinning weights from the model's w8, landmark slots (as int bits) from the list's head2
inline std::vector<Float4> vertex_table(const std::vector<float>& w8, const std::vector<int>& head2, int V) {
    std::vector<Float4> vtab(V);
    for (int v = 0; v < V; ++v) {
        const float* w = &w8[(size_t)v * 8];
        float fh, fn;
        memcpy(&fh, &head2[(size_t)v * 2], 4), memcpy(&fn, &head2[(size_t)v * 2 + 1], 4);
        vtab[v] = Float4{w[5] + w[2], w[2], fh, fn};  // W = (w0 + w1 + w3 + w4) + w_jaw
    }
    return vtab;
}

// The sub-model of list idx[0..n): the model's pipelined pack restricted to the distinct vertices the list names, in ascending vertex order.
// None (an empty selection) when the list names more than a third of the mesh.
inline std::vector<int> landmark_sub_vertices(const int64_t* idx, int n, int V) {
    std::vector<char> named(V, 0);
    for (int s = 0; s < n; ++s) named[idx[s]] = 1;
    std::vector<int> uniq;
    for (int v = 0; v < V; ++v)
        if (named[v]) uniq.push_back(v);
    if (uniq.size() * 3 > (size_t)V) uniq.clear();
    return uniq;
}
// ... copied out of the model's pack (`full`) fragment by fragment. A column's 416 values do not depend on which tile holds it (the jaw-joint
// columns are the same in every tile), so the sub-model multiplies the same numbers in the same order: a landmark-only launch returns the
// bits a full-output launch of the same handle returns for those vertices (tests/test_gpu_landmark_subset.py).
struct LandmarkSub {
    int n_tiles = 0;
    std::vector<float> pack;
    std::vector<Float4> vtab;  // [uniq.size()] the rows of the model's table of its vertices
};
inline LandmarkSub landmark_sub(const std::vector<int>& uniq, const std::vector<float>& full, const std::vector<Float4>& vtab) {
    LandmarkSub sub;
    const int nu = (int)uniq.size(), nt = (nu + kPipeTileVerts - 1) / kPipeTileVerts;
    sub.pack.assign(pack_floats(nt, kPipeKGroups), 0.0f);
    for_each_fragment(sub.pack, nt, kPipeKGroups, [&](int t, int g, int col, int q, float* dst) {
        int src_tile = 0, src_col = col;  // the jaw-joint columns (and the zero pad) are the same in every tile
        if (col < 3 * kPipeTileVerts) {
            const int u = t * kPipeTileVerts + col / 3;
            if (u >= nu) return;
            src_tile = uniq[u] / kPipeTileVerts, src_col = (uniq[u] % kPipeTileVerts) * 3 + col % 3;
        }
        std::copy_n(&full[frag_offset(src_tile, kPipeKGroups, g, src_col, q)], 4, dst);
    });
    sub.vtab.resize(nu);
    for (int u = 0; u < nu; ++u) sub.vtab[u] = vtab[uniq[u]];
    sub.n_tiles = nt;
    return sub;
}

}  // namespace plan
}  // namespace dad3d
