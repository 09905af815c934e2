// Stand-alone driver of the host planners (csrc/flame_plan.hpp, csrc/mesh_plan.hpp) for tests/test_model_plan.py: plain C++, its own main,
// no HIP, no GPU. `model_plan <flame|mesh|tex|uv> <dir>` reads the raw little-endian arrays the test wrote into <dir> (meta.i32 first) and
// writes every planner output next to them, one raw array per file.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../dad-3dheads_amd/csrc/flame_plan.hpp"
#include "../dad-3dheads_amd/csrc/mesh_plan.hpp"

using namespace dad3d::plan;

static std::string g_dir;

template <typename T>
static std::vector<T> read(const char* name) {
    const std::string path = g_dir + "/" + name;
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path.c_str());
        exit(2);
    }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<T> v((size_t)bytes / sizeof(T));
    if (!v.empty() && fread(v.data(), sizeof(T), v.size(), f) != v.size()) exit(2);
    fclose(f);
    return v;
}
template <typename T>
static void write(const std::string& name, const std::vector<T>& v) {
    const std::string path = g_dir + "/" + name;
    FILE* f = fopen(path.c_str(), "wb");
    if (!f || (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size())) {
        fprintf(stderr, "cannot write %s\n", path.c_str());
        exit(2);
    }
    fclose(f);
}

struct Layout {  // the members of common.hpp's ParamLayout
    int n_params, shape_off, shape_n, expr_off, expr_n, jaw_off, jaw_n, rot_off, eye_off, eye_n, neck_off, neck_n, trans_off, scale_off;
};

// meta: V, NB, {shape, expression, jaw, rotation, eyeballs, neck, translation, scale}, parents[5], number of landmark lists
static void flame() {
    const std::vector<int> meta = read<int>("meta.i32");
    const std::vector<float> v_template = read<float>("v_template.f32"), shapedirs = read<float>("shapedirs.f32"),
                             posedirs = read<float>("posedirs.f32"), j_regressor = read<float>("j_regressor.f32"),
                             lbs_weights = read<float>("lbs_weights.f32");
    int parents[kJoints];
    for (int j = 0; j < kJoints; ++j) parents[j] = meta[10 + j];
    dad3d_flame_model m{};
    m.n_verts = meta[0], m.n_betas = meta[1], m.n_joints = kJoints;
    m.v_template = v_template.data(), m.shapedirs = shapedirs.data(), m.posedirs = posedirs.data(), m.j_regressor = j_regressor.data();
    m.parents = parents, m.lbs_weights = lbs_weights.data();
    dad3d_flame_consts c{};
    c.shape = meta[2], c.expression = meta[3], c.jaw = meta[4], c.rotation = meta[5], c.eyeballs = meta[6], c.neck = meta[7];
    c.translation = meta[8], c.scale = meta[9];

    const FlameDims<Layout> d = flame_dims<Layout>(m, c);
    const Layout& L = d.lay;
    write<int>("dims.i32", {L.n_params, L.shape_off, L.shape_n, L.expr_off, L.expr_n, L.jaw_off, L.jaw_n, L.rot_off, L.eye_off, L.eye_n, L.neck_off,
                            L.neck_n, L.trans_off, L.scale_off, d.jaw_only, d.pipe_ok, d.n_pose_feats, d.pose_feat_first, d.k_used, d.kgroups,
                            d.n_tiles, d.n_tiles_pipe});
    write("bpack.f32", basis_pack(m, d));
    std::vector<float> j0, jdirs, full;
    joint_regressors(m, &j0, &jdirs);
    write("j0.f32", j0), write("jdirs.f32", jdirs);
    const std::vector<float> w8 = weights8(m);
    write("w8.f32", w8);
    if (d.pipe_ok) {
        full = basis_pack_pipe(m, d, j0, jdirs);
        write("bpack_pipe.f32", full);
        write<float>("max_abs.f32", {max_abs(full)});
    }
    for (int k = 0; k < meta[15]; ++k) {
        const std::string tag = std::to_string(k);
        const std::vector<int64_t> idx = read<int64_t>(("idx_" + tag + ".i64").c_str());
        std::vector<int> head2, next;
        landmark_chains(idx.data(), (int)idx.size(), m.n_verts, &head2, &next);
        write("head2_" + tag + ".i32", head2), write("next_" + tag + ".i32", next);
        if (!d.pipe_ok) continue;
        const std::vector<Float4> vtab = vertex_table(w8, head2, m.n_verts);
        write("vtab_" + tag + ".f32", vtab);
        const std::vector<int> uniq = landmark_sub_vertices(idx.data(), (int)idx.size(), m.n_verts);
        write("uniq_" + tag + ".i32", uniq);
        if (uniq.empty()) continue;
        const LandmarkSub sub = landmark_sub(uniq, full, vtab);
        write<int>("sub_tiles_" + tag + ".i32", {sub.n_tiles});
        write("sub_pack_" + tag + ".f32", sub.pack), write("sub_vtab_" + tag + ".f32", sub.vtab);
    }
}

// the LDS bytes of the normals' face table (sim3dr_kernels.hip): the staged vertices, 3 floats each and 8 more, in whole float4s, then one
// float4 per face
static size_t table_lds_bytes(int nver, int max_faces) { return ((size_t)((nver * 3 + 8 + 3) & ~3) + 4 * (size_t)max_faces) * sizeof(float); }

// meta: ntri, nver
static void mesh() {
    const std::vector<int> meta = read<int>("meta.i32"), tri = read<int>("tri.i32");
    const int ntri = meta[0], nver = meta[1];
    const MeshAdjacency adj = mesh_adjacency(tri.data(), ntri, nver);
    write("ptr.i32", adj.ptr), write("face.i32", adj.face), write("adj_tri.i32", adj.adj_tri);
    for (int k = 0; k < 4; ++k) {
        const NormalChunkPlan p = plan_normal_chunks(tri.data(), ntri, nver, adj, 1 << k, table_lds_bytes);
        const std::string tag = "nc" + std::to_string(k) + "_";
        write<int>(tag + "meta.i32", {p.built, p.chunks, p.vpb, p.max_faces});
        if (!p.built) continue;
        write(tag + "face_ptr.i32", p.face_ptr), write(tag + "full_groups.i32", p.full_groups), write(tag + "faces.u32", p.faces);
        write(tag + "slot.u16", p.slot), write(tag + "row8.u32", p.row8);
    }
}

// meta: ntri, n_tex, stride
static void tex() {
    const std::vector<int> meta = read<int>("meta.i32"), tri = read<int>("tri.i32"), tex_triangles = read<int>("tex_triangles.i32");
    const std::vector<float> tex_coords = read<float>("tex_coords.f32");
    const TexcoordTables T = plan_texcoords(tri, tex_coords.data(), meta[1], meta[2], tex_triangles.data());
    write<int>("ref_ok.i32", {T.ref_ok});
    write("corner.f32", T.corner), write("ref.f32", T.ref);
}

// meta: ntri, nver, n candidates, n_tex
static void uv() {
    const std::vector<int> meta = read<int>("meta.i32"), faces = read<int>("faces.i32"), cand_texel = read<int>("cand_texel.i32"),
                           cand_verts = read<int>("cand_verts.i32");
    const std::vector<double> cand_bary = read<double>("cand_bary.f64");
    const UvAdjacency a = uv_adjacency(faces.data(), meta[0], meta[1]);
    write("ptr.i32", a.ptr), write("adj.i32", a.adj);
    const UvTexelTables T = uv_texel_tables(cand_texel.data(), cand_verts.data(), cand_bary.data(), meta[2], meta[3]);
    write("tptr.i32", T.tptr), write("verts.i32", T.verts), write("bary.f64", T.bary);
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const std::string mode = argv[1];
    g_dir = argv[2];
    if (mode == "flame") flame();
    else if (mode == "mesh") mesh();
    else if (mode == "tex") tex();
    else if (mode == "uv") uv();
    else return 2;
    return 0;
}
