// What dad3d_mesh_create, dad3d_mesh_set_texcoords and dad3d_uvmap_create work out on the host before they upload anything: adjacency
// lists, the normals kernels' chunk face lists, the texel tables. Plain C++ over host arrays: no HIP call, no error string, value results --
// capi_render.cpp validates, plans with these, uploads. Compiles without the HIP headers (tests/model_plan_main.cpp runs it under the
// sanitizers); its vector types are plan_pods.hpp's.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "plan_pods.hpp"

namespace dad3d {
namespace plan {

// vertex -> incident (face, corner) list; faces ascending, so a gather reproduces the serial scatter-add order of
// rasterize_kernel.cpp:188-198. adj_tri[e]: the three corner indices of face[e] and the face index (MeshDev)
struct MeshAdjacency {
    std::vector<int> ptr, face;
    std::vector<Int4> adj_tri;
};
inline MeshAdjacency mesh_adjacency(const int32_t* tri, int ntri, int nver) {
    MeshAdjacency a;
    a.ptr.assign(nver + 1, 0), a.face.resize(3 * (size_t)ntri);
    for (int i = 0; i < 3 * ntri; ++i) ++a.ptr[tri[i] + 1];
    for (int v = 0; v < nver; ++v) a.ptr[v + 1] += a.ptr[v];
    std::vector<int> fill(a.ptr.begin(), a.ptr.end() - 1);
    for (int f = 0; f < ntri; ++f)
        for (int c = 0; c < 3; ++c) a.face[fill[tri[3 * f + c]]++] = f;
    a.adj_tri.resize(a.face.size());
    for (size_t e = 0; e < a.face.size(); ++e) {
        const int f = a.face[e];
        a.adj_tri[e] = Int4{tri[3 * f], tri[3 * f + 1], tri[3 * f + 2], f};
    }
    return a;
}

// The chunk face lists of the normals kernels for `chunks` vertex chunks per image (NormalChunksDev, common.hpp). built = false: the mesh
// is empty, has more than 65535 vertices, or its largest chunk does not fit the 16-bit slots or the LDS table (table_lds_bytes:
// normal_table_lds_bytes of sim3dr_kernels.hip, passed in so that this header stands alone).
struct NormalChunkPlan {
    bool built = false;
    int chunks = 0, vpb = 0, max_faces = 0;
    std::vector<int> face_ptr;          // [chunks + 1] the running sum of the chunk list lengths
    std::vector<int> full_groups;       // [chunks] groups of 32 at the front of each list that hold 32 distinct banks per corner
    std::vector<UInt2> faces;           // (i0 | i1 << 16, i2), chunk after chunk
    std::vector<unsigned short> slot;   // [3*ntri] aligned with MeshAdjacency::face: position of face[e] in the list of its vertex's chunk
    std::vector<UInt4> row8;            // [nver] the first eight slots as 8 x u16 (0xFFFF = no more faces; more than eight: 0xFFFE in the last)
};
inline NormalChunkPlan plan_normal_chunks(const int32_t* tri, int ntri, int nver, const MeshAdjacency& adj, int chunks,
                                          size_t (*table_lds_bytes)(int nver, int max_faces)) {
    NormalChunkPlan P;
    if (!(nver > 0 && ntri > 0 && nver <= 65535)) return P;
    const std::vector<int>& ptr = adj.ptr;
    const int vpb = (nver + chunks - 1) / chunks;
    std::vector<int> fptr(chunks + 1, 0), slot(adj.face.size(), 0);
    std::vector<std::vector<Int4>> lists(chunks);
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
                lists[ch].push_back(Int4{tri[3 * f], tri[3 * f + 1], tri[3 * f + 2], f});
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
    P.full_groups.assign(chunks, 0);
    for (int ch = 0; ch < chunks; ++ch) {
        std::vector<Int4>& L = lists[ch];
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
            if (members[g].size() == 32) order.insert(order.end(), members[g].begin(), members[g].end()), ++P.full_groups[ch];
        for (int g = 0; g < ngroups; ++g)
            if (members[g].size() != 32) order.insert(order.end(), members[g].begin(), members[g].end());
        order.insert(order.end(), spill.begin(), spill.end());
        std::vector<int> new_of(n);
        std::vector<Int4> R(n);
        for (int np = 0; np < n; ++np) new_of[order[np]] = np, R[np] = L[order[np]];
        L.swap(R);
        const int lo = ch * vpb, hi = std::min(nver, lo + vpb);
        for (int v = lo; v < hi; ++v)
            for (int e = ptr[v]; e < ptr[v + 1]; ++e) slot[e] = new_of[slot[e]];
    }
    int max_faces = 0;
    for (int ch = 0; ch < chunks; ++ch) {
        fptr[ch] = (int)P.faces.size();
        for (const Int4& f : lists[ch]) P.faces.push_back(UInt2{(unsigned)f.x | ((unsigned)f.y << 16), (unsigned)f.z});
        max_faces = std::max(max_faces, (int)lists[ch].size());
    }
    fptr[chunks] = (int)P.faces.size();
    if (max_faces > 65535 || table_lds_bytes(nver, max_faces) > 160 * 1024 - 1024) return P;
    P.slot.assign(slot.begin(), slot.end());
    P.row8.resize(nver);
    for (int v = 0; v < nver; ++v) {
        unsigned short r[8];
        const int deg = ptr[v + 1] - ptr[v];
        for (int j = 0; j < 8; ++j) r[j] = j < deg ? P.slot[ptr[v] + j] : (unsigned short)0xFFFF;
        if (deg > 8) r[7] = 0xFFFE;
        P.row8[v] = UInt4{r[0] | ((unsigned)r[1] << 16), r[2] | ((unsigned)r[3] << 16), r[4] | ((unsigned)r[5] << 16), r[6] | ((unsigned)r[7] << 16)};
    }
    if (max_faces >= 0xFFFE) return P;
    P.built = true, P.chunks = chunks, P.vpb = vpb, P.max_faces = max_faces;
    P.face_ptr.swap(fptr);
    return P;
}

// Texel coordinates per triangle corner, [ntri][2] (x0 y0 x1 y1 | x2 y2 - -): `corner` reads row tex_triangles[i] for x and y; `ref`, the
// reference's indexing (rasterize_kernel.cpp:398-403), reads row tri[i] of tex_coords for y -- possible (ref_ok) when the rows have three
// floats and every mesh index is a row
struct TexcoordTables {
    bool ref_ok = false;
    std::vector<Float4> corner, ref;
};
inline TexcoordTables plan_texcoords(const std::vector<int>& tri, const float* tex_coords, int n_tex, int stride, const int32_t* tex_triangles) {
    TexcoordTables T;
    const size_t nt = tri.size() / 3;
    bool ref_ok = stride == 3;
    for (size_t i = 0; i < 3 * nt && ref_ok; ++i) ref_ok = tri[i] < n_tex;
    T.ref_ok = ref_ok;
    T.corner.resize(2 * nt), T.ref.resize(ref_ok ? 2 * nt : 0);
    for (size_t f = 0; f < nt; ++f) {
        float cx[3], cy[3], ry[3];
        for (int k = 0; k < 3; ++k) {
            const size_t t = (size_t)tex_triangles[3 * f + k];
            cx[k] = tex_coords[stride * t], cy[k] = tex_coords[stride * t + 1];
            ry[k] = ref_ok ? tex_coords[stride * (size_t)tri[3 * f + k] + 1] : 0.0f;
        }
        T.corner[2 * f] = Float4{cx[0], cy[0], cx[1], cy[1]};
        T.corner[2 * f + 1] = Float4{cx[2], cy[2], 0.0f, 0.0f};
        if (ref_ok) {
            T.ref[2 * f] = Float4{cx[0], ry[0], cx[1], ry[1]};
            T.ref[2 * f + 1] = Float4{cx[2], ry[2], 0.0f, 0.0f};
        }
    }
    return T;
}

// UV map: vertex -> faces in ascending face order, each face once with its multiplicity in w: the rows of psbody's faces_by_vertex
// CSR after scipy summed the duplicate (vertex, face) entries
struct UvAdjacency {
    std::vector<int> ptr;
    std::vector<Int4> adj;
};
inline UvAdjacency uv_adjacency(const int32_t* faces, int ntri, int nver) {
    UvAdjacency a;
    a.ptr.assign(nver + 1, 0);
    std::vector<std::vector<Int4>> rows(nver);
    for (int f = 0; f < ntri; ++f) {
        const int* t = faces + 3 * (size_t)f;
        for (int c = 0; c < 3; ++c) {
            std::vector<Int4>& r = rows[t[c]];
            if ((c > 0 && t[c] == t[0]) || (c == 2 && t[c] == t[1])) {
                ++r.back().w;  // the same face names this vertex again
                continue;
            }
            r.push_back(Int4{t[0], t[1], t[2], 1});
        }
    }
    for (int v = 0; v < nver; ++v) a.ptr[v + 1] = a.ptr[v] + (int)rows[v].size();
    a.adj.reserve(a.ptr[nver]);
    for (int v = 0; v < nver; ++v) a.adj.insert(a.adj.end(), rows[v].begin(), rows[v].end());
    return a;
}

// UV map: texel -> candidates, descending candidate index: the first that passes is the reference's last writer
struct UvTexelTables {
    std::vector<int> tptr, verts;  // [n_tex + 1], [n][3]
    std::vector<double> bary;      // [n][3]
};
inline UvTexelTables uv_texel_tables(const int32_t* cand_texel, const int32_t* cand_verts, const double* cand_bary, int n, int n_tex) {
    UvTexelTables T;
    T.tptr.assign(n_tex + 1, 0);
    for (int i = 0; i < n; ++i) ++T.tptr[cand_texel[i] + 1];
    for (int t = 0; t < n_tex; ++t) T.tptr[t + 1] += T.tptr[t];
    std::vector<int> fill(T.tptr.begin(), T.tptr.end() - 1);
    T.verts.resize(3 * (size_t)n), T.bary.resize(3 * (size_t)n);
    for (int i = n - 1; i >= 0; --i) {
        const int j = fill[cand_texel[i]]++;
        for (int c = 0; c < 3; ++c) T.verts[3 * (size_t)j + c] = cand_verts[3 * (size_t)i + c], T.bary[3 * (size_t)j + c] = cand_bary[3 * (size_t)i + c];
    }
    return T;
}

}  // namespace plan
}  // namespace dad3d
