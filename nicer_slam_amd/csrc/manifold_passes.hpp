// manifold_passes.hpp -- the per-item bodies of the fan split (csrc/mesh_manifold.hip; C ABI Section 26) on uf_find /
// uf_unite of uf_passes.hpp, unchanged.  Like topo_passes.hpp the bodies compile for the device and, unchanged, as host C++, so that
// many host threads can run them in a CPU test (tests/manifold_host_check.cpp).  Every index read from a table is checked before it is
// used: arrays that nsa_mesh_edges did not write for these faces give meaningless fans, never an access out of bounds.
//
// Corners: c = 3 f + k of a contributing face (face_edges[3 f] >= 0) sits at vertex faces[c].  The union-find runs over the 3 F corners;
// parent[x] <= x, so the root of a fan is its smallest corner -- the LEADER -- whatever the interleaving.
#pragma once
#include <cstdint>
#include "uf_passes.hpp"

namespace nsa {

constexpr uint32_t kSplitCutInconsistent = 1u;           // flags (NSA_SPLIT_CUT_INCONSISTENT)

NSA_UF_FN uint32_t mf_next(uint32_t c) { return c % 3u == 2u ? c - 2u : c + 1u; }          // the next corner of the same face

// the vertex of corner c, V when the corner is out of range or its face does not contribute or the index is no vertex
NSA_UF_FN uint32_t mf_corner_vertex(const int32_t* faces, const int32_t* face_edges, uint32_t H, uint32_t V, uint32_t c) {
    if (c >= H || face_edges[c - c % 3u] < 0) return V;
    const int32_t v = faces[c];
    return v >= 0 && (uint32_t)v < V ? (uint32_t)v : V;
}

// the regular-edge test of edge e, on whose run the half-edges h0 < h1 lie: two half-edges, traversed once each way when the flag
// asks for it, and both faces of one label when labels are given
NSA_UF_FN bool mf_regular(int32_t count, int32_t forward, uint32_t flags, const int32_t* face_label, uint32_t h0, uint32_t h1) {
    if (count != 2) return false;
    if ((flags & kSplitCutInconsistent) && forward != 1) return false;
    return !face_label || face_label[h0 / 3u] == face_label[h1 / 3u];
}

// the join pass, one call per edge e < E.  A regular edge (lo, hi) unites its two faces' corners at lo, and their corners at hi; a cut
// edge (count >= 2, not regular) marks its two ends (on_cut = 1, the same value from every edge).  Returns whether the edge is cut.
NSA_UF_FN bool mf_pass_join(int32_t* parent, int32_t* on_cut, const int32_t* faces, uint32_t F, uint32_t V, const int32_t* face_label,
                            uint32_t flags, const int32_t* edges, const int32_t* edge_count, const int32_t* edge_forward,
                            const int32_t* edge_start, const int32_t* edge_halfedges, const int32_t* face_edges, uint32_t e,
                            uint32_t* status) {
    const uint32_t H = 3u * F;
    const int32_t count = edge_count[e], s = edge_start[e];
    const int32_t lo = edges[2ull * e], hi = edges[2ull * e + 1];
    if (count < 2 || s < 0 || (uint32_t)s >= H || (uint32_t)s + 1u >= H) return false;
    if (lo < 0 || hi < 0 || (uint32_t)lo >= V || (uint32_t)hi >= V || lo == hi) return false;
    const int32_t h0 = edge_halfedges[s], h1 = edge_halfedges[s + 1];
    if (h0 < 0 || h1 < 0 || (uint32_t)h0 >= H || (uint32_t)h1 >= H || h0 / 3 == h1 / 3) return false;
    if (!mf_regular(count, edge_forward[e], flags, face_label, (uint32_t)h0, (uint32_t)h1)) {
        uf_store(on_cut + lo, 1);
        uf_store(on_cut + hi, 1);
        return true;
    }
    // half-edge h runs from corner h to corner mf_next(h): one of them sits at lo, the other at hi
    const uint32_t a0 = mf_corner_vertex(faces, face_edges, H, V, (uint32_t)h0), a1 = mf_corner_vertex(faces, face_edges, H, V, (uint32_t)h1);
    const uint32_t b0 = mf_corner_vertex(faces, face_edges, H, V, mf_next((uint32_t)h0));
    const uint32_t b1 = mf_corner_vertex(faces, face_edges, H, V, mf_next((uint32_t)h1));
    const uint32_t ulo = (uint32_t)lo, uhi = (uint32_t)hi;
    if (!((a0 == ulo && b0 == uhi) || (a0 == uhi && b0 == ulo)) || !((a1 == ulo && b1 == uhi) || (a1 == uhi && b1 == ulo))) return false;
    const int32_t l0 = (int32_t)(a0 == ulo ? (uint32_t)h0 : mf_next((uint32_t)h0)), l1 = (int32_t)(a1 == ulo ? (uint32_t)h1 : mf_next((uint32_t)h1));
    const int32_t g0 = (int32_t)(a0 == uhi ? (uint32_t)h0 : mf_next((uint32_t)h0)), g1 = (int32_t)(a1 == uhi ? (uint32_t)h1 : mf_next((uint32_t)h1));
    uf_unite(parent, l0, l1, H, status);
    uf_unite(parent, g0, g1, H, status);
    return false;
}

// the leader pass, one call per corner c < 3 F after every call of mf_pass_join has returned: the corner's fan (-1 for a corner of a
// face that does not contribute) and its sort key -- the vertex for a leader, V for every other corner, which sorts last.  The
// leader flag is fan == c.
NSA_UF_FN int32_t mf_pass_leader(int32_t* parent, const int32_t* faces, const int32_t* face_edges, uint32_t F, uint32_t V, uint32_t c,
                                 uint32_t* key, uint32_t* status) {
    const uint32_t H = 3u * F, v = mf_corner_vertex(faces, face_edges, H, V, c);
    *key = V;
    if (v == V) return -1;
    const int32_t fan = uf_find(parent, (int32_t)c, H, status);
    if (fan == (int32_t)c) *key = v;
    return fan;
}

// the fan at sorted position i, if there is one: order[] is the stable argsort of the keys, so the leaders come first, in ascending
// (vertex, leader).  Returns the leader corner and its vertex; false for a position past the fans.
NSA_UF_FN bool mf_fan_at(const int32_t* corner_fan, const int32_t* faces, const int32_t* face_edges, const uint32_t* order, uint32_t H,
                         uint32_t V, uint32_t i, uint32_t* corner, uint32_t* vertex) {
    if (i >= H) return false;
    const uint32_t c = order[i];
    if (c >= H || corner_fan[c] != (int32_t)c) return false;
    const uint32_t v = mf_corner_vertex(faces, face_edges, H, V, c);
    if (v == V) return false;
    *corner = c;
    *vertex = v;
    return true;
}

// the run-head flag of sorted position i: 0 no fan here, 1 the first fan of its vertex (it keeps the name), 2 a further fan
NSA_UF_FN int mf_run_head(const int32_t* corner_fan, const int32_t* faces, const int32_t* face_edges, const uint32_t* order, uint32_t H,
                          uint32_t V, uint32_t i, uint32_t* corner, uint32_t* vertex) {
    if (!mf_fan_at(corner_fan, faces, face_edges, order, H, V, i, corner, vertex)) return 0;
    uint32_t pc, pv;
    if (i == 0 || !mf_fan_at(corner_fan, faces, face_edges, order, H, V, i - 1, &pc, &pv)) return 1;
    return pv == *vertex ? 2 : 1;
}

// the name pass, one call per sorted position i with r = the further fans before it (the exclusive scan of kind == 2): the fan's
// name into fan_name[leader]; a further fan records its source; the first and the last fan of a vertex leave r there, so that
// vertex_fans = last - first + 1 (mf_vertex_fans)
NSA_UF_FN void mf_pass_name(const int32_t* corner_fan, const int32_t* faces, const int32_t* face_edges, const uint32_t* order, uint32_t F,
                            uint32_t V, uint32_t i, uint32_t r, int32_t* fan_name, int32_t* new_source, int32_t* first_r, int32_t* last_r) {
    const uint32_t H = 3u * F;
    uint32_t c, v, nc, nv;
    const int kind = mf_run_head(corner_fan, faces, face_edges, order, H, V, i, &c, &v);
    if (kind == 0 || r >= H) return;
    fan_name[c] = kind == 1 ? (int32_t)v : (int32_t)(V + r);
    if (kind == 2) new_source[r] = (int32_t)v;
    else first_r[v] = (int32_t)r;
    if (mf_run_head(corner_fan, faces, face_edges, order, H, V, i + 1, &nc, &nv) != 2) last_r[v] = (int32_t)(r + (kind == 2 ? 1u : 0u));
}

// one call per vertex after the name pass: its number of fans (first_r was set to -1 before the name pass: an unused vertex)
NSA_UF_FN int32_t mf_vertex_fans(const int32_t* first_r, const int32_t* last_r, uint32_t v) {
    const int32_t a = first_r[v], b = last_r[v];
    return a < 0 || b < a ? 0 : b - a + 1;
}

// the face rewrite, one call per corner c < 3 F: a contributing face is renamed by fan; another face is copied, except that an index
// >= V becomes -1 (no such face reaches a new vertex)
NSA_UF_FN int32_t mf_pass_face(const int32_t* faces, const int32_t* corner_fan, const int32_t* fan_name, uint32_t F, uint32_t V, uint32_t c) {
    const uint32_t H = 3u * F;
    const int32_t fan = corner_fan[c], x = faces[c];
    if (fan >= 0 && (uint32_t)fan < H) return fan_name[fan];
    return x >= 0 && (uint32_t)x >= V ? -1 : x;
}

}  // namespace nsa
