// topo_passes.hpp -- the union-find passes of the mesh topology (csrc/mesh_topology.hip) on uf_find / uf_unite of
// uf_passes.hpp, unchanged.  Like those, the bodies compile for the device and, unchanged, as host C++, so that many host threads can
// run them in a CPU test (tests/topology_host_check.cpp).  Every index read from a table is checked before it is used: arrays that
// nsa_mesh_edges did not write give meaningless labels, never an access out of bounds.
#pragma once
#include <cstdint>
#include "uf_passes.hpp"

namespace nsa {

// boundary loops, one call per edge e with its half-edge count: a boundary edge marks its two ends (boundary_mark = 0, the same value
// from every edge) and joins them in the union-find over the V vertices
NSA_UF_FN void topo_pass_boundary(int32_t* parent, int32_t* boundary_mark, uint32_t V, const int32_t* edges, uint32_t e, int32_t count,
                                  uint32_t* status) {
    if (count != 1) return;
    const int32_t a = edges[2ull * e], b = edges[2ull * e + 1];
    if (a < 0 || b < 0 || (uint32_t)a >= V || (uint32_t)b >= V) return;
    uf_store(boundary_mark + a, 0);
    uf_store(boundary_mark + b, 0);
    uf_unite(parent, a, b, V, status);
}

// face components, one call per sorted position i of edge_halfedges[3 F]: a half-edge that is not the first of its edge's run joins its
// face with its predecessor's in the union-find over the F faces
NSA_UF_FN void topo_pass_join(int32_t* parent, uint32_t F, const int32_t* face_edges, const int32_t* edge_start,
                              const int32_t* edge_halfedges, uint32_t i, uint32_t* status) {
    const uint32_t H = 3u * F;
    if (i == 0 || i >= H) return;
    const int32_t h = edge_halfedges[i], hp = edge_halfedges[i - 1];
    if (h < 0 || hp < 0 || (uint32_t)h >= H || (uint32_t)hp >= H) return;
    const int32_t e = face_edges[h];
    if (e < 0 || (uint32_t)e >= H || edge_start[e] == (int32_t)i) return;       // the head of its run
    uf_unite(parent, h / 3, hp / 3, F, status);
}

// face components, one call per face after every call of topo_pass_join has returned: the label (-1 for a face that does not contribute)
NSA_UF_FN int32_t topo_pass_label(int32_t* parent, uint32_t F, const int32_t* face_edges, uint32_t f, uint32_t* status) {
    return face_edges[3ull * f] >= 0 ? uf_find(parent, (int32_t)f, F, status) : -1;
}

}  // namespace nsa
