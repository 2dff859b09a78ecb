// orient_passes.hpp -- the union-find passes of the mesh orientation (csrc/mesh_orient.hip) on uf_find / uf_unite of
// uf_passes.hpp, unchanged, over the orientation double cover: node 2 f is face f as given, node 2 f + 1 is face f reversed.  Like
// topo_passes.hpp the bodies compile for the device and, unchanged, as host C++ (tests/orient_host_check.cpp runs them on many host
// threads).  Every index read from a table is checked before it is used: arrays that nsa_mesh_edges did not write give meaningless
// labels, never an access out of bounds.
#pragma once
#include <cstdint>
#include "uf_passes.hpp"

namespace nsa {

// one call per edge e < E: an edge with exactly two half-edges joins its two faces.  Half-edge 3 f + k runs faces[f][k] ->
// faces[f][(k + 1) % 3]; the faces AGREE when the two run in opposite directions (they start at different ends of the edge).
// agree: 2 f ~ 2 g and 2 f + 1 ~ 2 g + 1; disagree: 2 f ~ 2 g + 1 and 2 f + 1 ~ 2 g
NSA_UF_FN void orient_pass_join(int32_t* parent, uint32_t F, const int32_t* faces, const int32_t* edge_start,
                                const int32_t* edge_halfedges, uint32_t e, uint32_t E, uint32_t* status) {
    const uint32_t H = 3u * F;
    if (e >= E || e >= H) return;
    const int32_t s = edge_start[e], t = edge_start[e + 1];
    if (s < 0 || t != s + 2 || (uint32_t)t > H) return;                      // one half-edge, or three and more: joins nothing
    const int32_t h0 = edge_halfedges[s], h1 = edge_halfedges[s + 1];
    if (h0 < 0 || h1 < 0 || (uint32_t)h0 >= H || (uint32_t)h1 >= H) return;
    const int32_t f = h0 / 3, g = h1 / 3;
    if (f == g) return;                                                      // (never: a contributing face has three distinct edges)
    const bool agree = faces[h0] != faces[h1];                               // faces[3 f + k]: where half-edge 3 f + k starts
    uf_unite(parent, 2 * f, 2 * g + (agree ? 0 : 1), 2u * F, status);
    uf_unite(parent, 2 * f + 1, 2 * g + (agree ? 1 : 0), 2u * F, status);
}

// one call per face after every call of orient_pass_join has returned.  r0 = find(2 f), r1 = find(2 f + 1):
// label = min(r0, r1) >> 1 (-1 for a face that does not contribute), orientable = r0 != r1, flip = orientable and r0 > r1
NSA_UF_FN int32_t orient_pass_label(int32_t* parent, uint32_t F, const int32_t* face_edges, uint32_t f, uint8_t* orientable,
                                    uint8_t* flip, uint32_t* status) {
    *orientable = 0;
    *flip = 0;
    if (face_edges[3ull * f] < 0) return -1;
    const int32_t r0 = uf_find(parent, (int32_t)(2u * f), 2u * F, status), r1 = uf_find(parent, (int32_t)(2u * f + 1u), 2u * F, status);
    *orientable = r0 != r1;
    *flip = r0 > r1;                                                         // (r0 > r1 implies r0 != r1)
    return (r0 < r1 ? r0 : r1) >> 1;
}

}  // namespace nsa
