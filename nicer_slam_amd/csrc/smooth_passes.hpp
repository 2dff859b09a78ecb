// smooth_passes.hpp -- the per-item bodies of mesh smoothing (csrc/mesh_smooth.hip): the vertex ring's offsets, fill and
// row lookup, the per-vertex state and neighbour list, one vertex's step and one vertex's normal.  Like topo_passes.hpp and
// orient_passes.hpp the bodies compile for the device and, unchanged, as host C++ (tests/smooth_host_check.cpp calls them one item
// at a time and is held to tests/smooth_ref.py bit for bit).  Every floating-point operation is rounded on its own: the pragma below
// keeps clang from contracting a * b + c, a host compiler that does not know it is given -ffp-contract=off.  Every index read from a
// table is checked before it is used: arrays that the earlier entry points did not write give meaningless results, never an access
// out of bounds.
#pragma once
#include <cmath>
#include <cstdint>
#include "bulk_grid.hpp"

#if defined(__HIPCC__)
#define NSA_SM_FN __host__ __device__ inline
#else
#define NSA_SM_FN static inline
#endif
#if defined(__clang__)
#define NSA_SM_EXACT _Pragma("clang fp contract(off)")
#else
#define NSA_SM_EXACT
#endif

namespace nsa {
namespace smooth {

constexpr uint8_t kLive = 1, kOnBoundary = 2, kMoves = 4, kSteps = 8;    // the state byte of a vertex
constexpr int kFree = 0, kFixed = 1, kCurve = 2;                         // NSA_SMOOTH_*
constexpr int kArea = 0, kAngle = 1;                                     // NSA_NORMALS_*

NSA_SM_FN bool finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; }      // false for a NaN

// ---- the vertex ring ----------------------------------------------------------------------------------------------------------------

// the end `which` (0: lo, 1: hi) of edge i, or V when i is no edge or one of its ends lies outside [0, V)
NSA_SM_FN uint32_t ring_key(const int32_t* edges, uint32_t E, uint32_t V, uint32_t i, int which) {
    if (i >= E) return V;
    const uint32_t lo = (uint32_t)edges[2ull * i], hi = (uint32_t)edges[2ull * i + 1];
    return lo < V && hi < V ? (which ? hi : lo) : V;
}

// one call per v in [0, V]: lo[0, H) are the lo keys in edge order, hs[0, H) the hi keys in (hi, lo) order, both ascending.
// below_lo[v] = #{lo < v}, below_hi[v] = #{hi < v}, ring_start[v] = their sum
NSA_SM_FN void ring_pass_start(const uint32_t* lo, const uint32_t* hs, uint32_t H, uint32_t v, int32_t* below_lo, int32_t* below_hi,
                               int32_t* ring_start) {
    const uint32_t a = bulk::lower_bound(lo, H, v), b = bulk::lower_bound(hs, H, v);
    below_lo[v] = (int32_t)a;
    below_hi[v] = (int32_t)b;
    ring_start[v] = (int32_t)(a + b);
}

// one call per i in [0, H).  As a position of the (hi, lo) order: edge order[i] = {u, v}, u < v, enters row v as neighbour u, at
// ring_start[v] + (i - below_hi[v]) = below_lo[v] + i.  As an edge id: edge i = {v, u}, v < u, enters row v as neighbour u after the
// row's lower neighbours, at ring_start[v] + (below_hi[v + 1] - below_hi[v]) + (i - below_lo[v]) = below_hi[v + 1] + i.
NSA_SM_FN void ring_pass_fill(const int32_t* edges, uint32_t E, const uint32_t* hs, const uint32_t* order, const int32_t* below_lo,
                              const int32_t* below_hi, uint32_t H, uint32_t V, uint32_t cap, uint32_t i, int32_t* ring,
                              int32_t* ring_edge) {
    const uint32_t hv = hs[i], e = order[i];
    if (hv < V && e < H) {
        const uint32_t u = ring_key(edges, E, V, e, 0), slot = (uint32_t)below_lo[hv] + i;
        if (u < V && slot < cap) {
            ring[slot] = (int32_t)u;
            ring_edge[slot] = (int32_t)e;
        }
    }
    const uint32_t lv = ring_key(edges, E, V, i, 0);
    if (lv < V) {
        const uint32_t slot = (uint32_t)below_hi[lv + 1] + i;
        if (slot < cap) {
            ring[slot] = (int32_t)ring_key(edges, E, V, i, 1);
            ring_edge[slot] = (int32_t)i;
        }
    }
}

// row v of the ring: the entries [*s, *e) of ring and ring_edge; empty when v or the offsets lie outside their range
NSA_SM_FN void ring_row(const int32_t* ring_start, uint32_t V, uint32_t cap, uint32_t v, uint32_t* s, uint32_t* e) {
    *s = *e = 0;
    if (v >= V) return;
    const int32_t a = ring_start[v], b = ring_start[v + 1];
    if (a < 0 || b < a || (uint32_t)b > cap) return;
    *s = (uint32_t)a;
    *e = (uint32_t)b;
}

// ---- smoothing ------------------------------------------------------------------------------------------------------------------------

// one call per vertex: x0 = double(verts[v]) into pos0, and the state byte -- live, on the boundary, moves.  H = edges the table holds
NSA_SM_FN uint8_t smooth_pass_state(const float* verts, const int32_t* ring_start, const int32_t* ring_edge, const int32_t* edge_count,
                                    const uint8_t* fixed, uint32_t V, uint32_t cap, uint32_t H, int boundary, uint32_t v, double* pos0) {
    bool finite = true;
    for (int k = 0; k < 3; ++k) {
        const double x = (double)verts[3ull * v + k];
        pos0[3ull * v + k] = x;
        finite = finite && finite_d(x);
    }
    uint32_t s, e;
    ring_row(ring_start, V, cap, v, &s, &e);
    bool on_boundary = false;
    for (uint32_t j = s; j < e; ++j) {
        const uint32_t ed = (uint32_t)ring_edge[j];
        on_boundary = on_boundary || (ed < H && edge_count[ed] == 1);
    }
    const bool live = finite && e > s;
    const bool moves = live && !(fixed && fixed[v] != 0) && !(boundary == kFixed && on_boundary);
    return (uint8_t)((live ? kLive : 0) | (on_boundary ? kOnBoundary : 0) | (moves ? kMoves : 0));
}

// one call per vertex after every call of smooth_pass_state has returned: N'(v) in row order into member[ring_start[v] ...), its size
// into count[v] (0 for a vertex that does not move: it keeps its input).  Returns the state with kSteps set when count[v] > 0
NSA_SM_FN uint8_t smooth_pass_members(const int32_t* ring_start, const int32_t* ring, const int32_t* ring_edge, const int32_t* edge_count,
                                      const uint8_t* state, uint32_t V, uint32_t cap, uint32_t H, int boundary, uint32_t v,
                                      int32_t* member, int32_t* count) {
    const uint8_t st = state[v];
    uint32_t s, e, n = 0;
    ring_row(ring_start, V, cap, v, &s, &e);
    if (st & kMoves) {
        const bool along = boundary == kCurve && (st & kOnBoundary);
        for (uint32_t j = s; j < e; ++j) {
            const uint32_t u = (uint32_t)ring[j], ed = (uint32_t)ring_edge[j];
            if (u >= V || !(state[u] & kLive)) continue;
            if (along && !(ed < H && edge_count[ed] == 1)) continue;
            member[s + n++] = (int32_t)u;
        }
    }
    count[v] = (int32_t)n;
    return (uint8_t)(st | (n ? kSteps : 0));
}

// one vertex's step with factor f from the positions cur: y = x + f (mean of N' - x), clamped per component to x0 +- max_move when
// clamp is set.  False (and y = x) for a vertex that keeps its input
NSA_SM_FN bool smooth_pass_step(const double* cur, const float* verts, const int32_t* ring_start, const int32_t* member,
                                const int32_t* count, uint32_t V, uint32_t cap, uint32_t v, double f, double max_move, bool clamp,
                                double (&y)[3]) {
    NSA_SM_EXACT
    for (int k = 0; k < 3; ++k) y[k] = cur[3ull * v + k];
    const int32_t n = count[v], s = ring_start[v];
    if (n <= 0 || s < 0 || (uint64_t)s + (uint64_t)n > cap) return false;
    double sum[3] = {0.0, 0.0, 0.0};
    for (int32_t j = 0; j < n; ++j) {
        const uint32_t u = (uint32_t)member[s + j];
        if (u >= V) return false;                                        // (never: smooth_pass_members wrote vertices)
        for (int k = 0; k < 3; ++k) sum[k] = j ? sum[k] + cur[3ull * u + k] : cur[3ull * u + k];
    }
    for (int k = 0; k < 3; ++k) {
        const double m = sum[k] / (double)n;
        const double d = m - y[k];
        double r = y[k] + f * d;
        if (clamp) {
            const double x0 = (double)verts[3ull * v + k], lo = x0 - max_move, hi = x0 + max_move;
            r = r < lo ? lo : r;
            r = r > hi ? hi : r;
        }
        y[k] = r;
    }
    return true;
}

// ---- vertex normals -------------------------------------------------------------------------------------------------------------------

// corner c = 3 f + k of a face that contributes (indices in [0, V), pairwise distinct) and whose three vertices are finite: its vertex,
// the next and the previous vertex of the face into p; false otherwise
NSA_SM_FN bool normal_corner(const float* verts, uint32_t V, const int32_t* faces, uint32_t F, uint32_t c, double (&p)[3][3]) {
    const uint32_t f = c / 3u, k = c - 3u * f;
    if (f >= F) return false;
    const uint32_t i0 = (uint32_t)faces[3ull * f], i1 = (uint32_t)faces[3ull * f + 1], i2 = (uint32_t)faces[3ull * f + 2];
    if (i0 >= V || i1 >= V || i2 >= V || i0 == i1 || i1 == i2 || i2 == i0) return false;
    const uint32_t idx[3] = {k == 0 ? i0 : k == 1 ? i1 : i2, k == 0 ? i1 : k == 1 ? i2 : i0, k == 0 ? i2 : k == 1 ? i0 : i1};
    bool finite = true;
    for (int j = 0; j < 3; ++j)
        for (int d = 0; d < 3; ++d) {
            p[j][d] = (double)verts[3ull * idx[j] + d];
            finite = finite && finite_d(p[j][d]);
        }
    return finite;
}

// the key of corner c in the corner-by-vertex sort: its vertex, V when the corner takes no part
NSA_SM_FN uint32_t normal_corner_key(const float* verts, uint32_t V, const int32_t* faces, uint32_t F, uint32_t c) {
    double p[3][3];
    return normal_corner(verts, V, faces, F, c, p) ? (uint32_t)faces[c] : V;
}

// one vertex's normal: over corner[s, e) -- its corners in ascending id -- N = sum of n = (p1 - p0) x (p2 - p0) (area) or of
// theta n / |n| with theta = atan2(|n|, (p1 - p0) . (p2 - p0)), corners with |n| = 0 skipped (angle); out = N / |N| rounded to fp32,
// zero when |N| is zero or not finite
NSA_SM_FN void normal_pass_vertex(const float* verts, uint32_t V, const int32_t* faces, uint32_t F, const uint32_t* corner, uint32_t s,
                                  uint32_t e, int weighting, float (&out)[3]) {
    NSA_SM_EXACT
    double N[3] = {0.0, 0.0, 0.0};
    for (uint32_t t = s; t < e; ++t) {
        double p[3][3], a[3], b[3], n[3];
        if (!normal_corner(verts, V, faces, F, corner[t], p)) continue;
        for (int d = 0; d < 3; ++d) {
            a[d] = p[1][d] - p[0][d];
            b[d] = p[2][d] - p[0][d];
        }
        n[0] = a[1] * b[2] - a[2] * b[1];
        n[1] = a[2] * b[0] - a[0] * b[2];
        n[2] = a[0] * b[1] - a[1] * b[0];
        if (weighting == kAngle) {
            const double len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
            if (!(len > 0.0)) continue;
            const double theta = atan2(len, (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]);
            for (int d = 0; d < 3; ++d) N[d] = N[d] + theta * (n[d] / len);
        } else {
            for (int d = 0; d < 3; ++d) N[d] = N[d] + n[d];
        }
    }
    const double len = sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]);
    const bool ok = len > 0.0 && finite_d(len);
    for (int d = 0; d < 3; ++d) out[d] = ok ? (float)(N[d] / len) : 0.0f;
}

}  // namespace smooth
}  // namespace nsa
