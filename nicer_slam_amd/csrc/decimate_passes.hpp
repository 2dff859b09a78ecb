// decimate_passes.hpp -- the per-item bodies of edge-collapse decimation (csrc/mesh_decimate.hip; header Section 22): the
// initial quadric and the lock of a vertex, one edge's placement, cost, link count and fold test, the two minimum passes and the
// selection, the prefix rule, and the application of one collapse.  Like smooth_passes.hpp the bodies compile for the device and,
// unchanged, as host C++ (tests/decimate_host_check.cpp calls them one item at a time and is held to tests/decimate_ref.py bit for
// bit).  Float64 throughout, + - * / only, every operation rounded on its own: the pragma keeps clang from contracting a * b + c, a
// host compiler that does not know it is given -ffp-contract=off.  Every index read from a table is checked before it is used, and
// every loop runs over a row or a run whose ends were checked against the table's length.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include "smooth_passes.hpp"

namespace nsa {
namespace decimate {

using smooth::finite_d;
using smooth::ring_row;

constexpr int kQuadric = 0, kFixed = 1;                                  // NSA_DECIMATE_BOUNDARY_*
constexpr uint8_t kCandidate = 0, kRejLock = 1, kRejError = 2, kRejLink = 3, kRejFold = 4, kNoEdge = 5;      // the code of an edge
constexpr uint64_t kNoKey = 0xFFFFFFFFFFFFFFFFull;
constexpr uint32_t kNoEdgeId = 0xFFFFFFFFu;
constexpr int kQ = 11;                                                   // a00 a01 a02 a11 a12 a22 b0 b1 b2 c w

NSA_SM_FN uint64_t bits_of(double x) {
    uint64_t u;
    memcpy(&u, &x, 8);
    return u;
}

NSA_SM_FN double dot3(const double* u, const double* w) {
    NSA_SM_EXACT
    return (u[0] * w[0] + u[1] * w[1]) + u[2] * w[2];
}

NSA_SM_FN void cross3(const double* u, const double* w, double* n) {
    NSA_SM_EXACT
    n[0] = u[1] * w[2] - u[2] * w[1];
    n[1] = u[2] * w[0] - u[0] * w[2];
    n[2] = u[0] * w[1] - u[1] * w[0];
}

// n = (p1 - p0) x (p2 - p0)
NSA_SM_FN void face_normal(const double* p0, const double* p1, const double* p2, double* n) {
    NSA_SM_EXACT
    double a[3], b[3];
    for (int d = 0; d < 3; ++d) {
        a[d] = p1[d] - p0[d];
        b[d] = p2[d] - p0[d];
    }
    cross3(a, b, n);
}

// q += s * (n n^T, n d, d^2, n . n) with d = -(n . p): the plane through p with normal n, weight s
NSA_SM_FN void add_plane(double* q, const double* n, const double* p, double s, bool scaled) {
    NSA_SM_EXACT
    const double d = -dot3(n, p);
    double sn[3];
    for (int k = 0; k < 3; ++k) sn[k] = scaled ? s * n[k] : n[k];
    q[0] = q[0] + sn[0] * n[0];
    q[1] = q[1] + sn[0] * n[1];
    q[2] = q[2] + sn[0] * n[2];
    q[3] = q[3] + sn[1] * n[1];
    q[4] = q[4] + sn[1] * n[2];
    q[5] = q[5] + sn[2] * n[2];
    q[6] = q[6] + sn[0] * d;
    q[7] = q[7] + sn[1] * d;
    q[8] = q[8] + sn[2] * d;
    const double sd = scaled ? s * d : d, nn = dot3(n, n);
    q[9] = q[9] + sd * d;
    q[10] = q[10] + (scaled ? s * nn : nn);
}

// the three float64 positions of face f when it contributes (Section 18's rule) and all nine coordinates are finite
NSA_SM_FN bool finite_face(const double* pos, uint32_t V, const int32_t* faces, uint32_t F, uint32_t f, uint32_t (&idx)[3]) {
    if (f >= F) return false;
    for (int k = 0; k < 3; ++k) idx[k] = (uint32_t)faces[3ull * f + k];
    if (idx[0] >= V || idx[1] >= V || idx[2] >= V || idx[0] == idx[1] || idx[1] == idx[2] || idx[2] == idx[0]) return false;
    bool finite = true;
    for (int k = 0; k < 3; ++k)
        for (int d = 0; d < 3; ++d) finite = finite && finite_d(pos[3ull * idx[k] + d]);
    return finite;
}

// ---- the initial state ----------------------------------------------------------------------------------------------------------------

// one call per vertex, first: x_v = double(verts[v]), the colour likewise, vertex_map[v] = v, moved[v] = 0
NSA_SM_FN void init_pass_position(const float* verts, const float* colors, uint32_t v, double* pos, double* col, int32_t* vmap,
                                  uint8_t* moved) {
    for (int k = 0; k < 3; ++k) {
        pos[3ull * v + k] = (double)verts[3ull * v + k];
        if (colors) col[3ull * v + k] = (double)colors[3ull * v + k];
    }
    vmap[v] = (int32_t)v;
    moved[v] = 0;
}

// one call per vertex after every position is written: the lock byte and the quadric.  corner[cs, ce) are the corners of v in
// ascending id (the corner-by-vertex table keyed as the vertex normals key it: finite contributing faces only); H = 3 F
NSA_SM_FN void init_pass_vertex(const double* pos, uint32_t V, const int32_t* faces, uint32_t F, const uint32_t* corner, uint32_t cs,
                                uint32_t ce, const int32_t* ring_start, const int32_t* ring, const int32_t* ring_edge,
                                const int32_t* edge_count, const int32_t* edge_start, const int32_t* edge_halfedges,
                                const uint8_t* fixed, int boundary, double boundary_weight, uint32_t v, uint8_t* locked, double* quad) {
    NSA_SM_EXACT
    const uint32_t H = 3u * F, cap = 6u * F;
    double q[kQ];
    for (int k = 0; k < kQ; ++k) q[k] = 0.0;
    bool lock = fixed && fixed[v] != 0;
    for (int d = 0; d < 3; ++d) lock = lock || !finite_d(pos[3ull * v + d]);
    // the faces, in ascending corner id
    for (uint32_t t = cs; t < ce; ++t) {
        uint32_t idx[3];
        const uint32_t c = corner[t];
        if (!finite_face(pos, V, faces, F, c / 3u, idx)) continue;
        double n[3];
        face_normal(&pos[3ull * idx[0]], &pos[3ull * idx[1]], &pos[3ull * idx[2]], n);
        add_plane(q, n, &pos[3ull * idx[0]], 1.0, false);
    }
    // then the row: locks, and the boundary planes in ascending neighbour
    uint32_t s, e;
    ring_row(ring_start, V, cap, v, &s, &e);
    for (uint32_t j = s; j < e; ++j) {
        const uint32_t u = (uint32_t)ring[j], ed = (uint32_t)ring_edge[j];
        if (u >= V || ed >= H) continue;
        for (int d = 0; d < 3; ++d) lock = lock || !finite_d(pos[3ull * u + d]);
        const int32_t cnt = edge_count[ed];
        lock = lock || cnt > 2 || (boundary == kFixed && cnt == 1);
        if (cnt != 1) continue;
        const int32_t hs = edge_start[ed];
        if (hs < 0 || (uint32_t)hs >= H) continue;
        const uint32_t h = (uint32_t)edge_halfedges[hs];
        uint32_t idx[3];
        if (h >= H || !finite_face(pos, V, faces, F, h / 3u, idx)) continue;
        const uint32_t lo = u < v ? u : v, hi = u < v ? v : u;
        double n[3], ev[3], m[3];
        face_normal(&pos[3ull * idx[0]], &pos[3ull * idx[1]], &pos[3ull * idx[2]], n);
        for (int d = 0; d < 3; ++d) ev[d] = pos[3ull * hi + d] - pos[3ull * lo + d];
        cross3(ev, n, m);
        const double ee = dot3(ev, ev);
        if (!(ee > 0.0)) continue;
        const double sc = boundary_weight / ee;
        if (!finite_d(sc)) continue;
        add_plane(q, m, &pos[3ull * lo], sc, true);
    }
    locked[v] = lock ? 1 : 0;
    for (int k = 0; k < kQ; ++k) quad[(uint64_t)kQ * v + k] = q[k];
}

// ---- one edge -------------------------------------------------------------------------------------------------------------------------

// the placement of Q (kQ values) between the ends a and b: the solution of (A + mu I) x = -b + mu m by LDL^T in the pivot order 0, 1,
// 2, or the midpoint m; and cost = max(0, x^T A x + 2 b . x + c).  False when the cost is not finite
NSA_SM_FN bool place_and_cost(const double* q, const double* a, const double* b, double eps, double (&x)[3], double* cost) {
    NSA_SM_EXACT
    double m[3];
    for (int d = 0; d < 3; ++d) m[d] = (a[d] + b[d]) * 0.5;
    const double tr = (q[0] + q[3]) + q[5];
    bool solved = false;
    if (tr != 0.0 && finite_d(tr)) {
        const double mu = eps * tr;
        const double a00 = q[0] + mu, a11 = q[3] + mu, a22 = q[5] + mu, a01 = q[1], a02 = q[2], a12 = q[4];
        const double r0 = mu * m[0] - q[6], r1 = mu * m[1] - q[7], r2 = mu * m[2] - q[8];
        const double d0 = a00;
        if (d0 > 0.0) {
            const double l10 = a01 / d0, l20 = a02 / d0;
            const double d1 = a11 - l10 * a01;
            if (d1 > 0.0) {
                const double t = a12 - l20 * a01;
                const double l21 = t / d1;
                const double d2 = (a22 - l20 * a02) - l21 * t;
                if (d2 > 0.0) {
                    const double y0 = r0, y1 = r1 - l10 * y0, y2 = (r2 - l20 * y0) - l21 * y1;
                    const double x2 = y2 / d2, x1 = y1 / d1 - l21 * x2, x0 = (y0 / d0 - l10 * x1) - l20 * x2;
                    if (finite_d(x0) && finite_d(x1) && finite_d(x2)) {
                        x[0] = x0;
                        x[1] = x1;
                        x[2] = x2;
                        solved = true;
                    }
                }
            }
        }
    }
    if (!solved)
        for (int d = 0; d < 3; ++d) x[d] = m[d];
    const double ax0 = (q[0] * x[0] + q[1] * x[1]) + q[2] * x[2];
    const double ax1 = (q[1] * x[0] + q[3] * x[1]) + q[4] * x[2];
    const double ax2 = (q[2] * x[0] + q[4] * x[1]) + q[5] * x[2];
    const double xax = (x[0] * ax0 + x[1] * ax1) + x[2] * ax2;
    const double bx = (q[6] * x[0] + q[7] * x[1]) + q[8] * x[2];
    const double c = (xax + 2.0 * bx) + q[9];
    if (!finite_d(c)) return false;
    *cost = c > 0.0 ? c : 0.0;
    return true;
}

// the tables one edge reads
struct EdgeTables {
    const int32_t* faces;        // [F, 3] the current faces
    const int32_t* edges;        // Section 18, of the current faces
    const int32_t* edge_count;
    const int32_t* edge_start;
    const int32_t* edge_halfedges;
    const int32_t* ring_start;   // Section 21, of the same table
    const int32_t* ring;
    const int32_t* ring_edge;
    const double* pos;           // [V, 3]
    const double* quad;          // [V, kQ]
    const uint8_t* locked;       // [V]
    uint32_t V, F, E;
};

// row v: is some entry on an edge with one half-edge?
NSA_SM_FN bool on_boundary(const EdgeTables& t, uint32_t s, uint32_t e) {
    bool on = false;
    for (uint32_t j = s; j < e; ++j) {
        const uint32_t ed = (uint32_t)t.ring_edge[j];
        on = on || (ed < 3u * t.F && t.edge_count[ed] == 1);
    }
    return on;
}

// the faces around `end` that do not hold `other`, each once: true when every one keeps its side and its shape with `end` at x
NSA_SM_FN bool no_fold(const EdgeTables& t, uint32_t end, uint32_t other, const double* x, double min_cos2) {
    NSA_SM_EXACT
    const uint32_t H = 3u * t.F;
    uint32_t s, e;
    ring_row(t.ring_start, t.V, 6u * t.F, end, &s, &e);
    for (uint32_t j = s; j < e; ++j) {
        const uint32_t u = (uint32_t)t.ring[j], ed = (uint32_t)t.ring_edge[j];
        if (u >= t.V || u == other || ed >= H) continue;
        const int32_t a = t.edge_start[ed], b = t.edge_start[ed + 1];
        if (a < 0 || b < a || (uint32_t)b > H) continue;
        for (int32_t k = a; k < b; ++k) {
            const uint32_t h = (uint32_t)t.edge_halfedges[k];
            if (h >= H) continue;
            const uint32_t g = h / 3u;
            uint32_t idx[3];
            for (int c = 0; c < 3; ++c) idx[c] = (uint32_t)t.faces[3ull * g + c];
            if (idx[0] >= t.V || idx[1] >= t.V || idx[2] >= t.V) continue;
            int at = -1;
            uint32_t w = t.V;
            for (int c = 0; c < 3; ++c) {
                if (idx[c] == end) at = c;
                else if (idx[c] != u) w = idx[c];
            }
            if (at < 0 || w >= t.V || w == other || !(u < w)) continue;            // the face is visited from its smaller far vertex
            const double* p[3] = {&t.pos[3ull * idx[0]], &t.pos[3ull * idx[1]], &t.pos[3ull * idx[2]]};
            double n[3], n2[3];
            face_normal(p[0], p[1], p[2], n);
            face_normal(at == 0 ? x : p[0], at == 1 ? x : p[1], at == 2 ? x : p[2], n2);
            const double d = dot3(n, n2), nn = dot3(n, n), mm = dot3(n2, n2);
            if (!(d > 0.0) || !(d * d > (min_cos2 * nn) * mm)) return false;
        }
    }
    return true;
}

// one call per edge slot i in [0, 3 F): the code of the edge, its cost bits (kNoKey unless it is a candidate) and its placement
NSA_SM_FN uint8_t edge_pass(const EdgeTables& t, uint32_t i, double eps, bool has_limit, double max_error2, double min_cos2,
                            uint64_t* cost_bits, double* place) {
    NSA_SM_EXACT
    cost_bits[i] = kNoKey;
    for (int d = 0; d < 3; ++d) place[3ull * i + d] = 0.0;
    if (i >= t.E) return kNoEdge;
    const uint32_t lo = (uint32_t)t.edges[2ull * i], hi = (uint32_t)t.edges[2ull * i + 1];
    if (lo >= t.V || hi >= t.V || lo == hi) return kNoEdge;
    const int32_t cnt = t.edge_count[i];
    if (t.locked[lo] || t.locked[hi] || cnt < 1 || cnt > 2) return kRejLock;
    double q[kQ], x[3], cost;
    for (int k = 0; k < kQ; ++k) q[k] = t.quad[(uint64_t)kQ * lo + k] + t.quad[(uint64_t)kQ * hi + k];
    if (!place_and_cost(q, &t.pos[3ull * lo], &t.pos[3ull * hi], eps, x, &cost)) return kRejError;
    for (int d = 0; d < 3; ++d) place[3ull * i + d] = x[d];
    if (has_limit && !(cost <= max_error2 * q[10])) return kRejError;
    // the link: the two ascending rows
    uint32_t ls, le, hs, he;
    ring_row(t.ring_start, t.V, 6u * t.F, lo, &ls, &le);
    ring_row(t.ring_start, t.V, 6u * t.F, hi, &hs, &he);
    uint32_t common = 0, a = ls, b = hs;
    while (a < le && b < he) {
        const int32_t ua = t.ring[a], ub = t.ring[b];
        common += ua == ub ? 1u : 0u;
        a += ua <= ub ? 1u : 0u;
        b += ub <= ua ? 1u : 0u;
    }
    const uint32_t virt = cnt == 2 && on_boundary(t, ls, le) && on_boundary(t, hs, he) ? 1u : 0u;
    const uint32_t merged = (le - ls) + (he - hs) - common;               // the union of the rows, both ends included
    if (common + virt != (uint32_t)cnt || merged < (cnt == 1 ? 4u : 5u)) return kRejLink;
    if (!no_fold(t, lo, hi, x, min_cos2) || !no_fold(t, hi, lo, x, min_cos2)) return kRejFold;
    cost_bits[i] = bits_of(cost);
    return kCandidate;
}

// ---- the selection --------------------------------------------------------------------------------------------------------------------

// the second word of an edge's key: a bijection of lo << 32 | hi (the finaliser of splitmix64: an odd constant added, two
// xor-shifts each followed by an odd multiplier, one more xor-shift), so every key stays distinct and equal costs -- a flat region
// costs exactly 0 everywhere -- are ordered without regard to how the vertices are numbered
NSA_SM_FN uint64_t mix64(uint64_t w) {
    uint64_t z = w + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

NSA_SM_FN uint64_t edge_word(const int32_t* edges, uint32_t i) {
    return mix64(((uint64_t)(uint32_t)edges[2ull * i] << 32) | (uint64_t)(uint32_t)edges[2ull * i + 1]);
}

NSA_SM_FN bool key_less(uint64_t c0, uint64_t w0, uint64_t c1, uint64_t w1) { return c0 < c1 || (c0 == c1 && w0 < w1); }

// m1(v): the smallest key (cost bits, edge word) over the candidate edges of row v, and the edge that has it
NSA_SM_FN void min1_pass(const int32_t* ring_start, const int32_t* ring_edge, const int32_t* edges, const uint8_t* code,
                         const uint64_t* cost_bits, uint32_t V, uint32_t F, uint32_t v, uint64_t* m1c, uint64_t* m1w, uint32_t* m1e) {
    uint32_t s, e, be = kNoEdgeId;
    uint64_t bc = kNoKey, bw = kNoKey;
    ring_row(ring_start, V, 6u * F, v, &s, &e);
    for (uint32_t j = s; j < e; ++j) {
        const uint32_t ed = (uint32_t)ring_edge[j];
        if (ed >= 3u * F || code[ed] != kCandidate) continue;
        const uint64_t w = edge_word(edges, ed);
        if (be == kNoEdgeId || key_less(cost_bits[ed], w, bc, bw)) {
            bc = cost_bits[ed];
            bw = w;
            be = ed;
        }
    }
    m1c[v] = bc;
    m1w[v] = bw;
    m1e[v] = be;
}

// m2(v): the smallest m1 over v and its row
NSA_SM_FN void min2_pass(const int32_t* ring_start, const int32_t* ring, const uint64_t* m1c, const uint64_t* m1w, const uint32_t* m1e,
                         uint32_t V, uint32_t F, uint32_t v, uint32_t* m2e) {
    uint32_t s, e, be = m1e[v];
    uint64_t bc = m1c[v], bw = m1w[v];
    ring_row(ring_start, V, 6u * F, v, &s, &e);
    for (uint32_t j = s; j < e; ++j) {
        const uint32_t u = (uint32_t)ring[j];
        if (u >= V || m1e[u] == kNoEdgeId) continue;
        if (be == kNoEdgeId || key_less(m1c[u], m1w[u], bc, bw)) {
            bc = m1c[u];
            bw = m1w[u];
            be = m1e[u];
        }
    }
    m2e[v] = be;
}

// edge slot i is selected iff it is a candidate and both its ends name it; returns its sort key (kNoKey when it is not selected)
NSA_SM_FN uint64_t select_pass(const int32_t* edges, const uint8_t* code, const uint64_t* cost_bits, const uint32_t* m2e, uint32_t V,
                               uint32_t i) {
    if (code[i] != kCandidate) return kNoKey;
    const uint32_t lo = (uint32_t)edges[2ull * i], hi = (uint32_t)edges[2ull * i + 1];
    if (lo >= V || hi >= V) return kNoKey;
    return m2e[lo] == i && m2e[hi] == i ? cost_bits[i] : kNoKey;
}

// the 32-bit word `k` (0, 1: the edge word's low and high half; 2, 3: the cost's) of edge slot i for the four stable argsorts that
// put the selected edges in key order; all ones for a slot that is not selected, which sorts it last
NSA_SM_FN uint32_t sort_word(const int32_t* edges, const uint64_t* skey, uint32_t i, int k) {
    if (skey[i] == kNoKey) return 0xFFFFFFFFu;
    const uint64_t w = k < 2 ? edge_word(edges, i) : skey[i];
    return (uint32_t)((k & 1) ? w >> 32 : w & 0xFFFFFFFFull);
}

// the prefix rule: the selected edge at sorted position p, with `before` faces removed by the positions ahead of it, is taken iff
// there is no target or the count is still above it
NSA_SM_FN bool prefix_take(bool has_target, uint64_t n_faces, uint64_t before, uint64_t target) {
    return !has_target || (before < n_faces && n_faces - before > target);
}

// ---- the application ------------------------------------------------------------------------------------------------------------------

// one taken edge: x_lo = x, Q_lo = Q_lo + Q_hi, the colour at the clamped projection of x onto the edge, vertex_map[hi] = lo
NSA_SM_FN void apply_pass(const int32_t* edges, const double* place, uint32_t V, uint32_t i, double* pos, double* quad, double* col,
                          int32_t* vmap, uint8_t* moved, uint32_t* lo_out, uint32_t* hi_out) {
    NSA_SM_EXACT
    const uint32_t lo = (uint32_t)edges[2ull * i], hi = (uint32_t)edges[2ull * i + 1];
    *lo_out = lo;
    *hi_out = hi;
    if (lo >= V || hi >= V) return;                                       // (never: a selected edge has its ends in range)
    const double* x = &place[3ull * i];
    if (col) {
        double ev[3], dx[3];
        for (int d = 0; d < 3; ++d) {
            ev[d] = pos[3ull * hi + d] - pos[3ull * lo + d];
            dx[d] = x[d] - pos[3ull * lo + d];
        }
        const double ee = dot3(ev, ev);
        double t = ee > 0.0 ? dot3(dx, ev) / ee : 0.0;
        t = t > 0.0 ? t : 0.0;                                             // (a NaN gives 0)
        t = t < 1.0 ? t : 1.0;
        for (int d = 0; d < 3; ++d) col[3ull * lo + d] = col[3ull * lo + d] + t * (col[3ull * hi + d] - col[3ull * lo + d]);
    }
    for (int d = 0; d < 3; ++d) pos[3ull * lo + d] = x[d];
    for (int k = 0; k < kQ; ++k) quad[(uint64_t)kQ * lo + k] = quad[(uint64_t)kQ * lo + k] + quad[(uint64_t)kQ * hi + k];
    vmap[hi] = (int32_t)lo;
    moved[lo] = 1;
}

// one corner after the round's collapses: hi becomes lo
NSA_SM_FN void rename_pass(const int32_t* vmap, uint32_t V, uint64_t c, int32_t* faces) {
    const uint32_t v = (uint32_t)faces[c];
    if (v < V) faces[c] = vmap[v];
}

// one vertex after the round's collapses: vertex_map stays composed (every entry names a vertex that maps to itself)
NSA_SM_FN void compose_pass(uint32_t V, uint32_t v, int32_t* vmap) {
    const uint32_t r = (uint32_t)vmap[v];
    if (r >= V) return;
    const int32_t r2 = vmap[r];
    if ((uint32_t)r2 != r && (uint32_t)r2 < V) vmap[v] = r2;
}

}  // namespace decimate
}  // namespace nsa
