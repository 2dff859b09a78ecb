// fill_passes.hpp -- the per-item bodies of hole filling (csrc/mesh_fill.hip; header Section 23): the boundary test of a
// half-edge, the successor of a boundary half-edge by rotation inside the face fan, the pinch mark, one round of pointer jumping and
// of list ranking, the row of one loop (sums in rank order, class, ring count) and one face of the polar patch with the vertex it
// owns.  Like decimate_passes.hpp the bodies compile for the device and, unchanged, as host C++ (tests/fill_host_check.cpp calls them
// one item at a time and is held to tests/fill_ref.py bit for bit).  Float64 throughout, + - * / only, every operation rounded on its
// own: the pragma keeps clang from contracting a * b + c, a host compiler that does not know it is given -ffp-contract=off.  Every
// index read from a table is checked before it is used, and every loop is capped by the length of the table it walks.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include "smooth_passes.hpp"

namespace nsa {
namespace fill {

using smooth::finite_d;

constexpr int64_t kFilled = 0, kNonFinite = 1, kPinched = 2, kTooManyEdges = 3, kTooLarge = 4, kFolded = 5;      // the class of a loop
constexpr int kClasses = 6;
constexpr uint8_t kBlocked = 1, kPinch = 2, kOpenChain = 4, kCapHit = 8;                                         // the flags of an item
constexpr int kLoopInts = 9;       // leader, n, start, class, rings, new_verts, new_faces, vert_offset, face_offset
constexpr int kLoopReals = 18;     // centre 3, mean colour 3, box lo 3, box hi 3, D2, R2, L2, A 3
constexpr int kTotals = 12;
constexpr uint32_t kMaxRings = 65535;
constexpr uint32_t kNone = 0xFFFFFFFFu;

struct Topo {                      // the edge table of Section 18 on the face list the topology is read from
    const int32_t* names;          // [F, 3]: that face list
    const int32_t* face_edges;
    const int32_t* edge_count;
    const int32_t* edge_forward;
    const int32_t* edge_start;
    const int32_t* edge_halfedges;
    uint32_t V, F, E;              // E <= 3 F, checked by the caller
};

// the edge of half-edge g when it lies in the table, kNone otherwise
NSA_SM_FN uint32_t edge_of(const Topo& t, uint32_t g) {
    if (g >= 3u * t.F) return kNone;
    const int32_t e = t.face_edges[g];
    return e >= 0 && (uint32_t)e < t.E ? (uint32_t)e : kNone;
}

NSA_SM_FN bool boundary_halfedge(const Topo& t, uint32_t h) {
    const uint32_t e = edge_of(t, h);
    return e != kNone && t.edge_count[e] == 1;
}

NSA_SM_FN uint32_t leaving(uint32_t h) { return 3u * (h / 3u) + (h % 3u + 1u) % 3u; }      // the half-edge of h's face that leaves h's end

// The successor of the boundary half-edge at item i: next[i] = the item of the boundary half-edge that leaves its end vertex after
// rotating through the fan, i itself when the rotation is blocked.  Returns the flags kBlocked (| kCapHit).
NSA_SM_FN uint8_t next_pass(const Topo& t, const uint32_t* bh, const int32_t* hslot, uint32_t B, uint32_t i, uint32_t* next) {
    next[i] = i;
    const uint32_t H = 3u * t.F, h = bh[i];
    if (h >= H) return kBlocked;
    uint32_t g = leaving(h);
    for (uint32_t steps = 0;; ++steps) {
        const uint32_t e = edge_of(t, g);
        if (e == kNone) return kBlocked;
        const int32_t c = t.edge_count[e];
        if (c == 1) break;
        if (c != 2 || t.edge_forward[e] != 1) return kBlocked;
        if (steps >= t.F) return kBlocked | kCapHit;
        const int32_t s = t.edge_start[e];
        if (s < 0 || (uint32_t)s + 1u >= H) return kBlocked;
        const int32_t a = t.edge_halfedges[s], b = t.edge_halfedges[s + 1];
        const int32_t tw = (uint32_t)a == g ? b : a;
        if (tw < 0 || (uint32_t)tw >= H) return kBlocked;
        g = leaving((uint32_t)tw);
    }
    const int32_t j = hslot[g];
    if (j < 0 || (uint32_t)j >= B) return kBlocked;
    next[i] = (uint32_t)j;
    return 0;
}

// the start vertex of item i by name; V for an item outside the list
NSA_SM_FN uint32_t start_key(const Topo& t, const uint32_t* bh, uint32_t B, uint32_t i) {
    if (i >= B) return t.V;
    const uint32_t h = bh[i];
    if (h >= 3u * t.F) return t.V;
    const int32_t v = t.names[h];
    return v >= 0 && (uint32_t)v < t.V ? (uint32_t)v : t.V;
}

// position p of the items sorted by start vertex: the item is pinched when a neighbour in that order starts at the same vertex
NSA_SM_FN void pinch_pass(const Topo& t, const uint32_t* bh, const uint32_t* order, uint32_t B, uint32_t p, uint8_t* pinch) {
    const uint32_t i = order[p];
    if (i >= B) return;
    const uint32_t k = start_key(t, bh, B, i);
    bool same = false;
    if (p > 0) same = same || start_key(t, bh, B, order[p - 1]) == k;
    if (p + 1 < B) same = same || start_key(t, bh, B, order[p + 1]) == k;
    pinch[i] = same ? kPinch : 0;
}

// one round of pointer jumping: (smallest item seen, jump pointer, reached a terminal)
NSA_SM_FN void jump_pass(const uint32_t* min_in, const uint32_t* ptr_in, const uint8_t* term_in, uint32_t B, uint32_t i, uint32_t* min_out,
                         uint32_t* ptr_out, uint8_t* term_out) {
    uint32_t p = ptr_in[i];
    if (p >= B) p = i;
    const uint32_t a = min_in[i], b = min_in[p];
    min_out[i] = a < b ? a : b;
    term_out[i] = term_in[i] | term_in[p];
    const uint32_t q = ptr_in[p];
    ptr_out[i] = q < B ? q : i;
}

// the start of list ranking: the cycle is cut in front of its leader; (steps to the last item, pointer)
NSA_SM_FN void rank_init_pass(const uint32_t* mn, const uint8_t* term, const uint32_t* next, uint32_t B, uint32_t i, uint32_t* leader,
                              uint32_t* dist, uint32_t* ptr) {
    const bool open = term[i] != 0;
    const uint32_t lead = open ? kNone : mn[i];
    const bool last = open || next[i] == lead || next[i] >= B;
    leader[i] = lead;
    dist[i] = last ? 0u : 1u;
    ptr[i] = last ? i : next[i];
}

NSA_SM_FN void rank_pass(const uint32_t* dist_in, const uint32_t* ptr_in, uint32_t B, uint32_t i, uint32_t* dist_out, uint32_t* ptr_out) {
    uint32_t p = ptr_in[i];
    if (p >= B) p = i;
    dist_out[i] = dist_in[i] + (p == i ? 0u : dist_in[p]);
    const uint32_t q = ptr_in[p];
    ptr_out[i] = q < B ? q : i;
}

NSA_SM_FN bool is_leader(const uint32_t* leader, uint32_t i) { return leader[i] == i; }

// the rank of item i and the place of its half-edge in `order`, given the start of its loop at its leader
NSA_SM_FN void order_pass(const uint32_t* bh, const uint32_t* leader, const uint32_t* dist, const uint32_t* item_start, uint32_t B, uint32_t i,
                          int32_t* rank, uint32_t* order_item, int32_t* order) {
    const uint32_t lead = leader[i];
    rank[i] = 0;
    if (lead >= B) return;
    const uint32_t r = dist[lead] - dist[i];
    rank[i] = (int32_t)r;
    const uint64_t at = (uint64_t)item_start[lead] + r;
    if (at >= B) return;
    order_item[at] = i;
    order[at] = (int32_t)bh[i];
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

struct Shape {                     // the mesh the patch is made for
    const float* verts;
    const float* colors;           // or NULL
    const int32_t* faces;          // [F, 3]: the start vertex of half-edge h is faces[h]
    uint32_t V, F;
};

// the start vertex of half-edge h, kNone when it is outside the mesh
NSA_SM_FN uint32_t start_vertex(const Shape& m, uint32_t h) {
    if (h >= 3u * m.F) return kNone;
    const int32_t v = m.faces[h];
    return v >= 0 && (uint32_t)v < m.V ? (uint32_t)v : kNone;
}

NSA_SM_FN bool load_point(const Shape& m, const uint32_t* bh, const uint32_t* order_item, uint32_t B, uint64_t at, double* p) {
    p[0] = p[1] = p[2] = 0.0;
    if (at >= B) return false;
    const uint32_t i = order_item[at];
    if (i >= B) return false;
    const uint32_t v = start_vertex(m, bh[i]);
    if (v == kNone) return false;
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
        p[k] = (double)m.verts[3ull * v + k];
        ok = ok && finite_d(p[k]);
    }
    return ok;
}

struct Limits {
    bool has_max_edges;
    uint64_t max_edges;
    bool has_max_size;
    double max_size2;
    uint32_t rings;                // 0: auto
    uint32_t max_rings;
    bool skip_folded;
};

// The row of loop l, whose leader, n and start are in ints[9 l ..] already: the sums in rank order, the class and the ring count.
NSA_SM_FN void loop_pass(const Shape& m, const uint32_t* bh, const uint32_t* order_item, const uint8_t* pinch, uint32_t B, const Limits& lim,
                         uint32_t l, int64_t* ints, double* reals) {
    NSA_SM_EXACT
    int64_t* row = ints + (uint64_t)kLoopInts * l;
    double* out = reals + (uint64_t)kLoopReals * l;
    for (int k = 0; k < kLoopReals; ++k) out[k] = 0.0;
    for (int k = 3; k < kLoopInts; ++k) row[k] = 0;
    const uint64_t n = (uint64_t)row[1], s = (uint64_t)row[2];
    if (n == 0 || s + n > B) {
        row[3] = kNonFinite;
        return;
    }
    const double nd = (double)n;
    bool finite = true, pinched = false;
    double sum[3] = {0.0, 0.0, 0.0}, csum[3] = {0.0, 0.0, 0.0}, lo[3], hi[3], p[3];
    for (uint64_t i = 0; i < n; ++i) {
        finite = load_point(m, bh, order_item, B, s + i, p) && finite;
        const uint32_t it = order_item[s + i];
        if (it < B) {
            pinched = pinched || pinch[it] != 0;
            const uint32_t v = start_vertex(m, bh[it]);
            if (m.colors && v != kNone)
                for (int k = 0; k < 3; ++k) csum[k] = csum[k] + (double)m.colors[3ull * v + k];
        }
        for (int k = 0; k < 3; ++k) {
            sum[k] = sum[k] + p[k];
            if (i == 0 || p[k] < lo[k]) lo[k] = p[k];
            if (i == 0 || p[k] > hi[k]) hi[k] = p[k];
        }
    }
    if (!finite) {
        row[3] = kNonFinite;
        return;
    }
    double c[3], e[3];
    for (int k = 0; k < 3; ++k) {
        c[k] = sum[k] / nd;
        out[k] = c[k];
        out[3 + k] = m.colors ? csum[k] / nd : 0.0;
        out[6 + k] = lo[k];
        out[9 + k] = hi[k];
        e[k] = hi[k] - lo[k];
    }
    const double D2 = dot3(e, e);
    double r2 = 0.0, l2 = 0.0, A[3] = {0.0, 0.0, 0.0}, q[3], d[3], u[3], g[3], ni[3];
    load_point(m, bh, order_item, B, s, p);
    for (uint64_t i = 0; i < n; ++i) {
        load_point(m, bh, order_item, B, s + (i + 1 < n ? i + 1 : 0), q);
        for (int k = 0; k < 3; ++k) {
            d[k] = p[k] - c[k];
            u[k] = q[k] - c[k];
            g[k] = q[k] - p[k];
        }
        r2 = r2 + dot3(d, d);
        l2 = l2 + dot3(g, g);
        cross3(u, d, ni);
        for (int k = 0; k < 3; ++k) {
            A[k] = A[k] + ni[k];
            p[k] = q[k];
        }
    }
    const double R2 = r2 / nd, L2 = l2 / nd;
    out[12] = D2;
    out[13] = R2;
    out[14] = L2;
    for (int k = 0; k < 3; ++k) out[15 + k] = A[k];
    uint32_t K = lim.rings;
    if (K == 0) {
        K = 1;
        while (K < lim.max_rings && !(((double)K * (double)K) * L2 >= R2)) ++K;
    }
    int64_t cls = kFilled;
    if (pinched) cls = kPinched;
    else if (lim.has_max_edges && n > lim.max_edges) cls = kTooManyEdges;
    else if (lim.has_max_size && D2 > lim.max_size2) cls = kTooLarge;
    else if (lim.skip_folded) {
        load_point(m, bh, order_item, B, s, p);
        for (uint64_t i = 0; i < n && cls == kFilled; ++i) {
            load_point(m, bh, order_item, B, s + (i + 1 < n ? i + 1 : 0), q);
            for (int k = 0; k < 3; ++k) {
                d[k] = p[k] - c[k];
                u[k] = q[k] - c[k];
                p[k] = q[k];
            }
            cross3(u, d, ni);
            if (dot3(ni, A) <= 0.0) cls = kFolded;
        }
    }
    row[3] = cls;
    row[4] = (int64_t)K;
    if (cls == kFilled) {
        row[5] = (int64_t)((uint64_t)(K - 1) * n + 1);
        row[6] = (int64_t)(n * (2ull * K - 1));
    }
}

// the loop that owns new face x: the last loop whose face_offset is not above x (an unfilled loop owns no face and shares its offset
// with the filled loop after it)
NSA_SM_FN uint32_t loop_of_face(const int64_t* ints, uint32_t L, uint64_t x) {
    uint32_t lo = 0, hi = L;                                              // the first loop with face_offset > x
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((uint64_t)ints[(uint64_t)kLoopInts * mid + 8] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;                                                        // (face_offset[0] = 0 <= x: lo >= 1 when L >= 1)
}

// New face x of the patch, with the new vertex it owns: the first face of (ring j >= 1, i) owns vertex (j, i), the face (K - 1, 0) the
// centre as well.  new_verts / new_colors / new_faces are the appended rows alone ([NV, 3], [NV, 3], [NF, 3]).
NSA_SM_FN void emit_pass(const Shape& m, const int32_t* order, uint32_t B, const int64_t* ints, const double* reals, uint32_t L, uint64_t NV,
                         uint64_t NF, uint64_t x, float* new_verts, float* new_colors, int32_t* new_faces) {
    NSA_SM_EXACT
    if (x >= NF || L == 0) return;
    const uint32_t l = loop_of_face(ints, L, x);
    if (l >= L) return;
    const int64_t* row = ints + (uint64_t)kLoopInts * l;
    const double* c = reals + (uint64_t)kLoopReals * l;
    const uint64_t n = (uint64_t)row[1], s = (uint64_t)row[2], K = (uint64_t)row[4], vo = (uint64_t)row[7], fo = (uint64_t)row[8];
    int32_t* tri = new_faces + 3 * x;
    tri[0] = tri[1] = tri[2] = -1;
    if (row[3] != kFilled || n == 0 || K == 0 || s + n > B || x < fo || x - fo >= (uint64_t)row[6]) return;
    const uint64_t y = x - fo, body = 2 * n * (K - 1);
    uint64_t j, i, w;
    if (y < body) {
        j = y / (2 * n);
        i = (y - 2 * n * j) >> 1;
        w = y & 1;
    } else {
        j = K - 1;
        i = y - body;
        w = 0;
    }
    const uint64_t i1 = i + 1 < n ? i + 1 : 0, centre = m.V + vo + (K - 1) * n;
    auto ring = [&](uint64_t jj, uint64_t ii) -> int32_t {
        if (jj == 0) {
            const int32_t h = order[s + ii];
            const uint32_t v = h >= 0 ? start_vertex(m, (uint32_t)h) : kNone;
            return v == kNone ? -1 : (int32_t)v;
        }
        return (int32_t)(m.V + vo + (jj - 1) * n + ii);
    };
    if (j + 1 < K) {
        tri[0] = ring(j, i1);
        tri[1] = w ? ring(j + 1, i) : ring(j, i);
        tri[2] = w ? ring(j + 1, i1) : ring(j + 1, i);
    } else {
        tri[0] = ring(j, i1);
        tri[1] = ring(j, i);
        tri[2] = (int32_t)centre;
    }
    if (w == 0 && j >= 1) {
        const uint64_t at = vo + (j - 1) * n + i;
        const int32_t v = ring(0, i);
        if (at < NV && v >= 0) {
            const double t = (double)(K - j) / (double)K;
            for (int k = 0; k < 3; ++k) {
                const double d = (double)m.verts[3ull * (uint32_t)v + k] - c[k];
                new_verts[3 * at + k] = (float)(c[k] + t * d);
                if (m.colors && new_colors) {
                    const double dc = (double)m.colors[3ull * (uint32_t)v + k] - c[3 + k];
                    new_colors[3 * at + k] = (float)(c[3 + k] + t * dc);
                }
            }
        }
    }
    if (j + 1 == K && i == 0) {
        const uint64_t at = vo + (K - 1) * n;
        if (at < NV)
            for (int k = 0; k < 3; ++k) {
                new_verts[3 * at + k] = (float)c[k];
                if (m.colors && new_colors) new_colors[3 * at + k] = (float)c[3 + k];
            }
    }
}

}  // namespace fill
}  // namespace nsa
