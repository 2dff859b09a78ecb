// fill_area_passes.hpp -- the per-item bodies of minimum-area hole patches (csrc/mesh_fill_area.hip; header Section 24):
// the plan row of a loop, the position and name of a loop vertex, the chord mask and the start values of a table cell, the weight
// of a triangle, the (value, j) minimum of a cell over a strided set of candidates and the rule that merges two such minima, the
// final class of a loop and one face of the patch by descent from the root of the choice tree.  Like fill_passes.hpp the bodies
// compile for the device and, unchanged, as host C++ (tests/fill_area_host_check.cpp calls them one item at a time and is held to
// tests/fill_area_ref.py bit for bit).  Float64, + - * rounded one by one and one correctly rounded square root per triangle.  Every
// index read from a table is checked before it is used, and every loop is capped by the length of the table it walks.
#pragma once
#include <cmath>
#include <cstdint>
#include "fill_passes.hpp"

namespace nsa {
namespace fill_area {

using fill::cross3;
using fill::dot3;
using fill::kLoopInts;
using fill::kNone;
using fill::Shape;
using fill::start_vertex;

constexpr int64_t kNotSelected = -1, kAreaFilled = 0, kAreaTooManyEdges = 1, kNoTriangulation = 2;      // the area class of a loop
constexpr int kAreaInts = 6;       // class, n, table_offset, plan_face_offset, row_offset, face_offset
constexpr int kPlanTotals = 8;     // selected, loops with a table, too many edges, cells, max n, plan faces, rows, 0
constexpr int kFinalTotals = 4;    // area_filled, area_too_many_edges, no_triangulation, faces
constexpr uint32_t kMaxAreaEdges = 16384;
constexpr uint32_t kWaveCandidates = 64;               // a cell with at least this many candidates is one wave's work

NSA_SM_FN double infinity() { return HUGE_VAL; }

// The plan class of loop l and, through n_out, the side of its table (0: it takes none).
NSA_SM_FN int64_t plan_class(const int64_t* loop_ints, uint32_t l, uint32_t class_mask, uint32_t max_area_edges, uint64_t B,
                             uint64_t* n_out) {
    const int64_t* row = loop_ints + (uint64_t)kLoopInts * l;
    const int64_t c = row[3], n = row[1], s = row[2];
    *n_out = 0;
    if (c < 0 || c >= fill::kClasses || !((class_mask >> c) & 1u)) return kNotSelected;
    if (n < 0 || s < 0 || (uint64_t)s + (uint64_t)n > B) return kNotSelected;
    if ((uint64_t)n > max_area_edges) return kAreaTooManyEdges;
    if (n < 3) return kNoTriangulation;
    *n_out = (uint64_t)n;
    return kAreaFilled;
}

// the last loop whose column `col` is not above x (a loop without extent shares its offset with the loop after it); kNone when L = 0
NSA_SM_FN uint32_t owner(const int64_t* area_ints, uint32_t L, int col, uint64_t x) {
    uint32_t lo = 0, hi = L;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((uint64_t)area_ints[(uint64_t)kAreaInts * mid + col] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo == 0 ? kNone : lo - 1;
}

struct Table {                     // the table of one loop, checked against the sizes the caller allocated
    uint64_t n, off, ro, s;
    uint32_t l;
    bool ok;
};

// the table of loop l when it has one that lies inside the buffers
NSA_SM_FN Table table_at(const int64_t* loop_ints, const int64_t* area_ints, uint32_t L, uint64_t B, uint64_t cells, uint64_t rows,
                         uint32_t l) {
    Table t{0, 0, 0, 0, l, false};
    if (t.l == kNone || t.l >= L) return t;
    const int64_t* a = area_ints + (uint64_t)kAreaInts * t.l;
    const int64_t cls = a[0];
    if ((cls != kAreaFilled && cls != kNoTriangulation) || a[1] < 3 || a[2] < 0 || a[4] < 0) return t;
    t.n = (uint64_t)a[1];
    t.off = (uint64_t)a[2];
    t.ro = (uint64_t)a[4];
    const int64_t s = loop_ints[(uint64_t)kLoopInts * t.l + 2];
    if (t.n > kMaxAreaEdges || s < 0 || (uint64_t)s + t.n > B || t.off + t.n * t.n > cells || t.ro + t.n > rows) return t;
    t.s = (uint64_t)s;
    t.ok = true;
    return t;
}

// the loop that owns item x of column col (2: cells, 3: plan faces, 4: rows) when that loop has a table that lies inside the buffers
NSA_SM_FN Table table_of(const int64_t* loop_ints, const int64_t* area_ints, uint32_t L, uint64_t B, uint64_t cells, uint64_t rows, int col,
                         uint64_t x) {
    return table_at(loop_ints, area_ints, L, B, cells, rows, owner(area_ints, L, col, x));
}

// Row r of the tabled loops: the loop it belongs to, its position in float64 and its name (names = the face list of the topology).
NSA_SM_FN void row_pass(const Shape& m, const int32_t* names, const int32_t* order, uint64_t B, const int64_t* loop_ints,
                        const int64_t* area_ints, uint32_t L, uint64_t cells, uint64_t rows, uint64_t r, uint32_t* row_loop, int32_t* row_name,
                        double* pos) {
    if (r >= rows) return;
    row_loop[r] = kNone;
    row_name[r] = -1;
    for (int k = 0; k < 3; ++k) pos[3 * r + k] = infinity();
    const Table t = table_of(loop_ints, area_ints, L, B, cells, rows, 4, r);
    if (!t.ok || r - t.ro >= t.n) return;
    row_loop[r] = t.l;
    const int32_t h = order[t.s + (r - t.ro)];
    const uint32_t v = h >= 0 ? start_vertex(m, (uint32_t)h) : kNone;
    if (v == kNone) return;
    for (int k = 0; k < 3; ++k) pos[3 * r + k] = (double)m.verts[3ull * v + k];
    const int32_t name = names[h];
    row_name[r] = name >= 0 && (uint32_t)name < m.V ? name : -1;
}

// true when the edge table (rows (lo, hi), sorted, E of them) holds the edge between the names a and b
NSA_SM_FN bool has_edge(const int32_t* edges, uint32_t E, int32_t a, int32_t b) {
    const int32_t lo_v = a < b ? a : b, hi_v = a < b ? b : a;
    uint32_t lo = 0, hi = E;                               // the first row not below (lo_v, hi_v)
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        const int32_t e0 = edges[2ull * mid], e1 = edges[2ull * mid + 1];
        if (e0 < lo_v || (e0 == lo_v && e1 < hi_v)) lo = mid + 1;
        else hi = mid;
    }
    return lo < E && edges[2ull * lo] == lo_v && edges[2ull * lo + 1] == hi_v;
}

// Cell x of the tables: the chord mask, and the start values W = 0 on the loop's edges (i, i + 1), +inf elsewhere, J = -1.  The cell
// (i, k) writes W[i][k] and the transposed copy's [k][i], which is the same value.
NSA_SM_FN void mask_pass(const int32_t* edges, uint32_t E, const int64_t* loop_ints, const int64_t* area_ints, uint32_t L, uint64_t B,
                         uint64_t cells, uint64_t rows, const int32_t* row_name, uint64_t x, uint8_t* mask, double* W, double* WT, int32_t* J) {
    if (x >= cells) return;
    mask[x] = 0;
    J[x] = -1;
    W[x] = infinity();
    const Table t = table_of(loop_ints, area_ints, L, B, cells, rows, 2, x);
    if (!t.ok || x - t.off >= t.n * t.n) {
        WT[x] = infinity();
        return;
    }
    const uint64_t i = (x - t.off) / t.n, k = (x - t.off) - i * t.n;
    const double w = k == i + 1 ? 0.0 : infinity();
    W[x] = w;
    WT[t.off + k * t.n + i] = w;
    if (i >= k || k == i + 1 || (i == 0 && k + 1 == t.n)) return;
    const int32_t a = row_name[t.ro + i], b = row_name[t.ro + k];
    mask[x] = (a < 0 || b < 0 || a == b || has_edge(edges, E, a, b)) ? 1 : 0;
}

// IEEE square root of a double, correctly rounded (tests/test_mesh_fill_area_gpu.py pins the device's against numpy's)
NSA_SM_FN double root(double x) { return sqrt(x); }

// T of the triangle of the rows ri < rj < rk of pos
NSA_SM_FN double weight(const double* pos, uint64_t ri, uint64_t rj, uint64_t rk, double min_sin2) {
    NSA_SM_EXACT
    double a[3], b[3], g[3], c[3];
    for (int d = 0; d < 3; ++d) {
        a[d] = pos[3 * rj + d] - pos[3 * ri + d];
        b[d] = pos[3 * rk + d] - pos[3 * ri + d];
        g[d] = b[d] - a[d];
    }
    cross3(a, b, c);
    const double n2 = dot3(c, c), aa = dot3(a, a), bb = dot3(b, b), gg = dot3(g, g);
    double e = aa;
    if (bb > e) e = bb;
    if (gg > e) e = gg;
    return n2 > min_sin2 * (e * e) ? 0.5 * root(n2) : infinity();
}

// the rule of the minimum: (v, j) beats (best, bj) on a smaller value, or an equal one with a smaller j.  Associative and commutative,
// so any order of reduction gives the same pair; (inf, kNone) is its identity.
NSA_SM_FN bool beats(double v, uint32_t j, double best, uint32_t bj) { return v < best || (v == best && j < bj); }

// The minimum of cell (i, k) of table t over the candidates j = j0, j0 + stride, ... < k: W[i][j] along the row of W, W[j][k] along
// the row k of the transposed copy.
NSA_SM_FN void cell_scan(const double* W, const double* WT, const double* pos, const Table& t, uint64_t i, uint64_t k, uint64_t j0,
                         uint64_t stride, double min_sin2, double* best, uint32_t* bj) {
    NSA_SM_EXACT
    double b = infinity();
    uint32_t at = kNone;
    const double* wi = W + t.off + i * t.n;
    const double* wk = WT + t.off + k * t.n;
    for (uint64_t j = j0; j < k; j += stride) {
        const double v = (wi[j] + wk[j]) + weight(pos, t.ro + i, t.ro + j, t.ro + k, min_sin2);
        if (beats(v, (uint32_t)j, b, at)) {
            b = v;
            at = (uint32_t)j;
        }
    }
    *best = b;
    *bj = at;
}

NSA_SM_FN void cell_store(const Table& t, uint64_t i, uint64_t k, double best, uint32_t bj, const uint8_t* mask, double* W, double* WT,
                          int32_t* J) {
    const uint64_t x = t.off + i * t.n + k;
    const double w = mask[x] ? infinity() : best;
    W[x] = w;
    WT[t.off + k * t.n + i] = w;
    J[x] = bj == kNone ? -1 : (int32_t)bj;
}

// the table of row r when the cell (i, i + d) of that row exists
NSA_SM_FN bool cell_of(const int64_t* loop_ints, const int64_t* area_ints, uint32_t L, uint64_t B, uint64_t cells, uint64_t rows,
                       const uint32_t* row_loop, uint64_t r, uint32_t d, Table* t, uint64_t* i) {
    if (r >= rows) return false;
    *t = table_at(loop_ints, area_ints, L, B, cells, rows, row_loop[r]);
    if (!t->ok || r < t->ro || r - t->ro >= t->n) return false;
    *i = r - t->ro;
    return *i + d < t->n;
}

// The final class of loop l and its area W[0][n - 1] (0 for a loop without a table).
NSA_SM_FN int64_t final_class(const int64_t* loop_ints, const int64_t* area_ints, uint32_t L, uint64_t B, uint64_t cells, uint64_t rows,
                              const double* W, uint32_t l, double* area) {
    const int64_t cls = area_ints[(uint64_t)kAreaInts * l];
    *area = 0.0;
    if (cls != kAreaFilled) return cls;
    const Table t = table_at(loop_ints, area_ints, L, B, cells, rows, l);
    if (!t.ok) return kNoTriangulation;
    *area = W[t.off + t.n - 1];
    return fill::finite_d(*area) ? kAreaFilled : kNoTriangulation;
}

// Face x of the plan's numbering: the descent from the root (0, n - 1) of its loop to the node whose number is x, (-1, -1, -1) for
// a loop that has no triangulation or a table that does not describe a tree.
NSA_SM_FN void emit_pass(const Shape& m, const int32_t* order, uint64_t B, const int64_t* loop_ints, const int64_t* area_ints, uint32_t L,
                         uint64_t cells, uint64_t rows, const int32_t* J, uint64_t NF, uint64_t x, int32_t* new_faces) {
    if (x >= NF) return;
    int32_t* tri = new_faces + 3 * x;
    tri[0] = tri[1] = tri[2] = -1;
    const Table t = table_of(loop_ints, area_ints, L, B, cells, rows, 3, x);
    if (!t.ok || area_ints[(uint64_t)kAreaInts * t.l] != kAreaFilled) return;
    const uint64_t fo = (uint64_t)area_ints[(uint64_t)kAreaInts * t.l + 3];
    if (x < fo || x - fo >= t.n - 2) return;
    const uint64_t y = x - fo;
    uint64_t i = 0, k = t.n - 1, base = 0;
    for (uint64_t step = 0; step < t.n; ++step) {
        const int32_t jj = J[t.off + i * t.n + k];
        if (jj < 0 || (uint64_t)jj <= i || (uint64_t)jj >= k) return;
        const uint64_t j = (uint64_t)jj, left = j - i - 1;
        if (y == base) {
            const uint64_t at[3] = {k, j, i};
            int32_t out[3];
            for (int c = 0; c < 3; ++c) {
                const int32_t h = order[t.s + at[c]];
                const uint32_t v = h >= 0 ? start_vertex(m, (uint32_t)h) : kNone;
                if (v == kNone) return;
                out[c] = (int32_t)v;
            }
            tri[0] = out[0];
            tri[1] = out[1];
            tri[2] = out[2];
            return;
        }
        if (y < base || y - base > k - i - 2) return;
        if (y <= base + left) {
            k = j;
            base = base + 1;
        } else {
            i = j;
            base = base + 1 + left;
        }
    }
}

}  // namespace fill_area
}  // namespace nsa
