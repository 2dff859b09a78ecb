// tri_common.hpp -- the index layout, the per-face closest point and the ring walk of the closest-point index (DESIGN 4m, C ABI
// Section 14), shared by mesh_closest.hip (build, unsigned query) and mesh_sdf.hip (signed and range-limited queries, Section 15).
// The contract, the bounds and their margins are stated at the head of mesh_closest.hip; the grid under the index is bulk_grid.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include "../../include/nicer_slam_amd.h"
#include "bulk_grid.hpp"
#include "grid_common.hpp"
#include "radix_sort.hpp"

namespace nsa {
namespace tri {

using bulk::axis_cell;
using bulk::finite3;
using bulk::kMaxCells;
using bulk::lower_bound;
using bulk::up256;

constexpr uint32_t kMaxCount = 0x7FFFFFFFu;
constexpr double kLargeCells = 2.0;          // a grid face's box is at most this many cells long on every axis
constexpr double kSigmaCells = 0x1p16;       // a grid face's sigma is at most this / hmax^2: rho <= 1/4 up to 2^12.5 cells from q,
                                             // beyond the 2^10 sqrt(3) cells a grid can measure; height >= hmax / 256
constexpr double kStrayCells = 256.0;        // a grid face's centroid is at most this many cells outside the grid
constexpr double kRhoUnit = 0x1p-43;         // rho = kRhoUnit * sigma * D^2
constexpr double kRhoMax = 0.25;
constexpr double kPad = 0x1p-40;             // box padding, relative to the coordinate's magnitude
constexpr double kSlack = 1.0 + 0x1p-40;     // a bound must exceed best * kSlack

struct Grid : bulk::Grid {       // written by k_tri_bounds, read by every later kernel of the build and by k_tri_query.  gmin / gmax:
                                 // the box of the vertices of the usable faces, clipped to kStrayCells + 3 cells around the grid:
                                 // the vertices of every grid face lie inside
    double sigma_max;            // kSigmaCells / hmax^2
    double diag_max;             // upper bound of a grid face's longest edge: kLargeCells * |h|
};
// mesh_eval.TriIndex.layout() reads h, R, ncells and the three counts behind start[ncells] at these offsets of the index buffer (the
// head is the first base of Grid: at offset 0)
static_assert(offsetof(bulk::Grid, h) == 12 && offsetof(bulk::Grid, R) == 36 && offsetof(bulk::Grid, ncells) == 48 &&
                  sizeof(Grid) == sizeof(bulk::Grid) + 16 && sizeof(Grid) <= 256,
              "struct Grid moved: update TriIndex.layout() in nicer_slam_amd/mesh_eval.py");

struct Index {                   // views into the caller's index buffer (nsa_tri_workspace bytes)
    Grid* grid;
    uint32_t* start;             // [B + 3]: first sorted position of key c; keys: cell, ncells = large list, ncells + 1 = skipped
    float* box;                  // [B][6]: union of the record boxes of the cell
    float4* rec;                 // [2 F]: per sorted face (box lo xyz, face index bits), (box hi xyz, sigma)
    uint32_t* skey;              // [F]: sorted keys
    uint32_t* keys[2];           // [F] each: radix ping-pong
    uint32_t* tmp;               // [F]
    uint32_t* order;             // [F]
    uint32_t* counts;            // [256 * 256]
};

__host__ __device__ inline uint32_t budget(uint32_t F) {
    const uint64_t b = 2ull * F;
    return (uint32_t)(b > kMaxCells ? kMaxCells : b);
}

__host__ __device__ inline uint64_t carve(void* ws, uint32_t F, Index* out) {
    const uint32_t B = budget(F);
    char* base = static_cast<char*>(ws);
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) { char* p = base ? base + o : nullptr; o += up256(bytes); return p; };
    Index x;
    x.grid = reinterpret_cast<Grid*>(take(sizeof(Grid)));
    x.start = reinterpret_cast<uint32_t*>(take(4ull * (B + 3)));
    x.box = reinterpret_cast<float*>(take(24ull * B));
    x.rec = reinterpret_cast<float4*>(take(32ull * F));
    x.skey = reinterpret_cast<uint32_t*>(take(4ull * F));
    x.keys[0] = reinterpret_cast<uint32_t*>(take(4ull * F));
    x.keys[1] = reinterpret_cast<uint32_t*>(take(4ull * F));
    x.tmp = reinterpret_cast<uint32_t*>(take(4ull * F));
    x.order = reinterpret_cast<uint32_t*>(take(4ull * F));
    x.counts = reinterpret_cast<uint32_t*>(take(4ull * kRadixCountWords));
    if (out) *out = x;
    return o;
}

// the vertices of face i; 0 = usable, else the cause it is skipped for (1 index, 2 non-finite vertex, 3 zero area)
__device__ __forceinline__ int load_face(const float* __restrict__ v, uint32_t V, const int32_t* __restrict__ f, uint32_t i,
                                         float (&a)[3], float (&b)[3], float (&c)[3]) {
#pragma clang fp contract(off)
    const int32_t i0 = f[3ull * i], i1 = f[3ull * i + 1], i2 = f[3ull * i + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || (uint32_t)i0 >= V || (uint32_t)i1 >= V || (uint32_t)i2 >= V) return 1;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a[k] = v[3ull * i0 + k];
        b[k] = v[3ull * i1 + k];
        c[k] = v[3ull * i2 + k];
    }
    if (!finite3(a) || !finite3(b) || !finite3(c)) return 2;
    const double abx = (double)b[0] - a[0], aby = (double)b[1] - a[1], abz = (double)b[2] - a[2];
    const double acx = (double)c[0] - a[0], acy = (double)c[1] - a[1], acz = (double)c[2] - a[2];
    const double nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
    if (nx == 0.0 && ny == 0.0 && nz == 0.0) return 3;
    return 0;
}

struct Best {
    double d2, p[3];
    int32_t face;
    uint32_t evaluated;          // faces that went through closest_on_face (a measurement, not part of the answer)
    uint32_t cells;              // grid cells looked at, empty ones included (a measurement too)
};

__device__ __forceinline__ double dot3(const double (&u)[3], const double (&w)[3]) {
#pragma clang fp contract(off)
    return (u[0] * w[0] + u[1] * w[1]) + u[2] * w[2];
}

// the header's closest point of q on face (a, b, c), operation by operation; returns the feature code of Section 15: the branch
// that gave (s, t) -- 0 interior, 1 vertex a, 2 vertex b, 3 edge ab, 4 vertex c, 5 edge ac, 6 edge bc
__device__ __forceinline__ int closest_on_face(const double (&q)[3], const float (&a)[3], const float (&b)[3], const float (&c)[3],
                                                double (&p)[3], double& dist2) {
#pragma clang fp contract(off)
    double ab[3], ac[3], ap[3], bp[3], cp[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ab[k] = (double)b[k] - (double)a[k];
        ac[k] = (double)c[k] - (double)a[k];
        ap[k] = q[k] - (double)a[k];
        bp[k] = q[k] - (double)b[k];
        cp[k] = q[k] - (double)c[k];
    }
    const double d1 = dot3(ab, ap), d2 = dot3(ac, ap), d3 = dot3(ab, bp), d4 = dot3(ac, bp), d5 = dot3(ab, cp), d6 = dot3(ac, cp);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    double s, t;
    int feature;
    if (d1 <= 0.0 && d2 <= 0.0) {
        s = 0.0; t = 0.0; feature = 1;
    } else if (d3 >= 0.0 && d4 <= d3) {
        s = 1.0; t = 0.0; feature = 2;
    } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        s = d1 / (d1 - d3); t = 0.0; feature = 3;
    } else if (d6 >= 0.0 && d5 <= d6) {
        s = 0.0; t = 1.0; feature = 4;
    } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        s = 0.0; t = d2 / (d2 - d6); feature = 5;
    } else if (va <= 0.0 && d4 - d3 >= 0.0 && d5 - d6 >= 0.0) {
        const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        s = 1.0 - w; t = w; feature = 6;
    } else {
        const double e = 1.0 / ((va + vb) + vc);
        s = vb * e; t = vc * e; feature = 0;
    }
    double e[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        p[k] = ((double)a[k] + s * ab[k]) + t * ac[k];
        e[k] = q[k] - p[k];
    }
    dist2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
    return feature;
}

__device__ __forceinline__ double box_gap(double q, double lo, double hi) {
#pragma clang fp contract(off)
    return q < lo ? lo - q : (q > hi ? q - hi : 0.0);
}

// true when nothing at squared distance >= g2 that may be displaced by eps can reach the best (NaN or infinite eps: never)
__device__ __forceinline__ bool out_of_reach(double g2, double eps, double best) {
#pragma clang fp contract(off)
    if (!(g2 > best)) return false;
    const double r = sqrt(g2) - eps;
    return r > 0.0 && r * r > best * kSlack;
}

__device__ __forceinline__ void evaluate(const float* __restrict__ v, uint32_t V, const int32_t* __restrict__ f, uint32_t face,
                                         const double (&q)[3], Best& best) {
    const int32_t i0 = f[3ull * face], i1 = f[3ull * face + 1], i2 = f[3ull * face + 2];
    if ((uint32_t)i0 >= V || (uint32_t)i1 >= V || (uint32_t)i2 >= V) return;       // (not the mesh the index was built on)
    float a[3], b[3], c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a[k] = v[3ull * i0 + k];
        b[k] = v[3ull * i1 + k];
        c[k] = v[3ull * i2 + k];
    }
    double p[3], d2;
    closest_on_face(q, a, b, c, p, d2);
    best.evaluated++;
    if (d2 < best.d2 || (d2 == best.d2 && (int32_t)face < best.face)) {
        best.d2 = d2;
        best.face = (int32_t)face;
        best.p[0] = p[0]; best.p[1] = p[1]; best.p[2] = p[2];
    }
}

__device__ __forceinline__ double rec_gap2(const float4& lo, const float4& hi, const double (&q)[3]) {
#pragma clang fp contract(off)
    const double gx = box_gap(q[0], lo.x, hi.x), gy = box_gap(q[1], lo.y, hi.y), gz = box_gap(q[2], lo.z, hi.z);
    return (gx * gx + gy * gy) + gz * gz;
}

__device__ __forceinline__ void visit(const Index& ix, uint32_t c, const float* __restrict__ v, uint32_t V,
                                      const int32_t* __restrict__ f, const double (&q)[3], double eps, Best& best) {
#pragma clang fp contract(off)
    best.cells++;
    const uint32_t s = ix.start[c], e = ix.start[c + 1];
    if (s == e) return;
    const float* bx = ix.box + 6ull * c;
    const double gx = box_gap(q[0], bx[0], bx[3]), gy = box_gap(q[1], bx[1], bx[4]), gz = box_gap(q[2], bx[2], bx[5]);
    if (out_of_reach((gx * gx + gy * gy) + gz * gz, eps, best.d2)) return;
    for (uint32_t i = s; i < e; ++i) {
        const float4 lo = ix.rec[2ull * i], hi = ix.rec[2ull * i + 1];
        if (out_of_reach(rec_gap2(lo, hi, q), eps, best.d2)) continue;
        evaluate(v, V, f, __float_as_uint(lo.w), q, best);
    }
}

// the large list: every face on it, each with its own sigma and D <= its box's distance + diagonal
__device__ __forceinline__ void walk_large(const Index& ix, uint32_t first, uint32_t last, const float* __restrict__ v, uint32_t V,
                                           const int32_t* __restrict__ f, const double (&q)[3], Best& best) {
#pragma clang fp contract(off)
    for (uint32_t i = first; i < last; ++i) {
        const float4 lo = ix.rec[2ull * i], hi = ix.rec[2ull * i + 1];
        const double g2 = rec_gap2(lo, hi, q);
        if (g2 > best.d2) {
            const double ex = (double)hi.x - lo.x, ey = (double)hi.y - lo.y, ez = (double)hi.z - lo.z;
            const double diag = sqrt((ex * ex + ey * ey) + ez * ez), far = sqrt(g2) + diag;
            const double rho = kRhoUnit * (double)hi.w * (far * far);
            if (rho <= kRhoMax && out_of_reach(g2, rho * diag, best.d2)) continue;
        }
        evaluate(v, V, f, __float_as_uint(lo.w), q, best);
    }
}

// the walk of one finite query: its own cell, the large list, then the rings until the stop rule holds.  `best` comes in as the
// answer to beat -- (+inf, no face) for an unbounded query -- and every skip rule prunes against it from the first cell on
__device__ __forceinline__ void walk(const Index& ix, const float* __restrict__ v, uint32_t V, const int32_t* __restrict__ f,
                                     const float (&qf)[3], const double (&q)[3], Best& best) {
#pragma clang fp contract(off)
    const Grid g = *ix.grid;
    const uint32_t n_grid = ix.start[g.ncells], n_usable = ix.start[g.ncells + 1];
    if (n_grid > 0) {
        int c0[3];
        double out2[3], gpad[3], far2 = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            c0[k] = (int)axis_cell(qf[k], g.lo[k], g.inv_h[k], g.R[k]);
            gpad[k] = fmax(fabs((double)g.gmin[k]), fabs((double)g.gmax[k])) * (2.0 * kPad);
            const double o = fmax(fmax(((double)g.gmin[k] - q[k]) - gpad[k], (q[k] - (double)g.gmax[k]) - gpad[k]), 0.0);
            out2[k] = o * o;
            const double w = fmax(fabs(q[k] - (double)g.gmin[k]), fabs(q[k] - (double)g.gmax[k]));
            far2 += w * w;
        }
        // one displacement bound for every grid face: their sigma, edge length and distance from q are all bounded
        const double rho = kRhoUnit * g.sigma_max * far2 * (1.0 + 0x1p-30);
        const double eps = rho <= kRhoMax ? rho * g.diag_max : INFINITY;
        const int R0 = (int)g.R[0], R1 = (int)g.R[1], R2 = (int)g.R[2];
        for (int r = 0;; ++r) {
            if (r > 0) {                                // lower bound over every face keyed at index distance >= r
                // the list goes between the query's own cell and the rings: behind that cell its box tests prune against a
                // small best, and a query that a listed face answers stops the rings at once
                if (r == 1) walk_large(ix, n_grid, n_usable, v, V, f, q, best);
                double lb2 = INFINITY;
                bool any = false;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double h = g.h[k], back = h * 0x1p-9 + kLargeCells * h + gpad[k], lo = g.lo[k];
                    const double rest = out2[0] + out2[1] + out2[2] - out2[k];
                    const double ok = sqrt(out2[k]);
                    if (c0[k] + r <= (int)g.R[k] - 1) {
                        const double gap = fmax(fmax(lo + (double)(c0[k] + r) * h - q[k] - back, ok), 0.0);
                        lb2 = fmin(lb2, gap * gap + rest);
                        any = true;
                    }
                    if (c0[k] - r >= 0) {
                        const double gap = fmax(fmax(q[k] - (lo + (double)(c0[k] - r + 1) * h) - back, ok), 0.0);
                        lb2 = fmin(lb2, gap * gap + rest);
                        any = true;
                    }
                }
                if (!any || out_of_reach(lb2 * (1.0 - 0x1p-40), eps, best.d2)) break;
            }
            const int x0 = max(c0[0] - r, 0), x1 = min(c0[0] + r, R0 - 1);
            const int y0 = max(c0[1] - r, 0), y1 = min(c0[1] + r, R1 - 1);
            const int z0 = max(c0[2] - r, 0), z1 = min(c0[2] + r, R2 - 1);
            for (int x = x0; x <= x1; ++x) {
                const bool ex = x == c0[0] - r || x == c0[0] + r;
                for (int y = y0; y <= y1; ++y) {
                    const uint32_t row = ((uint32_t)x * g.R[1] + (uint32_t)y) * g.R[2];
                    if (ex || y == c0[1] - r || y == c0[1] + r) {
                        for (int z = z0; z <= z1; ++z) visit(ix, row + z, v, V, f, q, eps, best);
                    } else {
                        if (c0[2] - r >= 0) visit(ix, row + (c0[2] - r), v, V, f, q, eps, best);
                        if (r > 0 && c0[2] + r < R2) visit(ix, row + (c0[2] + r), v, V, f, q, eps, best);
                    }
                }
            }
        }
    }
    if (n_grid == 0) walk_large(ix, n_grid, n_usable, v, V, f, q, best);
}

}  // namespace tri
}  // namespace nsa
