// mesh_closest.hip -- exact closest point on a triangle mesh for a batch of query points (DESIGN 4m, C ABI Section 14).
// Reference: code/evaluation/eval_rec.py:120-129 (distance_p2m, through trimesh.proximity.closest_point; carried by the reference,
// never called there: too slow on the host).
//
// Contract (restated by tests/p2m_ref.py in numpy float64): for query q and face (a, b, c), all in float64 on the fp32 inputs, every
// operation rounded on its own, dot(u, v) = (u_x v_x + u_y v_y) + u_z v_z:
//     ab = b - a, ac = c - a, ap = q - a, bp = q - b, cp = q - c
//     d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp)
//     vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4
//     (s, t) = the first of   d1 <= 0 and d2 <= 0                      -> (0, 0)                                     vertex a
//                             d3 >= 0 and d4 <= d3                     -> (1, 0)                                     vertex b
//                             vc <= 0 and d1 >= 0 and d3 <= 0          -> (d1 / (d1 - d3), 0)                        edge ab
//                             d6 >= 0 and d5 <= d6                     -> (0, 1)                                     vertex c
//                             vb <= 0 and d2 >= 0 and d6 <= 0          -> (0, d2 / (d2 - d6))                        edge ac
//                             va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0 -> w = (d4 - d3) / ((d4 - d3) + (d5 - d6)): (1 - w, w)   edge bc
//                             otherwise                                -> e = 1 / ((va + vb) + vc): (vb e, vc e)     interior
//     p = (a + s ab) + t ac ;  e = q - p ;  d2(q, face) = (e_x e_x + e_y e_y) + e_z e_z
// The winner is the usable face with the smallest d2 (a NaN d2 never wins), ties to the lowest face index.
//
// Index: the grid of mesh_eval.hip (bulk quantiles of a strided subsample, near-cubic cells, border clamping), over the fp32 centroids
// cf = fp32(((a + b) + c) / 3) of the usable faces, at most B = min(2F, 2^22) cells.  A face whose box is longer than 2 cells on an
// axis, or whose shape factor sigma = Lmax^2 / |ab x ac|^2 (Lmax the longest edge) exceeds 2^16 / hmax^2 (hmax the longest cell
// edge), or whose centroid lies more than 256 cells outside the grid (a stray component far from the bulk), goes on the LARGE LIST
// instead, which every query walks; skipped faces sort behind both.  Every face record holds the face's
// fp32 box, each bound moved outwards by 2^-40 of the larger bound's magnitude and rounded outwards, and every cell the union of
// its records' boxes.
//
// Bounds and their margins.  The computed p of a face differs from a point of the triangle by (1) the rounding of (a + s ab) + t ac,
// below 2^-50 of the coordinates' magnitude per axis -- inside the 2^-40 the boxes are padded by -- and (2), in the interior branch
// only, the error of (s, t): va, vb, vc are differences of products of magnitude L^2 D^2 (D = the largest distance from q to a
// vertex of the face) and carry an error below 40 u L^2 D^2 (u = 2^-53), against their exact sum |ab x ac|^2; p moves by less than
// rho L with rho = 2^-43 sigma D^2 (a factor 6 above that count) as long as rho <= 1/4.  So a box at distance g from q is skipped
// only when rho <= 1/4 and (g - rho diag)^2 > best (1 + 2^-40), diag >= L the box diagonal and 2^-40 far above the float64 rounding of
// the bound itself; with rho > 1/4 nothing is skipped.  For grid faces sigma <= 2^16 / hmax^2, diag <= 2 |h| and D <= the distance
// from q to the far corner of the grid faces' box (the mesh's box clipped to 259 cells around the grid: rho <= 0.053 for any query
// inside it), one rho per query; a large face uses its own sigma and D <= g + diag.  The ring walk
// stops when, per axis and side, the cell plane at the ring less 2^-9 cell (the fp32 cell index is off by less than 2^-12 cell) less
// the reach of a grid face beyond its centroid (2 cells, plus the padding) -- combined with the query's distance to the grid faces'
// box on the other axes -- passes that same test.  A query visits its own cell, then the large list, then the rings.  Worst cases:
// every face in one cell, every face large, or a query so far away (2^12.5 cells from the far corner of that box) that rho > 1/4:
// each is a brute force over the faces, slow and never wrong.
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include "../../include/nicer_slam_amd.h"
#include "grid_common.hpp"
#include "radix_sort.hpp"

namespace nsa {
namespace tri {

constexpr uint32_t kMaxCells = 1u << 22;
constexpr uint32_t kMaxRes = 1024;
constexpr uint32_t kSubsample = 2048;
constexpr uint32_t kMaxCount = 0x7FFFFFFFu;
constexpr double kLargeCells = 2.0;          // a grid face's box is at most this many cells long on every axis
constexpr double kSigmaCells = 0x1p16;       // a grid face's sigma is at most this / hmax^2: rho <= 1/4 up to 2^12.5 cells from q,
                                             // beyond the 2^10 sqrt(3) cells a grid can measure; height >= hmax / 256
constexpr double kStrayCells = 256.0;        // a grid face's centroid is at most this many cells outside the grid
constexpr double kRhoUnit = 0x1p-43;         // rho = kRhoUnit * sigma * D^2
constexpr double kRhoMax = 0.25;
constexpr double kPad = 0x1p-40;             // box padding, relative to the coordinate's magnitude
constexpr double kSlack = 1.0 + 0x1p-40;     // a bound must exceed best * kSlack

struct Grid {                    // written by k_tri_bounds, read by every later kernel of the build and by k_tri_query
    float lo[3], h[3], inv_h[3];
    uint32_t R[3], ncells, pad;
    float gmin[3], gmax[3];      // bounding box of the vertices of the usable faces (+inf / -inf when there are none), clipped to
                                 // kStrayCells + 3 cells around the grid: the vertices of every grid face lie inside
    double sigma_max;            // kSigmaCells / hmax^2
    double diag_max;             // upper bound of a grid face's longest edge: kLargeCells * |h|
};
// mesh_eval.TriIndex.layout() reads h, R, ncells and the three counts behind start[ncells] at these offsets of the index buffer
static_assert(offsetof(Grid, h) == 12 && offsetof(Grid, R) == 36 && offsetof(Grid, ncells) == 48 && sizeof(Grid) <= 256,
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

__host__ __device__ inline uint64_t up256(uint64_t b) { return (b + 255) & ~uint64_t(255); }
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

__device__ __forceinline__ bool finite3(const float (&p)[3]) {
    return __builtin_isfinite(p[0]) && __builtin_isfinite(p[1]) && __builtin_isfinite(p[2]);
}

// the fp32 value at or above / at or below x (one rounding, outwards)
__device__ __forceinline__ float round_up(double x) {
    float f = (float)x;
    if ((double)f < x) {
        const uint32_t u = __float_as_uint(f);
        f = f == 0.0f ? __uint_as_float(1u) : __uint_as_float(f > 0.0f ? u + 1 : u - 1);
    }
    return f;
}
__device__ __forceinline__ float round_down(double x) { return -round_up(-x); }

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

__device__ __forceinline__ float centroid(float a, float b, float c) {
#pragma clang fp contract(off)
    return (float)((((double)a + (double)b) + (double)c) / 3.0);
}

// cell index along one axis, clamped into [0, R - 1] (x finite)
__device__ __forceinline__ uint32_t axis_cell(float x, float lo, float inv_h, uint32_t R) {
#pragma clang fp contract(off)
    const float u = (x - lo) * inv_h;
    return (uint32_t)fminf(fmaxf(u, 0.0f), (float)(R - 1));
}

// the record of a usable face: padded box, sigma (rounded up) and its key (a cell, or ncells for the large list)
__device__ __forceinline__ uint32_t face_record(const Grid& g, const float (&a)[3], const float (&b)[3], const float (&c)[3],
                                                float (&plo)[3], float (&phi)[3], float& sigma) {
#pragma clang fp contract(off)
    bool large = false;
    uint32_t cell[3];
    double ab[3], ac[3], bc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float lo = fminf(fminf(a[k], b[k]), c[k]), hi = fmaxf(fmaxf(a[k], b[k]), c[k]);
        const double pad = fmax(fabs((double)lo), fabs((double)hi)) * kPad;
        plo[k] = round_down((double)lo - pad);
        phi[k] = round_up((double)hi + pad);
        large |= !((double)hi - (double)lo <= kLargeCells * (double)g.h[k]);
        const float cf = centroid(a[k], b[k], c[k]);
        large |= !((double)cf >= (double)g.lo[k] - kStrayCells * (double)g.h[k] &&
                   (double)cf <= (double)g.lo[k] + ((double)g.R[k] + kStrayCells) * (double)g.h[k]);
        cell[k] = axis_cell(cf, g.lo[k], g.inv_h[k], g.R[k]);
        ab[k] = (double)b[k] - a[k];
        ac[k] = (double)c[k] - a[k];
        bc[k] = (double)c[k] - b[k];
    }
    const double nx = ab[1] * ac[2] - ab[2] * ac[1], ny = ab[2] * ac[0] - ab[0] * ac[2], nz = ab[0] * ac[1] - ab[1] * ac[0];
    const double n2 = (nx * nx + ny * ny) + nz * nz;
    const double l0 = (ab[0] * ab[0] + ab[1] * ab[1]) + ab[2] * ab[2], l1 = (ac[0] * ac[0] + ac[1] * ac[1]) + ac[2] * ac[2],
                 l2 = (bc[0] * bc[0] + bc[1] * bc[1]) + bc[2] * bc[2];
    const double s = fmax(fmax(l0, l1), l2) / n2;
    sigma = round_up(s);
    large |= !(s <= g.sigma_max);
    return large ? g.ncells : (cell[0] * g.R[1] + cell[1]) * g.R[2] + cell[2];
}

template <typename T, typename Op>
__device__ __forceinline__ T block_reduce(T v, Op op, T* red) {    // 1024 threads; red[16]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    T r = red[0];
    for (int w = 1; w < 16; ++w) r = op(r, red[w]);
    return r;
}

// one workgroup: skip counts, the box of the usable faces' vertices, the bulk of their centroids and the grid over it
__global__ __launch_bounds__(1024) void k_tri_bounds(const float* __restrict__ v, uint32_t V, const int32_t* __restrict__ f,
                                                     uint32_t F, uint32_t cells, Index ix, uint32_t* __restrict__ totals) {
    __shared__ float sv[3][kSubsample];
    __shared__ float red[16];
    __shared__ uint32_t redu[16];
    __shared__ float bulk[2][3];
    const uint32_t tid = threadIdx.x;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    uint32_t skipped[3] = {0, 0, 0};
    float a[3], b[3], c[3];
    for (uint32_t i = tid; i < F; i += 1024) {
        const int cause = load_face(v, V, f, i, a, b, c);
        if (cause) {
            skipped[cause - 1]++;
            continue;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            mn[k] = fminf(mn[k], fminf(fminf(a[k], b[k]), c[k]));
            mx[k] = fmaxf(mx[k], fmaxf(fmaxf(a[k], b[k]), c[k]));
        }
    }
    float gmin[3], gmax[3];
    uint32_t tot[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        gmin[k] = block_reduce(mn[k], [](float p, float q) { return fminf(p, q); }, red);
        gmax[k] = block_reduce(mx[k], [](float p, float q) { return fmaxf(p, q); }, red);
        tot[k] = block_reduce(skipped[k], [](uint32_t p, uint32_t q) { return p + q; }, redu);
    }
    // strided subsample of the centroids; skipped faces are left out of the ranking (+inf and not counted)
    const uint32_t m = F < kSubsample ? F : kSubsample;
    uint32_t nf = 0;
    for (uint32_t j = tid; j < kSubsample; j += 1024) {
        bool ok = false;
        if (j < m) ok = load_face(v, V, f, (uint32_t)((uint64_t)j * F / m), a, b, c) == 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) sv[k][j] = ok ? centroid(a[k], b[k], c[k]) : INFINITY;
        nf += ok;
    }
    const uint32_t m_f = block_reduce(nf, [](uint32_t p, uint32_t q) { return p + q; }, redu);
    __syncthreads();
    const uint32_t k_lo = m_f >> 6, k_hi = m_f ? m_f - 1 - k_lo : 0;
    for (int ax = 0; ax < 3; ++ax) {
        for (uint32_t j = tid; j < m; j += 1024) {
            const float x = sv[ax][j];
            if (!__builtin_isfinite(x)) continue;
            uint32_t rank = 0;
            for (uint32_t i = 0; i < m; ++i) {
                const float w = sv[ax][i];
                rank += (w < x) || (w == x && i < j);
            }
            if (rank == k_lo) bulk[0][ax] = x;
            if (rank == k_hi) bulk[1][ax] = x;
        }
    }
    __syncthreads();
    if (tid != 0) return;
    if (totals) {
        totals[0] = tot[0];
        totals[1] = tot[1];
        totals[2] = tot[2];
    }
    Grid g;
    double e[3], emax = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        g.gmin[k] = gmin[k];
        g.gmax[k] = gmax[k];
        g.lo[k] = m_f ? bulk[0][k] : 0.0f;
        e[k] = m_f ? (double)bulk[1][k] - (double)bulk[0][k] : 0.0;
        emax = e[k] > emax ? e[k] : emax;
    }
    uint32_t R[3] = {1, 1, 1};
    if (emax > 0.0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) e[k] = e[k] > emax * 0x1p-10 ? e[k] : emax * 0x1p-10;
        double cs = cbrt(e[0] * e[1] * e[2] / cells);
        for (int it = 0; it < 200; ++it) {             // near-cubic cells, at most `cells` of them
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double r = floor(e[k] / cs);
                R[k] = r < 1.0 ? 1u : (r > kMaxRes ? kMaxRes : (uint32_t)r);
            }
            if ((uint64_t)R[0] * R[1] * R[2] <= cells) break;
            cs *= 1.0625;
        }
        if ((uint64_t)R[0] * R[1] * R[2] > cells) R[0] = R[1] = R[2] = 1;     // (never reached; keeps the cell arrays in bounds)
    }
    double hmax = 0.0, h2 = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float h = emax > 0.0 ? (float)(e[k] / R[k]) : 1.0f;
        g.h[k] = h > 1e-30f ? h : 1e-30f;
        g.inv_h[k] = 1.0f / g.h[k];
        g.R[k] = R[k];
        hmax = fmax(hmax, (double)g.h[k]);
        h2 += (double)g.h[k] * (double)g.h[k];
    }
    if (m_f) {
        // a grid face's centroid lies within kStrayCells of the grid and its box is at most 2 cells long: 3 cells cover its vertices
        // and the rounding of the centroid; the bounds themselves are rounded outwards
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double lo = g.lo[k], h = g.h[k];
            g.gmin[k] = fmaxf(g.gmin[k], round_down(lo - (kStrayCells + 3.0) * h));
            g.gmax[k] = fminf(g.gmax[k], round_up(lo + ((double)R[k] + kStrayCells + 3.0) * h));
        }
    }
    g.ncells = R[0] * R[1] * R[2];
    g.pad = 0;
    g.sigma_max = kSigmaCells / (hmax * hmax);
    g.diag_max = kLargeCells * sqrt(h2) * (1.0 + 0x1p-30);
    *ix.grid = g;
}

__global__ __launch_bounds__(256) void k_tri_keys(const float* __restrict__ v, uint32_t V, const int32_t* __restrict__ f, uint32_t F,
                                                  Index ix) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= F) return;
    const Grid& g = *ix.grid;
    float a[3], b[3], c[3], plo[3], phi[3], sigma;
    ix.keys[0][i] = load_face(v, V, f, i, a, b, c) ? g.ncells + 1 : face_record(g, a, b, c, plo, phi, sigma);
}

__global__ __launch_bounds__(256) void k_tri_gather(const float* __restrict__ v, uint32_t V, const int32_t* __restrict__ f,
                                                    uint32_t F, Index ix) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= F) return;
    const Grid& g = *ix.grid;
    const uint32_t face = ix.order[i];
    float a[3], b[3], c[3], sigma = INFINITY;
    float plo[3] = {INFINITY, INFINITY, INFINITY}, phi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const uint32_t key = load_face(v, V, f, face, a, b, c) ? g.ncells + 1 : face_record(g, a, b, c, plo, phi, sigma);
    ix.rec[2ull * i] = make_float4(plo[0], plo[1], plo[2], __uint_as_float(face));
    ix.rec[2ull * i + 1] = make_float4(phi[0], phi[1], phi[2], sigma);
    ix.skey[i] = key;
}

__device__ __forceinline__ uint32_t lower_bound(const uint32_t* __restrict__ a, uint32_t n, uint32_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// one lane per key c in [0, ncells + 2]: start[c], and the union of the record boxes of cell c < ncells
__global__ __launch_bounds__(256) void k_tri_cells(uint32_t F, Index ix) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    const uint32_t ncells = ix.grid->ncells;
    if (c > ncells + 2) return;
    const uint32_t s = lower_bound(ix.skey, F, c);
    ix.start[c] = s;
    if (c >= ncells) return;
    const uint32_t e = lower_bound(ix.skey, F, c + 1);
    float b[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (uint32_t i = s; i < e; ++i) {
        const float4 lo = ix.rec[2ull * i], hi = ix.rec[2ull * i + 1];
        b[0] = fminf(b[0], lo.x); b[1] = fminf(b[1], lo.y); b[2] = fminf(b[2], lo.z);
        b[3] = fmaxf(b[3], hi.x); b[4] = fmaxf(b[4], hi.y); b[5] = fmaxf(b[5], hi.z);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) ix.box[6ull * c + k] = b[k];
}

// ---- query ----------------------------------------------------------------------------------------------------------------------

struct Best {
    double d2, p[3];
    int32_t face;
    uint32_t evaluated;          // faces that went through closest_on_face (a measurement, not part of the answer)
};

__device__ __forceinline__ double dot3(const double (&u)[3], const double (&w)[3]) {
#pragma clang fp contract(off)
    return (u[0] * w[0] + u[1] * w[1]) + u[2] * w[2];
}

// the header's closest point of q on face (a, b, c), operation by operation
__device__ __forceinline__ void closest_on_face(const double (&q)[3], const float (&a)[3], const float (&b)[3], const float (&c)[3],
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
    if (d1 <= 0.0 && d2 <= 0.0) {
        s = 0.0; t = 0.0;
    } else if (d3 >= 0.0 && d4 <= d3) {
        s = 1.0; t = 0.0;
    } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        s = d1 / (d1 - d3); t = 0.0;
    } else if (d6 >= 0.0 && d5 <= d6) {
        s = 0.0; t = 1.0;
    } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        s = 0.0; t = d2 / (d2 - d6);
    } else if (va <= 0.0 && d4 - d3 >= 0.0 && d5 - d6 >= 0.0) {
        const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        s = 1.0 - w; t = w;
    } else {
        const double e = 1.0 / ((va + vb) + vc);
        s = vb * e; t = vc * e;
    }
    double e[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        p[k] = ((double)a[k] + s * ab[k]) + t * ac[k];
        e[k] = q[k] - p[k];
    }
    dist2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
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

__global__ __launch_bounds__(256) void k_tri_query(Index ix, const float* __restrict__ v, uint32_t V, const int32_t* __restrict__ f,
                                                   const float* __restrict__ qs, uint32_t m, int32_t* __restrict__ out_face,
                                                   double* __restrict__ out_d2, float* __restrict__ out_p,
                                                   uint32_t* __restrict__ out_evaluated) {
#pragma clang fp contract(off)
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const float qf[3] = {qs[3ull * j], qs[3ull * j + 1], qs[3ull * j + 2]};
    const double q[3] = {qf[0], qf[1], qf[2]};
    const double nan = __builtin_nan("");
    Best best{INFINITY, {nan, nan, nan}, -1, 0};
    if (finite3(qf)) {
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
    } else {
        best.d2 = nan;
    }
    out_face[j] = best.face;
    out_d2[j] = best.d2;
    if (out_evaluated) out_evaluated[j] = best.evaluated;
    if (out_p) {
        out_p[3ull * j] = (float)best.p[0];
        out_p[3ull * j + 1] = (float)best.p[1];
        out_p[3ull * j + 2] = (float)best.p[2];
    }
}

}  // namespace tri
}  // namespace nsa

extern "C" {

uint64_t nsa_tri_workspace(uint32_t n_faces) {
    if (n_faces == 0 || n_faces > nsa::tri::kMaxCount) return 0;
    return nsa::tri::carve(nullptr, n_faces, nullptr);
}

int nsa_tri_build(const float* verts, uint32_t n_verts, const int32_t* faces, uint32_t n_faces, void* index, uint32_t* totals,
                  nsa_stream_t stream) {
    using namespace nsa;
    using namespace nsa::tri;
    if (!verts || !faces || !index || n_verts == 0 || n_faces == 0 || n_verts > kMaxCount || n_faces > kMaxCount) return NSA_EBADARG;
    Index ix;
    carve(index, n_faces, &ix);
    const uint32_t B = budget(n_faces), nb = (n_faces + 255) / 256;
    uint32_t bits = 1;
    while ((1ull << bits) <= (uint64_t)B + 1) ++bits;  // keys are <= ncells + 1 <= B + 1
    launch_begin();
    hipLaunchKernelGGL(k_tri_bounds, dim3(1), dim3(1024), 0, (hipStream_t)stream, verts, n_verts, faces, n_faces, B, ix, totals);
    hipLaunchKernelGGL(k_tri_keys, dim3(nb), dim3(256), 0, (hipStream_t)stream, verts, n_verts, faces, n_faces, ix);
    radix_argsort(ix.keys, ix.tmp, ix.order, ix.counts, n_faces, 0, (bits + 7) / 8, stream);
    hipLaunchKernelGGL(k_tri_gather, dim3(nb), dim3(256), 0, (hipStream_t)stream, verts, n_verts, faces, n_faces, ix);
    hipLaunchKernelGGL(k_tri_cells, dim3((B + 3 + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_faces, ix);
    return launch_end();
}

int nsa_tri_query_counted(const void* index, const float* verts, uint32_t n_verts, const int32_t* faces, uint32_t n_faces,
                          const float* queries, uint32_t n_queries, int32_t* face_idx, double* d2, float* closest,
                          uint32_t* evaluated, nsa_stream_t stream) {
    using namespace nsa;
    using namespace nsa::tri;
    if (!index || !verts || !faces || n_verts == 0 || n_faces == 0 || n_verts > kMaxCount || n_faces > kMaxCount ||
        n_queries > kMaxCount)
        return NSA_EBADARG;
    if (n_queries && (!queries || !face_idx || !d2)) return NSA_EBADARG;
    if (n_queries == 0) return NSA_OK;
    Index ix;
    carve(const_cast<void*>(index), n_faces, &ix);
    launch_begin();
    hipLaunchKernelGGL(k_tri_query, dim3((n_queries + 255) / 256), dim3(256), 0, (hipStream_t)stream, ix, verts, n_verts, faces,
                       queries, n_queries, face_idx, d2, closest, evaluated);
    return launch_end();
}

int nsa_tri_query(const void* index, const float* verts, uint32_t n_verts, const int32_t* faces, uint32_t n_faces,
                  const float* queries, uint32_t n_queries, int32_t* face_idx, double* d2, float* closest, nsa_stream_t stream) {
    return nsa_tri_query_counted(index, verts, n_verts, faces, n_faces, queries, n_queries, face_idx, d2, closest, nullptr, stream);
}

}  // extern "C"
