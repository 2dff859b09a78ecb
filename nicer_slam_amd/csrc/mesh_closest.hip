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
// Index: the grid of bulk_grid.hpp (bulk quantiles of a strided subsample, near-cubic cells, border clamping), over the fp32 centroids
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
#include "tri_common.hpp"

namespace nsa {
namespace tri {

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

__device__ __forceinline__ float centroid(float a, float b, float c) {
#pragma clang fp contract(off)
    return (float)((((double)a + (double)b) + (double)c) / 3.0);
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

// one workgroup: skip counts, the box of the usable faces' vertices, the bulk of their centroids and the grid over it
__global__ __launch_bounds__(1024) void k_tri_bounds(const float* __restrict__ v, uint32_t V, const int32_t* __restrict__ f,
                                                     uint32_t F, uint32_t cells, Index ix, uint32_t* __restrict__ totals) {
    using bulk::block_reduce;
    using bulk::kSubsample;
    __shared__ float sv[3][kSubsample];
    __shared__ float red[16];
    __shared__ uint32_t redu[16];
    __shared__ float s_bulk[2][3];
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
    bulk::rank_bulk(sv, m, m_f, s_bulk);
    if (tid != 0) return;
    if (totals) {
        totals[0] = tot[0];
        totals[1] = tot[1];
        totals[2] = tot[2];
    }
    Grid g;
    bulk::solve(s_bulk[0], s_bulk[1], m_f, cells, g);
    double hmax = 0.0, h2 = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        g.gmin[k] = gmin[k];
        g.gmax[k] = gmax[k];
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
            g.gmax[k] = fminf(g.gmax[k], round_up(lo + ((double)g.R[k] + kStrayCells + 3.0) * h));
        }
    }
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
    Best best{INFINITY, {nan, nan, nan}, -1, 0, 0};
    if (finite3(qf)) {
        walk(ix, v, V, f, qf, q, best);
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
