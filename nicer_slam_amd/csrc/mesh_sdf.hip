// mesh_sdf.hip -- signed distance to a triangle mesh and range-limited closest-point queries on the index of mesh_closest.hip
// (DESIGN 4n, C ABI Section 15).  The winner -- face, d2, closest point -- is Section 14's, found by the same walk (tri_common.hpp);
// this file adds the vertex -> face adjacency, the angle-weighted pseudo-normal of the winner's feature (Baerentzen & Aanaes,
// "Signed distance computation using the angle weighted pseudonormal", IEEE TVCG 11(3), 2005) and the bound.
//
// Contract (restated by tests/sdf_ref.py in numpy float64), all float64 with every operation rounded on its own:
//     feature   the branch of closest_on_face that gave the winner's (s, t): 0 interior, 1 vertex a, 2 vertex b, 3 edge ab, 4 vertex c,
//               5 edge ac, 6 edge bc; -1 without a winner
//     n_g       = (ab x ac) / sqrt((x^2 + y^2) + z^2) of face g, ab x ac = (ab_y ac_z - ab_z ac_y, ab_z ac_x - ab_x ac_z, ab_x ac_y - ab_y ac_x)
//     N, W      interior: n_f, 1.  Edge {i, j}: the sum of n_g over the contributing faces g that list both i and j, ascending g, and
//               their count.  Vertex i: the sum of alpha_g n_g over the contributing corners at i, ascending g, alpha_g =
//               atan2(|u x w|, u . w) with u, w the edges to the next and the previous corner of g, and the sum of alpha_g
//     sign      -1 when e . N < 0 for e = q - p (p in float64), else +1; `flip` negates it
// i, j are ADJACENCY indices: a second face array with the numbering of the index's faces, whose vertices are named so that
// coincident ones share a name.  A face contributes when it is usable under Section 14 and its three adjacency indices lie in [0, V).
//
// Bound: the walk starts from best = the float64 after max_d2 with no face, so a face is taken exactly when its d2 <= max_d2, and
// every skip rule of Section 14 prunes against min(best so far, that) from the first cell on.  Those rules never skip a face whose d2
// is <= the value they prune against, and that value never falls below the unbounded winner's d2 while it is <= max_d2: the bounded
// answer is the unbounded one, or none.
//
// Adjacency: the 3F corners keyed by adjacency vertex (V for a face that does not contribute), the stable radix argsort of
// radix_sort.hpp -- corner 3g + k in index order, so ascending g within a vertex -- and the start offsets by binary search
// (corner_table.hpp).  No atomic takes part; the order of every sum is fixed by the sort.  A query that lands on a vertex of valence k
// walks k corners.
#include "tri_common.hpp"
#include "corner_table.hpp"

namespace nsa {
namespace tri {

// the adjacency buffer (nsa_tri_adjacency_workspace bytes) is the corner table of corner_table.hpp, which the vertex normals of
// mesh_smooth.hip share: start [V + 2], corner [3 F] sorted by key and ascending within a key, and the sort's buffers
using Adjacency = corners::Table;

__host__ __device__ inline uint64_t carve_adjacency(void* ws, uint32_t V, uint32_t F, Adjacency* out) {
    return corners::carve(ws, V, F, out);
}

// the key of corner i = 3 g + k: its adjacency vertex, or V when face g does not contribute
struct AdjacencyKey {
    const float* v;
    uint32_t V;
    const int32_t* f;
    const int32_t* adj;
    __device__ uint32_t operator()(uint32_t i) const {
        const uint32_t g = i / 3;
        const int32_t j0 = adj[3ull * g], j1 = adj[3ull * g + 1], j2 = adj[3ull * g + 2];
        if ((uint32_t)j0 >= V || (uint32_t)j1 >= V || (uint32_t)j2 >= V) return V;
        float a[3], b[3], c[3];
        if (load_face(v, V, f, g, a, b, c)) return V;
        return (uint32_t)adj[i];
    }
};

// ---- the pseudo-normal ----------------------------------------------------------------------------------------------------------

// the vertices of face g of the index's mesh; false when an index lies outside [0, V) (not the mesh the index was built on)
__device__ __forceinline__ bool face_vertices(const float* __restrict__ v, uint32_t V, const int32_t* __restrict__ f, uint32_t g,
                                              float (&x)[3][3]) {
    const int32_t i0 = f[3ull * g], i1 = f[3ull * g + 1], i2 = f[3ull * g + 2];
    if ((uint32_t)i0 >= V || (uint32_t)i1 >= V || (uint32_t)i2 >= V) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        x[0][k] = v[3ull * i0 + k];
        x[1][k] = v[3ull * i1 + k];
        x[2][k] = v[3ull * i2 + k];
    }
    return true;
}

using bulk::cross3;

// n = weight * (ab x ac) / |ab x ac| added to N, component by component
__device__ __forceinline__ void add_unit_normal(const float (&x)[3][3], double weight, bool weighted, double (&N)[3]) {
#pragma clang fp contract(off)
    double ab[3], ac[3], n[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ab[k] = (double)x[1][k] - (double)x[0][k];
        ac[k] = (double)x[2][k] - (double)x[0][k];
    }
    cross3(ab, ac, n);
    const double len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double unit = n[k] / len;
        N[k] = N[k] + (weighted ? weight * unit : unit);
    }
}

// the angle of face x at its corner k, between the edges to the next and to the previous corner
__device__ __forceinline__ double corner_angle(const float (&x)[3][3], uint32_t k) {
#pragma clang fp contract(off)
    const uint32_t kn = k == 2 ? 0 : k + 1, kp = k == 0 ? 2 : k - 1;
    double u[3], w[3], n[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        u[d] = (double)x[kn][d] - (double)x[k][d];
        w[d] = (double)x[kp][d] - (double)x[k][d];
    }
    cross3(u, w, n);
    return atan2(sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]), dot3(u, w));
}

// N and W of vertex i: every contributing corner at i, in ascending face order
__device__ __forceinline__ void vertex_normal(const Adjacency& ad, const float* __restrict__ v, uint32_t V,
                                              const int32_t* __restrict__ f, uint32_t F, uint32_t i, double (&N)[3], double& W) {
#pragma clang fp contract(off)
    if (i >= V) return;
    const uint32_t s = ad.start[i], e = ad.start[i + 1];
    for (uint32_t t = s; t < e; ++t) {
        const uint32_t c = ad.corner[t], g = c / 3;
        float x[3][3];
        if (g >= F || !face_vertices(v, V, f, g, x)) continue;
        const double alpha = corner_angle(x, c - 3 * g);
        add_unit_normal(x, alpha, true, N);
        W = W + alpha;
    }
}

// N and W of edge {i, j}: every contributing face that lists both, once, in ascending face order -- found on the shorter list
__device__ __forceinline__ void edge_normal(const Adjacency& ad, const float* __restrict__ v, uint32_t V, const int32_t* __restrict__ f,
                                            const int32_t* __restrict__ adj, uint32_t F, uint32_t i, uint32_t j, double (&N)[3],
                                            double& W) {
#pragma clang fp contract(off)
    if (i >= V || j >= V) return;
    if (ad.start[j + 1] - ad.start[j] < ad.start[i + 1] - ad.start[i]) {
        const uint32_t t = i;
        i = j;
        j = t;
    }
    const uint32_t s = ad.start[i], e = ad.start[i + 1];
    for (uint32_t t = s; t < e; ++t) {
        const uint32_t c = ad.corner[t], g = c / 3, k = c - 3 * g;
        if (g >= F) continue;
        const uint32_t j0 = (uint32_t)adj[3ull * g], j1 = (uint32_t)adj[3ull * g + 1], j2 = (uint32_t)adj[3ull * g + 2];
        const uint32_t first = j0 == i ? 0 : (j1 == i ? 1 : 2);            // a face that lists i twice counts at its first corner
        if (k != first || !(j0 == j || j1 == j || j2 == j)) continue;
        float x[3][3];
        if (!face_vertices(v, V, f, g, x)) continue;
        add_unit_normal(x, 1.0, false, N);
        W = W + 1.0;
    }
}

// ---- query ----------------------------------------------------------------------------------------------------------------------

struct SignedOut {
    int32_t* face;
    double* d2;
    float* closest;              // may be null
    int8_t* feature;             // may be null when not SIGNED
    int8_t* sign;                // may be null when not SIGNED
    double* normal;              // [m, 3], may be null
    double* weight;              // [m], may be null
    uint32_t* evaluated;         // may be null
    uint32_t* cells;             // may be null
};

// one lane per query: Section 14's walk from `limit` (the float64 after max_d2; +inf unbounded), then, SIGNED, the pseudo-normal of the
// winner's feature
template <bool SIGNED>
__global__ __launch_bounds__(256) void k_tri_signed(Index ix, Adjacency ad, const float* __restrict__ v, uint32_t V,
                                                    const int32_t* __restrict__ f, const int32_t* __restrict__ adj, uint32_t F,
                                                    const float* __restrict__ qs, uint32_t m, double limit, int flip, SignedOut out) {
#pragma clang fp contract(off)
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const float qf[3] = {qs[3ull * j], qs[3ull * j + 1], qs[3ull * j + 2]};
    const double q[3] = {qf[0], qf[1], qf[2]};
    const double nan = __builtin_nan("");
    Best best{limit, {nan, nan, nan}, -1, 0, 0};
    if (finite3(qf)) {
        walk(ix, v, V, f, qf, q, best);
        if (best.face < 0) best.d2 = INFINITY;
    } else {
        best.d2 = nan;
    }
    out.face[j] = best.face;
    out.d2[j] = best.d2;
    if (out.evaluated) out.evaluated[j] = best.evaluated;
    if (out.cells) out.cells[j] = best.cells;
    if (out.closest) {
        out.closest[3ull * j] = (float)best.p[0];
        out.closest[3ull * j + 1] = (float)best.p[1];
        out.closest[3ull * j + 2] = (float)best.p[2];
    }
    if (!SIGNED) return;
    int feature = -1;
    double N[3] = {0.0, 0.0, 0.0}, W = 0.0, side = 0.0;
    float x[3][3];
    if (best.face >= 0 && face_vertices(v, V, f, (uint32_t)best.face, x)) {
        double p[3], d2;
        feature = closest_on_face(q, x[0], x[1], x[2], p, d2);             // the winner again: the same operations, the same p
        const uint32_t w0 = (uint32_t)adj[3ull * best.face], w1 = (uint32_t)adj[3ull * best.face + 1],
                       w2 = (uint32_t)adj[3ull * best.face + 2];
        switch (feature) {
            case 0: add_unit_normal(x, 1.0, false, N); W = 1.0; break;
            case 1: vertex_normal(ad, v, V, f, F, w0, N, W); break;
            case 2: vertex_normal(ad, v, V, f, F, w1, N, W); break;
            case 4: vertex_normal(ad, v, V, f, F, w2, N, W); break;
            case 3: edge_normal(ad, v, V, f, adj, F, w0, w1, N, W); break;
            case 5: edge_normal(ad, v, V, f, adj, F, w0, w2, N, W); break;
            default: edge_normal(ad, v, V, f, adj, F, w1, w2, N, W); break;
        }
        const double e[3] = {q[0] - p[0], q[1] - p[1], q[2] - p[2]};
        side = dot3(e, N);
    }
    int sign = side < 0.0 ? -1 : 1;
    if (flip) sign = -sign;
    out.feature[j] = (int8_t)feature;
    out.sign[j] = (int8_t)sign;
    if (out.normal) {
        out.normal[3ull * j] = N[0];
        out.normal[3ull * j + 1] = N[1];
        out.normal[3ull * j + 2] = N[2];
    }
    if (out.weight) out.weight[j] = W;
}

// the value the walk starts from for max_d2: the next float64 above it (+inf stays), so that d2 == max_d2 is taken
inline double start_limit(double max_d2) { return __builtin_nextafter(max_d2, __builtin_inf()); }

inline bool bad_mesh_args(const void* index, const float* verts, uint32_t n_verts, const int32_t* faces, uint32_t n_faces,
                          uint32_t n_queries, double max_d2) {
    return !index || !verts || !faces || n_verts == 0 || n_faces == 0 || n_verts > kMaxCount || n_faces > kMaxCount ||
           n_queries > kMaxCount || !(max_d2 >= 0.0);
}

}  // namespace tri
}  // namespace nsa

extern "C" {

uint64_t nsa_tri_adjacency_workspace(uint32_t n_verts, uint32_t n_faces) {
    using namespace nsa::tri;
    if (n_verts == 0 || n_faces == 0 || n_verts > kMaxCount || n_faces > kMaxCount / 3) return 0;
    return carve_adjacency(nullptr, n_verts, n_faces, nullptr);
}

int nsa_tri_adjacency_build(const float* verts, uint32_t n_verts, const int32_t* faces, const int32_t* adjacency_faces,
                            uint32_t n_faces, void* adjacency, nsa_stream_t stream) {
    using namespace nsa;
    using namespace nsa::tri;
    if (!verts || !faces || !adjacency_faces || !adjacency || n_verts == 0 || n_faces == 0 || n_verts > kMaxCount ||
        n_faces > kMaxCount / 3)
        return NSA_EBADARG;
    Adjacency ad;
    carve_adjacency(adjacency, n_verts, n_faces, &ad);
    launch_begin();
    corners::build(AdjacencyKey{verts, n_verts, faces, adjacency_faces}, n_verts, n_faces, ad, stream);
    return launch_end();
}

int nsa_tri_signed_query_counted(const void* index, const void* adjacency, const float* verts, uint32_t n_verts, const int32_t* faces,
                                 const int32_t* adjacency_faces, uint32_t n_faces, const float* queries, uint32_t n_queries,
                                 double max_d2, int flip, int32_t* face_idx, double* d2, float* closest, int8_t* feature, int8_t* sign,
                                 double* normal, double* weight, uint32_t* evaluated, uint32_t* cells, nsa_stream_t stream) {
    using namespace nsa;
    using namespace nsa::tri;
    if (bad_mesh_args(index, verts, n_verts, faces, n_faces, n_queries, max_d2) || !adjacency || !adjacency_faces ||
        n_faces > kMaxCount / 3)
        return NSA_EBADARG;
    if (n_queries && (!queries || !face_idx || !d2 || !feature || !sign)) return NSA_EBADARG;
    if (n_queries == 0) return NSA_OK;
    Index ix;
    carve(const_cast<void*>(index), n_faces, &ix);
    Adjacency ad;
    carve_adjacency(const_cast<void*>(adjacency), n_verts, n_faces, &ad);
    const SignedOut out{face_idx, d2, closest, feature, sign, normal, weight, evaluated, cells};
    launch_begin();
    hipLaunchKernelGGL(k_tri_signed<true>, dim3((n_queries + 255) / 256), dim3(256), 0, (hipStream_t)stream, ix, ad, verts, n_verts,
                       faces, adjacency_faces, n_faces, queries, n_queries, start_limit(max_d2), flip, out);
    return launch_end();
}

int nsa_tri_signed_query(const void* index, const void* adjacency, const float* verts, uint32_t n_verts, const int32_t* faces,
                         const int32_t* adjacency_faces, uint32_t n_faces, const float* queries, uint32_t n_queries, double max_d2,
                         int flip, int32_t* face_idx, double* d2, float* closest, int8_t* feature, int8_t* sign, nsa_stream_t stream) {
    return nsa_tri_signed_query_counted(index, adjacency, verts, n_verts, faces, adjacency_faces, n_faces, queries, n_queries, max_d2,
                                        flip, face_idx, d2, closest, feature, sign, nullptr, nullptr, nullptr, nullptr, stream);
}

int nsa_tri_query_bounded(const void* index, const float* verts, uint32_t n_verts, const int32_t* faces, uint32_t n_faces,
                          const float* queries, uint32_t n_queries, double max_d2, int32_t* face_idx, double* d2, float* closest,
                          uint32_t* evaluated, uint32_t* cells, nsa_stream_t stream) {
    using namespace nsa;
    using namespace nsa::tri;
    if (bad_mesh_args(index, verts, n_verts, faces, n_faces, n_queries, max_d2)) return NSA_EBADARG;
    if (n_queries && (!queries || !face_idx || !d2)) return NSA_EBADARG;
    if (n_queries == 0) return NSA_OK;
    Index ix;
    carve(const_cast<void*>(index), n_faces, &ix);
    const SignedOut out{face_idx, d2, closest, nullptr, nullptr, nullptr, nullptr, evaluated, cells};
    launch_begin();
    hipLaunchKernelGGL(k_tri_signed<false>, dim3((n_queries + 255) / 256), dim3(256), 0, (hipStream_t)stream, ix, Adjacency{}, verts,
                       n_verts, faces, static_cast<const int32_t*>(nullptr), n_faces, queries, n_queries, start_limit(max_d2), 0, out);
    return launch_end();
}

}  // extern "C"
