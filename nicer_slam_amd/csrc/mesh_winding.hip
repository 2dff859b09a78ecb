// mesh_winding.hip -- the generalised winding number of a triangle mesh at query points (DESIGN 4o, C ABI Section 16): the exact sum
// of the faces' solid angles (Jacobson, Kavan & Sorkine-Hornung, "Robust inside-outside segmentation using generalized winding
// numbers", SIGGRAPH 2013) and its hierarchical first-order approximation (Barill, Dickson, Schmidt, Levin & Jacobson, "Fast winding
// numbers for soups and clouds", SIGGRAPH 2018).  An inside / outside field that stays meaningful on a mesh with holes: 1 inside and 0
// outside a closed mesh with outward normals, smooth across an opening, 1/2 on the opening's virtual closure.
//
// Contract (restated by tests/winding_ref.py in numpy float64).  Usable faces are Section 14's (tri::load_face returns 0).  All
// arithmetic is float64 on the fp32 inputs, every operation rounded on its own, dot(u, w) = (u_x w_x + u_y w_y) + u_z w_z and
// u x w = (u_y w_z - u_z w_y, u_z w_x - u_x w_z, u_x w_y - u_y w_x).
//
// Solid angle of face (a, b, c) from q (Van Oosterom & Strackee 1983):
//     A = a - q, B = b - q, C = c - q ;  lA = sqrt(dot(A, A)), lB, lC alike
//     det = dot(A, B x C)
//     den = ((lA lB) lC + dot(A, B) lC) + (dot(A, C) lB + dot(B, C) lA)
//     Omega = 2 atan2(det, den), and Omega = 0 when det == 0 (a query on a vertex or in the face's plane: a defined value)
// A face whose ab x ac points away from q has Omega > 0.
//
// Tree.  The linear octree of octree_build.hpp over the usable faces: L, the cube, the Morton keys of the centroids
// centroid_t = ((a + b) + c) / 3, the stable radix argsort, a node per level and distinct key prefix over a contiguous range of the
// sorted faces, pre-order numbering with `skip`.  That header builds the topology; this unit adds the moments.  Per face
// n_t = (ab x ac) / 2 (component by component), area_t = sqrt((n_x n_x + n_y n_y) + n_z n_z).  Per node, every sum from +0:
//     leaf     N = sum n_t, area = sum area_t, M = sum area_t centroid_t, over its faces in sorted order
//     parent   the same three sums over its children in ascending key order
//     P = M / area ;  r2 = the largest (x_x x_x + x_y x_y) + x_z x_z, x = v - P, over the vertices v of its faces (a maximum: any order)
// No atomic takes part in the build: the order of every sum is fixed by the sort.
//
// Query.  S = +0, i = 0; while i < nodes: d = P_i - q, d2 = dot(d, d);
//     d2 > beta^2 r2_i      S += dot(N_i, d) / (d2 sqrt(d2)), i = skip_i                                       (accepted += 1)
//     else, at a leaf       S += Omega of each of its faces in sorted order, i = skip_i = i + 1                (evaluated += faces)
//     else                  i = i + 1
// w = S / (4 pi), 4 pi = 0x1.921fb54442d18p+3; `flip` negates it.  beta^2 is formed once on the host.  beta = +inf never accepts a
// node -- the exact sum over the usable faces in sorted order -- and runs k_winding_exact, which adds the same terms in the same
// order.  A non-finite query gives NaN (counts 0); no usable face gives +0.
//
// Worst cases, slow and never wrong: every face in one leaf (coincident centroids: one lane sums the leaf in the build and every
// query near it evaluates all of them); a query on the surface descends to the leaves about it.  A query far from the mesh accepts
// the root: one node.  A node whose only child repeats it (a chain down to a lone face) costs the walk one step per level.
#include "octree_build.hpp"

namespace nsa {
namespace wn {

using bulk::cross3;
using bulk::up256;
using octree::Head;
using octree::kLeafBit;
using octree::max_nodes;
using tri::dot3;

constexpr double kFourPi = 0x1.921fb54442d18p+3;
constexpr uint32_t kTile = 256;              // faces per LDS tile of k_winding_exact: 9 KiB a workgroup

struct Node {                    // 64 bytes
    double P[3], N[3], r2;
    uint32_t skip;               // first node behind the subtree; kLeafBit set on a leaf
    uint32_t begin;              // first sorted face
};
static_assert(sizeof(Node) == 64, "Node is read as one 64-byte record");

struct Tree {                    // views into the caller's buffer (nsa_tri_winding_workspace bytes)
    Head* head;
    uint32_t* order;             // [F]: face indices in sorted order, the usable ones first
    uint32_t* skey;              // [F]: sorted keys
    uint32_t* base;              // [F + 1]: exclusive prefix sum of h
    Node* node;                  // [max_nodes(F)]
    uint32_t* end;               // [max_nodes(F)]: one past the node's last sorted face
    double* area;                // [max_nodes(F)]
    double* M;                   // [max_nodes(F)][3]
    uint32_t* keys[2];           // [F] each: radix ping-pong
    uint32_t* tmp;               // [F]
    uint32_t* counts;            // [256 * 256]

    // the hooks of octree_build.hpp: the topology is all this tree takes from the shared kernels
    static __device__ __forceinline__ void sorted_face(const Tree&, const float*, uint32_t, const int32_t*, uint32_t, uint32_t, bool) {}
    static __device__ __forceinline__ void new_node(const Tree&, uint32_t) {}
};

__host__ __device__ inline uint64_t carve(void* ws, uint32_t F, Tree* out) {
    const uint64_t nmax = max_nodes(F);
    char* base = static_cast<char*>(ws);
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) { char* p = base ? base + o : nullptr; o += up256(bytes); return p; };
    Tree t;
    t.head = reinterpret_cast<Head*>(take(sizeof(Head)));
    t.order = reinterpret_cast<uint32_t*>(take(4ull * F));
    t.skey = reinterpret_cast<uint32_t*>(take(4ull * F));
    t.base = reinterpret_cast<uint32_t*>(take(4ull * ((uint64_t)F + 1)));
    t.node = reinterpret_cast<Node*>(take(sizeof(Node) * nmax));
    t.end = reinterpret_cast<uint32_t*>(take(4ull * nmax));
    t.area = reinterpret_cast<double*>(take(8ull * nmax));
    t.M = reinterpret_cast<double*>(take(24ull * nmax));
    t.keys[0] = reinterpret_cast<uint32_t*>(take(4ull * F));
    t.keys[1] = reinterpret_cast<uint32_t*>(take(4ull * F));
    t.tmp = reinterpret_cast<uint32_t*>(take(4ull * F));
    t.counts = reinterpret_cast<uint32_t*>(take(4ull * kRadixCountWords));
    if (out) *out = t;
    return o;
}

// ---- build: the topology is octree_build.hpp's; the moments and radii of its nodes ------------------------------------------------

__device__ __forceinline__ bool load_sorted(const Tree& t, const float* __restrict__ v, uint32_t V, const int32_t* __restrict__ f,
                                            uint32_t F, uint32_t pos, float (&a)[3], float (&b)[3], float (&c)[3]) {
    const uint32_t g = t.order[pos];
    if (g >= F) return false;                                              // (not the mesh the tree was built on)
    const int32_t i0 = f[3ull * g], i1 = f[3ull * g + 1], i2 = f[3ull * g + 2];
    if ((uint32_t)i0 >= V || (uint32_t)i1 >= V || (uint32_t)i2 >= V) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a[k] = v[3ull * i0 + k];
        b[k] = v[3ull * i1 + k];
        c[k] = v[3ull * i2 + k];
    }
    return true;
}

// one lane per sorted position, one launch per level from the leaves up: N, area, M and P of the level's node that begins there
__global__ __launch_bounds__(256) void k_wn_moments(const float* __restrict__ v, uint32_t V, const int32_t* __restrict__ f, uint32_t F,
                                                    uint32_t l, Tree t) {
#pragma clang fp contract(off)
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const Head h = *t.head;
    if (i >= F || i >= h.n_usable || l > h.L) return;
    const uint32_t first = t.base[i], cnt = t.base[i + 1] - first;
    if (cnt == 0 || l < h.L + 1 - cnt) return;
    const uint32_t n = first + (l - (h.L + 1 - cnt)), e = t.end[n];
    double N[3] = {0.0, 0.0, 0.0}, M[3] = {0.0, 0.0, 0.0}, area = 0.0;
    if (l == h.L) {
        for (uint32_t pos = i; pos < e; ++pos) {
            float a[3], b[3], c[3];
            if (!load_sorted(t, v, V, f, F, pos, a, b, c)) continue;
            double ab[3], ac[3], nt[3], cen[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                ab[k] = (double)b[k] - (double)a[k];
                ac[k] = (double)c[k] - (double)a[k];
                cen[k] = (((double)a[k] + (double)b[k]) + (double)c[k]) / 3.0;
            }
            cross3(ab, ac, nt);
#pragma unroll
            for (int k = 0; k < 3; ++k) nt[k] = nt[k] * 0.5;
            const double at = sqrt((nt[0] * nt[0] + nt[1] * nt[1]) + nt[2] * nt[2]);
            area = area + at;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                N[k] = N[k] + nt[k];
                M[k] = M[k] + at * cen[k];
            }
        }
    } else {
        for (uint32_t j = i; j < e;) {                                     // the children: the level l + 1 nodes of the range
            const uint32_t cf = t.base[j], cc = t.base[j + 1] - cf;
            if (cc == 0 || cc > h.L + 1 || l + 1 < h.L + 1 - cc) break;    // (a damaged buffer: j begins no node of level l + 1)
            const uint32_t c = cf + ((l + 1) - (h.L + 1 - cc));
            area = area + t.area[c];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                N[k] = N[k] + t.node[c].N[k];
                M[k] = M[k] + t.M[3ull * c + k];
            }
            const uint32_t next = t.end[c];
            if (next <= j) break;                                          // (a damaged buffer: never loop)
            j = next;
        }
    }
    t.area[n] = area;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        t.M[3ull * n + k] = M[k];
        t.node[n].N[k] = N[k];
        t.node[n].P[k] = M[k] / area;
    }
}

// one wave per node: r2 over the vertices of the node's faces
__global__ __launch_bounds__(256) void k_wn_radius(const float* __restrict__ v, uint32_t V, const int32_t* __restrict__ f, uint32_t F,
                                                   Tree t) {
#pragma clang fp contract(off)
    const uint32_t n = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x & 63;
    if (n >= t.head->n_nodes) return;
    const double P[3] = {t.node[n].P[0], t.node[n].P[1], t.node[n].P[2]};
    const uint32_t s = t.node[n].begin, e = t.end[n];
    double r2 = 0.0;
    for (uint32_t pos = s + lane; pos < e; pos += 64) {
        float x[3][3];
        if (!load_sorted(t, v, V, f, F, pos, x[0], x[1], x[2])) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double d[3] = {(double)x[c][0] - P[0], (double)x[c][1] - P[1], (double)x[c][2] - P[2]};
            const double d2 = dot3(d, d);
            r2 = d2 > r2 ? d2 : r2;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(r2, off);
        r2 = o > r2 ? o : r2;
    }
    if (lane == 0) t.node[n].r2 = r2;
}

// ---- query ----------------------------------------------------------------------------------------------------------------------

// Omega of face (a, b, c) from q
__device__ __forceinline__ double solid_angle(const double (&q)[3], const float (&a)[3], const float (&b)[3], const float (&c)[3]) {
#pragma clang fp contract(off)
    double A[3], B[3], C[3], BC[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        A[k] = (double)a[k] - q[k];
        B[k] = (double)b[k] - q[k];
        C[k] = (double)c[k] - q[k];
    }
    const double lA = sqrt(dot3(A, A)), lB = sqrt(dot3(B, B)), lC = sqrt(dot3(C, C));
    cross3(B, C, BC);
    const double det = dot3(A, BC);
    const double den = ((lA * lB) * lC + dot3(A, B) * lC) + (dot3(A, C) * lB + dot3(B, C) * lA);
    return det == 0.0 ? 0.0 : 2.0 * atan2(det, den);
}

// one lane per query: the pre-order walk
__global__ __launch_bounds__(256) void k_winding_tree(Tree t, const float* __restrict__ v, uint32_t V, const int32_t* __restrict__ f,
                                                      uint32_t F, const float* __restrict__ qs, uint32_t m, double beta2, int flip,
                                                      double* __restrict__ w, uint32_t* __restrict__ accepted,
                                                      uint32_t* __restrict__ evaluated) {
#pragma clang fp contract(off)
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const float qf[3] = {qs[3ull * j], qs[3ull * j + 1], qs[3ull * j + 2]};
    const double q[3] = {qf[0], qf[1], qf[2]};
    double S = 0.0;
    uint32_t n_acc = 0, n_eval = 0;
    if (tri::finite3(qf)) {
        const uint32_t n_nodes = t.head->n_nodes;
        for (uint32_t i = 0; i < n_nodes;) {
            const Node nd = t.node[i];
            const double d[3] = {nd.P[0] - q[0], nd.P[1] - q[1], nd.P[2] - q[2]};
            const double d2 = dot3(d, d);
            uint32_t next = i + 1;
            if (d2 > beta2 * nd.r2) {
                S = S + dot3(nd.N, d) / (d2 * sqrt(d2));
                ++n_acc;
                next = nd.skip & ~kLeafBit;
            } else if (nd.skip & kLeafBit) {
                const uint32_t e = t.end[i];
                for (uint32_t pos = nd.begin; pos < e; ++pos) {
                    float a[3], b[3], c[3];
                    if (!load_sorted(t, v, V, f, F, pos, a, b, c)) continue;
                    S = S + solid_angle(q, a, b, c);
                    ++n_eval;
                }
            }
            if (next <= i) break;                                          // (a damaged buffer: never loop)
            i = next;
        }
        S = S / kFourPi;
        if (flip) S = -S;
    } else {
        S = __builtin_nan("");
    }
    w[j] = S;
    if (accepted) accepted[j] = n_acc;
    if (evaluated) evaluated[j] = n_eval;
}

// one lane per query, every usable face in sorted order: tiles of kTile faces through LDS, every lane reading the same face
__global__ __launch_bounds__(256) void k_winding_exact(Tree t, const float* __restrict__ v, uint32_t V, const int32_t* __restrict__ f,
                                                       uint32_t F, const float* __restrict__ qs, uint32_t m, int flip,
                                                       double* __restrict__ w, uint32_t* __restrict__ accepted,
                                                       uint32_t* __restrict__ evaluated) {
#pragma clang fp contract(off)
    __shared__ float tile[kTile][9];
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    const bool live = j < m;
    float qf[3] = {0.0f, 0.0f, 0.0f};
    if (live) {
        qf[0] = qs[3ull * j];
        qf[1] = qs[3ull * j + 1];
        qf[2] = qs[3ull * j + 2];
    }
    const double q[3] = {qf[0], qf[1], qf[2]};
    const bool finite = tri::finite3(qf);
    const uint32_t n_usable = min(t.head->n_usable, F);
    double S = 0.0;
    uint32_t n_eval = 0;
    for (uint32_t base = 0; base < n_usable; base += kTile) {
        const uint32_t count = min(kTile, n_usable - base);
        if (threadIdx.x < count) {
            float a[3] = {0.0f, 0.0f, 0.0f}, b[3] = {0.0f, 0.0f, 0.0f}, c[3] = {0.0f, 0.0f, 0.0f};
            const bool ok = load_sorted(t, v, V, f, F, base + threadIdx.x, a, b, c);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                tile[threadIdx.x][k] = ok ? a[k] : __builtin_nanf("");    // a usable face has finite vertices: NaN marks "none"
                tile[threadIdx.x][3 + k] = b[k];
                tile[threadIdx.x][6 + k] = c[k];
            }
        }
        __syncthreads();
        if (live && finite) {
            for (uint32_t s = 0; s < count; ++s) {
                const float a[3] = {tile[s][0], tile[s][1], tile[s][2]};
                const float b[3] = {tile[s][3], tile[s][4], tile[s][5]};
                const float c[3] = {tile[s][6], tile[s][7], tile[s][8]};
                if (a[0] != a[0]) continue;
                S = S + solid_angle(q, a, b, c);
                ++n_eval;
            }
        }
        __syncthreads();
    }
    if (!live) return;
    if (finite) {
        S = S / kFourPi;
        if (flip) S = -S;
    } else {
        S = __builtin_nan("");
        n_eval = 0;
    }
    w[j] = S;
    if (accepted) accepted[j] = 0;
    if (evaluated) evaluated[j] = n_eval;
}

}  // namespace wn
}  // namespace nsa

extern "C" {

uint64_t nsa_tri_winding_workspace(uint32_t n_faces) {
    using namespace nsa;
    if (n_faces == 0 || n_faces > tri::kMaxCount) return 0;
    return wn::carve(nullptr, n_faces, nullptr);
}

int nsa_tri_winding_build(const float* verts, uint32_t n_verts, const int32_t* faces, uint32_t n_faces, void* tree, uint32_t* info,
                          nsa_stream_t stream) {
    using namespace nsa;
    using namespace nsa::wn;
    if (n_verts > tri::kMaxCount || n_faces > tri::kMaxCount) return NSA_EBADARG;
    if (n_faces == 0) return NSA_OK;
    if (!verts || !faces || !tree || n_verts == 0) return NSA_EBADARG;
    Tree t;
    carve(tree, n_faces, &t);
    const uint32_t Lmax = octree::level_of(n_faces), nb = (n_faces + 255) / 256;
    hipStream_t s = (hipStream_t)stream;
    launch_begin();
    octree::build(verts, n_verts, faces, n_faces, t, s);
    for (uint32_t l = Lmax + 1; l-- > 0;)
        hipLaunchKernelGGL(k_wn_moments, dim3(nb), dim3(256), 0, s, verts, n_verts, faces, n_faces, l, t);
    hipLaunchKernelGGL(k_wn_radius, dim3((uint32_t)((max_nodes(n_faces) + 3) / 4)), dim3(256), 0, s, verts, n_verts, faces, n_faces, t);
    if (info) hipLaunchKernelGGL(octree::k_info<Tree>, dim3(1), dim3(1), 0, s, t, info);
    return launch_end();
}

int nsa_tri_winding_query(const void* tree, const float* verts, uint32_t n_verts, const int32_t* faces, uint32_t n_faces,
                          const float* queries, uint32_t n_queries, double beta, int flip, double* w, uint32_t* accepted,
                          uint32_t* evaluated, nsa_stream_t stream) {
    using namespace nsa;
    using namespace nsa::wn;
    if (!(beta >= 1.0) || n_verts > tri::kMaxCount || n_faces > tri::kMaxCount || n_queries > tri::kMaxCount) return NSA_EBADARG;
    if (n_queries == 0 || n_faces == 0) return NSA_OK;
    if (!tree || !verts || !faces || !queries || !w || n_verts == 0) return NSA_EBADARG;
    Tree t;
    carve(const_cast<void*>(tree), n_faces, &t);
    const dim3 grid((n_queries + 255) / 256);
    launch_begin();
    if (beta == INFINITY)
        hipLaunchKernelGGL(k_winding_exact, grid, dim3(256), 0, (hipStream_t)stream, t, verts, n_verts, faces, n_faces, queries,
                           n_queries, flip, w, accepted, evaluated);
    else
        hipLaunchKernelGGL(k_winding_tree, grid, dim3(256), 0, (hipStream_t)stream, t, verts, n_verts, faces, n_faces, queries,
                           n_queries, beta * beta, flip, w, accepted, evaluated);
    return launch_end();
}

}  // extern "C"
