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
// Tree.  lo_k = the least coordinate k over the vertices of the usable faces, side = the largest extent over the three axes,
// L = the smallest integer with 8 * 4^L >= F_usable, at most 10.  Face t has centroid_t = ((a + b) + c) / 3 and lies in the leaf cell
// cell_k = min(2^L - 1, (uint32) max((centroid_k - lo_k) * (2^L / side), 0)); its key is the 3 L-bit Morton code of the cell (x the highest
// bit of each triple).  The faces are in the order of the stable radix argsort of their keys: ascending face index within a leaf.  A
// node (l, p) exists for every level l in [0, L] and every distinct prefix p = key >> 3 (L - l); its faces are a contiguous range
// of that order.  Per face n_t = (ab x ac) / 2 (component by component), area_t = sqrt((n_x n_x + n_y n_y) + n_z n_z).  Per node, every
// sum from +0:
//     leaf     N = sum n_t, area = sum area_t, M = sum area_t centroid_t, over its faces in sorted order
//     parent   the same three sums over its children in ascending key order
//     P = M / area ;  r2 = the largest (x_x x_x + x_y x_y) + x_z x_z, x = v - P, over the vertices v of its faces (a maximum: any order)
// The nodes are stored in pre-order, children in ascending key order, each with the index `skip` of the first node behind its
// subtree.  With h(i) the number of levels at which sorted position i begins a node and base = the exclusive prefix sum of h, node
// (l, first face i) has pre-order index base[i] + (l - lmin(i)), lmin(i) = L + 1 - h(i), and skip = base[end of its range]: no second
// sort is needed.  No atomic takes part in the build: the order of every sum is fixed by the sort.
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
#include "tri_common.hpp"

namespace nsa {
namespace wn {

using tri::dot3;
using tri::up256;

constexpr uint32_t kMaxLevel = 10;
constexpr uint32_t kLeafBit = 0x80000000u;
constexpr double kFourPi = 0x1.921fb54442d18p+3;
constexpr uint32_t kTile = 256;              // faces per LDS tile of k_winding_exact: 9 KiB a workgroup

struct Head {                    // written by k_wn_bounds and k_wn_scan
    uint32_t L, n_nodes, n_usable, pad;
    double lo[3], scale;         // scale = 2^L / side
};

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
};

// the level of a mesh of n usable faces, and the most nodes a mesh of F faces can have: at level l at most min(8^l, F)
__host__ __device__ inline uint32_t level_of(uint32_t n) {
    uint32_t L = 0;
    while (L < kMaxLevel && (8ull << (2 * L)) < (uint64_t)n) ++L;
    return L;
}
__host__ __device__ inline uint64_t max_nodes(uint32_t F) {
    uint64_t total = 0;
    for (uint32_t l = 0; l <= level_of(F); ++l) {
        const uint64_t cells = 1ull << (3 * l);
        total += cells < F ? cells : F;
    }
    return total;
}

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

__device__ __forceinline__ void cross3(const double (&u)[3], const double (&w)[3], double (&n)[3]) {
#pragma clang fp contract(off)
    n[0] = u[1] * w[2] - u[2] * w[1];
    n[1] = u[2] * w[0] - u[0] * w[2];
    n[2] = u[0] * w[1] - u[1] * w[0];
}

// ---- build ----------------------------------------------------------------------------------------------------------------------

// one workgroup of 1024: the usable faces' count and the box of their vertices, then L and the cube
__global__ __launch_bounds__(1024) void k_wn_bounds(const float* __restrict__ v, uint32_t V, const int32_t* __restrict__ f, uint32_t F,
                                                    Tree t) {
#pragma clang fp contract(off)
    __shared__ float s_lo[3][1024], s_hi[3][1024];
    __shared__ uint32_t s_n[1024];
    const uint32_t tid = threadIdx.x;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    uint32_t n = 0;
    for (uint32_t i = tid; i < F; i += 1024) {
        float a[3], b[3], c[3];
        if (tri::load_face(v, V, f, i, a, b, c)) continue;
        ++n;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lo[k] = fminf(lo[k], fminf(fminf(a[k], b[k]), c[k]));
            hi[k] = fmaxf(hi[k], fmaxf(fmaxf(a[k], b[k]), c[k]));
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        s_lo[k][tid] = lo[k];
        s_hi[k][tid] = hi[k];
    }
    s_n[tid] = n;
    __syncthreads();
    for (uint32_t w = 512; w > 0; w >>= 1) {
        if (tid < w) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                s_lo[k][tid] = fminf(s_lo[k][tid], s_lo[k][tid + w]);
                s_hi[k][tid] = fmaxf(s_hi[k][tid], s_hi[k][tid + w]);
            }
            s_n[tid] += s_n[tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        Head h{};
        h.n_usable = s_n[0];
        h.L = level_of(h.n_usable);
        h.n_nodes = 0;
        double side = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            h.lo[k] = h.n_usable ? (double)s_lo[k][0] + 0.0 : 0.0;         // + 0.0: -0 becomes +0
            side = fmax(side, h.n_usable ? (double)s_hi[k][0] - (double)s_lo[k][0] : 0.0);
        }
        h.scale = h.n_usable ? (double)(1u << h.L) / side : 0.0;
        *t.head = h;
    }
}

__device__ __forceinline__ uint32_t spread3(uint32_t x) {       // bit i of a 10-bit x to bit 3 i
    x &= 0x3FFu;
    x = (x | (x << 16)) & 0x030000FFu;
    x = (x | (x << 8)) & 0x0300F00Fu;
    x = (x | (x << 4)) & 0x030C30C3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

// the key of face i: the Morton code of its leaf cell, or `unusable` (above every code)
__device__ __forceinline__ uint32_t face_key(const Head& h, const float* __restrict__ v, uint32_t V, const int32_t* __restrict__ f,
                                             uint32_t i, uint32_t unusable) {
#pragma clang fp contract(off)
    float a[3], b[3], c[3];
    if (tri::load_face(v, V, f, i, a, b, c)) return unusable;
    uint32_t cell[3];
    const double top = (double)((1u << h.L) - 1);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double cen = (((double)a[k] + (double)b[k]) + (double)c[k]) / 3.0;
        const double u = (cen - h.lo[k]) * h.scale;
        cell[k] = (uint32_t)fmin(fmax(u, 0.0), top);
    }
    return (spread3(cell[0]) << 2) | (spread3(cell[1]) << 1) | spread3(cell[2]);
}

__global__ __launch_bounds__(256) void k_wn_keys(const float* __restrict__ v, uint32_t V, const int32_t* __restrict__ f, uint32_t F,
                                                 uint32_t unusable, Tree t) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= F) return;
    t.keys[0][i] = face_key(*t.head, v, V, f, i, unusable);
}

// sorted keys, and h(i) -- at how many levels position i begins a node -- into base[i] (base[F] = 0), for the scan
__global__ __launch_bounds__(256) void k_wn_heads(const float* __restrict__ v, uint32_t V, const int32_t* __restrict__ f, uint32_t F,
                                                  uint32_t unusable, Tree t) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i > F) return;
    if (i == F) {
        t.base[F] = 0;
        return;
    }
    const Head h = *t.head;
    const uint32_t key = face_key(h, v, V, f, t.order[i], unusable);
    t.skey[i] = key;
    uint32_t n = 0;
    if (i < h.n_usable) {
        if (i == 0) {
            n = h.L + 1;
        } else {
            const uint32_t x = key ^ face_key(h, v, V, f, t.order[i - 1], unusable);
            if (x) n = (31u - (uint32_t)__clz((int)x)) / 3u + 1u;
        }
    }
    t.base[i] = n;
}

// one workgroup of 1024: base[0 .. F] becomes its exclusive prefix sum; the total is the node count
__global__ __launch_bounds__(1024) void k_wn_scan(uint32_t F, Tree t) {
    __shared__ uint32_t s_sum[1024];
    const uint32_t tid = threadIdx.x;
    const uint64_t n = (uint64_t)F + 1, chunk = (n + 1023) / 1024;
    const uint64_t lo = tid * chunk < n ? tid * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
    uint32_t sum = 0;
    for (uint64_t i = lo; i < hi; ++i) sum += t.base[i];
    s_sum[tid] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) {                // Hillis-Steele, inclusive
        const uint32_t add = tid >= off ? s_sum[tid - off] : 0;
        __syncthreads();
        s_sum[tid] += add;
        __syncthreads();
    }
    uint32_t run = s_sum[tid] - sum;
    for (uint64_t i = lo; i < hi; ++i) {
        const uint32_t x = t.base[i];
        t.base[i] = run;
        run += x;
    }
    if (tid == 1023) t.head->n_nodes = s_sum[1023];
}

// the first position in (i, n) whose key >> sh exceeds p (n when there is none)
__device__ __forceinline__ uint32_t range_end(const uint32_t* __restrict__ skey, uint32_t i, uint32_t n, uint32_t sh, uint32_t p) {
    uint32_t lo = i + 1, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((skey[mid] >> sh) > p) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// one lane per sorted position: the nodes that begin there, their ranges and skip indices
__global__ __launch_bounds__(256) void k_wn_nodes(uint32_t F, Tree t) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const Head h = *t.head;
    if (i >= F || i >= h.n_usable) return;
    const uint32_t first = t.base[i], cnt = t.base[i + 1] - first;
    if (cnt == 0) return;
    const uint32_t lmin = h.L + 1 - cnt, key = t.skey[i];
    for (uint32_t l = lmin; l <= h.L; ++l) {
        const uint32_t n = first + (l - lmin), sh = 3 * (h.L - l);
        const uint32_t e = range_end(t.skey, i, h.n_usable, sh, key >> sh);
        t.end[n] = e;
        t.node[n].begin = i;
        t.node[n].skip = t.base[e] | (l == h.L ? kLeafBit : 0u);
    }
}

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

__global__ void k_wn_info(Tree t, uint32_t* __restrict__ info) {
    info[0] = t.head->L;
    info[1] = t.head->n_nodes;
    info[2] = t.head->n_usable;
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
    const uint32_t Lmax = level_of(n_faces), unusable = 1u << (3 * Lmax), nb = (n_faces + 255) / 256;
    hipStream_t s = (hipStream_t)stream;
    launch_begin();
    hipLaunchKernelGGL(k_wn_bounds, dim3(1), dim3(1024), 0, s, verts, n_verts, faces, n_faces, t);
    hipLaunchKernelGGL(k_wn_keys, dim3(nb), dim3(256), 0, s, verts, n_verts, faces, n_faces, unusable, t);
    radix_argsort(t.keys, t.tmp, t.order, t.counts, n_faces, 0, (3 * Lmax + 1 + 7) / 8, stream);
    hipLaunchKernelGGL(k_wn_heads, dim3(n_faces / 256 + 1), dim3(256), 0, s, verts, n_verts, faces, n_faces, unusable, t);
    hipLaunchKernelGGL(k_wn_scan, dim3(1), dim3(1024), 0, s, n_faces, t);
    hipLaunchKernelGGL(k_wn_nodes, dim3(nb), dim3(256), 0, s, n_faces, t);
    for (uint32_t l = Lmax + 1; l-- > 0;)
        hipLaunchKernelGGL(k_wn_moments, dim3(nb), dim3(256), 0, s, verts, n_verts, faces, n_faces, l, t);
    hipLaunchKernelGGL(k_wn_radius, dim3((uint32_t)((max_nodes(n_faces) + 3) / 4)), dim3(256), 0, s, verts, n_verts, faces, n_faces, t);
    if (info) hipLaunchKernelGGL(k_wn_info, dim3(1), dim3(1), 0, s, t, info);
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
