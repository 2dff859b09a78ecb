// octree_build.hpp -- the topology of the linear octree over a mesh's faces (C ABI Section 16), built once for the two
// units that walk one: the winding number's (mesh_winding.hip) and the ray cast's (mesh_raycast.hip).
//
// lo_k = the least coordinate k over the vertices of the usable faces (tri::load_face returns 0), side = the largest extent over the
// three axes, L = the smallest integer with 8 * 4^L >= F_usable, at most kMaxLevel.  Face t has centroid_t = ((a + b) + c) / 3 in float64
// and lies in the leaf cell cell_k = min(2^L - 1, (uint32) max((centroid_k - lo_k) * (2^L / side), 0)); its key is the 3 L-bit Morton
// code of the cell (x the highest bit of each triple), an unusable face's lies above every code.  The faces are in the order of the
// stable radix argsort of their keys: ascending face index within a leaf, the unusable ones last.  A node (l, p) exists for every
// level l in [0, L] and every distinct prefix p = key >> 3 (L - l); its faces are a contiguous range of that order.  The nodes are
// stored in pre-order, children in ascending key order, each with the index `skip` of the first node behind its subtree.  With h(i)
// the number of levels at which sorted position i begins a node and base = the exclusive prefix sum of h, node (l, first face i) has
// pre-order index base[i] + (l - lmin(i)), lmin(i) = L + 1 - h(i), and skip = base[end of its range]: no second sort is needed, and
// no atomic takes part.
//
// A unit brings its own tree type: views `head`, `order`, `skey`, `base`, `node` (records with `skip` and `begin`, written in place),
// `end`, `keys[2]`, `tmp`, `counts` into its buffer, carved in its own order, and two hooks that ride on the kernels here:
//     static __device__ void sorted_face(const Tree&, v, V, f, i, g, live)    k_heads, every sorted position i < F: g = order[i]; live when
//                                                                            i is a usable position and g a face of the mesh
//     static __device__ void new_node(const Tree&, n)                         k_nodes, every node n as its range and skip are written
// The guards against a buffer the build did not write (g < F, a count above L + 1) never fire on one it did.
//
// level_of, max_nodes and the Morton code also compile as host C++ (tests/index_host_check.cpp).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include "block_scan.hpp"
#include "tri_common.hpp"
#define NSA_OCTREE_FN __host__ __device__ inline
#else
#define NSA_OCTREE_FN static inline
#endif

namespace nsa {
namespace octree {

constexpr uint32_t kMaxLevel = 10;
constexpr uint32_t kLeafBit = 0x80000000u;

struct Head {                    // written by k_bounds and k_scan
    uint32_t L, n_nodes, n_usable, pad;
    double lo[3], scale;         // scale = 2^L / side
};

// the level of a mesh of n usable faces, and the most nodes a mesh of F faces can have: at level l at most min(8^l, F)
NSA_OCTREE_FN uint32_t level_of(uint32_t n) {
    uint32_t L = 0;
    while (L < kMaxLevel && (8ull << (2 * L)) < (uint64_t)n) ++L;
    return L;
}
NSA_OCTREE_FN uint64_t max_nodes(uint32_t F) {
    uint64_t total = 0;
    for (uint32_t l = 0; l <= level_of(F); ++l) {
        const uint64_t cells = 1ull << (3 * l);
        total += cells < F ? cells : F;
    }
    return total;
}

NSA_OCTREE_FN uint32_t spread3(uint32_t x) {                      // bit i of a 10-bit x to bit 3 i
    x &= 0x3FFu;
    x = (x | (x << 16)) & 0x030000FFu;
    x = (x | (x << 8)) & 0x0300F00Fu;
    x = (x | (x << 4)) & 0x030C30C3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}
NSA_OCTREE_FN uint32_t morton3(const uint32_t (&cell)[3]) { return (spread3(cell[0]) << 2) | (spread3(cell[1]) << 1) | spread3(cell[2]); }

#if defined(__HIPCC__)

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
    return morton3(cell);
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

// one workgroup of 1024: the usable faces' count and the box of their vertices, then L and the cube
template <typename Tree>
__global__ __launch_bounds__(1024) void k_bounds(const float* __restrict__ v, uint32_t V, const int32_t* __restrict__ f, uint32_t F,
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

template <typename Tree>
__global__ __launch_bounds__(256) void k_keys(const float* __restrict__ v, uint32_t V, const int32_t* __restrict__ f, uint32_t F,
                                              uint32_t unusable, Tree t) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= F) return;
    t.keys[0][i] = face_key(*t.head, v, V, f, i, unusable);
}

// sorted keys, the unit's share of each sorted face, and h(i) -- at how many levels position i begins a node -- into base[i]
// (base[F] = 0), for the scan
template <typename Tree>
__global__ __launch_bounds__(256) void k_heads(const float* __restrict__ v, uint32_t V, const int32_t* __restrict__ f, uint32_t F,
                                               uint32_t unusable, Tree t) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i > F) return;
    if (i == F) {
        t.base[F] = 0;
        return;
    }
    const Head h = *t.head;
    const uint32_t g = t.order[i];
    const uint32_t key = g < F ? face_key(h, v, V, f, g, unusable) : unusable;
    t.skey[i] = key;
    const bool live = i < h.n_usable && g < F;
    Tree::sorted_face(t, v, V, f, i, g, live);
    uint32_t n = 0;
    if (live) {
        if (i == 0) {
            n = h.L + 1;
        } else {
            const uint32_t gp = t.order[i - 1];
            const uint32_t x = key ^ (gp < F ? face_key(h, v, V, f, gp, unusable) : unusable);
            if (x) n = (31u - (uint32_t)__clz((int)x)) / 3u + 1u;
        }
    }
    t.base[i] = n;
}

// one workgroup of 1024: base[0 .. F] becomes its exclusive prefix sum (block_scan.hpp); the total is the node count
template <typename Tree>
__global__ __launch_bounds__(1024) void k_scan(uint32_t F, Tree t) {
    uint32_t total[1];
    scan::offsets<1, uint32_t, 1024>(t.base, t.base, (uint64_t)F + 1, total);
    if (threadIdx.x == 1023) t.head->n_nodes = total[0];
}

// one lane per sorted position: the nodes that begin there, their ranges and skip indices
template <typename Tree>
__global__ __launch_bounds__(256) void k_nodes(uint32_t F, Tree t) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const Head h = *t.head;
    if (i >= F || i >= h.n_usable) return;
    const uint32_t first = t.base[i], cnt = t.base[i + 1] - first;
    if (cnt == 0 || cnt > h.L + 1) return;
    const uint32_t lmin = h.L + 1 - cnt, key = t.skey[i];
    for (uint32_t l = lmin; l <= h.L; ++l) {
        const uint32_t n = first + (l - lmin), sh = 3 * (h.L - l);
        const uint32_t e = range_end(t.skey, i, h.n_usable, sh, key >> sh);
        t.end[n] = e;
        t.node[n].begin = i;
        t.node[n].skip = t.base[e] | (l == h.L ? kLeafBit : 0u);
        Tree::new_node(t, n);
    }
}

template <typename Tree>
__global__ void k_info(Tree t, uint32_t* __restrict__ info) {
    info[0] = t.head->L;
    info[1] = t.head->n_nodes;
    info[2] = t.head->n_usable;
}

// the six steps of the topology on stream s, between the caller's launch_begin() and launch_end(); the unit's own kernels follow
template <typename Tree>
inline void build(const float* verts, uint32_t n_verts, const int32_t* faces, uint32_t n_faces, const Tree& t, hipStream_t s) {
    const uint32_t Lmax = level_of(n_faces), unusable = 1u << (3 * Lmax), nb = (n_faces + 255) / 256;
    hipLaunchKernelGGL(k_bounds<Tree>, dim3(1), dim3(1024), 0, s, verts, n_verts, faces, n_faces, t);
    hipLaunchKernelGGL(k_keys<Tree>, dim3(nb), dim3(256), 0, s, verts, n_verts, faces, n_faces, unusable, t);
    radix_argsort(t.keys, t.tmp, t.order, t.counts, n_faces, 0, (3 * Lmax + 1 + 7) / 8, (nsa_stream_t)s);
    hipLaunchKernelGGL(k_heads<Tree>, dim3(n_faces / 256 + 1), dim3(256), 0, s, verts, n_verts, faces, n_faces, unusable, t);
    hipLaunchKernelGGL(k_scan<Tree>, dim3(1), dim3(1024), 0, s, n_faces, t);
    hipLaunchKernelGGL(k_nodes<Tree>, dim3(nb), dim3(256), 0, s, n_faces, t);
}

#endif  // __HIPCC__

}  // namespace octree
}  // namespace nsa
