// mesh_clean.hip -- connected components of a triangle mesh and their per-component statistics on the device (DESIGN 4j;
// C ABI Section 11).  Reference: the two manual steps of code/evaluation/eval_rec.py:269-272 (Meshlab's "select connected
// components in a region", delete) and the commented trimesh code of code/utils/viz.py:136-141 (keep the largest component).
//
// Labelling: a lock-free union-find over the vertex indices in three straight passes (uf_passes.hpp, which also compiles as
// host C++): parent[v] = v; one lane per face joins (a, b) and (b, c), hooking the larger root under the smaller with a
// compare-and-swap on the root's own slot; one lane per vertex writes find(v).  parent[x] <= x always, so every walk descends
// and the final root is the smallest index of the component whatever the interleaving: the atomics reach the fixed point, they
// decide nothing in the output.  Every loop has a step cap that reports through totals[2] instead of spinning.
//
// Statistics: the roots, in index order, are the components (rank = exclusive count of the roots below: flag_scan inside each
// block and k_offsets over the block counts, both block_scan.hpp's).  Counts and bounding boxes are integer atomics (add; min / max on an
// order-preserving integer image of the fp32 value), which give the same result in any order.  Areas are summed in a fixed
// order: the faces are argsorted stably by rank (radix_sort.hpp), each aligned block of 1024 sorted positions is cut at the
// component boundaries and every piece summed left to right, and a component adds its pieces in block order.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/nicer_slam_amd.h"
#include "block_scan.hpp"
#include "grid_common.hpp"
#include "mesh_area.hpp"
#include "radix_sort.hpp"
#include "uf_passes.hpp"

namespace nsa {

constexpr uint32_t kCcMaxCount = 0x7FFFFFFFu;
constexpr uint32_t kCcBlock = 1024;          // block of the rank scan and of the area pieces

using scan::ull;

__host__ __device__ inline uint64_t cc_align(uint64_t b) { return (b + 255) & ~uint64_t(255); }

// ---- labelling ----------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_cc_init(int32_t* __restrict__ parent, int32_t* __restrict__ vlabel, uint32_t V,
                                                 ull* __restrict__ totals) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v < 3) totals[v] = 0;
    if (v < V) uf_pass_init(parent, vlabel, v);
}

__global__ __launch_bounds__(256) void k_cc_faces(int32_t* parent, int32_t* vlabel, const int32_t* __restrict__ faces, uint32_t F,
                                                  uint32_t V, ull* totals) {
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    uint32_t status = 0;
    uf_pass_face(parent, vlabel, faces, f, V, &status);
    if (status) atomicOr(totals + 2, (ull)status);
}

__global__ __launch_bounds__(256) void k_cc_label(int32_t* parent, int32_t* vlabel, uint32_t V, ull* totals) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    uint32_t status = 0;
    int32_t l = -1;
    if (v < V) l = uf_pass_label(parent, vlabel, v, V, &status);
    if (status) atomicOr(totals + 2, (ull)status);
    // the two counts: integer sums, the same in any order
    const ull roots = __ballot(v < V && l == (int32_t)v), used = __ballot(l >= 0);
    if ((threadIdx.x & 63) == 0) {
        if (roots) atomicAdd(totals + 0, (ull)__popcll(roots));
        if (used) atomicAdd(totals + 1, (ull)__popcll(used));
    }
}

__global__ __launch_bounds__(256) void k_cc_face_label(const int32_t* __restrict__ vlabel, const int32_t* __restrict__ faces,
                                                       uint32_t F, uint32_t V, int32_t* __restrict__ flabel) {
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int32_t a = faces[3ull * f], b = faces[3ull * f + 1], c = faces[3ull * f + 2];
    flabel[f] = uf_valid_face(a, b, c, V) ? vlabel[a] : -1;
}

// ---- statistics ---------------------------------------------------------------------------------------------------------------

struct StatWork {                // views into the caller's workspace (nsa_mesh_component_stats_workspace bytes)
    int32_t* rank;               // [V]: rank of the component whose label is v (written at the roots only)
    uint32_t* bcount;            // [nbv]: roots per block of 1024 vertices, then their exclusive scan
    uint32_t* keys[2];           // [F] each: radix ping-pong (key = rank, C for an invalid face)
    uint32_t* tmp;               // [F]
    uint32_t* order;             // [F]: faces sorted stably by key
    uint32_t* skey;              // [F]: the sorted keys
    uint32_t* counts;            // [256 * 256]
    double* cont;                // [nbf]: the piece at the head of block b when it continues the previous block's component
    uint32_t* box;               // [C][6]: integer images of lo xyz, hi xyz
};

__host__ __device__ inline uint64_t stat_carve(void* ws, uint32_t V, uint32_t F, uint32_t C, StatWork* out) {
    const uint64_t nbv = ((uint64_t)V + kCcBlock - 1) / kCcBlock, nbf = ((uint64_t)F + kCcBlock - 1) / kCcBlock;
    char* base = static_cast<char*>(ws);
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) { char* p = base ? base + o : nullptr; o += cc_align(bytes ? bytes : 1); return p; };
    StatWork w;
    w.rank = reinterpret_cast<int32_t*>(take(4ull * V));
    w.bcount = reinterpret_cast<uint32_t*>(take(4ull * nbv));
    w.keys[0] = reinterpret_cast<uint32_t*>(take(4ull * F));
    w.keys[1] = reinterpret_cast<uint32_t*>(take(4ull * F));
    w.tmp = reinterpret_cast<uint32_t*>(take(4ull * F));
    w.order = reinterpret_cast<uint32_t*>(take(4ull * F));
    w.skey = reinterpret_cast<uint32_t*>(take(4ull * F));
    w.counts = reinterpret_cast<uint32_t*>(take(4ull * kRadixCountWords));
    w.cont = reinterpret_cast<double*>(take(8ull * nbf));
    w.box = reinterpret_cast<uint32_t*>(take(24ull * C));
    if (out) *out = w;
    return o;
}

// order-preserving integer image of an fp32 value (-0 below +0), and back
__device__ __forceinline__ uint32_t f2ord(float x) {
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t e) { return __uint_as_float((e & 0x80000000u) ? (e ^ 0x80000000u) : ~e); }

__device__ __forceinline__ bool is_root(const int32_t* __restrict__ vlabel, uint32_t v, uint32_t V) {
    return v < V && vlabel[v] == (int32_t)v;
}

__global__ __launch_bounds__(kCcBlock) void k_st_count(const int32_t* __restrict__ vlabel, uint32_t V, StatWork w) {
    uint32_t total;
    scan::flag_scan<kCcBlock>(is_root(vlabel, blockIdx.x * kCcBlock + threadIdx.x, V), total);
    if (threadIdx.x == 0) w.bcount[blockIdx.x] = total;
}

// rank of every root; label[], and the identities of the per-component accumulators
__global__ __launch_bounds__(kCcBlock) void k_st_rank(const int32_t* __restrict__ vlabel, uint32_t V, uint32_t C, StatWork w,
                                                      int32_t* __restrict__ label, int32_t* __restrict__ n_verts) {
    const uint32_t v = blockIdx.x * kCcBlock + threadIdx.x;
    const bool root = is_root(vlabel, v, V);
    uint32_t total;
    const uint32_t r = w.bcount[blockIdx.x] + scan::flag_scan<kCcBlock>(root, total);
    if (!root || r >= C) return;         // (r >= C: a caller that passed another count than the labelling gave)
    w.rank[v] = (int32_t)r;
    label[r] = (int32_t)v;
    n_verts[r] = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        w.box[6ull * r + k] = f2ord(INFINITY);
        w.box[6ull * r + 3 + k] = f2ord(-INFINITY);
    }
}

__device__ __forceinline__ int32_t rank_of(const StatWork& w, int32_t l, uint32_t V, uint32_t C) {
    if (l < 0 || (uint32_t)l >= V) return -1;
    const int32_t r = w.rank[l];
    return (r < 0 || (uint32_t)r >= C) ? -1 : r;
}

// one lane per vertex: its rank, and its share of the component's vertex count and box.  A wave whose vertices all belong to
// one component (the rule for a marching-cubes mesh) reduces first and issues one set of atomics.
__global__ __launch_bounds__(256) void k_st_verts(const float* __restrict__ verts, const int32_t* __restrict__ vlabel, uint32_t V,
                                                  uint32_t C, StatWork w, int32_t* __restrict__ vertex_comp,
                                                  int32_t* __restrict__ n_verts) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    const bool active = v < V;
    int32_t c = -1;
    uint32_t e[6] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u};      // identities of min / max
    if (active) {
        c = rank_of(w, vlabel[v], V, C);
        vertex_comp[v] = c;
        if (c >= 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float x = verts[3ull * v + k];
                if (__builtin_isfinite(x)) e[k] = e[3 + k] = f2ord(x);
            }
        }
    }
    const int32_t c0 = __shfl(c, 0, 64);
    if (__all(!active || c == c0)) {
        if (c0 < 0) return;
        const uint32_t n = (uint32_t)__popcll(__ballot(active));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                e[k] = min(e[k], (uint32_t)__shfl_xor((int)e[k], o, 64));
                e[3 + k] = max(e[3 + k], (uint32_t)__shfl_xor((int)e[3 + k], o, 64));
            }
        }
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(n_verts + c0, (int32_t)n);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                atomicMin(w.box + 6ull * c0 + k, e[k]);
                atomicMax(w.box + 6ull * c0 + 3 + k, e[3 + k]);
            }
        }
        return;
    }
    if (c < 0) return;
    atomicAdd(n_verts + c, 1);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        atomicMin(w.box + 6ull * c + k, e[k]);
        atomicMax(w.box + 6ull * c + 3 + k, e[3 + k]);
    }
}

__global__ __launch_bounds__(256) void k_st_face_keys(const int32_t* __restrict__ flabel, uint32_t F, uint32_t V, uint32_t C,
                                                      StatWork w, int32_t* __restrict__ face_comp) {
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int32_t c = rank_of(w, flabel[f], V, C);
    face_comp[f] = c;
    w.keys[0][f] = c < 0 ? C : (uint32_t)c;
}

__device__ __forceinline__ uint32_t key_of(int32_t c, uint32_t C) { return c < 0 ? C : (uint32_t)c; }

// one block per 1024 sorted positions: the pieces between component boundaries, each summed left to right by the lane at its head
__global__ __launch_bounds__(kCcBlock) void k_st_area_pieces(const float* __restrict__ verts, uint32_t V,
                                                             const int32_t* __restrict__ faces, uint32_t F, uint32_t C, StatWork w,
                                                             const int32_t* __restrict__ face_comp, double* __restrict__ area) {
    __shared__ double s[kCcBlock];
    __shared__ uint32_t key[kCcBlock];
    const uint32_t t = threadIdx.x, i = blockIdx.x * kCcBlock + t;
    uint32_t k = 0xFFFFFFFFu;                             // past the end: a key no face has
    double a = 0.0;
    if (i < F) {
        const uint32_t f = w.order[i];
        k = key_of(face_comp[f], C);
        w.skey[i] = k;
        if (k < C) {
            const int32_t i0 = faces[3ull * f], i1 = faces[3ull * f + 1], i2 = faces[3ull * f + 2];
            bool fin = uf_valid_face(i0, i1, i2, V);      // (true for the labelling's own face_label; keeps any other in bounds)
#pragma unroll
            for (int j = 0; j < 3; ++j)
                fin = fin && __builtin_isfinite(verts[3ull * (uint32_t)i0 + j]) && __builtin_isfinite(verts[3ull * (uint32_t)i1 + j]) &&
                      __builtin_isfinite(verts[3ull * (uint32_t)i2 + j]);
            a = fin ? face_area(verts, V, faces, f) : 0.0;
        }
    }
    s[t] = a;
    key[t] = k;
    __syncthreads();
    if (k >= C || (t > 0 && key[t - 1] == k)) return;    // not the head of a piece of a component
    double c = 0.0;
    for (uint32_t j = t; j < kCcBlock && key[j] == k; ++j) c = c + s[j];
    const bool continues = t == 0 && i > 0 && key_of(face_comp[w.order[i - 1]], C) == k;
    if (continues) w.cont[blockIdx.x] = c;
    else area[k] = c;                                     // the component's first piece: one writer
}

__device__ __forceinline__ uint32_t cc_lower_bound(const uint32_t* __restrict__ a, uint32_t n, uint32_t v) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// one lane per component: its face count (its run of the sorted keys), its area (the first piece, then the heads of the later
// blocks of its run, in block order) and its box
__global__ __launch_bounds__(256) void k_st_finish(uint32_t F, uint32_t C, StatWork w, int32_t* __restrict__ n_faces,
                                                   double* __restrict__ area, float* __restrict__ lo, float* __restrict__ hi) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const uint32_t s = cc_lower_bound(w.skey, F, c), e = cc_lower_bound(w.skey, F, c + 1);
    n_faces[c] = (int32_t)(e - s);
    double acc = e > s ? area[c] : 0.0;
    for (uint64_t p = ((uint64_t)s / kCcBlock + 1) * kCcBlock; p < e; p += kCcBlock) acc = acc + w.cont[p / kCcBlock];
    area[c] = acc;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lo[3ull * c + k] = ord2f(w.box[6ull * c + k]);
        hi[3ull * c + k] = ord2f(w.box[6ull * c + 3 + k]);
    }
}

}  // namespace nsa

extern "C" {

uint64_t nsa_mesh_components_workspace(uint32_t n_verts) {
    if (n_verts == 0 || n_verts > nsa::kCcMaxCount) return 0;
    return nsa::cc_align(4ull * n_verts);
}

int nsa_mesh_components(const int32_t* faces, uint32_t n_faces, uint32_t n_verts, void* workspace, int32_t* vertex_label,
                        int32_t* face_label, uint64_t* totals, nsa_stream_t stream) {
    using namespace nsa;
    if (n_verts > kCcMaxCount || n_faces > kCcMaxCount) return NSA_EBADARG;
    if (n_verts == 0 && n_faces == 0) return NSA_OK;
    if (!totals || (n_faces && (!faces || !face_label)) || (n_verts && (!workspace || !vertex_label))) return NSA_EBADARG;
    int32_t* parent = static_cast<int32_t*>(workspace);
    ull* tot = reinterpret_cast<ull*>(totals);
    const uint32_t gv = (n_verts + 255) / 256, gf = (n_faces + 255) / 256;
    launch_begin();
    hipLaunchKernelGGL(k_cc_init, dim3(gv ? gv : 1), dim3(256), 0, (hipStream_t)stream, parent, vertex_label, n_verts, tot);
    if (n_verts && n_faces) {
        hipLaunchKernelGGL(k_cc_faces, dim3(gf), dim3(256), 0, (hipStream_t)stream, parent, vertex_label, faces, n_faces, n_verts,
                           tot);
        hipLaunchKernelGGL(k_cc_label, dim3(gv), dim3(256), 0, (hipStream_t)stream, parent, vertex_label, n_verts, tot);
    }
    if (n_faces)
        hipLaunchKernelGGL(k_cc_face_label, dim3(gf), dim3(256), 0, (hipStream_t)stream, vertex_label, faces, n_faces, n_verts,
                           face_label);
    return launch_end();
}

uint64_t nsa_mesh_component_stats_workspace(uint32_t n_verts, uint32_t n_faces, uint32_t n_components) {
    if (n_verts == 0 || n_verts > nsa::kCcMaxCount || n_faces > nsa::kCcMaxCount || n_components > n_faces ||
        n_components > n_verts)
        return 0;
    return nsa::stat_carve(nullptr, n_verts, n_faces, n_components, nullptr);
}

int nsa_mesh_component_stats(const float* verts, uint32_t n_verts, const int32_t* faces, uint32_t n_faces,
                             const int32_t* vertex_label, const int32_t* face_label, uint32_t n_components, void* workspace,
                             int32_t* label, int32_t* n_faces_out, int32_t* n_verts_out, double* area, float* lo, float* hi,
                             int32_t* vertex_comp, int32_t* face_comp, nsa_stream_t stream) {
    using namespace nsa;
    const uint32_t V = n_verts, F = n_faces, C = n_components;
    if (V > kCcMaxCount || F > kCcMaxCount || C > F || C > V) return NSA_EBADARG;
    if (V == 0 && F == 0) return NSA_OK;
    if ((V && (!verts || !vertex_label || !vertex_comp || !workspace)) || (F && (!faces || !face_label || !face_comp)))
        return NSA_EBADARG;
    if (F && !V) return NSA_EBADARG;                       // (faces without vertices: nothing to rank them by)
    if (C && (!label || !n_faces_out || !n_verts_out || !area || !lo || !hi)) return NSA_EBADARG;
    StatWork w;
    stat_carve(workspace, V, F, C, &w);
    const uint32_t nbv = (V + kCcBlock - 1) / kCcBlock, nbf = (F + kCcBlock - 1) / kCcBlock;
    launch_begin();
    hipLaunchKernelGGL(k_st_count, dim3(nbv), dim3(kCcBlock), 0, (hipStream_t)stream, vertex_label, V, w);
    hipLaunchKernelGGL((scan::k_offsets<1, uint32_t, kCcBlock>), dim3(1), dim3(kCcBlock), 0, (hipStream_t)stream,
                       (const uint32_t*)w.bcount, w.bcount, nbv, (ull*)nullptr);
    hipLaunchKernelGGL(k_st_rank, dim3(nbv), dim3(kCcBlock), 0, (hipStream_t)stream, vertex_label, V, C, w, label, n_verts_out);
    hipLaunchKernelGGL(k_st_verts, dim3((V + 255) / 256), dim3(256), 0, (hipStream_t)stream, verts, vertex_label, V, C, w,
                       vertex_comp, n_verts_out);
    if (F) {
        hipLaunchKernelGGL(k_st_face_keys, dim3((F + 255) / 256), dim3(256), 0, (hipStream_t)stream, face_label, F, V, C, w,
                           face_comp);
        if (C) {
            uint32_t bits = 1;
            while ((1ull << bits) <= (uint64_t)C) ++bits;  // keys are <= C
            radix_argsort(w.keys, w.tmp, w.order, w.counts, F, 0, (bits + 7) / 8, stream);
            hipLaunchKernelGGL(k_st_area_pieces, dim3(nbf), dim3(kCcBlock), 0, (hipStream_t)stream, verts, V, faces, F, C, w,
                               face_comp, area);
            hipLaunchKernelGGL(k_st_finish, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, F, C, w, n_faces_out, area,
                               lo, hi);
        }
    }
    return launch_end();
}

}  // extern "C"
