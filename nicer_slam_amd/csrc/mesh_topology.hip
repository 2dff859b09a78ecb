// mesh_topology.hip -- the undirected edge table of a triangle mesh, its classes and totals, and the components of faces joined
// across edges, on the device (C ABI Section 18).  Reference: trimesh's edges_unique / face_adjacency / split, which
// code/utils/viz.py:136-141 wanted, and the is_closed / euler helpers of tests/mc_ref.py.
//
// Edge table: one key per half-edge h = 3f + k, (lo, hi) of its two vertices, V for both when the face does not contribute.  The
// 64-bit order lo << 32 | hi is two stable radix argsorts (radix_sort.hpp), hi then lo, each with only the 8-bit passes V needs; the
// second sorts positions of the first, so the half-edges of an edge stay in ascending id.  Run heads come from comparing neighbours
// in the sorted order, edge ids and forward counts from one exclusive scan of (head, forward) flags, counts from the difference of
// consecutive run starts.  Every total is a sum of per-block partial counts added by one workgroup.  The scan, the counts and the
// totals are block_scan.hpp's: integers throughout, no floating point, and no atomics except inside the union-find.
//
// Boundary loops: the vertex union-find of uf_passes.hpp with the boundary edges in place of faces; a loop is a root that some
// boundary edge marked.  Face components: the same uf_find / uf_unite with faces as nodes -- every half-edge of a run after the
// first unites its face with its predecessor's.  parent[x] <= x throughout, so the root is the smallest index whatever the
// interleaving; step caps report through status.  The bodies of the three union-find passes live in topo_passes.hpp, which also
// compiles as host C++ (tests/topology_host_check.cpp runs them on many host threads).
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/nicer_slam_amd.h"
#include "block_scan.hpp"
#include "grid_common.hpp"
#include "radix_sort.hpp"
#include "topo_passes.hpp"
#include "uf_passes.hpp"

namespace nsa {

constexpr uint32_t kTopoMaxVerts = 0x7FFFFFFFu;
constexpr uint32_t kTopoMaxFaces = 0x7FFFFFFFu / 3u;    // H = 3 F < 2^31
constexpr uint32_t kTopoBlock = 1024;                   // block of the scans and of the partial counts
constexpr uint32_t kFwdBit = 0x80000000u;               // in the sorted hi word: the half-edge runs lo -> hi

using scan::ull;

__host__ __device__ inline uint64_t topo_align(uint64_t b) { return (b + 255) & ~uint64_t(255); }
__host__ __device__ inline uint64_t topo_blocks(uint64_t n) { return (n + kTopoBlock - 1) / kTopoBlock; }

struct EdgeWork {                // views into the caller's workspace (nsa_mesh_edges_workspace bytes)
    uint32_t* keys[2];           // [H] each: radix ping-pong; after the sorts the sorted lo and hi | kFwdBit words
    uint32_t* tmp;               // [H + 1]: radix payload ping-pong; after the sorts fpre: forward half-edges before each run
    uint32_t* order1;            // [H]: half-edges sorted stably by hi
    uint32_t* order2;            // [H]: positions of order1 sorted stably by lo
    uint32_t* counts;            // [256 * 256]
    uint32_t* bcount;            // [2 nbh]: heads, forwards per block of 1024 sorted positions, then their exclusive scans
    uint32_t* part_e;            // [4 nbh]: boundary, non-manifold, inconsistent edges and the status of a block of edges
    uint32_t* part_v;            // [2 nbv]: used vertices and loop roots of a block of vertices
    uint32_t* fwd_total;         // [1]
    int32_t* parent;             // [V]: union-find over the vertices
    int32_t* bmark;              // [V]: -1, 0 for a vertex of a boundary edge
    int32_t* used;               // [V]: 1 for a vertex of a contributing face
};

__host__ __device__ inline uint64_t edge_carve(void* ws, uint32_t V, uint32_t F, EdgeWork* out) {
    const uint64_t H = 3ull * F, nbh = topo_blocks(H), nbv = topo_blocks(V);
    char* base = static_cast<char*>(ws);
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) { char* p = base ? base + o : nullptr; o += topo_align(bytes ? bytes : 1); return p; };
    EdgeWork w;
    w.keys[0] = reinterpret_cast<uint32_t*>(take(4 * H));
    w.keys[1] = reinterpret_cast<uint32_t*>(take(4 * H));
    w.tmp = reinterpret_cast<uint32_t*>(take(4 * (H + 1)));
    w.order1 = reinterpret_cast<uint32_t*>(take(4 * H));
    w.order2 = reinterpret_cast<uint32_t*>(take(4 * H));
    w.counts = reinterpret_cast<uint32_t*>(take(4ull * kRadixCountWords));
    w.bcount = reinterpret_cast<uint32_t*>(take(8 * nbh));
    w.part_e = reinterpret_cast<uint32_t*>(take(16 * nbh));
    w.part_v = reinterpret_cast<uint32_t*>(take(8 * nbv));
    w.fwd_total = reinterpret_cast<uint32_t*>(take(4));
    w.parent = reinterpret_cast<int32_t*>(take(4ull * V));
    w.bmark = reinterpret_cast<int32_t*>(take(4ull * V));
    w.used = reinterpret_cast<int32_t*>(take(4ull * V));
    if (out) *out = w;
    return o;
}

// whether face f contributes: indices in [0, V), pairwise distinct, mask set
__device__ __forceinline__ bool face_contributes(const int32_t* __restrict__ faces, const uint8_t* __restrict__ mask, uint32_t f,
                                                 uint32_t V, int32_t v[3]) {
    v[0] = faces[3ull * f];
    v[1] = faces[3ull * f + 1];
    v[2] = faces[3ull * f + 2];
    return uf_valid_face(v[0], v[1], v[2], V) && v[0] != v[1] && v[1] != v[2] && v[2] != v[0] && (!mask || mask[f] != 0);
}

// half-edge h = 3 f + k: its (lo, hi) and direction; false (lo = hi = V) when its face does not contribute
__device__ __forceinline__ bool half_edge(const int32_t* __restrict__ faces, const uint8_t* __restrict__ mask, uint32_t V, uint32_t h,
                                          uint32_t* lo, uint32_t* hi, bool* fwd) {
    const uint32_t f = h / 3u, k = h - 3u * f;
    int32_t v[3];
    *lo = *hi = V;
    *fwd = false;
    if (!face_contributes(faces, mask, f, V, v)) return false;
    const uint32_t a = (uint32_t)(k == 0 ? v[0] : k == 1 ? v[1] : v[2]), b = (uint32_t)(k == 0 ? v[1] : k == 1 ? v[2] : v[0]);
    *fwd = a < b;
    *lo = a < b ? a : b;
    *hi = a < b ? b : a;
    return true;
}

// ---- keys and the two sorts ----------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_te_init(EdgeWork w, uint32_t V) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    uf_pass_init(w.parent, w.bmark, v);
    w.used[v] = 0;
}

// one lane per face: the hi keys of its three half-edges; marks its vertices as used (the same value from every face)
__global__ __launch_bounds__(256) void k_te_keys_hi(const int32_t* __restrict__ faces, const uint8_t* __restrict__ mask, uint32_t F,
                                                    uint32_t V, EdgeWork w) {
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int32_t v[3];
    const bool c = face_contributes(faces, mask, f, V, v);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int32_t a = v[k], b = v[k == 2 ? 0 : k + 1];
        w.keys[0][3ull * f + k] = c ? (uint32_t)(a > b ? a : b) : V;
        if (c) w.used[a] = 1;
    }
}

__global__ __launch_bounds__(256) void k_te_keys_lo(const int32_t* __restrict__ faces, const uint8_t* __restrict__ mask, uint32_t H,
                                                    uint32_t V, EdgeWork w) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H) return;
    uint32_t lo, hi;
    bool fwd;
    const uint32_t h = w.order1[i];
    if (h >= H) return;                                   // (never: the order is a permutation of [0, H))
    half_edge(faces, mask, V, h, &lo, &hi, &fwd);
    w.keys[0][i] = lo;
}

// sorted position i: its half-edge, its (lo, hi | direction) words; -1 edge ids for the faces that do not contribute
__global__ __launch_bounds__(256) void k_te_gather(const int32_t* __restrict__ faces, const uint8_t* __restrict__ mask, uint32_t H,
                                                   uint32_t V, EdgeWork w, int32_t* __restrict__ edge_halfedges,
                                                   int32_t* __restrict__ face_edges) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H) return;
    const uint32_t p = w.order2[i];
    const uint32_t h = p < H ? w.order1[p] : H;
    if (h >= H) return;                                   // (never: both orders are permutations of [0, H))
    uint32_t lo, hi;
    bool fwd;
    const bool c = half_edge(faces, mask, V, h, &lo, &hi, &fwd);
    w.keys[0][i] = lo;
    w.keys[1][i] = hi | (fwd ? kFwdBit : 0u);
    edge_halfedges[i] = c ? (int32_t)h : -1;
    if (!c) face_edges[h] = -1;
}

// ---- run heads, edge ids --------------------------------------------------------------------------------------------------------

__device__ __forceinline__ bool te_contrib(const EdgeWork& w, uint32_t i, uint32_t V) { return w.keys[0][i] != V; }

__device__ __forceinline__ bool te_head(const EdgeWork& w, uint32_t i, uint32_t V) {
    const uint32_t lo = w.keys[0][i];
    if (lo == V) return false;
    if (i == 0) return true;
    return w.keys[0][i - 1] != lo || ((w.keys[1][i - 1] ^ w.keys[1][i]) & ~kFwdBit) != 0;
}

__global__ __launch_bounds__(kTopoBlock) void k_te_count(EdgeWork w, uint32_t H, uint32_t V) {
    const uint32_t i = blockIdx.x * kTopoBlock + threadIdx.x;
    const bool in = i < H;
    const bool flag[2] = {in && te_head(w, i, V), in && te_contrib(w, i, V) && (w.keys[1][i] & kFwdBit)};      // head, forward
    uint32_t pre[2], total[2];
    scan::flag_scan<2, kTopoBlock>(flag, pre, total);
    if (threadIdx.x == 0) {
        w.bcount[2ull * blockIdx.x] = total[0];
        w.bcount[2ull * blockIdx.x + 1] = total[1];
    }
}

// one workgroup: bcount[0, nb) pairs -> their exclusive scans; the two grand totals
__global__ __launch_bounds__(kTopoBlock) void k_te_scan(EdgeWork w, uint32_t nb, ull* __restrict__ totals) {
    uint32_t total[2];
    scan::offsets<2, uint32_t, kTopoBlock>(w.bcount, w.bcount, nb, total);
    if (threadIdx.x == 0) {
        totals[0] = total[0];                             // E
        *w.fwd_total = total[1];
    }
}

// sorted position i: the edge id of its half-edge; a head also writes the edge, where its run starts and the forward half-edges
// before it; the position where the contributing half-edges end closes both offset arrays and gives F_c
__global__ __launch_bounds__(kTopoBlock) void k_te_rank(EdgeWork w, uint32_t H, uint32_t V, const int32_t* __restrict__ edge_halfedges,
                                                        int32_t* __restrict__ edges, int32_t* __restrict__ edge_start,
                                                        int32_t* __restrict__ face_edges, ull* __restrict__ totals) {
    const uint32_t i = blockIdx.x * kTopoBlock + threadIdx.x;
    const bool in = i < H;
    const bool contrib = in && te_contrib(w, i, V);
    const bool head = in && te_head(w, i, V);
    const bool flag[2] = {head, contrib && (w.keys[1][i] & kFwdBit)};
    uint32_t pre[2], total[2];
    scan::flag_scan<2, kTopoBlock>(flag, pre, total);
    if (!in) return;
    const uint32_t E = (uint32_t)totals[0];
    // the end of the contributing half-edges: the first position that does not contribute, or H
    const bool prev = i > 0 && te_contrib(w, i - 1, V);
    uint32_t Hc = 0xFFFFFFFFu;
    if (!contrib && (i == 0 || prev)) Hc = i;
    else if (contrib && i == H - 1) Hc = H;
    if (Hc != 0xFFFFFFFFu && E <= H) {
        edge_start[E] = (int32_t)Hc;
        w.tmp[E] = *w.fwd_total;
        totals[1] = Hc / 3u;                              // F_c
    }
    if (!contrib) return;
    const uint32_t e = w.bcount[2ull * blockIdx.x] + pre[0] + (head ? 1u : 0u) - 1u;
    if (e >= H) return;                                   // (never: a contributing position has a head at or before it)
    const int32_t h = edge_halfedges[i];
    if (h >= 0 && (uint32_t)h < H) face_edges[h] = (int32_t)e;
    if (head) {
        edges[2ull * e] = (int32_t)w.keys[0][i];
        edges[2ull * e + 1] = (int32_t)(w.keys[1][i] & ~kFwdBit);
        edge_start[e] = (int32_t)i;
        w.tmp[e] = w.bcount[2ull * blockIdx.x + 1] + pre[1];
    }
}

// ---- classes, boundary loops, totals ------------------------------------------------------------------------------------------------

// one lane per edge: count and forward count from the offsets of its run and of the next; a boundary edge marks and joins its ends
__global__ __launch_bounds__(kTopoBlock) void k_te_classify(EdgeWork w, uint32_t H, uint32_t V, const ull* __restrict__ totals,
                                                            const int32_t* __restrict__ edges, const int32_t* __restrict__ edge_start,
                                                            int32_t* __restrict__ edge_count, int32_t* __restrict__ edge_forward) {
    const uint32_t e = blockIdx.x * kTopoBlock + threadIdx.x;
    const uint32_t E = min((uint32_t)totals[0], H);
    bool flag[5] = {false, false, false, false, false};
    uint32_t status = 0;
    if (e < E) {
        const int32_t count = edge_start[e + 1] - edge_start[e], forward = (int32_t)(w.tmp[e + 1] - w.tmp[e]);
        edge_count[e] = count;
        edge_forward[e] = forward;
        flag[0] = count == 1;
        flag[1] = count > 2;
        flag[2] = count == 2 && forward != 1;
        topo_pass_boundary(w.parent, w.bmark, V, edges, e, count, &status);
    }
    flag[3] = (status & kUfCapFind) != 0;
    flag[4] = (status & kUfCapHook) != 0;
    uint32_t pre[5], out[5];
    scan::flag_scan<5, kTopoBlock>(flag, pre, out);
    if (threadIdx.x == 0) {
        w.part_e[4ull * blockIdx.x] = out[0];
        w.part_e[4ull * blockIdx.x + 1] = out[1];
        w.part_e[4ull * blockIdx.x + 2] = out[2];
        w.part_e[4ull * blockIdx.x + 3] = (out[3] ? kUfCapFind : 0u) | (out[4] ? kUfCapHook : 0u);
    }
}

// one lane per vertex: used by a contributing face; the root of a tree some boundary edge marked = one boundary loop
__global__ __launch_bounds__(kTopoBlock) void k_te_verts(EdgeWork w, uint32_t V) {
    const uint32_t v = blockIdx.x * kTopoBlock + threadIdx.x;
    bool flag[2] = {false, false};
    if (v < V) {
        flag[0] = w.used[v] != 0;
        flag[1] = w.bmark[v] == 0 && w.parent[v] == (int32_t)v;
    }
    uint32_t pre[2], out[2];
    scan::flag_scan<2, kTopoBlock>(flag, pre, out);
    if (threadIdx.x == 0) {
        w.part_v[2ull * blockIdx.x] = out[0];
        w.part_v[2ull * blockIdx.x + 1] = out[1];
    }
}

// one workgroup: the partial counts of every block, added
__global__ __launch_bounds__(kTopoBlock) void k_te_totals(EdgeWork w, uint32_t nbe, uint32_t nbv, ull* __restrict__ totals) {
    ull e[4], v[2];
    scan::block_totals<3, 1, kTopoBlock>(w.part_e, nbe, e);
    scan::block_totals<2, 0, kTopoBlock>(w.part_v, nbv, v);
    if (threadIdx.x == 0) {
        totals[2] = v[0];                                 // used vertices
        totals[3] = e[0];                                 // boundary edges
        totals[4] = e[1];                                 // non-manifold edges
        totals[5] = e[2];                                 // inconsistent edges
        totals[6] = v[1];                                 // boundary loops
        totals[7] = e[3];                                 // status
    }
}

// ---- face components --------------------------------------------------------------------------------------------------------------

struct FaceWork {
    int32_t* parent;             // [F]
    uint32_t* part;              // [2 nbf]: roots and the status of a block of faces
    uint32_t* status;            // [1]: step caps of the unions
};

__host__ __device__ inline uint64_t face_carve(void* ws, uint32_t F, FaceWork* out) {
    char* base = static_cast<char*>(ws);
    const uint64_t a = topo_align(4ull * F), b = topo_align(8 * topo_blocks(F));
    if (out) {
        out->parent = reinterpret_cast<int32_t*>(base);
        out->part = reinterpret_cast<uint32_t*>(base ? base + a : nullptr);
        out->status = reinterpret_cast<uint32_t*>(base ? base + a + b : nullptr);
    }
    return a + b + topo_align(4);
}

__global__ __launch_bounds__(256) void k_fc_init(FaceWork w, uint32_t F) {
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    if (f == 0) *w.status = 0;
    if (f < F) w.parent[f] = (int32_t)f;
}

// one lane per sorted position: a half-edge that is not the first of its run joins its face with its predecessor's
__global__ __launch_bounds__(256) void k_fc_unite(FaceWork w, uint32_t F, const int32_t* __restrict__ face_edges,
                                                  const int32_t* __restrict__ edge_start, const int32_t* __restrict__ edge_halfedges) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    uint32_t status = 0;
    topo_pass_join(w.parent, F, face_edges, edge_start, edge_halfedges, i, &status);
    if (status) atomicOr(w.status, status);             // (the union-find's own cap report)
}

__global__ __launch_bounds__(kTopoBlock) void k_fc_label(FaceWork w, uint32_t F, const int32_t* __restrict__ face_edges,
                                                         int32_t* __restrict__ face_label) {
    const uint32_t f = blockIdx.x * kTopoBlock + threadIdx.x;
    bool flag[2] = {false, false};
    uint32_t status = 0;
    if (f < F) {
        const int32_t l = topo_pass_label(w.parent, F, face_edges, f, &status);
        face_label[f] = l;
        flag[0] = l == (int32_t)f;
        flag[1] = (status & kUfCapFind) != 0;
    }
    uint32_t pre[2], out[2];
    scan::flag_scan<2, kTopoBlock>(flag, pre, out);
    if (threadIdx.x == 0) {
        w.part[2ull * blockIdx.x] = out[0];
        w.part[2ull * blockIdx.x + 1] = out[1] ? kUfCapFind : 0u;
    }
}

__global__ __launch_bounds__(kTopoBlock) void k_fc_totals(FaceWork w, uint32_t nbf, ull* __restrict__ totals) {
    ull t[2];
    scan::block_totals<1, 1, kTopoBlock>(w.part, nbf, t);
    if (threadIdx.x == 0) {
        totals[0] = t[0];
        totals[1] = t[1] | *w.status;
    }
}

}  // namespace nsa

extern "C" {

uint64_t nsa_mesh_edges_workspace(uint32_t n_verts, uint32_t n_faces) {
    if (n_faces == 0 || n_faces > nsa::kTopoMaxFaces || n_verts > nsa::kTopoMaxVerts) return 0;
    return nsa::edge_carve(nullptr, n_verts, n_faces, nullptr);
}

int nsa_mesh_edges(const int32_t* faces, uint32_t n_faces, uint32_t n_verts, const uint8_t* face_mask, void* workspace,
                   int32_t* edges, int32_t* edge_count, int32_t* edge_forward, int32_t* edge_start, int32_t* edge_halfedges,
                   int32_t* face_edges, uint64_t* totals, nsa_stream_t stream) {
    using namespace nsa;
    const uint32_t V = n_verts, F = n_faces;
    if (V > kTopoMaxVerts || F > kTopoMaxFaces) return NSA_EBADARG;
    if (F == 0) return NSA_OK;
    if (!faces || !workspace || !edges || !edge_count || !edge_forward || !edge_start || !edge_halfedges || !face_edges || !totals)
        return NSA_EBADARG;
    EdgeWork w;
    edge_carve(workspace, V, F, &w);
    const uint32_t H = 3u * F, nbh = (uint32_t)topo_blocks(H), nbv = (uint32_t)topo_blocks(V);
    uint32_t bits = 1;
    while ((1ull << bits) <= (uint64_t)V) ++bits;             // keys are <= V
    const uint32_t passes = (bits + 7) / 8;
    ull* tot = reinterpret_cast<ull*>(totals);
    hipStream_t s = (hipStream_t)stream;
    launch_begin();
    if (V) hipLaunchKernelGGL(k_te_init, dim3((V + 255) / 256), dim3(256), 0, s, w, V);
    hipLaunchKernelGGL(k_te_keys_hi, dim3((F + 255) / 256), dim3(256), 0, s, faces, face_mask, F, V, w);
    radix_argsort(w.keys, w.tmp, w.order1, w.counts, H, 0, passes, stream);
    hipLaunchKernelGGL(k_te_keys_lo, dim3((H + 255) / 256), dim3(256), 0, s, faces, face_mask, H, V, w);
    radix_argsort(w.keys, w.tmp, w.order2, w.counts, H, 0, passes, stream);
    hipLaunchKernelGGL(k_te_gather, dim3((H + 255) / 256), dim3(256), 0, s, faces, face_mask, H, V, w, edge_halfedges, face_edges);
    hipLaunchKernelGGL(k_te_count, dim3(nbh), dim3(kTopoBlock), 0, s, w, H, V);
    hipLaunchKernelGGL(k_te_scan, dim3(1), dim3(kTopoBlock), 0, s, w, nbh, tot);
    hipLaunchKernelGGL(k_te_rank, dim3(nbh), dim3(kTopoBlock), 0, s, w, H, V, edge_halfedges, edges, edge_start, face_edges, tot);
    hipLaunchKernelGGL(k_te_classify, dim3(nbh), dim3(kTopoBlock), 0, s, w, H, V, tot, edges, edge_start, edge_count, edge_forward);
    if (V) hipLaunchKernelGGL(k_te_verts, dim3(nbv), dim3(kTopoBlock), 0, s, w, V);
    hipLaunchKernelGGL(k_te_totals, dim3(1), dim3(kTopoBlock), 0, s, w, nbh, nbv, tot);
    return launch_end();
}

uint64_t nsa_mesh_face_components_workspace(uint32_t n_faces) {
    if (n_faces == 0 || n_faces > nsa::kTopoMaxFaces) return 0;
    return nsa::face_carve(nullptr, n_faces, nullptr);
}

int nsa_mesh_face_components(const int32_t* face_edges, const int32_t* edge_start, const int32_t* edge_halfedges, uint32_t n_faces,
                             void* workspace, int32_t* face_label, uint64_t* totals, nsa_stream_t stream) {
    using namespace nsa;
    const uint32_t F = n_faces;
    if (F > kTopoMaxFaces) return NSA_EBADARG;
    if (F == 0) return NSA_OK;
    if (!face_edges || !edge_start || !edge_halfedges || !workspace || !face_label || !totals) return NSA_EBADARG;
    FaceWork w;
    face_carve(workspace, F, &w);
    const uint32_t H = 3u * F, nbf = (uint32_t)topo_blocks(F);
    hipStream_t s = (hipStream_t)stream;
    launch_begin();
    hipLaunchKernelGGL(k_fc_init, dim3((F + 255) / 256), dim3(256), 0, s, w, F);
    hipLaunchKernelGGL(k_fc_unite, dim3((H + 255) / 256), dim3(256), 0, s, w, F, face_edges, edge_start, edge_halfedges);
    hipLaunchKernelGGL(k_fc_label, dim3(nbf), dim3(kTopoBlock), 0, s, w, F, face_edges, face_label);
    hipLaunchKernelGGL(k_fc_totals, dim3(1), dim3(kTopoBlock), 0, s, w, nbf, reinterpret_cast<ull*>(totals));
    return launch_end();
}

}  // extern "C"
