// mesh_manifold.hip -- one vertex per fan of faces: the cutting step that makes a triangle mesh a 2-manifold, on the device (DESIGN 4y;
// C ABI Section 26).  Reference: the "cutting" of Gueziec, Taubin, Lazarus and Horn, Cutting and Stitching (IEEE TVCG 7(2), 2001).
//
// All of it runs on the edge table nsa_mesh_edges wrote (Section 18) and is integer work.  One union-find over the 3 F corners: a
// regular edge unites its two faces' corners at each of its ends (manifold_passes.hpp on uf_passes.hpp, unchanged); parent[x] <= x, so
// the root of a fan is its smallest corner whatever the interleaving.  Every corner then carries a key -- its vertex when it leads its
// fan, V otherwise -- and one stable radix argsort of the keys (radix_sort.hpp), with only the 8-bit passes V needs, puts the leaders
// first in ascending (vertex, leader).  (The sort's length is a host number, so compacting the leaders first would not shorten it: the
// key V does the compaction.)  The first fan of a run keeps the vertex's name; the others are ranked by one exclusive scan of the
// "not head of its run" flags (block_scan.hpp).  Every total is a sum, an OR or a maximum of per-block integers: no atomics outside the
// union-find, and those decide nothing in the output.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/nicer_slam_amd.h"
#include "block_scan.hpp"
#include "grid_common.hpp"
#include "manifold_passes.hpp"
#include "radix_sort.hpp"
#include "uf_passes.hpp"

namespace nsa {

constexpr uint32_t kMfBlock = 1024;                       // block of the scans and of the partial counts

using scan::ull;

__host__ __device__ inline uint64_t mf_align(uint64_t b) { return (b + 255) & ~uint64_t(255); }
__host__ __device__ inline uint64_t mf_blocks(uint64_t n) { return (n + kMfBlock - 1) / kMfBlock; }

struct FanWork {                 // views into the caller's workspace (nsa_mesh_split_fans_workspace bytes)
    int32_t* parent;             // [H]: union-find over the corners
    int32_t* fan_name;           // [H]: the output vertex of the fan that corner leads, -1 elsewhere
    uint32_t* keys[2];           // [H] each: radix ping-pong
    uint32_t* tmp;               // [H]: radix payload ping-pong
    uint32_t* order;             // [H]: corners sorted stably by key
    uint32_t* counts;            // [256 * 256]
    uint32_t* bfurther;          // [nbh]: further fans per block of 1024 sorted positions, then their exclusive scan
    uint32_t* part_e;            // [2 nbh]: cut edges and the status of a block of edges
    uint32_t* part_c;            // [3 nbh]: contributing faces, fans and the status of a block of corners
    uint32_t* part_v;            // [2 nbv]: singular and pinch-only vertices of a block of vertices
    uint32_t* part_m;            // [nbv]: the most fans at a vertex of the block
    int32_t* on_cut;             // [V]: 1 for an end of a cut edge
    int32_t* first_r;            // [V]: further fans before the vertex's first fan, -1 for an unused vertex
    int32_t* last_r;             // [V]: further fans up to and including its last fan
};

__host__ __device__ inline uint64_t fan_carve(void* ws, uint32_t V, uint32_t F, FanWork* out) {
    const uint64_t H = 3ull * F, nbh = mf_blocks(H), nbv = mf_blocks(V);
    char* base = static_cast<char*>(ws);
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) { char* p = base ? base + o : nullptr; o += mf_align(bytes ? bytes : 1); return p; };
    FanWork w;
    w.parent = reinterpret_cast<int32_t*>(take(4 * H));
    w.fan_name = reinterpret_cast<int32_t*>(take(4 * H));
    w.keys[0] = reinterpret_cast<uint32_t*>(take(4 * H));
    w.keys[1] = reinterpret_cast<uint32_t*>(take(4 * H));
    w.tmp = reinterpret_cast<uint32_t*>(take(4 * H));
    w.order = reinterpret_cast<uint32_t*>(take(4 * H));
    w.counts = reinterpret_cast<uint32_t*>(take(4ull * kRadixCountWords));
    w.bfurther = reinterpret_cast<uint32_t*>(take(4 * nbh));
    w.part_e = reinterpret_cast<uint32_t*>(take(8 * nbh));
    w.part_c = reinterpret_cast<uint32_t*>(take(12 * nbh));
    w.part_v = reinterpret_cast<uint32_t*>(take(8 * nbv));
    w.part_m = reinterpret_cast<uint32_t*>(take(4 * nbv));
    w.on_cut = reinterpret_cast<int32_t*>(take(4ull * V));
    w.first_r = reinterpret_cast<int32_t*>(take(4ull * V));
    w.last_r = reinterpret_cast<int32_t*>(take(4ull * V));
    if (out) *out = w;
    return o;
}

// the largest v of the workgroup, in every lane (every lane calls it; blockDim.x == kMfBlock)
__device__ __forceinline__ uint32_t mf_block_max(uint32_t v) {
    __shared__ uint32_t sh[kMfBlock];
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (uint32_t o = kMfBlock / 2; o > 0; o >>= 1) {
        if (t < o) sh[t] = max(sh[t], sh[t + o]);
        __syncthreads();
    }
    const uint32_t out = sh[0];
    __syncthreads();
    return out;
}

__global__ __launch_bounds__(256) void k_mf_init(FanWork w, uint32_t H, uint32_t V) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < H) {
        w.parent[i] = (int32_t)i;
        w.fan_name[i] = -1;
    }
    if (i < V) {
        w.on_cut[i] = 0;
        w.first_r[i] = -1;
        w.last_r[i] = -1;
    }
}

// one lane per edge: the join pass; cut edges counted per block
__global__ __launch_bounds__(kMfBlock) void k_mf_join(FanWork w, const int32_t* __restrict__ faces, uint32_t F, uint32_t V,
                                                      const int32_t* __restrict__ face_label, uint32_t flags,
                                                      const int32_t* __restrict__ edges, const int32_t* __restrict__ edge_count,
                                                      const int32_t* __restrict__ edge_forward, const int32_t* __restrict__ edge_start,
                                                      const int32_t* __restrict__ edge_halfedges, const int32_t* __restrict__ face_edges,
                                                      const ull* __restrict__ edge_totals) {
    const uint32_t e = blockIdx.x * kMfBlock + threadIdx.x;
    const uint32_t E = scan::capped(edge_totals[0], 3u * F);
    uint32_t status = 0;
    bool flag[3] = {false, false, false};
    if (e < E)
        flag[0] = mf_pass_join(w.parent, w.on_cut, faces, F, V, face_label, flags, edges, edge_count, edge_forward, edge_start,
                               edge_halfedges, face_edges, e, &status);
    flag[1] = (status & kUfCapFind) != 0;
    flag[2] = (status & kUfCapHook) != 0;
    uint32_t pre[3], out[3];
    scan::flag_scan<3, kMfBlock>(flag, pre, out);
    if (threadIdx.x == 0) {
        w.part_e[2ull * blockIdx.x] = out[0];
        w.part_e[2ull * blockIdx.x + 1] = (out[1] ? kUfCapFind : 0u) | (out[2] ? kUfCapHook : 0u);
    }
}

// one lane per corner: its fan and its sort key; contributing faces and fans counted per block
__global__ __launch_bounds__(kMfBlock) void k_mf_leader(FanWork w, const int32_t* __restrict__ faces, const int32_t* __restrict__ face_edges,
                                                        uint32_t F, uint32_t V, int32_t* __restrict__ corner_fan) {
    const uint32_t c = blockIdx.x * kMfBlock + threadIdx.x, H = 3u * F;
    uint32_t status = 0;
    bool flag[3] = {false, false, false};
    if (c < H) {
        uint32_t key;
        const int32_t fan = mf_pass_leader(w.parent, faces, face_edges, F, V, c, &key, &status);
        corner_fan[c] = fan;
        w.keys[0][c] = key;
        flag[0] = fan >= 0 && c % 3u == 0;
        flag[1] = fan == (int32_t)c;
    }
    flag[2] = status != 0;
    uint32_t pre[3], out[3];
    scan::flag_scan<3, kMfBlock>(flag, pre, out);
    if (threadIdx.x == 0) {
        w.part_c[3ull * blockIdx.x] = out[0];
        w.part_c[3ull * blockIdx.x + 1] = out[1];
        w.part_c[3ull * blockIdx.x + 2] = out[2] ? kUfCapFind : 0u;
    }
}

// one lane per sorted position: the further fans of its block
__global__ __launch_bounds__(kMfBlock) void k_mf_count(FanWork w, const int32_t* __restrict__ faces, const int32_t* __restrict__ face_edges,
                                                       uint32_t F, uint32_t V, const int32_t* __restrict__ corner_fan) {
    const uint32_t i = blockIdx.x * kMfBlock + threadIdx.x, H = 3u * F;
    uint32_t c, v, total;
    const bool further = i < H && mf_run_head(corner_fan, faces, face_edges, w.order, H, V, i, &c, &v) == 2;
    scan::flag_scan<kMfBlock>(further, total);
    if (threadIdx.x == 0) w.bfurther[blockIdx.x] = total;
}

// one lane per sorted position: the name pass with r from the block's offset and the lanes below
__global__ __launch_bounds__(kMfBlock) void k_mf_name(FanWork w, const int32_t* __restrict__ faces, const int32_t* __restrict__ face_edges,
                                                      uint32_t F, uint32_t V, const int32_t* __restrict__ corner_fan,
                                                      int32_t* __restrict__ new_source) {
    const uint32_t i = blockIdx.x * kMfBlock + threadIdx.x, H = 3u * F;
    uint32_t c, v, total;
    const bool further = i < H && mf_run_head(corner_fan, faces, face_edges, w.order, H, V, i, &c, &v) == 2;
    const uint32_t pre = scan::flag_scan<kMfBlock>(further, total);
    if (i >= H) return;
    mf_pass_name(corner_fan, faces, face_edges, w.order, F, V, i, w.bfurther[blockIdx.x] + pre, w.fan_name, new_source, w.first_r, w.last_r);
}

// one lane per vertex: its fans; singular and pinch-only vertices counted and the most fans found per block
__global__ __launch_bounds__(kMfBlock) void k_mf_verts(FanWork w, uint32_t V, int32_t* __restrict__ vertex_fans) {
    const uint32_t v = blockIdx.x * kMfBlock + threadIdx.x;
    bool flag[2] = {false, false};
    uint32_t n = 0;
    if (v < V) {
        n = (uint32_t)mf_vertex_fans(w.first_r, w.last_r, v);
        vertex_fans[v] = (int32_t)n;
        flag[0] = n > 1;
        flag[1] = n > 1 && w.on_cut[v] == 0;
    }
    uint32_t pre[2], out[2];
    scan::flag_scan<2, kMfBlock>(flag, pre, out);
    const uint32_t most = mf_block_max(n);
    if (threadIdx.x == 0) {
        w.part_v[2ull * blockIdx.x] = out[0];
        w.part_v[2ull * blockIdx.x + 1] = out[1];
        w.part_m[blockIdx.x] = most;
    }
}

__global__ __launch_bounds__(256) void k_mf_faces(FanWork w, const int32_t* __restrict__ faces, uint32_t F, uint32_t V,
                                                  const int32_t* __restrict__ corner_fan, int32_t* __restrict__ faces_out) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c < 3u * F) faces_out[c] = mf_pass_face(faces, corner_fan, w.fan_name, F, V, c);
}

// one workgroup: the partial counts of every block, added (or-ed; the largest taken).  totals[5], the new vertices, is already there:
// the scan of the further fans left it.
__global__ __launch_bounds__(kMfBlock) void k_mf_totals(FanWork w, uint32_t nbh, uint32_t nbv, ull* totals) {
    ull e[2], c[3], v[2];
    scan::block_totals<1, 1, kMfBlock>(w.part_e, nbh, e);
    scan::block_totals<2, 1, kMfBlock>(w.part_c, nbh, c);
    scan::block_totals<2, 0, kMfBlock>(w.part_v, nbv, v);
    uint32_t most = 0;
    for (uint32_t b = threadIdx.x; b < nbv; b += kMfBlock) most = max(most, w.part_m[b]);
    most = mf_block_max(most);
    if (threadIdx.x == 0) {
        totals[0] = c[0];                                 // contributing faces
        totals[1] = c[1];                                 // fans
        totals[2] = v[0];                                 // singular vertices
        totals[3] = v[1];                                 // of those, with no cut edge
        totals[4] = e[0];                                 // cut edges
        totals[6] = most;                                 // the most fans at one vertex
        totals[7] = e[1] | c[2];                          // status
    }
}

}  // namespace nsa

extern "C" {

uint64_t nsa_mesh_split_fans_workspace(uint32_t n_verts, uint32_t n_faces) {
    if (n_faces == 0 || 3ull * n_faces + n_verts >= 0x80000000ull) return 0;
    return nsa::fan_carve(nullptr, n_verts, n_faces, nullptr);
}

int nsa_mesh_split_fans(const int32_t* faces, uint32_t n_faces, uint32_t n_verts, const int32_t* face_label, uint32_t flags,
                        const int32_t* edges, const int32_t* edge_count, const int32_t* edge_forward, const int32_t* edge_start,
                        const int32_t* edge_halfedges, const int32_t* face_edges, const uint64_t* edge_totals, void* workspace,
                        int32_t* corner_fan, int32_t* vertex_fans, int32_t* faces_out, int32_t* new_source, uint64_t* totals,
                        nsa_stream_t stream) {
    using namespace nsa;
    const uint32_t V = n_verts, F = n_faces;
    if (3ull * F + V >= 0x80000000ull || (flags & ~kSplitCutInconsistent)) return NSA_EBADARG;
    if (F == 0) return NSA_OK;
    if (!faces || !edges || !edge_count || !edge_forward || !edge_start || !edge_halfedges || !face_edges || !edge_totals || !workspace ||
        !corner_fan || (V && !vertex_fans) || !faces_out || !new_source || !totals)
        return NSA_EBADARG;
    FanWork w;
    fan_carve(workspace, V, F, &w);
    const uint32_t H = 3u * F, nbh = (uint32_t)mf_blocks(H), nbv = (uint32_t)mf_blocks(V);
    uint32_t bits = 1;
    while ((1ull << bits) <= (uint64_t)V) ++bits;             // keys are <= V
    const uint32_t passes = (bits + 7) / 8;
    ull* tot = reinterpret_cast<ull*>(totals);
    const ull* etot = reinterpret_cast<const ull*>(edge_totals);
    hipStream_t s = (hipStream_t)stream;
    launch_begin();
    hipLaunchKernelGGL(k_mf_init, dim3((max(H, V) + 255) / 256), dim3(256), 0, s, w, H, V);
    hipLaunchKernelGGL(k_mf_join, dim3(nbh), dim3(kMfBlock), 0, s, w, faces, F, V, face_label, flags, edges, edge_count, edge_forward,
                       edge_start, edge_halfedges, face_edges, etot);
    hipLaunchKernelGGL(k_mf_leader, dim3(nbh), dim3(kMfBlock), 0, s, w, faces, face_edges, F, V, corner_fan);
    radix_argsort(w.keys, w.tmp, w.order, w.counts, H, 0, passes, stream);
    hipLaunchKernelGGL(k_mf_count, dim3(nbh), dim3(kMfBlock), 0, s, w, faces, face_edges, F, V, corner_fan);
    // (the scan's grand total is n_new: it goes straight to totals[5])
    hipLaunchKernelGGL((scan::k_offsets<1, uint32_t, kMfBlock>), dim3(1), dim3(kMfBlock), 0, s, w.bfurther, w.bfurther, nbh, tot + 5);
    hipLaunchKernelGGL(k_mf_name, dim3(nbh), dim3(kMfBlock), 0, s, w, faces, face_edges, F, V, corner_fan, new_source);
    if (V) hipLaunchKernelGGL(k_mf_verts, dim3(nbv), dim3(kMfBlock), 0, s, w, V, vertex_fans);
    hipLaunchKernelGGL(k_mf_faces, dim3((H + 255) / 256), dim3(256), 0, s, w, faces, F, V, corner_fan, faces_out);
    hipLaunchKernelGGL(k_mf_totals, dim3(1), dim3(kMfBlock), 0, s, w, nbh, nbv, tot);
    return launch_end();
}

}  // extern "C"
