// mesh_fill.hip -- hole filling: boundary loops traced, ranked and patched (C ABI Section 23).
// The bodies live in fill_passes.hpp, which also compiles as host C++; the kernels here are one lane per item around them.
//
// nsa_mesh_fill_loops reads the edge table (Section 18): a scan compacts the B boundary half-edges in ascending id; one lane per item
// rotates to its successor; a stable radix argsort of the start vertices and a neighbour comparison mark the pinches; pointer jumping
// finds open chains and the leader of every cycle, Wyllie's list ranking the rank and the length; a scan over the leaders numbers the
// loops and lays `order` out; one lane per loop fills its row; a last scan gives the offsets of the patches and the totals.
// nsa_mesh_fill_emit is one lane per new face, that is per (loop, ring, i) and face of the pair there, each writing the vertex it owns.
// No atomics anywhere: every output is a function of the arguments alone.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/nicer_slam_amd.h"
#include "block_scan.hpp"
#include "grid_common.hpp"
#include "radix_sort.hpp"
#include "fill_passes.hpp"

namespace nsa {
namespace fill {

constexpr uint32_t kMaxVerts = 0x7FFFFFFFu;
constexpr uint32_t kMaxHalfedges = 0x7FFFFFFFu;
constexpr int kScanMax = 8;                              // the most channels of a scan

using scan::capped;
using scan::ull;

using bulk::up256;

struct Work {                    // views into the caller's workspace; H = 3 F, B the boundary half-edges
    int32_t* hslot;              // [H]: the item of a boundary half-edge, -1 otherwise
    ull* partial;                // [kScanMax * ceil(max(H, B) / 256)]: block sums of the scan in flight, then their exclusive scans
    ull* misc;                   // [16]: B on the device; loops, their lengths, open-chain items, cap hits; patch totals and class counts
    uint32_t* bh;                // [B]: the boundary half-edges, ascending
    uint32_t* next;              // [B]
    uint32_t* a[2];              // [B] each: smallest item seen / steps to the last item, ping-pong
    uint32_t* b[2];              // [B] each: the jump pointers, ping-pong
    uint32_t* leader;            // [B]
    uint32_t* item_start;        // [B]: at a leader, the start of its loop in `order`
    uint32_t* order_item;        // [B]: `order` as items
    uint32_t* keys[2];           // [B] each: radix ping-pong
    uint32_t* tmp;               // [B]
    uint32_t* sorder;            // [B]: the items sorted by start vertex
    uint32_t* counts;            // [256 * 256]
    uint8_t* t[2];               // [B] each: reached a terminal, ping-pong
    uint8_t* blk;                // [B]: kBlocked | kCapHit
    uint8_t* pinch;              // [B]
};

__host__ __device__ inline uint64_t carve(void* ws, uint32_t F, uint32_t B, Work* out) {
    const uint64_t H = 3ull * F, nb = ((H > B ? H : B) + 255) / 256;
    char* base = static_cast<char*>(ws);
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) { char* p = base ? base + o : nullptr; o += up256(bytes); return p; };
    auto words = [&]() { return reinterpret_cast<uint32_t*>(take(4ull * B)); };
    Work w;
    w.hslot = reinterpret_cast<int32_t*>(take(4 * H));
    w.partial = reinterpret_cast<ull*>(take(8ull * kScanMax * nb));
    w.misc = reinterpret_cast<ull*>(take(8 * 16));
    w.bh = words();
    w.next = words();
    w.a[0] = words();
    w.a[1] = words();
    w.b[0] = words();
    w.b[1] = words();
    w.leader = words();
    w.item_start = words();
    w.order_item = words();
    w.keys[0] = words();
    w.keys[1] = words();
    w.tmp = words();
    w.sorder = words();
    w.counts = reinterpret_cast<uint32_t*>(take(4ull * kRadixCountWords));
    w.t[0] = reinterpret_cast<uint8_t*>(take(B));
    w.t[1] = reinterpret_cast<uint8_t*>(take(B));
    w.blk = reinterpret_cast<uint8_t*>(take(B));
    w.pinch = reinterpret_cast<uint8_t*>(take(B));
    if (out) *out = w;
    return o;
}

__device__ __forceinline__ Topo on_device(Topo t, const ull* __restrict__ edge_totals) {
    t.E = capped(edge_totals[0], 3u * t.F);
    return t;
}

// ---- scans of up to kScanMax integer channels over n items: block sums, one workgroup over the blocks (block_scan.hpp), the prefixes --

template <int C, class In>
__global__ __launch_bounds__(256) void k_scan_count(In in, uint32_t n, ull* __restrict__ partial) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    ull v[C], excl[C], total[C];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = 0;
    if (i < n) in(i, v);
    scan::lds_scan<C, ull, 256>(v, excl, total);
#pragma unroll
    for (int c = 0; c < C; ++c)
        if (threadIdx.x == c) partial[(ull)C * blockIdx.x + c] = total[c];
}

template <int C, class In, class Out>
__global__ __launch_bounds__(256) void k_scan_write(In in, Out out, uint32_t n, const ull* __restrict__ partial) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    ull v[C], excl[C], total[C];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = 0;
    if (i < n) in(i, v);
    scan::lds_scan<C, ull, 256>(v, excl, total);
    if (i >= n) return;
#pragma unroll
    for (int c = 0; c < C; ++c) excl[c] += partial[(ull)C * blockIdx.x + c];
    out(i, v, excl);
}

template <int C, class In, class Out>
void scan_items(In in, Out out, uint32_t n, const Work& w, ull* sums, hipStream_t s) {
    const uint32_t nb = (n + 255) / 256;
    hipLaunchKernelGGL((k_scan_count<C, In>), dim3(nb), dim3(256), 0, s, in, n, w.partial);
    hipLaunchKernelGGL((scan::k_offsets<C, ull, 256>), dim3(1), dim3(256), 0, s, (const ull*)w.partial, w.partial, nb, sums);
    hipLaunchKernelGGL((k_scan_write<C, In, Out>), dim3(nb), dim3(256), 0, s, in, out, n, (const ull*)w.partial);
}

// ---- the boundary half-edges --------------------------------------------------------------------------------------------------------

struct BoundaryIn {
    Topo t;
    const ull* edge_totals;
    __device__ void operator()(uint32_t h, ull (&v)[1]) const { v[0] = boundary_halfedge(on_device(t, edge_totals), h) ? 1 : 0; }
};

struct BoundaryOut {
    Work w;
    uint32_t B;
    __device__ void operator()(uint32_t h, const ull (&v)[1], const ull (&at)[1]) const {
        const bool in = v[0] != 0 && at[0] < B;
        w.hslot[h] = in ? (int32_t)at[0] : -1;
        if (in) w.bh[at[0]] = h;
    }
};

__global__ __launch_bounds__(256) void k_fl_next(Work w, Topo t, const ull* __restrict__ edge_totals, uint32_t B) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, Bd = capped(w.misc[0], B);
    if (i < B) w.keys[0][i] = start_key(t, w.bh, Bd, i);                  // the keys of the pinch sort; V beyond the list
    if (i >= Bd) return;
    const uint8_t f = next_pass(on_device(t, edge_totals), w.bh, w.hslot, Bd, i, w.next);
    w.blk[i] = f;
    w.a[0][i] = i;
    w.b[0][i] = w.next[i];
    w.t[0][i] = f & kBlocked;
}

__global__ __launch_bounds__(256) void k_fl_pinch(Work w, Topo t, uint32_t B) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x, Bd = capped(w.misc[0], B);
    if (p >= Bd) return;
    pinch_pass(t, w.bh, w.sorder, Bd, p, w.pinch);
}

__global__ __launch_bounds__(256) void k_fl_jump(Work w, uint32_t B, int cur) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, Bd = capped(w.misc[0], B);
    if (i >= Bd) return;
    jump_pass(w.a[cur], w.b[cur], w.t[cur], Bd, i, w.a[cur ^ 1], w.b[cur ^ 1], w.t[cur ^ 1]);
}

__global__ __launch_bounds__(256) void k_fl_rank_init(Work w, uint32_t B, int cur) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, Bd = capped(w.misc[0], B);
    if (i >= Bd) return;
    rank_init_pass(w.a[cur], w.t[cur], w.next, Bd, i, w.leader, w.a[cur ^ 1], w.b[cur ^ 1]);
}

__global__ __launch_bounds__(256) void k_fl_rank(Work w, uint32_t B, int cur) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, Bd = capped(w.misc[0], B);
    if (i >= Bd) return;
    rank_pass(w.a[cur], w.b[cur], Bd, i, w.a[cur ^ 1], w.b[cur ^ 1]);
}

struct LeaderIn {                // channels: leaders, their loop lengths, open-chain items, cap hits
    Work w;
    uint32_t B;
    int dist, term;              // which of the ping-pong buffers hold the steps and the terminal flags
    __device__ void operator()(uint32_t i, ull (&v)[4]) const {
        if (i >= capped(w.misc[0], B)) return;
        const bool lead = is_leader(w.leader, i);
        v[0] = lead ? 1 : 0;
        v[1] = lead ? (ull)w.a[dist][i] + 1 : 0;
        v[2] = w.t[term][i] != 0 ? 1 : 0;
        v[3] = (w.blk[i] & kCapHit) ? 1 : 0;
    }
};

struct LeaderOut {
    Work w;
    uint32_t B;
    int64_t* ints;
    __device__ void operator()(uint32_t i, const ull (&v)[4], const ull (&at)[4]) const {
        w.item_start[i] = capped(at[1], B);
        if (v[0] == 0 || at[0] >= B) return;
        int64_t* row = ints + (ull)kLoopInts * at[0];
        row[0] = (int64_t)w.bh[i];
        row[1] = (int64_t)v[1];
        row[2] = (int64_t)at[1];
    }
};

__global__ __launch_bounds__(256) void k_fl_order(Work w, uint32_t B, int dist, int term, int32_t* __restrict__ halfedges,
                                                  int32_t* __restrict__ next, uint8_t* __restrict__ flags, int32_t* __restrict__ leader,
                                                  int32_t* __restrict__ rank, int32_t* __restrict__ order) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, Bd = capped(w.misc[0], B);
    if (i >= Bd) return;
    order_pass(w.bh, w.leader, w.a[dist], w.item_start, Bd, i, rank, w.order_item, order);
    halfedges[i] = (int32_t)w.bh[i];
    next[i] = (int32_t)w.next[i];
    leader[i] = w.leader[i] < Bd ? (int32_t)w.leader[i] : -1;
    flags[i] = (uint8_t)((w.blk[i] & (kBlocked | kCapHit)) | w.pinch[i] | (w.t[term][i] ? kOpenChain : 0));
}

__global__ __launch_bounds__(256) void k_fl_loop(Work w, Shape m, Limits lim, uint32_t B, int64_t* __restrict__ ints,
                                                 double* __restrict__ reals) {
    const uint32_t l = blockIdx.x * 256 + threadIdx.x, Bd = capped(w.misc[0], B);
    if (l >= capped(w.misc[1], Bd)) return;
    loop_pass(m, w.bh, w.order_item, w.pinch, Bd, lim, l, ints, reals);
}

struct PatchIn {                 // channels: new vertices, new faces, one count per class
    Work w;
    uint32_t B;
    const int64_t* ints;
    __device__ void operator()(uint32_t l, ull (&v)[8]) const {
        if (l >= capped(w.misc[1], capped(w.misc[0], B))) return;
        const int64_t* row = ints + (ull)kLoopInts * l;
        v[0] = (ull)row[5];
        v[1] = (ull)row[6];
        const int64_t c = row[3];
#pragma unroll
        for (int k = 0; k < kClasses; ++k) v[2 + k] = c == k ? 1 : 0;
    }
};

struct PatchOut {
    Work w;
    uint32_t B;
    int64_t* ints;
    __device__ void operator()(uint32_t l, const ull (&)[8], const ull (&at)[8]) const {
        if (l >= capped(w.misc[1], capped(w.misc[0], B))) return;
        ints[(ull)kLoopInts * l + 7] = (int64_t)at[0];
        ints[(ull)kLoopInts * l + 8] = (int64_t)at[1];
    }
};

__global__ void k_fl_totals(Work w, uint32_t B, ull* __restrict__ totals) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const uint32_t Bd = capped(w.misc[0], B);
    totals[0] = Bd;
    totals[1] = capped(w.misc[1], Bd);
    for (int c = 0; c < kClasses; ++c) totals[2 + c] = w.misc[7 + c];
    totals[8] = w.misc[3];
    totals[9] = w.misc[5];
    totals[10] = w.misc[6];
    totals[11] = (w.misc[4] ? 1ull : 0ull) | (w.misc[0] != B ? 2ull : 0ull);
}

__global__ __launch_bounds__(256) void k_fl_emit(Shape m, const int32_t* __restrict__ order, uint32_t B, const int64_t* __restrict__ ints,
                                                 const double* __restrict__ reals, const ull* __restrict__ totals, ull NV, ull NF,
                                                 float* __restrict__ new_verts, float* __restrict__ new_colors,
                                                 int32_t* __restrict__ new_faces) {
    const ull x = (ull)blockIdx.x * 256 + threadIdx.x;
    if (x >= NF) return;
    emit_pass(m, order, B, ints, reals, capped(totals[1], B), NV, NF, x, new_verts, new_colors, new_faces);
}

inline uint32_t rounds_of(uint32_t B) {                  // ceil(log2(max(B, 2))) + 1
    uint32_t r = 1, n = B < 2 ? 2 : B;
    while ((1ull << r) < n) ++r;
    return r + 1;
}

inline bool counts_ok(uint32_t V, uint32_t F, uint32_t B) { return V <= kMaxVerts && 3ull * F <= kMaxHalfedges && B <= 3ull * F; }

}  // namespace fill
}  // namespace nsa

extern "C" {

uint64_t nsa_mesh_fill_workspace(uint32_t n_faces, uint32_t n_boundary) {
    if (n_faces == 0 || n_boundary == 0 || !nsa::fill::counts_ok(0, n_faces, n_boundary)) return 0;
    return nsa::fill::carve(nullptr, n_faces, n_boundary, nullptr);
}

int nsa_mesh_fill_loops(const float* verts, const float* colors, uint32_t n_verts, const int32_t* faces, const int32_t* names,
                        uint32_t n_faces, const int32_t* edge_count, const int32_t* edge_forward, const int32_t* edge_start,
                        const int32_t* edge_halfedges, const int32_t* face_edges, const uint64_t* edge_totals, uint32_t n_boundary,
                        int has_max_edges, uint64_t max_edges, int has_max_size, double max_size2, uint32_t rings, uint32_t max_rings,
                        int skip_folded, void* workspace, int32_t* halfedges, int32_t* next, uint8_t* flags, int32_t* leader, int32_t* rank,
                        int32_t* order, int64_t* loop_ints, double* loop_reals, uint64_t* totals, nsa_stream_t stream) {
    using namespace nsa;
    using namespace nsa::fill;
    const uint32_t V = n_verts, F = n_faces, B = n_boundary;
    if (!counts_ok(V, F, B)) return NSA_EBADARG;
    if (rings > kMaxRings || max_rings == 0 || max_rings > kMaxRings) return NSA_EBADARG;
    if (has_max_size && !(max_size2 >= 0.0)) return NSA_EBADARG;
    if (F == 0 || B == 0) return NSA_OK;
    if (!verts || !faces || !edge_count || !edge_forward || !edge_start || !edge_halfedges || !face_edges || !edge_totals || !workspace ||
        !halfedges || !next || !flags || !leader || !rank || !order || !loop_ints || !loop_reals || !totals)
        return NSA_EBADARG;
    Work w;
    carve(workspace, F, B, &w);
    const uint32_t H = 3u * F, nbb = (B + 255) / 256, R = rounds_of(B);
    const ull* etot = reinterpret_cast<const ull*>(edge_totals);
    const Topo t{names ? names : faces, face_edges, edge_count, edge_forward, edge_start, edge_halfedges, V, F, 0};
    const Shape m{verts, colors, faces, V, F};
    const Limits lim{has_max_edges != 0, (uint64_t)max_edges, has_max_size != 0, max_size2, rings, max_rings, skip_folded != 0};
    hipStream_t s = (hipStream_t)stream;
    launch_begin();
    scan_items<1>(BoundaryIn{t, etot}, BoundaryOut{w, B}, H, w, w.misc, s);
    hipLaunchKernelGGL(k_fl_next, dim3(nbb), dim3(256), 0, s, w, t, etot, B);
    radix_argsort(w.keys, w.tmp, w.sorder, w.counts, B, 0, V < 0xFFu ? 1 : V < 0xFFFFu ? 2 : V < 0xFFFFFFu ? 3 : 4, stream);
    hipLaunchKernelGGL(k_fl_pinch, dim3(nbb), dim3(256), 0, s, w, t, B);
    int cur = 0;
    for (uint32_t r = 0; r < R; ++r, cur ^= 1) hipLaunchKernelGGL(k_fl_jump, dim3(nbb), dim3(256), 0, s, w, B, cur);
    const int term = cur;
    hipLaunchKernelGGL(k_fl_rank_init, dim3(nbb), dim3(256), 0, s, w, B, cur);
    cur ^= 1;
    for (uint32_t r = 0; r < R; ++r, cur ^= 1) hipLaunchKernelGGL(k_fl_rank, dim3(nbb), dim3(256), 0, s, w, B, cur);
    scan_items<4>(LeaderIn{w, B, cur, term}, LeaderOut{w, B, loop_ints}, B, w, w.misc + 1, s);
    hipLaunchKernelGGL(k_fl_order, dim3(nbb), dim3(256), 0, s, w, B, cur, term, halfedges, next, flags, leader, rank, order);
    hipLaunchKernelGGL(k_fl_loop, dim3(nbb), dim3(256), 0, s, w, m, lim, B, loop_ints, loop_reals);
    scan_items<8>(PatchIn{w, B, loop_ints}, PatchOut{w, B, loop_ints}, B, w, w.misc + 5, s);
    hipLaunchKernelGGL(k_fl_totals, dim3(1), dim3(64), 0, s, w, B, reinterpret_cast<ull*>(totals));
    return launch_end();
}

int nsa_mesh_fill_emit(const float* verts, const float* colors, uint32_t n_verts, const int32_t* faces, uint32_t n_faces,
                       const int32_t* order, uint32_t n_boundary, const int64_t* loop_ints, const double* loop_reals,
                       const uint64_t* totals, uint64_t n_new_verts, uint64_t n_new_faces, float* new_verts, float* new_colors,
                       int32_t* new_faces, nsa_stream_t stream) {
    using namespace nsa;
    using namespace nsa::fill;
    const uint32_t V = n_verts, F = n_faces, B = n_boundary;
    if (!counts_ok(V, F, B)) return NSA_EBADARG;
    if ((uint64_t)V + n_new_verts > kMaxVerts || n_new_faces > kMaxHalfedges / 3u) return NSA_EBADARG;
    if (F == 0 || B == 0 || n_new_faces == 0) return NSA_OK;
    if (!verts || !faces || !order || !loop_ints || !loop_reals || !totals || !new_verts || !new_faces ||
        (colors != nullptr) != (new_colors != nullptr))
        return NSA_EBADARG;
    const Shape m{verts, colors, faces, V, F};
    launch_begin();
    hipLaunchKernelGGL(k_fl_emit, dim3((uint32_t)((n_new_faces + 255) / 256)), dim3(256), 0, (hipStream_t)stream, m, order, B, loop_ints,
                       loop_reals, reinterpret_cast<const ull*>(totals), (ull)n_new_verts, (ull)n_new_faces, new_verts, new_colors, new_faces);
    return launch_end();
}

}  // extern "C"
