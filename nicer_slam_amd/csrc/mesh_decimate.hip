// mesh_decimate.hip -- edge-collapse decimation with quadric error, in rounds of independent collapses (C ABI Section 22).
// The bodies live in decimate_passes.hpp, which also compiles as host C++; the kernels here are one lane per item around them.
//
// The state -- float64 positions, quadrics and colours, vertex_map, the lock and moved bytes -- lies in one buffer of the caller's
// between the calls; the face list is the caller's as well and is rewritten in place.  A round reads the edge table (Section 18)
// and the rings (Section 21) of the current faces: one lane per edge slot for placement, cost, link and fold; two passes of one lane
// per vertex for the minima m1 and m2; one lane per edge slot to select; four stable radix argsorts (the two halves of the edge word,
// then the two halves of the cost bits) to put the selected edges in key order; one workgroup for the totals and the prefix rule;
// then apply, rename and compose.  No atomics anywhere: every output is a function of the arguments alone.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/nicer_slam_amd.h"
#include "block_scan.hpp"
#include "corner_table.hpp"
#include "grid_common.hpp"
#include "radix_sort.hpp"
#include "decimate_passes.hpp"

namespace nsa {
namespace decimate {

constexpr uint32_t kMaxVerts = 0x7FFFFFFFu;
constexpr uint32_t kMaxFaces = 0x7FFFFFFFu / 6u;        // ring offsets up to 6 F are int32

using scan::ull;

using bulk::up256;

struct State {                   // views into the caller's state buffer (nsa_mesh_decimate_state_bytes)
    double* pos;                 // [3 V]
    double* quad;                // [11 V]
    double* col;                 // [3 V]
    int32_t* vmap;               // [V]
    uint8_t* locked;             // [V]
    uint8_t* moved;              // [V]
    ull* counters;               // [4]: log rows written so far
};

__host__ __device__ inline uint64_t state_carve(void* buf, uint32_t V, State* out) {
    char* base = static_cast<char*>(buf);
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) { char* p = base ? base + o : nullptr; o += up256(bytes); return p; };
    State s;
    s.pos = reinterpret_cast<double*>(take(24ull * V));
    s.quad = reinterpret_cast<double*>(take(8ull * kQ * V));
    s.col = reinterpret_cast<double*>(take(24ull * V));
    s.vmap = reinterpret_cast<int32_t*>(take(4ull * V));
    s.locked = reinterpret_cast<uint8_t*>(take(V));
    s.moved = reinterpret_cast<uint8_t*>(take(V));
    s.counters = reinterpret_cast<ull*>(take(32));
    if (out) *out = s;
    return o;
}

struct RoundWork {               // views into the caller's workspace; H = 3 F
    ull* cost_bits;              // [H]
    ull* skey;                   // [H]: the cost bits of a selected edge, kNoKey otherwise
    double* place;               // [3 H]
    ull* m1c;                    // [V]
    ull* m1w;                    // [V]
    uint32_t* m1e;               // [V]
    uint32_t* m2e;               // [V]
    uint32_t* keys[2];           // [H] each: radix ping-pong
    uint32_t* tmp;               // [H]
    uint32_t* order;             // [H]: one argsort's order
    uint32_t* perm;              // [H]: edge slots in the order of the sorts so far, ping-pong with `sorted`
    uint32_t* sorted;            // [H]: edge slots in key order, the selected ones first
    uint32_t* counts;            // [256 * 256]
    ull* scalars;                // [4]: selected, taken, log base
    uint32_t* partial;           // [6 * ceil(H / 256)]: per block of 256 edge slots the counts of the five codes and of the selected
    uint8_t* code;               // [H]
};

__host__ __device__ inline uint64_t round_carve(void* ws, uint32_t V, uint32_t F, RoundWork* out) {
    const uint64_t H = 3ull * F;
    char* base = static_cast<char*>(ws);
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) { char* p = base ? base + o : nullptr; o += up256(bytes); return p; };
    RoundWork w;
    w.cost_bits = reinterpret_cast<ull*>(take(8 * H));
    w.skey = reinterpret_cast<ull*>(take(8 * H));
    w.place = reinterpret_cast<double*>(take(24 * H));
    w.m1c = reinterpret_cast<ull*>(take(8ull * V));
    w.m1w = reinterpret_cast<ull*>(take(8ull * V));
    w.m1e = reinterpret_cast<uint32_t*>(take(4ull * V));
    w.m2e = reinterpret_cast<uint32_t*>(take(4ull * V));
    w.keys[0] = reinterpret_cast<uint32_t*>(take(4 * H));
    w.keys[1] = reinterpret_cast<uint32_t*>(take(4 * H));
    w.tmp = reinterpret_cast<uint32_t*>(take(4 * H));
    w.order = reinterpret_cast<uint32_t*>(take(4 * H));
    w.perm = reinterpret_cast<uint32_t*>(take(4 * H));
    w.sorted = reinterpret_cast<uint32_t*>(take(4 * H));
    w.counts = reinterpret_cast<uint32_t*>(take(4ull * kRadixCountWords));
    w.scalars = reinterpret_cast<ull*>(take(32));
    w.partial = reinterpret_cast<uint32_t*>(take(24ull * ((H + 255) / 256)));
    w.code = reinterpret_cast<uint8_t*>(take(H));
    if (out) *out = w;
    return o;
}

__device__ __forceinline__ uint32_t edges_on_device(const ull* __restrict__ edge_totals, uint32_t H) {
    return scan::capped(edge_totals[0], H);
}

// ---- the initial state ----------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_dc_init_pos(State st, const float* __restrict__ verts, const float* __restrict__ colors,
                                                     uint32_t V) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v == 0) st.counters[0] = 0;
    if (v >= V) return;
    init_pass_position(verts, colors, v, st.pos, st.col, st.vmap, st.moved);
}

struct CornerKey {
    const float* verts;
    const int32_t* faces;
    uint32_t V, F;
    __device__ uint32_t operator()(uint32_t c) const { return smooth::normal_corner_key(verts, V, faces, F, c); }
};

__global__ __launch_bounds__(256) void k_dc_init_vertex(State st, corners::Table t, uint32_t V, const int32_t* __restrict__ faces,
                                                        uint32_t F, const int32_t* __restrict__ ring_start,
                                                        const int32_t* __restrict__ ring, const int32_t* __restrict__ ring_edge,
                                                        const int32_t* __restrict__ edge_count, const int32_t* __restrict__ edge_start,
                                                        const int32_t* __restrict__ edge_halfedges, const uint8_t* __restrict__ fixed,
                                                        int boundary, double boundary_weight) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    uint32_t s = t.start[v], e = t.start[v + 1];
    if (e > 3u * F || s > e) s = e = 0;                                   // (never: the offsets come from a search over 3 F keys)
    init_pass_vertex(st.pos, V, faces, F, t.corner, s, e, ring_start, ring, ring_edge, edge_count, edge_start, edge_halfedges, fixed,
                     boundary, boundary_weight, v, st.locked, st.quad);
}

// ---- one round ------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_dc_edge(RoundWork w, EdgeTables t, const ull* __restrict__ edge_totals, double eps,
                                                 bool has_limit, double max_error2, double min_cos2) {
    const uint32_t H = 3u * t.F, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H) return;
    t.E = edges_on_device(edge_totals, H);
    w.code[i] = edge_pass(t, i, eps, has_limit, max_error2, min_cos2, reinterpret_cast<uint64_t*>(w.cost_bits), w.place);
}

__global__ __launch_bounds__(256) void k_dc_min1(RoundWork w, const int32_t* __restrict__ ring_start, const int32_t* __restrict__ ring_edge,
                                                 const int32_t* __restrict__ edges, uint32_t V, uint32_t F) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    min1_pass(ring_start, ring_edge, edges, w.code, reinterpret_cast<const uint64_t*>(w.cost_bits), V, F, v,
              reinterpret_cast<uint64_t*>(w.m1c), reinterpret_cast<uint64_t*>(w.m1w), w.m1e);
}

__global__ __launch_bounds__(256) void k_dc_min2(RoundWork w, const int32_t* __restrict__ ring_start, const int32_t* __restrict__ ring,
                                                 uint32_t V, uint32_t F) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    min2_pass(ring_start, ring, reinterpret_cast<const uint64_t*>(w.m1c), reinterpret_cast<const uint64_t*>(w.m1w), w.m1e, V, F, v, w.m2e);
}

__global__ __launch_bounds__(256) void k_dc_select(RoundWork w, const int32_t* __restrict__ edges, uint32_t V, uint32_t H) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H) return;
    w.skey[i] = select_pass(edges, w.code, reinterpret_cast<const uint64_t*>(w.cost_bits), w.m2e, V, i);
}

// the keys of argsort k: word k of the edge slot at position p of the order so far (the slots themselves before the first sort)
__global__ __launch_bounds__(256) void k_dc_sort_keys(RoundWork w, const int32_t* __restrict__ edges, const uint32_t* __restrict__ cur,
                                                      uint32_t H, int k) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= H) return;
    const uint32_t i = cur ? cur[p] : p;
    w.keys[0][p] = i < H ? sort_word(edges, reinterpret_cast<const uint64_t*>(w.skey), i, k) : 0xFFFFFFFFu;      // (always: a permutation)
}

// next[p] = cur[order[p]]: the order so far carried through one more stable argsort
__global__ __launch_bounds__(256) void k_dc_sort_perm(const uint32_t* __restrict__ cur, const uint32_t* __restrict__ order,
                                                      uint32_t* __restrict__ next, uint32_t H) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= H) return;
    const uint32_t q = order[p];
    next[p] = q < H ? cur[q] : H;
}

// one lane per edge slot: the block's counts of the five codes and of the selected edges (integers, no atomics)
__global__ __launch_bounds__(256) void k_dc_count(RoundWork w, uint32_t H) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const uint8_t c = i < H ? w.code[i] : (uint8_t)255;
    const bool flag[6] = {c == 0, c == 1, c == 2, c == 3, c == 4, i < H && w.skey[i] != kNoKey};
    uint32_t pre[6], total[6];
    scan::flag_scan<6, 256>(flag, pre, total);
#pragma unroll
    for (int k = 0; k < 6; ++k)
        if (threadIdx.x == k) w.partial[6ull * blockIdx.x + k] = total[k];
}

// one workgroup: the sums of the block counts, then the prefix rule over the selected edges in key order
__global__ __launch_bounds__(256) void k_dc_totals(RoundWork w, State st, const int32_t* __restrict__ edge_count,
                                                   const ull* __restrict__ edge_totals, uint32_t H, uint32_t round, bool has_target,
                                                   ull target, ull* __restrict__ totals) {
    __shared__ uint32_t red[6][256];
    __shared__ uint32_t sums[8];
    const uint32_t t = threadIdx.x, nb = (H + 255) / 256;
    uint32_t cnt[6] = {0, 0, 0, 0, 0, 0};
    for (uint32_t j = t; j < nb; j += 256)
        for (int k = 0; k < 6; ++k) cnt[k] += w.partial[6ull * j + k];
    for (int k = 0; k < 6; ++k) red[k][t] = cnt[k];
    __syncthreads();
    if (t < 6) {
        uint32_t s = 0;
        for (uint32_t j = 0; j < 256; ++j) s += red[t][j];
        sums[t] = s;
    }
    __syncthreads();
    const uint32_t n_sel = sums[5] < H ? sums[5] : H;
    const ull n_faces = edge_totals[1];
    ull carry = 0;
    uint32_t n_take = 0, removed = 0, bad = 0;
    for (uint32_t base = 0; base < n_sel; base += 256) {
        const uint32_t p = base + t;
        uint32_t ec = 0;
        if (p < n_sel) {
            const uint32_t i = w.sorted[p];
            if (i < H) ec = (uint32_t)edge_count[i];
            else bad = 1;
        }
        const uint32_t own[1] = {ec};
        uint32_t excl[1], total[1];
        scan::lds_scan<1, uint32_t, 256>(own, excl, total);
        if (p < n_sel && prefix_take(has_target, n_faces, carry + excl[0], target)) {
            ++n_take;
            removed += ec;
        }
        carry += total[0];
    }
    red[0][t] = n_take;
    red[1][t] = removed;
    red[2][t] = bad;
    __syncthreads();
    if (t == 0) {
        ull nt = 0, rm = 0, bd = 0;
        for (uint32_t j = 0; j < 256; ++j) {
            nt += red[0][j];
            rm += red[1][j];
            bd += red[2][j];
        }
        const ull base = st.counters[0];
        w.scalars[0] = n_sel;
        w.scalars[1] = nt;
        w.scalars[2] = base;
        st.counters[0] = base + nt;
        totals[0] = round;
        totals[1] = edge_totals[0];
        totals[2] = n_faces;
        totals[3] = sums[0];
        totals[4] = sums[1];
        totals[5] = sums[2];
        totals[6] = sums[3];
        totals[7] = sums[4];
        totals[8] = n_sel;
        totals[9] = nt;
        totals[10] = rm;
        totals[11] = n_faces - (rm < n_faces ? rm : n_faces);
        totals[12] = base + nt;
        totals[13] = bd ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void k_dc_apply(RoundWork w, State st, const int32_t* __restrict__ edges, uint32_t V, uint32_t H,
                                                  bool has_color, uint32_t round, ull* __restrict__ log, uint32_t log_rows) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= H || p >= w.scalars[1]) return;
    const uint32_t i = w.sorted[p];
    if (i >= H) return;
    uint32_t lo, hi;
    apply_pass(edges, w.place, V, i, st.pos, st.quad, has_color ? st.col : nullptr, st.vmap, st.moved, &lo, &hi);
    const ull row = w.scalars[2] + p;
    if (row < log_rows) {
        log[4 * row] = round;
        log[4 * row + 1] = lo;
        log[4 * row + 2] = hi;
        log[4 * row + 3] = w.cost_bits[i];
    }
}

__global__ __launch_bounds__(256) void k_dc_rename(State st, uint32_t V, uint32_t H, int32_t* __restrict__ faces) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= H) return;
    rename_pass(st.vmap, V, c, faces);
}

__global__ __launch_bounds__(256) void k_dc_compose(State st, uint32_t V) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    compose_pass(V, v, st.vmap);
}

// ---- the end --------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_dc_finish(State st, const float* __restrict__ verts, const float* __restrict__ colors, uint32_t V,
                                                   float* __restrict__ out_verts, float* __restrict__ out_colors,
                                                   int32_t* __restrict__ vertex_map) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const bool moved = st.moved[v] != 0;
    const uint32_t* in = reinterpret_cast<const uint32_t*>(verts);
    uint32_t* o = reinterpret_cast<uint32_t*>(out_verts);
#pragma unroll
    for (int k = 0; k < 3; ++k) o[3ull * v + k] = moved ? __float_as_uint((float)st.pos[3ull * v + k]) : in[3ull * v + k];
    if (colors && out_colors) {
        const uint32_t* cin = reinterpret_cast<const uint32_t*>(colors);
        uint32_t* co = reinterpret_cast<uint32_t*>(out_colors);
#pragma unroll
        for (int k = 0; k < 3; ++k) co[3ull * v + k] = moved ? __float_as_uint((float)st.col[3ull * v + k]) : cin[3ull * v + k];
    }
    vertex_map[v] = st.vmap[v];
}

inline bool counts_ok(uint32_t V, uint32_t F) { return V <= kMaxVerts && F <= kMaxFaces; }

}  // namespace decimate
}  // namespace nsa

extern "C" {

uint64_t nsa_mesh_decimate_state_bytes(uint32_t n_verts) {
    if (n_verts == 0 || n_verts > nsa::decimate::kMaxVerts) return 0;
    return nsa::decimate::state_carve(nullptr, n_verts, nullptr);
}

uint64_t nsa_mesh_decimate_workspace(uint32_t n_verts, uint32_t n_faces) {
    if (n_verts == 0 || n_faces == 0 || !nsa::decimate::counts_ok(n_verts, n_faces)) return 0;
    const uint64_t a = nsa::corners::carve(nullptr, n_verts, n_faces, nullptr);
    const uint64_t b = nsa::decimate::round_carve(nullptr, n_verts, n_faces, nullptr);
    return a > b ? a : b;
}

int nsa_mesh_decimate_init(const float* verts, const float* colors, uint32_t n_verts, const int32_t* faces, uint32_t n_faces,
                           const int32_t* edge_count, const int32_t* edge_start, const int32_t* edge_halfedges, const int32_t* ring_start,
                           const int32_t* ring, const int32_t* ring_edge, const uint8_t* fixed, int boundary, double boundary_weight,
                           void* workspace, void* state, nsa_stream_t stream) {
    using namespace nsa;
    using namespace nsa::decimate;
    const uint32_t V = n_verts, F = n_faces;
    if (!counts_ok(V, F)) return NSA_EBADARG;
    if (boundary != kQuadric && boundary != kFixed) return NSA_EBADARG;
    if (!(boundary_weight >= 0.0) || !finite_d(boundary_weight)) return NSA_EBADARG;
    if (V == 0 || F == 0) return NSA_OK;
    if (!verts || !faces || !edge_count || !edge_start || !edge_halfedges || !ring_start || !ring || !ring_edge || !workspace || !state)
        return NSA_EBADARG;
    State st;
    state_carve(state, V, &st);
    corners::Table t;
    corners::carve(workspace, V, F, &t);
    const uint32_t nbv = (V + 255) / 256;
    hipStream_t s = (hipStream_t)stream;
    launch_begin();
    hipLaunchKernelGGL(k_dc_init_pos, dim3(nbv), dim3(256), 0, s, st, verts, colors, V);
    corners::build(CornerKey{verts, faces, V, F}, V, F, t, stream);
    hipLaunchKernelGGL(k_dc_init_vertex, dim3(nbv), dim3(256), 0, s, st, t, V, faces, F, ring_start, ring, ring_edge, edge_count,
                       edge_start, edge_halfedges, fixed, boundary, boundary_weight);
    return launch_end();
}

int nsa_mesh_decimate_round(uint32_t n_verts, int32_t* faces, uint32_t n_faces, const int32_t* edges, const int32_t* edge_count,
                            const int32_t* edge_start, const int32_t* edge_halfedges, const uint64_t* edge_totals,
                            const int32_t* ring_start, const int32_t* ring, const int32_t* ring_edge, uint32_t round, int has_target,
                            uint64_t target_faces, int has_limit, double max_error2, double min_cos2, double eps, int has_colors,
                            void* workspace, void* state, uint64_t* log, uint32_t log_rows, uint64_t* totals, nsa_stream_t stream) {
    using namespace nsa;
    using namespace nsa::decimate;
    const uint32_t V = n_verts, F = n_faces;
    if (!counts_ok(V, F)) return NSA_EBADARG;
    if (has_limit && !(max_error2 >= 0.0)) return NSA_EBADARG;
    if (!(min_cos2 >= 0.0 && min_cos2 < 1.0) || !(eps >= 0.0) || !finite_d(eps)) return NSA_EBADARG;
    if (V == 0 || F == 0) return NSA_OK;
    if (!faces || !edges || !edge_count || !edge_start || !edge_halfedges || !edge_totals || !ring_start || !ring || !ring_edge ||
        !workspace || !state || !totals || (log_rows && !log))
        return NSA_EBADARG;
    State st;
    state_carve(state, V, &st);
    RoundWork w;
    round_carve(workspace, V, F, &w);
    const uint32_t H = 3u * F, nbh = (H + 255) / 256, nbv = (V + 255) / 256;
    const ull* etot = reinterpret_cast<const ull*>(edge_totals);
    ull* tot = reinterpret_cast<ull*>(totals);
    EdgeTables t{faces, edges, edge_count, edge_start, edge_halfedges, ring_start, ring, ring_edge, st.pos, st.quad, st.locked, V, F, 0};
    hipStream_t s = (hipStream_t)stream;
    launch_begin();
    hipLaunchKernelGGL(k_dc_edge, dim3(nbh), dim3(256), 0, s, w, t, etot, eps, has_limit != 0, max_error2, min_cos2);
    hipLaunchKernelGGL(k_dc_min1, dim3(nbv), dim3(256), 0, s, w, ring_start, ring_edge, edges, V, F);
    hipLaunchKernelGGL(k_dc_min2, dim3(nbv), dim3(256), 0, s, w, ring_start, ring, V, F);
    hipLaunchKernelGGL(k_dc_select, dim3(nbh), dim3(256), 0, s, w, edges, V, H);
    // least significant word first; the order ends in w.sorted
    hipLaunchKernelGGL(k_dc_sort_keys, dim3(nbh), dim3(256), 0, s, w, edges, (const uint32_t*)nullptr, H, 0);
    radix_argsort(w.keys, w.tmp, w.perm, w.counts, H, 0, 4, stream);
    uint32_t* cur = w.perm;
    uint32_t* next = w.sorted;
    for (int k = 1; k < 4; ++k) {
        hipLaunchKernelGGL(k_dc_sort_keys, dim3(nbh), dim3(256), 0, s, w, edges, (const uint32_t*)cur, H, k);
        radix_argsort(w.keys, w.tmp, w.order, w.counts, H, 0, 4, stream);
        hipLaunchKernelGGL(k_dc_sort_perm, dim3(nbh), dim3(256), 0, s, (const uint32_t*)cur, (const uint32_t*)w.order, next, H);
        uint32_t* t2 = cur;
        cur = next;
        next = t2;
    }
    hipLaunchKernelGGL(k_dc_count, dim3(nbh), dim3(256), 0, s, w, H);
    hipLaunchKernelGGL(k_dc_totals, dim3(1), dim3(256), 0, s, w, st, edge_count, etot, H, round, has_target != 0, (ull)target_faces, tot);
    hipLaunchKernelGGL(k_dc_apply, dim3(nbh), dim3(256), 0, s, w, st, edges, V, H, has_colors != 0, round, reinterpret_cast<ull*>(log),
                       log_rows);
    hipLaunchKernelGGL(k_dc_rename, dim3(nbh), dim3(256), 0, s, st, V, H, faces);
    hipLaunchKernelGGL(k_dc_compose, dim3(nbv), dim3(256), 0, s, st, V);
    return launch_end();
}

int nsa_mesh_decimate_finish(const float* verts, const float* colors, uint32_t n_verts, const void* state, float* out_verts,
                             float* out_colors, int32_t* vertex_map, nsa_stream_t stream) {
    using namespace nsa;
    using namespace nsa::decimate;
    const uint32_t V = n_verts;
    if (V > kMaxVerts) return NSA_EBADARG;
    if (V == 0) return NSA_OK;
    if (!verts || !state || !out_verts || !vertex_map || (colors != nullptr) != (out_colors != nullptr)) return NSA_EBADARG;
    State st;
    state_carve(const_cast<void*>(state), V, &st);
    launch_begin();
    hipLaunchKernelGGL(k_dc_finish, dim3((V + 255) / 256), dim3(256), 0, (hipStream_t)stream, st, verts, colors, V, out_verts, out_colors,
                       vertex_map);
    return launch_end();
}

}  // extern "C"
