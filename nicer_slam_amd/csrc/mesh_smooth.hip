// mesh_smooth.hip -- the vertex rings of a triangle mesh, Laplacian / Taubin smoothing steps over them, and vertex normals from the
// faces, on the device (C ABI Section 21).  The bodies live in smooth_passes.hpp, which also compiles as host C++; the
// kernels here are one lane per item around them.
//
// Ring: input is the edge table of Section 18, which is sorted by (lo, hi).  One stable radix argsort of the edges by hi (radix_sort.hpp,
// only the 8-bit passes V needs; positions past E carry V and sort last, so E never leaves the device) gives the (hi, lo) order.  Row v
// is the hi == v run followed by the lo == v run: ring_start[v] = #{lo < v} + #{hi < v}, two binary searches and no scan, and every
// slot is a closed form of the two counts.  Integers only, no atomics.
//
// Smoothing: a prologue turns the input into float64 and writes a state byte per vertex, a second pass compacts each row to the
// neighbours that take part (both are constant over the steps), then one launch per step over ping-pong float64 positions; the last
// step rounds to fp32.  A step is + - * / on gathered neighbours in row order, each operation rounded on its own: no atomics, and the
// result is a function of the arguments alone.
//
// Normals: the corner-by-vertex table of corner_table.hpp (shared with mesh_sdf.hip), one lane per vertex over its corners in
// ascending id.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/nicer_slam_amd.h"
#include "corner_table.hpp"
#include "grid_common.hpp"
#include "radix_sort.hpp"
#include "smooth_passes.hpp"

namespace nsa {
namespace smooth {

constexpr uint32_t kMaxVerts = 0x7FFFFFFFu;
constexpr uint32_t kMaxFaces = 0x7FFFFFFFu / 6u;        // ring offsets up to 2 E <= 6 F are int32
constexpr uint32_t kNormalMaxFaces = 0x7FFFFFFFu / 3u;

typedef unsigned long long ull;

using bulk::up256;

// ---- the vertex ring ----------------------------------------------------------------------------------------------------------------

struct RingWork {                // views into the caller's workspace (nsa_mesh_ring_workspace bytes); H = 3 F
    uint32_t* keys[2];           // [H] each: radix ping-pong
    uint32_t* tmp;               // [H]
    uint32_t* order;             // [H]: edges sorted stably by hi, the positions past E last
    uint32_t* counts;            // [256 * 256]
    uint32_t* lo;                // [H]: lo of edge i, V past E
    uint32_t* hs;                // [H]: hi of edge order[i], V past E
    int32_t* below_lo;           // [V + 1]: #{lo < v}
    int32_t* below_hi;           // [V + 1]: #{hi < v}
};

__host__ __device__ inline uint64_t ring_carve(void* ws, uint32_t V, uint32_t F, RingWork* out) {
    const uint64_t H = 3ull * F;
    char* base = static_cast<char*>(ws);
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) { char* p = base ? base + o : nullptr; o += up256(bytes); return p; };
    RingWork w;
    w.keys[0] = reinterpret_cast<uint32_t*>(take(4 * H));
    w.keys[1] = reinterpret_cast<uint32_t*>(take(4 * H));
    w.tmp = reinterpret_cast<uint32_t*>(take(4 * H));
    w.order = reinterpret_cast<uint32_t*>(take(4 * H));
    w.counts = reinterpret_cast<uint32_t*>(take(4ull * kRadixCountWords));
    w.lo = reinterpret_cast<uint32_t*>(take(4 * H));
    w.hs = reinterpret_cast<uint32_t*>(take(4 * H));
    w.below_lo = reinterpret_cast<int32_t*>(take(4ull * ((uint64_t)V + 1)));
    w.below_hi = reinterpret_cast<int32_t*>(take(4ull * ((uint64_t)V + 1)));
    if (out) *out = w;
    return o;
}

// E as nsa_mesh_edges left it on the device, never above H
__device__ __forceinline__ uint32_t edges_on_device(const ull* __restrict__ edge_totals, uint32_t H) {
    const ull E = edge_totals[0];
    return E < H ? (uint32_t)E : H;
}

__global__ __launch_bounds__(256) void k_ring_keys(RingWork w, const int32_t* __restrict__ edges, const ull* __restrict__ edge_totals,
                                                   uint32_t H, uint32_t V) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H) return;
    const uint32_t E = edges_on_device(edge_totals, H);
    w.lo[i] = ring_key(edges, E, V, i, 0);
    w.keys[0][i] = ring_key(edges, E, V, i, 1);
}

__global__ __launch_bounds__(256) void k_ring_gather(RingWork w, const int32_t* __restrict__ edges, const ull* __restrict__ edge_totals,
                                                     uint32_t H, uint32_t V) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H) return;
    const uint32_t e = w.order[i];
    w.hs[i] = e < H ? ring_key(edges, edges_on_device(edge_totals, H), V, e, 1) : V;      // (always: the order is a permutation)
}

// one lane per v in [0, V]
__global__ __launch_bounds__(256) void k_ring_start(RingWork w, uint32_t H, uint32_t V, int32_t* __restrict__ ring_start) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v > V) return;
    ring_pass_start(w.lo, w.hs, H, v, w.below_lo, w.below_hi, ring_start);
}

__global__ __launch_bounds__(256) void k_ring_fill(RingWork w, const int32_t* __restrict__ edges, const ull* __restrict__ edge_totals,
                                                   uint32_t H, uint32_t V, int32_t* __restrict__ ring, int32_t* __restrict__ ring_edge) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H) return;
    ring_pass_fill(edges, edges_on_device(edge_totals, H), w.hs, w.order, w.below_lo, w.below_hi, H, V, 2u * H, i, ring, ring_edge);
}

// ---- smoothing ------------------------------------------------------------------------------------------------------------------------

struct SmoothWork {              // views into the caller's workspace (nsa_mesh_smooth_workspace bytes)
    double* pos[2];              // [3 V] each: the float64 positions, ping-pong
    int32_t* member;             // [6 F]: N'(v) at ring_start[v], in row order
    int32_t* count;              // [V]: |N'(v)|; 0 for a vertex that keeps its input
    uint8_t* state;              // [V]: live, on the boundary, moves
};

__host__ __device__ inline uint64_t smooth_carve(void* ws, uint32_t V, uint32_t F, SmoothWork* out) {
    char* base = static_cast<char*>(ws);
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) { char* p = base ? base + o : nullptr; o += up256(bytes); return p; };
    SmoothWork w;
    w.pos[0] = reinterpret_cast<double*>(take(24ull * V));
    w.pos[1] = reinterpret_cast<double*>(take(24ull * V));
    w.member = reinterpret_cast<int32_t*>(take(24ull * F));
    w.count = reinterpret_cast<int32_t*>(take(4ull * V));
    w.state = reinterpret_cast<uint8_t*>(take(V));
    if (out) *out = w;
    return o;
}

__global__ __launch_bounds__(256) void k_sm_state(SmoothWork w, const float* __restrict__ verts, const int32_t* __restrict__ ring_start,
                                                  const int32_t* __restrict__ ring_edge, const int32_t* __restrict__ edge_count,
                                                  const uint8_t* __restrict__ fixed, uint32_t V, uint32_t F, int boundary) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    w.state[v] = smooth_pass_state(verts, ring_start, ring_edge, edge_count, fixed, V, 6u * F, 3u * F, boundary, v, w.pos[0]);
}

__global__ __launch_bounds__(256) void k_sm_members(SmoothWork w, const int32_t* __restrict__ ring_start, const int32_t* __restrict__ ring,
                                                    const int32_t* __restrict__ ring_edge, const int32_t* __restrict__ edge_count,
                                                    uint32_t V, uint32_t F, int boundary, uint8_t* __restrict__ state_out) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    state_out[v] = smooth_pass_members(ring_start, ring, ring_edge, edge_count, w.state, V, 6u * F, 3u * F, boundary, v, w.member, w.count);
}

// one step, one lane per vertex; the last one rounds to fp32 and gives a vertex that keeps its input its input bits back
template <bool LAST>
__global__ __launch_bounds__(256) void k_sm_step(SmoothWork w, int from, const float* __restrict__ verts,
                                                 const int32_t* __restrict__ ring_start, uint32_t V, uint32_t F, double f, double max_move,
                                                 bool clamp, float* __restrict__ out) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    double y[3];
    const bool stepped = smooth_pass_step(w.pos[from], verts, ring_start, w.member, w.count, V, 6u * F, v, f, max_move, clamp, y);
    if (LAST) {
        const uint32_t* in = reinterpret_cast<const uint32_t*>(verts);
        uint32_t* o = reinterpret_cast<uint32_t*>(out);
#pragma unroll
        for (int k = 0; k < 3; ++k) o[3ull * v + k] = stepped ? __float_as_uint((float)y[k]) : in[3ull * v + k];
    } else {
        double* next = w.pos[from ^ 1];
#pragma unroll
        for (int k = 0; k < 3; ++k) next[3ull * v + k] = y[k];
    }
}

// out = the bits of verts; state = 0 where it is given
__global__ __launch_bounds__(256) void k_sm_copy(const float* __restrict__ verts, uint32_t V, float* __restrict__ out,
                                                 uint8_t* __restrict__ state) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const uint32_t* in = reinterpret_cast<const uint32_t*>(verts);
    uint32_t* o = reinterpret_cast<uint32_t*>(out);
#pragma unroll
    for (int k = 0; k < 3; ++k) o[3ull * v + k] = in[3ull * v + k];
    if (state) state[v] = 0;
}

// ---- vertex normals -------------------------------------------------------------------------------------------------------------------

struct NormalKey {
    const float* verts;
    const int32_t* faces;
    uint32_t V, F;
    __device__ uint32_t operator()(uint32_t c) const { return normal_corner_key(verts, V, faces, F, c); }
};

__global__ __launch_bounds__(256) void k_vn_normals(corners::Table t, const float* __restrict__ verts, uint32_t V,
                                                    const int32_t* __restrict__ faces, uint32_t F, int weighting,
                                                    float* __restrict__ normals) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    uint32_t s = t.start[v], e = t.start[v + 1];
    if (e > 3u * F || s > e) s = e = 0;                                   // (never: the offsets come from a search over 3 F keys)
    float n[3];
    normal_pass_vertex(verts, V, faces, F, t.corner, s, e, weighting, n);
#pragma unroll
    for (int k = 0; k < 3; ++k) normals[3ull * v + k] = n[k];
}

__global__ __launch_bounds__(256) void k_vn_zero(uint32_t V, float* __restrict__ normals) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) normals[3ull * v + k] = 0.0f;
}

}  // namespace smooth
}  // namespace nsa

extern "C" {

uint64_t nsa_mesh_ring_workspace(uint32_t n_verts, uint32_t n_faces) {
    if (n_faces == 0 || n_faces > nsa::smooth::kMaxFaces || n_verts > nsa::smooth::kMaxVerts) return 0;
    return nsa::smooth::ring_carve(nullptr, n_verts, n_faces, nullptr);
}

int nsa_mesh_ring(const int32_t* edges, const uint64_t* edge_totals, uint32_t n_verts, uint32_t n_faces, void* workspace,
                  int32_t* ring_start, int32_t* ring, int32_t* ring_edge, nsa_stream_t stream) {
    using namespace nsa;
    using namespace nsa::smooth;
    const uint32_t V = n_verts, F = n_faces;
    if (V > kMaxVerts || F > kMaxFaces) return NSA_EBADARG;
    if (F == 0) return NSA_OK;
    if (!edges || !edge_totals || !workspace || !ring_start || !ring || !ring_edge) return NSA_EBADARG;
    RingWork w;
    ring_carve(workspace, V, F, &w);
    const uint32_t H = 3u * F, nbh = (H + 255) / 256;
    uint32_t bits = 1;
    while ((1ull << bits) <= (uint64_t)V) ++bits;                          // keys are <= V
    const ull* tot = reinterpret_cast<const ull*>(edge_totals);
    hipStream_t s = (hipStream_t)stream;
    launch_begin();
    hipLaunchKernelGGL(k_ring_keys, dim3(nbh), dim3(256), 0, s, w, edges, tot, H, V);
    radix_argsort(w.keys, w.tmp, w.order, w.counts, H, 0, (bits + 7) / 8, stream);
    hipLaunchKernelGGL(k_ring_gather, dim3(nbh), dim3(256), 0, s, w, edges, tot, H, V);
    hipLaunchKernelGGL(k_ring_start, dim3(V / 256 + 1), dim3(256), 0, s, w, H, V, ring_start);
    hipLaunchKernelGGL(k_ring_fill, dim3(nbh), dim3(256), 0, s, w, edges, tot, H, V, ring, ring_edge);
    return launch_end();
}

uint64_t nsa_mesh_smooth_workspace(uint32_t n_verts, uint32_t n_faces) {
    if (n_verts == 0 || n_faces > nsa::smooth::kMaxFaces || n_verts > nsa::smooth::kMaxVerts) return 0;
    return nsa::smooth::smooth_carve(nullptr, n_verts, n_faces, nullptr);
}

int nsa_mesh_smooth(const float* verts, uint32_t n_verts, uint32_t n_faces, const int32_t* ring_start, const int32_t* ring,
                    const int32_t* ring_edge, const int32_t* edge_count, const uint8_t* fixed, const double* factors, uint32_t n_steps,
                    int boundary, double max_move, void* workspace, float* out, uint8_t* state, nsa_stream_t stream) {
    using namespace nsa;
    using namespace nsa::smooth;
    const uint32_t V = n_verts, F = n_faces;
    if (V > kMaxVerts || F > kMaxFaces) return NSA_EBADARG;
    if (boundary != kFree && boundary != kFixed && boundary != kCurve) return NSA_EBADARG;
    if (!(max_move > 0.0)) return NSA_EBADARG;                            // (a NaN fails too)
    if (n_steps && !factors) return NSA_EBADARG;
    for (uint32_t i = 0; i < n_steps; ++i)
        if (!(fabs(factors[i]) <= 1.0)) return NSA_EBADARG;
    if (V == 0) return NSA_OK;
    if (!verts || !out || !state || !workspace) return NSA_EBADARG;
    if (F && (!ring_start || !ring || !ring_edge || !edge_count)) return NSA_EBADARG;
    SmoothWork w;
    smooth_carve(workspace, V, F, &w);
    const uint32_t nbv = (V + 255) / 256;
    const bool clamp = max_move <= 1.7976931348623157e308;
    hipStream_t s = (hipStream_t)stream;
    launch_begin();
    if (F == 0) {                                                          // no rows: nothing is live
        hipLaunchKernelGGL(k_sm_copy, dim3(nbv), dim3(256), 0, s, verts, V, out, state);
        return launch_end();
    }
    hipLaunchKernelGGL(k_sm_state, dim3(nbv), dim3(256), 0, s, w, verts, ring_start, ring_edge, edge_count, fixed, V, F, boundary);
    hipLaunchKernelGGL(k_sm_members, dim3(nbv), dim3(256), 0, s, w, ring_start, ring, ring_edge, edge_count, V, F, boundary, state);
    if (n_steps == 0) hipLaunchKernelGGL(k_sm_copy, dim3(nbv), dim3(256), 0, s, verts, V, out, (uint8_t*)nullptr);
    for (uint32_t i = 0; i < n_steps; ++i) {
        const int from = (int)(i & 1u);
        if (i + 1 == n_steps)
            hipLaunchKernelGGL(k_sm_step<true>, dim3(nbv), dim3(256), 0, s, w, from, verts, ring_start, V, F, factors[i], max_move, clamp,
                               out);
        else
            hipLaunchKernelGGL(k_sm_step<false>, dim3(nbv), dim3(256), 0, s, w, from, verts, ring_start, V, F, factors[i], max_move, clamp,
                               out);
    }
    return launch_end();
}

uint64_t nsa_mesh_vertex_normals_workspace(uint32_t n_verts, uint32_t n_faces) {
    if (n_verts == 0 || n_faces == 0 || n_verts > nsa::smooth::kMaxVerts || n_faces > nsa::smooth::kNormalMaxFaces) return 0;
    return nsa::corners::carve(nullptr, n_verts, n_faces, nullptr);
}

int nsa_mesh_vertex_normals(const float* verts, uint32_t n_verts, const int32_t* faces, uint32_t n_faces, int weighting, void* workspace,
                            float* normals, nsa_stream_t stream) {
    using namespace nsa;
    using namespace nsa::smooth;
    const uint32_t V = n_verts, F = n_faces;
    if (V > kMaxVerts || F > kNormalMaxFaces) return NSA_EBADARG;
    if (weighting != kArea && weighting != kAngle) return NSA_EBADARG;
    if (V == 0) return NSA_OK;
    if (!verts || !normals || (F && (!faces || !workspace))) return NSA_EBADARG;
    const uint32_t nbv = (V + 255) / 256;
    hipStream_t s = (hipStream_t)stream;
    launch_begin();
    if (F == 0) {                                                          // no corner anywhere
        hipLaunchKernelGGL(k_vn_zero, dim3(nbv), dim3(256), 0, s, V, normals);
        return launch_end();
    }
    corners::Table t;
    corners::carve(workspace, V, F, &t);
    corners::build(NormalKey{verts, faces, V, F}, V, F, t, stream);
    hipLaunchKernelGGL(k_vn_normals, dim3(nbv), dim3(256), 0, s, t, verts, V, faces, F, weighting, normals);
    return launch_end();
}

}  // extern "C"
