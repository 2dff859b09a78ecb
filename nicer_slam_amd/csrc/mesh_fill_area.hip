// mesh_fill_area.hip -- minimum-area patches for the holes that are not star-shaped (C ABI Section 24).
// The bodies live in fill_area_passes.hpp, which also compiles as host C++; the kernels here are one lane, or one wave, per item.
//
// nsa_mesh_fill_area_plan is one workgroup: it classes the loops of Section 23 that the caller's mask selects and scans the sides of
// their tables.  nsa_mesh_fill_area_tables gathers the loops' positions and names (one lane per loop vertex), writes the chord mask
// and the start values (one lane per cell), then runs the interval programme one launch per diagonal d over the cells (i, i + d) of
// ALL tabled loops: below 64 candidates a cell is one lane, from 64 on it is one wave whose lanes stride j and merge their
// (value, j) minima by __shfl_xor.  The minimum is exact in any order (ties to the smaller j), so the two forms give the same bits.
// One workgroup then fixes the final classes and offsets, and emit is one lane per new face, descending from the root of its loop's
// choice tree to the node that carries its number.  The launch boundary is the only ordering between diagonals; no workgroup waits
// for another, and there are no atomics: every output is a function of the arguments alone.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/nicer_slam_amd.h"
#include "block_scan.hpp"
#include "grid_common.hpp"
#include "fill_area_passes.hpp"

namespace nsa {
namespace fill_area {

using scan::capped;
using scan::ull;

using bulk::up256;

constexpr uint32_t kMaxHalfedges = 0x7FFFFFFFu;
constexpr int kChannels = 6;

struct Work {                    // views into the caller's workspace: C cells, R rows
    double* W;                   // [C]
    double* WT;                  // [C]: W transposed inside every table
    double* pos;                 // [3 R]
    int32_t* J;                  // [C]
    uint32_t* row_loop;          // [R]
    int32_t* row_name;           // [R]
    uint8_t* mask;               // [C]
};

__host__ __device__ inline uint64_t carve(void* ws, uint64_t C, uint64_t R, Work* out) {
    char* base = static_cast<char*>(ws);
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) { char* p = base ? base + o : nullptr; o += up256(bytes); return p; };
    Work w;
    w.W = reinterpret_cast<double*>(take(8 * C));
    w.WT = reinterpret_cast<double*>(take(8 * C));
    w.pos = reinterpret_cast<double*>(take(24 * R));
    w.J = reinterpret_cast<int32_t*>(take(4 * C));
    w.row_loop = reinterpret_cast<uint32_t*>(take(4 * R));
    w.row_name = reinterpret_cast<int32_t*>(take(4 * R));
    w.mask = reinterpret_cast<uint8_t*>(take(C));
    if (out) *out = w;
    return o;
}

// channels: cells, plan faces, rows, selected, tabled, too many edges
__device__ __forceinline__ int64_t plan_row(const int64_t* loop_ints, uint32_t l, uint32_t class_mask, uint32_t cap, uint32_t B,
                                            ull (&v)[kChannels], ull* n_all) {
    uint64_t n = 0;
    const int64_t cls = plan_class(loop_ints, l, class_mask, cap, B, &n);
    v[0] = n * n;
    v[1] = n >= 3 ? n - 2 : 0;
    v[2] = n;
    v[3] = cls != kNotSelected ? 1 : 0;
    v[4] = n != 0 ? 1 : 0;
    v[5] = cls == kAreaTooManyEdges ? 1 : 0;
    *n_all = (ull)loop_ints[(ull)kLoopInts * l + 1];
    return cls;
}

__global__ __launch_bounds__(256) void k_fa_plan(const int64_t* __restrict__ loop_ints, const ull* __restrict__ fill_totals, uint32_t B,
                                                 uint32_t class_mask, uint32_t cap, int64_t* __restrict__ area_ints,
                                                 ull* __restrict__ plan_totals) {
    __shared__ ull biggest[256];
    const uint32_t t = threadIdx.x, L = capped(fill_totals[1], B), per = (L + 255) / 256;
    const uint32_t l0 = t * per < L ? t * per : L, l1 = l0 + per < L ? l0 + per : L;
    ull sum[kChannels], excl[kChannels], total[kChannels], v[kChannels], n_all, big = 0;
#pragma unroll
    for (int c = 0; c < kChannels; ++c) sum[c] = 0;
    for (uint32_t l = l0; l < l1; ++l) {
        plan_row(loop_ints, l, class_mask, cap, B, v, &n_all);
#pragma unroll
        for (int c = 0; c < kChannels; ++c) sum[c] += v[c];
        if (v[2] > big) big = v[2];
    }
    scan::lds_scan<kChannels, ull, 256>(sum, excl, total);
    for (uint32_t l = l0; l < l1; ++l) {
        const int64_t cls = plan_row(loop_ints, l, class_mask, cap, B, v, &n_all);
        int64_t* a = area_ints + (ull)kAreaInts * l;
        a[0] = cls;
        a[1] = (int64_t)n_all;
        a[2] = (int64_t)excl[0];
        a[3] = (int64_t)excl[1];
        a[4] = (int64_t)excl[2];
        a[5] = 0;
#pragma unroll
        for (int c = 0; c < kChannels; ++c) excl[c] += v[c];
    }
    biggest[t] = big;
    __syncthreads();
    if (t == 0) {
        for (uint32_t u = 1; u < 256; ++u)
            if (biggest[u] > big) big = biggest[u];
        plan_totals[0] = total[3];
        plan_totals[1] = total[4];
        plan_totals[2] = total[5];
        plan_totals[3] = total[0];
        plan_totals[4] = big;
        plan_totals[5] = total[1];
        plan_totals[6] = total[2];
        plan_totals[7] = 0;
    }
}

struct Args {                    // what every table kernel reads
    const int64_t* loop_ints;
    const int64_t* area_ints;
    const ull* fill_totals;
    uint32_t B;
    ull cells, rows;
    __device__ uint32_t L() const { return capped(fill_totals[1], B); }
};

__global__ __launch_bounds__(256) void k_fa_rows(Work w, Args a, Shape m, const int32_t* __restrict__ names,
                                                 const int32_t* __restrict__ order) {
    const ull r = (ull)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.rows) return;
    row_pass(m, names, order, a.B, a.loop_ints, a.area_ints, a.L(), a.cells, a.rows, r, w.row_loop, w.row_name, w.pos);
}

__global__ __launch_bounds__(256) void k_fa_mask(Work w, Args a, const int32_t* __restrict__ edges, const ull* __restrict__ edge_totals,
                                                 uint32_t max_edges) {
    const ull x = (ull)blockIdx.x * 256 + threadIdx.x;
    if (x >= a.cells) return;
    mask_pass(edges, capped(edge_totals[0], max_edges), a.loop_ints, a.area_ints, a.L(), a.B, a.cells, a.rows, w.row_name, x, w.mask, w.W,
              w.WT, w.J);
}

// diagonal d, fewer than kWaveCandidates candidates: one lane per row
__global__ __launch_bounds__(256) void k_fa_diag_lane(Work w, Args a, uint32_t d, double min_sin2) {
    const ull r = (ull)blockIdx.x * 256 + threadIdx.x;
    Table t;
    uint64_t i;
    if (!cell_of(a.loop_ints, a.area_ints, a.L(), a.B, a.cells, a.rows, w.row_loop, r, d, &t, &i)) return;
    double best;
    uint32_t bj;
    cell_scan(w.W, w.WT, w.pos, t, i, i + d, i + 1, 1, min_sin2, &best, &bj);
    cell_store(t, i, i + d, best, bj, w.mask, w.W, w.WT, w.J);
}

// diagonal d, at least kWaveCandidates candidates: one wave per row, the lanes striding j
__global__ __launch_bounds__(256) void k_fa_diag_wave(Work w, Args a, uint32_t d, double min_sin2) {
    const uint32_t lane = threadIdx.x & 63u;
    const ull r = (ull)blockIdx.x * 4 + (threadIdx.x >> 6);
    Table t;
    uint64_t i;
    if (!cell_of(a.loop_ints, a.area_ints, a.L(), a.B, a.cells, a.rows, w.row_loop, r, d, &t, &i)) return;      // (uniform in the wave)
    double best;
    uint32_t bj;
    cell_scan(w.W, w.WT, w.pos, t, i, i + d, i + 1 + lane, 64, min_sin2, &best, &bj);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const double ob = __shfl_xor(best, s, 64);
        const uint32_t oj = (uint32_t)__shfl_xor((int)bj, s, 64);
        if (beats(ob, oj, best, bj)) {
            best = ob;
            bj = oj;
        }
    }
    if (lane == 0) cell_store(t, i, i + d, best, bj, w.mask, w.W, w.WT, w.J);
}

// one workgroup: the final classes, the final face offsets and totals, the areas
__global__ __launch_bounds__(256) void k_fa_finish(Work w, Args a, int64_t* area_ints, double* __restrict__ area,
                                                   ull* __restrict__ final_totals) {      // (area_ints is a.area_ints: every lane
                                                                                          // writes columns 0 and 5 of its own rows)
    const uint32_t t = threadIdx.x, L = a.L(), per = (L + 255) / 256;
    const uint32_t l0 = t * per < L ? t * per : L, l1 = l0 + per < L ? l0 + per : L;
    ull sum[4] = {0, 0, 0, 0}, excl[4], total[4];
    auto row = [&](uint32_t l, ull (&v)[4], double* ar) {
        const int64_t cls = final_class(a.loop_ints, a.area_ints, L, a.B, a.cells, a.rows, w.W, l, ar);
        const ull n = (ull)a.area_ints[(ull)kAreaInts * l + 1];
        v[0] = cls == kAreaFilled ? n - 2 : 0;
        v[1] = cls == kAreaFilled ? 1 : 0;
        v[2] = cls == kAreaTooManyEdges ? 1 : 0;
        v[3] = cls == kNoTriangulation ? 1 : 0;
        return cls;
    };
    ull v[4];
    double ar;
    for (uint32_t l = l0; l < l1; ++l) {
        row(l, v, &ar);
#pragma unroll
        for (int c = 0; c < 4; ++c) sum[c] += v[c];
    }
    scan::lds_scan<4, ull, 256>(sum, excl, total);
    for (uint32_t l = l0; l < l1; ++l) {
        const int64_t cls = row(l, v, &ar);
        area[l] = ar;
        area_ints[(ull)kAreaInts * l] = cls;
        area_ints[(ull)kAreaInts * l + 5] = (int64_t)excl[0];
        excl[0] += v[0];
    }
    if (t == 0) {
        final_totals[0] = total[1];
        final_totals[1] = total[2];
        final_totals[2] = total[3];
        final_totals[3] = total[0];
    }
}

__global__ __launch_bounds__(256) void k_fa_emit(Work w, Args a, Shape m, const int32_t* __restrict__ order, ull NF,
                                                 int32_t* __restrict__ new_faces) {
    const ull x = (ull)blockIdx.x * 256 + threadIdx.x;
    if (x >= NF) return;
    emit_pass(m, order, a.B, a.loop_ints, a.area_ints, a.L(), a.cells, a.rows, w.J, NF, x, new_faces);
}

// the square root the weights use, on its own: what the test of its rounding calls
__global__ __launch_bounds__(256) void k_fa_roots(const double* __restrict__ x, ull n, double* __restrict__ out) {
    const ull i = (ull)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = root(x[i]);
}

inline bool counts_ok(uint32_t V, uint32_t F, uint32_t B) { return V <= 0x7FFFFFFFu && 3ull * F <= kMaxHalfedges && B <= 3ull * F; }

// (cells, rows) are sums of n^2 and n over loops of at most kMaxAreaEdges edges that share no boundary half-edge
inline bool sizes_ok(uint64_t cells, uint64_t rows, uint32_t max_n) {
    return max_n <= kMaxAreaEdges && rows <= kMaxHalfedges && cells <= rows * (uint64_t)kMaxAreaEdges && cells >= rows;
}

}  // namespace fill_area
}  // namespace nsa

extern "C" {

int nsa_mesh_fill_area_plan(const int64_t* loop_ints, const uint64_t* fill_totals, uint32_t n_faces, uint32_t n_boundary,
                            uint32_t class_mask, uint32_t max_area_edges, int64_t* area_ints, uint64_t* plan_totals, nsa_stream_t stream) {
    using namespace nsa;
    using namespace nsa::fill_area;
    if (!counts_ok(0, n_faces, n_boundary)) return NSA_EBADARG;
    if (max_area_edges == 0 || max_area_edges > kMaxAreaEdges || class_mask >= (1u << fill::kClasses)) return NSA_EBADARG;
    if (n_faces == 0 || n_boundary == 0) return NSA_OK;
    if (!loop_ints || !fill_totals || !area_ints || !plan_totals) return NSA_EBADARG;
    launch_begin();
    hipLaunchKernelGGL(k_fa_plan, dim3(1), dim3(256), 0, (hipStream_t)stream, loop_ints, reinterpret_cast<const ull*>(fill_totals),
                       n_boundary, class_mask, max_area_edges, area_ints, reinterpret_cast<ull*>(plan_totals));
    return launch_end();
}

uint64_t nsa_mesh_fill_area_workspace(uint64_t n_cells, uint64_t n_rows) {
    if (n_cells == 0 || n_rows == 0 || !nsa::fill_area::sizes_ok(n_cells, n_rows, 0)) return 0;
    return nsa::fill_area::carve(nullptr, n_cells, n_rows, nullptr);
}

int nsa_mesh_fill_area_tables(const float* verts, uint32_t n_verts, const int32_t* faces, const int32_t* names, uint32_t n_faces,
                              const int32_t* edges, const uint64_t* edge_totals, const int32_t* order, uint32_t n_boundary,
                              const int64_t* loop_ints, const uint64_t* fill_totals, int64_t* area_ints, uint64_t n_cells, uint64_t n_rows,
                              uint32_t max_n, uint64_t n_new_faces, double min_sin2, void* workspace, double* area, int32_t* new_faces,
                              uint64_t* final_totals, nsa_stream_t stream) {
    using namespace nsa;
    using namespace nsa::fill_area;
    const uint32_t V = n_verts, F = n_faces, B = n_boundary;
    if (!counts_ok(V, F, B)) return NSA_EBADARG;
    if (!(min_sin2 >= 0.0)) return NSA_EBADARG;
    if (n_cells == 0 && n_rows == 0 && max_n == 0 && n_new_faces == 0) return NSA_OK;
    if (max_n < 3 || !sizes_ok(n_cells, n_rows, max_n) || n_rows > B || n_new_faces > n_rows || n_cells < (uint64_t)max_n * max_n)
        return NSA_EBADARG;
    if (F == 0 || B == 0) return NSA_EBADARG;
    if (!verts || !faces || !edges || !edge_totals || !order || !loop_ints || !fill_totals || !area_ints || !workspace || !area ||
        !new_faces || !final_totals)
        return NSA_EBADARG;
    Work w;
    carve(workspace, n_cells, n_rows, &w);
    const Args a{loop_ints, area_ints, reinterpret_cast<const ull*>(fill_totals), B, (ull)n_cells, (ull)n_rows};
    const Shape m{verts, nullptr, faces, V, F};
    hipStream_t s = (hipStream_t)stream;
    const uint32_t row_blocks = (uint32_t)((n_rows + 255) / 256), wave_blocks = (uint32_t)((n_rows + 3) / 4);
    launch_begin();
    hipLaunchKernelGGL(k_fa_rows, dim3(row_blocks), dim3(256), 0, s, w, a, m, names ? names : faces, order);
    hipLaunchKernelGGL(k_fa_mask, dim3((uint32_t)((n_cells + 255) / 256)), dim3(256), 0, s, w, a, edges,
                       reinterpret_cast<const ull*>(edge_totals), 3u * F);
    for (uint32_t d = 2; d < max_n; ++d) {
        if (d - 1 < kWaveCandidates) hipLaunchKernelGGL(k_fa_diag_lane, dim3(row_blocks), dim3(256), 0, s, w, a, d, min_sin2);
        else hipLaunchKernelGGL(k_fa_diag_wave, dim3(wave_blocks), dim3(256), 0, s, w, a, d, min_sin2);
    }
    hipLaunchKernelGGL(k_fa_finish, dim3(1), dim3(256), 0, s, w, a, area_ints, area, reinterpret_cast<ull*>(final_totals));
    if (n_new_faces)
        hipLaunchKernelGGL(k_fa_emit, dim3((uint32_t)((n_new_faces + 255) / 256)), dim3(256), 0, s, w, a, m, order, (ull)n_new_faces,
                           new_faces);
    return launch_end();
}

int nsa_mesh_fill_area_roots(const double* x, uint64_t n, double* out, nsa_stream_t stream) {
    using namespace nsa;
    using namespace nsa::fill_area;
    if (n > 0x7FFFFFFFull * 256) return NSA_EBADARG;
    if (n == 0) return NSA_OK;
    if (!x || !out) return NSA_EBADARG;
    launch_begin();
    hipLaunchKernelGGL(k_fa_roots, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, (ull)n, out);
    return launch_end();
}

}  // extern "C"
