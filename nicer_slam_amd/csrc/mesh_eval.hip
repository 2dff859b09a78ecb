// mesh_eval.hip -- exact nearest neighbours between point clouds and area-weighted surface sampling on the device.
// Reference: code/evaluation/eval_rec.py -- scipy cKDTree queries (:18, :111, :172-186), open3d's KDTreeFlann hybrid search
// inside registration_icp (:197-203) and trimesh.sample.sample_surface (:158, :222, :225).
//
// Nearest neighbour.  For a query q and targets t_i the distance is the fp32 value
//     d2(q, t_i) = (dx * dx + dy * dy) + dz * dz,   dk = t_ik - q_k,   every operation rounded on its own (no FMA contraction)
// and the answer is the smallest d2, ties to the lowest target index; dist = the correctly rounded fp32 sqrt(d2).  Any fp32 brute force with this
// operation order reproduces (idx, dist) bit for bit.  Targets with a non-finite coordinate are never returned; a non-finite query
// gives (-1, NaN).  With a radius, a target is accepted only if d2 < r2 = (float)(max_dist * max_dist) (strict, as the radius
// search of open3d's SearchHybrid); a query with none gives (-1, +inf).
//
// Index (built once, reused by every query batch): the grid of bulk_grid.hpp, at most B = min(2n, 2^22) cells over the bulk of the
// targets.  k_nn_bounds (one workgroup) takes the bounding box of all finite targets and, from a strided subsample of 2048, the
// 1/64 and 63/64 per-axis quantiles ("bulk"); cells are near-cubic over the bulk, at most 1024 per axis, and every target outside
// the bulk is clamped into a border cell.  k_nn_keys gives each target its cell (non-finite: the sentinel cell `ncells`), the radix
// argsort of map_tail.hip orders them stably, k_nn_gather writes the sorted points (x, y, z, index bits) and keys, and k_nn_cells
// writes each cell's first sorted position (binary search) and the bounding box of the points actually in it.
//
// Query (k_nn_query, one lane per query): rings of cells at Chebyshev index distance r = 0, 1, 2, ... around the query's
// (clamped) cell.  A cell is skipped when its box distance, computed in fp32 with the same operation order, exceeds the current
// best: rounding is monotone, so that bound is never above the fp32 d2 of any point in the box, and a cell that could tie is
// always read.  The ring walk stops when a float64 lower bound on the distance to every cell at index distance >= r exceeds the
// best by a relative 2^-18 (the fp32 d2 is within 2^-21 of the exact value): per axis and side, the cell plane at the ring less a
// margin of 2^-9 cell (the fp32 cell index is off by less than 2^-12 cell), combined with the query's distance to the targets'
// bounding box on the other axes.  Clamped targets only lie beyond the border planes, so the bound holds for them too.
// Worst case: every target in one cell (exact duplicates) -- each query reads all n points.
// k_nn_query_k (C ABI Section 28) walks the same rings for the k smallest under the total order (d2, index).
//
// Surface sampling (trimesh.sample.sample_surface): areas 0.5 |(v1 - v0) x (v2 - v0)| in float64; a sequential inclusive scan
// in LDS per block of 1024 faces (k_area_scan; the blocks in parallel) and a sequential carry over the blocks (k_area_offsets)
// give cum[f] = boff[b] + local[f], which is non-decreasing (each step adds a non-negative value; rounding is monotone).  Sample s draws Philox4x32-10 (key = seed, counter = (s, 0, 0, 0)); face = first f with cum[f] >= u * total,
// u = ((c0 >> 8) + 1) 2^-24 in (0, 1], so zero-area faces are never picked; (a, b) = the engine's u01 of c1, c2, reflected to
// (1 - a, 1 - b) when a + b > 1 in fp32; point = (v0 + a (v1 - v0)) + b (v2 - v0) in fp32, each operation rounded on its own.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/nicer_slam_amd.h"
#include "bulk_grid.hpp"
#include "draw_common.hpp"
#include "grid_common.hpp"
#include "mesh_area.hpp"
#include "normals_passes.hpp"
#include "radix_sort.hpp"

namespace nsa {

using bulk::axis_cell;
using bulk::block_reduce;
using bulk::finite3;
using bulk::lower_bound;
using bulk::up256;

constexpr uint32_t kMaxCount = 0x7FFFFFFFu;

using NnGrid = bulk::Grid;       // written by k_nn_bounds, read by every later kernel of the build and by k_nn_query; gmin / gmax: the
                                 // bounding box of the finite targets

struct NnIndex {                 // views into the caller's index buffer (nsa_nn_workspace bytes)
    NnGrid* grid;
    uint32_t* start;             // [B + 2]: first sorted position of cell c; cell c is [start[c], start[c + 1])
    float* box;                  // [B][6]: min xyz, max xyz of the points in the cell
    float4* spts;                // [n]: sorted points, w = target index bits
    uint32_t* skey;              // [n]: sorted cell keys
    uint32_t* keys[2];           // [n] each: radix ping-pong
    uint32_t* tmp;               // [n]
    uint32_t* order;             // [n]
    uint32_t* counts;            // [256 * 256]
};

__host__ __device__ inline uint32_t nn_budget(uint32_t n) {
    const uint64_t b = 2ull * n;
    return (uint32_t)(b < 1 ? 1 : (b > bulk::kMaxCells ? bulk::kMaxCells : b));
}

__host__ __device__ inline uint64_t nn_carve(void* ws, uint32_t n, NnIndex* out) {
    const uint32_t B = nn_budget(n);
    char* base = static_cast<char*>(ws);
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) { char* p = base ? base + o : nullptr; o += up256(bytes); return p; };
    NnIndex x;
    x.grid = reinterpret_cast<NnGrid*>(take(sizeof(NnGrid)));
    x.start = reinterpret_cast<uint32_t*>(take(4ull * (B + 2)));
    x.box = reinterpret_cast<float*>(take(24ull * B));
    x.spts = reinterpret_cast<float4*>(take(16ull * n));
    x.skey = reinterpret_cast<uint32_t*>(take(4ull * n));
    x.keys[0] = reinterpret_cast<uint32_t*>(take(4ull * n));
    x.keys[1] = reinterpret_cast<uint32_t*>(take(4ull * n));
    x.tmp = reinterpret_cast<uint32_t*>(take(4ull * n));
    x.order = reinterpret_cast<uint32_t*>(take(4ull * n));
    x.counts = reinterpret_cast<uint32_t*>(take(4ull * kRadixCountWords));
    if (out) *out = x;
    return o;
}

__device__ __forceinline__ uint32_t cell_key(const NnGrid& g, float x, float y, float z) {
    if (!finite3(x, y, z)) return g.ncells;
    const uint32_t cx = axis_cell(x, g.lo[0], g.inv_h[0], g.R[0]), cy = axis_cell(y, g.lo[1], g.inv_h[1], g.R[1]),
                   cz = axis_cell(z, g.lo[2], g.inv_h[2], g.R[2]);
    return (cx * g.R[1] + cy) * g.R[2] + cz;
}

__global__ __launch_bounds__(1024) void k_nn_bounds(const float* __restrict__ t, uint32_t n, uint32_t budget, NnIndex ix) {
    __shared__ float sv[3][bulk::kSubsample];
    __shared__ float red[16];
    __shared__ uint32_t redu[16];
    __shared__ float s_bulk[2][3];
    const uint32_t tid = threadIdx.x;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t i = tid; i < n; i += 1024) {
        const float x = t[3ull * i], y = t[3ull * i + 1], z = t[3ull * i + 2];
        if (!finite3(x, y, z)) continue;
        mn[0] = fminf(mn[0], x); mn[1] = fminf(mn[1], y); mn[2] = fminf(mn[2], z);
        mx[0] = fmaxf(mx[0], x); mx[1] = fmaxf(mx[1], y); mx[2] = fmaxf(mx[2], z);
    }
    float gmin[3], gmax[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        gmin[k] = block_reduce(mn[k], [](float a, float b) { return fminf(a, b); }, red);
        gmax[k] = block_reduce(mx[k], [](float a, float b) { return fmaxf(a, b); }, red);
    }
    // strided subsample; non-finite points are left out of the ranking (+inf and not counted)
    const uint32_t m = n < bulk::kSubsample ? n : bulk::kSubsample;
    uint32_t nf = 0;
    for (uint32_t j = tid; j < bulk::kSubsample; j += 1024) {
        bool ok = false;
        float x = INFINITY, y = INFINITY, z = INFINITY;
        if (j < m) {
            const uint64_t i = (uint64_t)j * n / m;
            x = t[3 * i]; y = t[3 * i + 1]; z = t[3 * i + 2];
            ok = finite3(x, y, z);
        }
        sv[0][j] = ok ? x : INFINITY;
        sv[1][j] = ok ? y : INFINITY;
        sv[2][j] = ok ? z : INFINITY;
        nf += ok;
    }
    const uint32_t m_f = block_reduce(nf, [](uint32_t a, uint32_t b) { return a + b; }, redu);
    bulk::rank_bulk(sv, m, m_f, s_bulk);
    if (tid != 0) return;
    NnGrid g;
    bulk::solve(s_bulk[0], s_bulk[1], m_f, budget, g);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        g.gmin[k] = gmin[k];
        g.gmax[k] = gmax[k];
    }
    *ix.grid = g;
}

__global__ __launch_bounds__(256) void k_nn_keys(const float* __restrict__ t, uint32_t n, NnIndex ix) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const NnGrid& g = *ix.grid;
    ix.keys[0][i] = cell_key(g, t[3ull * i], t[3ull * i + 1], t[3ull * i + 2]);
}

__global__ __launch_bounds__(256) void k_nn_gather(const float* __restrict__ t, uint32_t n, NnIndex ix) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const NnGrid& g = *ix.grid;
    const uint32_t p = ix.order[i];
    const float x = t[3ull * p], y = t[3ull * p + 1], z = t[3ull * p + 2];
    ix.spts[i] = make_float4(x, y, z, __uint_as_float(p));
    ix.skey[i] = cell_key(g, x, y, z);
}

// one lane per cell c in [0, ncells + 1]: start[c], and the box of the points of cell c < ncells
__global__ __launch_bounds__(256) void k_nn_cells(uint32_t n, NnIndex ix) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    const uint32_t ncells = ix.grid->ncells;
    if (c > ncells + 1) return;
    const uint32_t s = lower_bound(ix.skey, n, c);
    ix.start[c] = s;
    if (c >= ncells) return;
    const uint32_t e = lower_bound(ix.skey, n, c + 1);
    float b[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (uint32_t i = s; i < e; ++i) {
        const float4 p = ix.spts[i];
        b[0] = fminf(b[0], p.x); b[1] = fminf(b[1], p.y); b[2] = fminf(b[2], p.z);
        b[3] = fmaxf(b[3], p.x); b[4] = fmaxf(b[4], p.y); b[5] = fmaxf(b[5], p.z);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) ix.box[6ull * c + k] = b[k];
}

struct NnBest {
    float d2;
    int32_t idx;
    bool strict;                 // radius form: a first candidate must be strictly inside r2
};

__device__ __forceinline__ void nn_take(NnBest& b, float d2, int32_t idx) {
    if (d2 < b.d2 || (d2 == b.d2 && (b.idx < 0 ? !b.strict : idx < b.idx))) {
        b.d2 = d2;
        b.idx = idx;
    }
}

__device__ __forceinline__ float sq_dist(float ax, float ay, float az, float qx, float qy, float qz) {
#pragma clang fp contract(off)
    const float dx = ax - qx, dy = ay - qy, dz = az - qz;
    return (dx * dx + dy * dy) + dz * dz;
}

// the correctly rounded fp32 square root: float64 sqrt (correctly rounded) then one rounding to fp32, which is exact for sqrt
// (53 >= 2 * 24 + 2).  (__fsqrt_rn lowers to a bare v_sqrt_f32 on gfx950, which is not correctly rounded.)
__device__ __forceinline__ float sqrt_rn(float x) { return (float)sqrt((double)x); }

__device__ __forceinline__ float box_gap(float q, float lo, float hi) {
#pragma clang fp contract(off)
    return q < lo ? lo - q : (q > hi ? q - hi : 0.0f);
}

__device__ __forceinline__ void nn_visit(const NnIndex& ix, uint32_t c, float qx, float qy, float qz, NnBest& b) {
#pragma clang fp contract(off)
    const uint32_t s = ix.start[c], e = ix.start[c + 1];
    if (s == e) return;
    const float* bx = ix.box + 6ull * c;
    const float gx = box_gap(qx, bx[0], bx[3]), gy = box_gap(qy, bx[1], bx[4]), gz = box_gap(qz, bx[2], bx[5]);
    if ((gx * gx + gy * gy) + gz * gz > b.d2) return;
    for (uint32_t i = s; i < e; ++i) {
        const float4 p = ix.spts[i];
        nn_take(b, sq_dist(p.x, p.y, p.z, qx, qy, qz), (int32_t)__float_as_uint(p.w));
    }
}

__global__ __launch_bounds__(256) void k_nn_query(NnIndex ix, const float* __restrict__ q, uint32_t m, float r2, bool strict,
                                                  int32_t* __restrict__ out_idx, float* __restrict__ out_dist) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const float qx = q[3ull * j], qy = q[3ull * j + 1], qz = q[3ull * j + 2];
    const NnGrid g = *ix.grid;
    if (!finite3(qx, qy, qz)) {
        out_idx[j] = -1;
        out_dist[j] = __builtin_nanf("");
        return;
    }
    NnBest b{r2, -1, strict};
    if (ix.start[g.ncells] > 0) {                      // some target is finite
        const float qv[3] = {qx, qy, qz};
        int c0[3];
        double out2[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            c0[k] = (int)axis_cell(qv[k], g.lo[k], g.inv_h[k], g.R[k]);
            const double o = fmax(fmax((double)g.gmin[k] - qv[k], (double)qv[k] - g.gmax[k]), 0.0);
            out2[k] = o * o;
        }
        const int R0 = (int)g.R[0], R1 = (int)g.R[1], R2 = (int)g.R[2];
        for (int r = 0;; ++r) {
            if (r > 0) {                                // lower bound over every cell at index distance >= r
                double lb2 = INFINITY;
                bool any = false;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double h = g.h[k], margin = h * 0x1p-9, lo = g.lo[k], qk = qv[k];
                    const double rest = out2[0] + out2[1] + out2[2] - out2[k];
                    const double ok = sqrt(out2[k]);
                    if (c0[k] + r <= (int)g.R[k] - 1) {
                        const double gap = fmax(fmax(lo + (double)(c0[k] + r) * h - qk - margin, ok), 0.0);
                        lb2 = fmin(lb2, gap * gap + rest);
                        any = true;
                    }
                    if (c0[k] - r >= 0) {
                        const double gap = fmax(fmax(qk - (lo + (double)(c0[k] - r + 1) * h) - margin, ok), 0.0);
                        lb2 = fmin(lb2, gap * gap + rest);
                        any = true;
                    }
                }
                if (!any || lb2 > (double)b.d2 * (1.0 + 0x1p-18)) break;
            }
            const int x0 = max(c0[0] - r, 0), x1 = min(c0[0] + r, R0 - 1);
            const int y0 = max(c0[1] - r, 0), y1 = min(c0[1] + r, R1 - 1);
            const int z0 = max(c0[2] - r, 0), z1 = min(c0[2] + r, R2 - 1);
            for (int x = x0; x <= x1; ++x) {
                const bool ex = x == c0[0] - r || x == c0[0] + r;
                for (int y = y0; y <= y1; ++y) {
                    const uint32_t row = ((uint32_t)x * g.R[1] + (uint32_t)y) * g.R[2];
                    if (ex || y == c0[1] - r || y == c0[1] + r) {
                        for (int z = z0; z <= z1; ++z) nn_visit(ix, row + z, qx, qy, qz, b);
                    } else {
                        if (c0[2] - r >= 0) nn_visit(ix, row + (c0[2] - r), qx, qy, qz, b);
                        if (r > 0 && c0[2] + r < R2) nn_visit(ix, row + (c0[2] + r), qx, qy, qz, b);
                    }
                }
            }
        }
    }
    out_idx[j] = b.idx;
    out_dist[j] = b.idx >= 0 ? sqrt_rn(b.d2) : INFINITY;
}

// ---- k nearest neighbours (header Section 28) ---------------------------------------------------------------------------
// The ring walk of k_nn_query with the k-th best in the place of the best: until k candidates are held the bound is r2.  Each lane keeps
// its candidates as 64-bit keys (normals_passes.hpp), ascending, in LDS: slot-major, s_keys[slot][lane], one wave per workgroup, so the
// lanes of a wave touch 64 different columns whatever slot each of them is at.  CAP slots: 8 bytes * 64 lanes * CAP per workgroup.

__device__ __forceinline__ void nn_visit_k(const NnIndex& ix, uint32_t c, float qx, float qy, float qz, uint64_t* keys, uint32_t k,
                                           uint32_t& held, uint64_t& worst, float r2, bool strict) {
#pragma clang fp contract(off)
    const uint32_t s = ix.start[c], e = ix.start[c + 1];
    if (s == e) return;
    const float* bx = ix.box + 6ull * c;
    const float gx = box_gap(qx, bx[0], bx[3]), gy = box_gap(qy, bx[1], bx[4]), gz = box_gap(qz, bx[2], bx[5]);
    if ((gx * gx + gy * gy) + gz * gz > cn::knn_bound(held, k, worst, r2)) return;
    for (uint32_t i = s; i < e; ++i) {
        const float4 p = ix.spts[i];
        cn::knn_offer(keys, 64, k, held, worst, sq_dist(p.x, p.y, p.z, qx, qy, qz), __float_as_uint(p.w), r2, strict);
    }
}

template <uint32_t CAP>
__global__ __launch_bounds__(64) void k_nn_query_k(NnIndex ix, const float* __restrict__ q, uint32_t m, uint32_t k, float r2, bool strict,
                                                   int32_t* __restrict__ out_idx, float* __restrict__ out_dist,
                                                   uint32_t* __restrict__ out_count) {
    __shared__ uint64_t s_keys[CAP * 64];
    const uint32_t j = blockIdx.x * 64 + threadIdx.x;
    if (j >= m) return;
    uint64_t* keys = s_keys + threadIdx.x;
    const float qx = q[3ull * j], qy = q[3ull * j + 1], qz = q[3ull * j + 2];
    const NnGrid g = *ix.grid;
    int32_t* oi = out_idx + (uint64_t)j * k;
    float* od = out_dist + (uint64_t)j * k;
    if (!finite3(qx, qy, qz)) {
        for (uint32_t s = 0; s < k; ++s) {
            oi[s] = -1;
            od[s] = __builtin_nanf("");
        }
        out_count[j] = 0;
        return;
    }
    uint32_t held = 0;
    uint64_t worst = 0;
    if (ix.start[g.ncells] > 0) {                      // some target is finite
        const float qv[3] = {qx, qy, qz};
        int c0[3];
        double out2[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            c0[a] = (int)axis_cell(qv[a], g.lo[a], g.inv_h[a], g.R[a]);
            const double o = fmax(fmax((double)g.gmin[a] - qv[a], (double)qv[a] - g.gmax[a]), 0.0);
            out2[a] = o * o;
        }
        const int R0 = (int)g.R[0], R1 = (int)g.R[1], R2 = (int)g.R[2];
        for (int r = 0;; ++r) {
            if (r > 0) {                                // lower bound over every cell at index distance >= r (as k_nn_query)
                double lb2 = INFINITY;
                bool any = false;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const double h = g.h[a], margin = h * 0x1p-9, lo = g.lo[a], qk = qv[a];
                    const double rest = out2[0] + out2[1] + out2[2] - out2[a];
                    const double ok = sqrt(out2[a]);
                    if (c0[a] + r <= (int)g.R[a] - 1) {
                        const double gap = fmax(fmax(lo + (double)(c0[a] + r) * h - qk - margin, ok), 0.0);
                        lb2 = fmin(lb2, gap * gap + rest);
                        any = true;
                    }
                    if (c0[a] - r >= 0) {
                        const double gap = fmax(fmax(qk - (lo + (double)(c0[a] - r + 1) * h) - margin, ok), 0.0);
                        lb2 = fmin(lb2, gap * gap + rest);
                        any = true;
                    }
                }
                if (!any || lb2 > (double)cn::knn_bound(held, k, worst, r2) * (1.0 + 0x1p-18)) break;
            }
            const int x0 = max(c0[0] - r, 0), x1 = min(c0[0] + r, R0 - 1);
            const int y0 = max(c0[1] - r, 0), y1 = min(c0[1] + r, R1 - 1);
            const int z0 = max(c0[2] - r, 0), z1 = min(c0[2] + r, R2 - 1);
            for (int x = x0; x <= x1; ++x) {
                const bool ex = x == c0[0] - r || x == c0[0] + r;
                for (int y = y0; y <= y1; ++y) {
                    const uint32_t row = ((uint32_t)x * g.R[1] + (uint32_t)y) * g.R[2];
                    if (ex || y == c0[1] - r || y == c0[1] + r) {
                        for (int z = z0; z <= z1; ++z) nn_visit_k(ix, row + z, qx, qy, qz, keys, k, held, worst, r2, strict);
                    } else {
                        if (c0[2] - r >= 0) nn_visit_k(ix, row + (c0[2] - r), qx, qy, qz, keys, k, held, worst, r2, strict);
                        if (r > 0 && c0[2] + r < R2) nn_visit_k(ix, row + (c0[2] + r), qx, qy, qz, keys, k, held, worst, r2, strict);
                    }
                }
            }
        }
    }
    for (uint32_t s = 0; s < k; ++s) {
        const uint64_t key = s < held ? keys[s * 64] : 0;
        oi[s] = s < held ? (int32_t)(uint32_t)key : -1;
        od[s] = s < held ? cn::knn_root(__uint_as_float((uint32_t)(key >> 32))) : INFINITY;
    }
    out_count[j] = held;
}

// ---- surface sampling ---------------------------------------------------------------------------------------------------------

constexpr uint32_t kAreaBlock = 1024;

struct SampleWork {              // views into the caller's workspace (nsa_surface_sample_workspace bytes)
    double* local;               // [F] inclusive scan of the areas within each block of 1024 faces
    double* btot;                // [nb] block totals
    double* boff;                // [nb + 1] exclusive block offsets; boff[nb] = total
};

__host__ __device__ inline uint64_t sample_carve(void* ws, uint32_t F, SampleWork* out) {
    const uint64_t nb = (F + kAreaBlock - 1) / kAreaBlock;
    char* base = static_cast<char*>(ws);
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) { char* p = base ? base + o : nullptr; o += up256(bytes); return p; };
    SampleWork w;
    w.local = reinterpret_cast<double*>(take(8ull * F));
    w.btot = reinterpret_cast<double*>(take(8ull * nb));
    w.boff = reinterpret_cast<double*>(take(8ull * (nb + 1)));
    if (out) *out = w;
    return o;
}

__global__ __launch_bounds__(1024) void k_area_scan(const float* __restrict__ v, uint32_t V, const int32_t* __restrict__ f,
                                                    uint32_t F, SampleWork w) {
    __shared__ double s[kAreaBlock];
    const uint32_t t = threadIdx.x, i = blockIdx.x * kAreaBlock + t;
    s[t] = i < F ? face_area(v, V, f, i) : 0.0;
    __syncthreads();
    if (t == 0) {         // sequential, so that local[] is non-decreasing (a tree scan's partial sums need not be)
        double c = 0.0;
        for (uint32_t k = 0; k < kAreaBlock; ++k) {
            c = c + s[k];
            s[k] = c;
        }
    }
    __syncthreads();
    if (i < F) w.local[i] = s[t];
    if (t == kAreaBlock - 1) w.btot[blockIdx.x] = s[t];
}

// one lane: boff[b + 1] = boff[b] + btot[b] in block order, so cum[f] = boff[b] + local[f] is non-decreasing over all faces
__global__ __launch_bounds__(64) void k_area_offsets(SampleWork w, uint32_t nb, double* __restrict__ total) {
    if (threadIdx.x != 0) return;
    double c = 0.0;
    for (uint32_t b = 0; b < nb; ++b) {
        w.boff[b] = c;
        c = c + w.btot[b];
    }
    w.boff[nb] = c;
    if (total) *total = c;
}

__global__ __launch_bounds__(256) void k_sample(const float* __restrict__ v, const int32_t* __restrict__ f, uint32_t V, uint32_t F,
                                                SampleWork w, uint32_t nb, uint32_t n, uint64_t seed,
                                                float* __restrict__ pts, int32_t* __restrict__ fidx) {
#pragma clang fp contract(off)
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    uint32_t c[4] = {s, 0u, 0u, 0u};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const double x = ((double)(c[0] >> 8) + 1.0) * 0x1p-24 * w.boff[nb];
    uint32_t lo = 0, hi = nb - 1;                      // block: first b with boff[b + 1] >= x
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (w.boff[mid + 1] >= x) hi = mid;
        else lo = mid + 1;
    }
    const double base = w.boff[lo];
    uint32_t a0 = lo * kAreaBlock, a1 = min(a0 + kAreaBlock, F) - 1;    // face: first i with base + local[i] >= x
    while (a0 < a1) {
        const uint32_t mid = (a0 + a1) >> 1;
        if (base + w.local[mid] >= x) a1 = mid;
        else a0 = mid + 1;
    }
    const uint32_t face = a0;
    float ua = u01(c[1]), ub = u01(c[2]);
    if (ua + ub > 1.0f) {
        ua = 1.0f - ua;
        ub = 1.0f - ub;
    }
    const int32_t i0 = f[3ull * face], i1 = f[3ull * face + 1], i2 = f[3ull * face + 2];
    const bool ok = i0 >= 0 && i1 >= 0 && i2 >= 0 && (uint32_t)i0 < V && (uint32_t)i1 < V && (uint32_t)i2 < V;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float p = __builtin_nanf("");
        if (ok) {
            const float p0 = v[3ull * i0 + k];
            p = (p0 + ua * (v[3ull * i1 + k] - p0)) + ub * (v[3ull * i2 + k] - p0);
        }
        pts[3ull * s + k] = p;
    }
    fidx[s] = (int32_t)face;
}

}  // namespace nsa

extern "C" {

uint64_t nsa_nn_workspace(uint32_t n_targets) {
    if (n_targets == 0 || n_targets > nsa::kMaxCount) return 0;
    return nsa::nn_carve(nullptr, n_targets, nullptr);
}

int nsa_nn_build(const float* targets, uint32_t n_targets, void* index, nsa_stream_t stream) {
    using namespace nsa;
    if (!targets || !index || n_targets == 0 || n_targets > kMaxCount) return NSA_EBADARG;
    NnIndex ix;
    nn_carve(index, n_targets, &ix);
    const uint32_t B = nn_budget(n_targets), nb = (n_targets + 255) / 256;
    uint32_t bits = 1;
    while ((1ull << bits) <= (uint64_t)B) ++bits;      // keys are <= ncells <= B
    launch_begin();
    hipLaunchKernelGGL(k_nn_bounds, dim3(1), dim3(1024), 0, (hipStream_t)stream, targets, n_targets, B, ix);
    hipLaunchKernelGGL(k_nn_keys, dim3(nb), dim3(256), 0, (hipStream_t)stream, targets, n_targets, ix);
    radix_argsort(ix.keys, ix.tmp, ix.order, ix.counts, n_targets, 0, (bits + 7) / 8, stream);
    hipLaunchKernelGGL(k_nn_gather, dim3(nb), dim3(256), 0, (hipStream_t)stream, targets, n_targets, ix);
    hipLaunchKernelGGL(k_nn_cells, dim3((B + 2 + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_targets, ix);
    return launch_end();
}

int nsa_nn_query(const void* index, uint32_t n_targets, const float* queries, uint32_t n_queries, double max_dist, int32_t* idx,
                 float* dist, nsa_stream_t stream) {
    using namespace nsa;
    if (!index || n_targets == 0 || n_targets > kMaxCount || n_queries > kMaxCount || !(max_dist > 0.0)) return NSA_EBADARG;
    if (n_queries && (!queries || !idx || !dist)) return NSA_EBADARG;
    if (n_queries == 0) return NSA_OK;
    NnIndex ix;
    nn_carve(const_cast<void*>(index), n_targets, &ix);
    const bool strict = max_dist < INFINITY;
    const float r2 = strict ? (float)(max_dist * max_dist) : INFINITY;
    launch_begin();
    hipLaunchKernelGGL(k_nn_query, dim3((n_queries + 255) / 256), dim3(256), 0, (hipStream_t)stream, ix, queries, n_queries, r2,
                       strict, idx, dist);
    return launch_end();
}

int nsa_nn_query_k(const void* index, uint32_t n_targets, const float* queries, uint32_t n_queries, uint32_t k, double max_dist,
                   int32_t* idx, float* dist, uint32_t* count, nsa_stream_t stream) {
    using namespace nsa;
    if (!index || n_targets == 0 || n_targets > kMaxCount || n_queries > kMaxCount || !(max_dist > 0.0)) return NSA_EBADARG;
    if (k < 1 || k > cn::kMaxK) return NSA_EBADARG;
    if (n_queries && (!queries || !idx || !dist || !count)) return NSA_EBADARG;
    if (n_queries == 0) return NSA_OK;
    NnIndex ix;
    nn_carve(const_cast<void*>(index), n_targets, &ix);
    const bool strict = max_dist < INFINITY;
    const float r2 = strict ? (float)(max_dist * max_dist) : INFINITY;
    const dim3 grid((n_queries + 63) / 64), block(64);
    hipStream_t s = (hipStream_t)stream;
    launch_begin();
    if (k <= 8) hipLaunchKernelGGL(k_nn_query_k<8>, grid, block, 0, s, ix, queries, n_queries, k, r2, strict, idx, dist, count);
    else if (k <= 16) hipLaunchKernelGGL(k_nn_query_k<16>, grid, block, 0, s, ix, queries, n_queries, k, r2, strict, idx, dist, count);
    else if (k <= 32) hipLaunchKernelGGL(k_nn_query_k<32>, grid, block, 0, s, ix, queries, n_queries, k, r2, strict, idx, dist, count);
    else hipLaunchKernelGGL(k_nn_query_k<64>, grid, block, 0, s, ix, queries, n_queries, k, r2, strict, idx, dist, count);
    return launch_end();
}

uint64_t nsa_surface_sample_workspace(uint32_t n_faces) {
    if (n_faces == 0 || n_faces > nsa::kMaxCount) return 0;
    return nsa::sample_carve(nullptr, n_faces, nullptr);
}

int nsa_surface_sample(const float* verts, uint32_t n_verts, const int32_t* faces, uint32_t n_faces, uint32_t n_samples,
                       uint64_t seed, void* workspace, float* points, int32_t* face_idx, double* total_area,
                       nsa_stream_t stream) {
    using namespace nsa;
    if (!verts || !faces || !workspace || n_verts == 0 || n_faces == 0 || n_verts > kMaxCount || n_faces > kMaxCount ||
        n_samples > kMaxCount)
        return NSA_EBADARG;
    if (n_samples && (!points || !face_idx)) return NSA_EBADARG;
    SampleWork w;
    sample_carve(workspace, n_faces, &w);
    const uint32_t nb = (n_faces + kAreaBlock - 1) / kAreaBlock;
    launch_begin();
    hipLaunchKernelGGL(k_area_scan, dim3(nb), dim3(kAreaBlock), 0, (hipStream_t)stream, verts, n_verts, faces, n_faces, w);
    hipLaunchKernelGGL(k_area_offsets, dim3(1), dim3(64), 0, (hipStream_t)stream, w, nb, total_area);
    if (n_samples)
        hipLaunchKernelGGL(k_sample, dim3((n_samples + 255) / 256), dim3(256), 0, (hipStream_t)stream, verts, faces, n_verts,
                           n_faces, w, nb, n_samples, seed, points, face_idx);
    return launch_end();
}

}  // extern "C"
