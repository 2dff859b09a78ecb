// bulk_grid.hpp -- the uniform grid over the bulk of a set of points that the nearest-neighbour index (mesh_eval.hip) and
// the closest-point index (tri_common.hpp / mesh_closest.hip) are both built on, once: the head of the grid, the pick of the
// bulk from a strided subsample, the resolution solve, and the small helpers around them.  (grid_common.hpp is the hash grid's.)
//
// Bulk: of a strided subsample of kSubsample points the caller put into LDS (+inf where a point does not count), the values of rank
// m_f / 64 and m_f - 1 - m_f / 64 per axis, m_f the number that count -- the 1/64 and 63/64 quantiles, by counting, ties by position.
// Resolution: near-cubic cells over the bulk, at most `budget` of them and kMaxRes per axis; an axis thinner than 2^-10 of the
// longest is taken as that wide; a cell is never smaller than 1e-30.  Points outside the bulk are clamped into the border cells.
//
// The solve and the integer helpers also compile as host C++ (tests/index_host_check.cpp), the way topo_passes.hpp does.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define NSA_GRID_FN __host__ __device__ inline
#else
#define NSA_GRID_FN static inline
#endif

namespace nsa {
namespace bulk {

constexpr uint32_t kMaxCells = 1u << 22;
constexpr uint32_t kMaxRes = 1024;
constexpr uint32_t kSubsample = 2048;

struct Grid {                    // the head of both indexes: written by the unit's bounds kernel, read by every later kernel
    float lo[3], h[3], inv_h[3];
    uint32_t R[3], ncells, pad;
    float gmin[3], gmax[3];      // bounding box of what was indexed (+inf / -inf when there is nothing); the unit's to fill
};
static_assert(sizeof(Grid) == 80, "bulk::Grid is the head of an index buffer that Python reads");

NSA_GRID_FN uint64_t up256(uint64_t b) { return (b + 255) & ~uint64_t(255); }

// the first position of the sorted a[0 .. n) whose value is not below x
NSA_GRID_FN uint32_t lower_bound(const uint32_t* a, uint32_t n, uint32_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// lo, h, inv_h, R, ncells and pad of a grid over the bulk [blo, bhi] of m_f points (m_f == 0: one unit cell at 0)
NSA_GRID_FN void solve(const float (&blo)[3], const float (&bhi)[3], uint32_t m_f, uint32_t budget, Grid& g) {
    double e[3], emax = 0.0;
    for (int k = 0; k < 3; ++k) {
        g.lo[k] = m_f ? blo[k] : 0.0f;
        e[k] = m_f ? (double)bhi[k] - (double)blo[k] : 0.0;
        emax = e[k] > emax ? e[k] : emax;
    }
    uint32_t R[3] = {1, 1, 1};
    if (emax > 0.0) {
        for (int k = 0; k < 3; ++k) e[k] = e[k] > emax * 0x1p-10 ? e[k] : emax * 0x1p-10;
        double c = cbrt(e[0] * e[1] * e[2] / budget);
        for (int it = 0; it < 200; ++it) {             // near-cubic cells, at most `budget` of them
            for (int k = 0; k < 3; ++k) {
                const double r = floor(e[k] / c);
                R[k] = r < 1.0 ? 1u : (r > kMaxRes ? kMaxRes : (uint32_t)r);
            }
            if ((uint64_t)R[0] * R[1] * R[2] <= budget) break;
            c *= 1.0625;
        }
        if ((uint64_t)R[0] * R[1] * R[2] > budget) R[0] = R[1] = R[2] = 1;     // (never reached; keeps the cell arrays in bounds)
    }
    for (int k = 0; k < 3; ++k) {
        const float h = emax > 0.0 ? (float)(e[k] / R[k]) : 1.0f;
        g.h[k] = h > 1e-30f ? h : 1e-30f;
        g.inv_h[k] = 1.0f / g.h[k];
        g.R[k] = R[k];
    }
    g.ncells = R[0] * R[1] * R[2];
    g.pad = 0;
}

#if defined(__HIPCC__)

__device__ __forceinline__ bool finite3(float x, float y, float z) {
    return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
}
__device__ __forceinline__ bool finite3(const float (&p)[3]) { return finite3(p[0], p[1], p[2]); }

// cell index along one axis, clamped into [0, R - 1] (x finite)
__device__ __forceinline__ uint32_t axis_cell(float x, float lo, float inv_h, uint32_t R) {
#pragma clang fp contract(off)
    const float u = (x - lo) * inv_h;
    return (uint32_t)fminf(fmaxf(u, 0.0f), (float)(R - 1));
}

__device__ __forceinline__ void cross3(const double (&u)[3], const double (&w)[3], double (&n)[3]) {
#pragma clang fp contract(off)
    n[0] = u[1] * w[2] - u[2] * w[1];
    n[1] = u[2] * w[0] - u[0] * w[2];
    n[2] = u[0] * w[1] - u[1] * w[0];
}

template <typename T, typename Op>
__device__ __forceinline__ T block_reduce(T v, Op op, T* red) {    // 1024 threads; red[16]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    T r = red[0];
    for (int w = 1; w < 16; ++w) r = op(r, red[w]);
    return r;
}

// one workgroup of 1024: bulk[0] / bulk[1] = the values of rank m_f / 64 and m_f - 1 - m_f / 64 per axis among the first m entries of
// the subsample sv (in LDS, +inf where an entry does not count, m_f that do).  Opens and closes with a barrier: sv may have been
// written just before, and every thread may read bulk after
__device__ __forceinline__ void rank_bulk(const float (&sv)[3][kSubsample], uint32_t m, uint32_t m_f, float (&bulk)[2][3]) {
    __syncthreads();
    const uint32_t tid = threadIdx.x, k_lo = m_f >> 6, k_hi = m_f ? m_f - 1 - k_lo : 0;
    for (int a = 0; a < 3; ++a) {
        for (uint32_t j = tid; j < m; j += 1024) {
            const float v = sv[a][j];
            if (!__builtin_isfinite(v)) continue;
            uint32_t rank = 0;
            for (uint32_t i = 0; i < m; ++i) {
                const float w = sv[a][i];
                rank += (w < v) || (w == v && i < j);
            }
            if (rank == k_lo) bulk[0][a] = v;
            if (rank == k_hi) bulk[1][a] = v;
        }
    }
    __syncthreads();
}

#endif  // __HIPCC__

}  // namespace bulk
}  // namespace nsa
