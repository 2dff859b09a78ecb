// block_scan.hpp -- the workgroup scan and count primitives of the mesh kernels, once each.  Device-only.
//
// Everything here adds or ORs integers, so any association gives the same bits: which lane adds what is no part of a result.
// The template parameters -- the channel count, the integer type and the workgroup's width -- are the only knobs; the integer
// type at a site is that of the caller's workspace array, which the C ABI fixes.
//
// The contract, the same for every primitive: EVERY lane of the workgroup calls it (no early return ahead of it: the barriers
// inside would hang), with blockDim.x == kThreads.  Each keeps its working words in LDS of its own and closes with a barrier, so
// it may be called more than once in a kernel and straight after the caller's own LDS writes; its results are in registers.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace nsa {
namespace scan {

typedef unsigned long long ull;

// a count the device holds, bounded by what the caller allocated for
__device__ __forceinline__ uint32_t capped(ull x, uint32_t cap) { return x < cap ? (uint32_t)x : cap; }

// excl[c] = the sum of v[c] over the lanes below this one, total[c] = over all kThreads lanes (Hillis-Steele in LDS)
template <int C, class T, uint32_t kThreads>
__device__ __forceinline__ void lds_scan(const T (&v)[C], T (&excl)[C], T (&total)[C]) {
    __shared__ T sh[C][kThreads];
    const uint32_t t = threadIdx.x;
#pragma unroll
    for (int c = 0; c < C; ++c) sh[c][t] = v[c];
    __syncthreads();
    for (uint32_t d = 1; d < kThreads; d <<= 1) {
        T add[C];
#pragma unroll
        for (int c = 0; c < C; ++c) add[c] = t >= d ? sh[c][t - d] : T(0);
        __syncthreads();
#pragma unroll
        for (int c = 0; c < C; ++c) sh[c][t] += add[c];
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        excl[c] = sh[c][t] - v[c];
        total[c] = sh[c][kThreads - 1];
    }
    __syncthreads();
}

// pre[k] = the lanes below this one that hold flag[k], total[k] = the lanes of the workgroup that do (ballots and popcounts, one
// LDS word per wave and flag).  A caller that wants the totals alone drops pre.
template <int N, uint32_t kThreads>
__device__ __forceinline__ void flag_scan(const bool (&flag)[N], uint32_t (&pre)[N], uint32_t (&total)[N]) {
    static_assert(kThreads % 64 == 0 && kThreads <= 1024, "whole waves of 64, one workgroup");
    constexpr uint32_t kWaves = kThreads / 64;
    __shared__ uint32_t ws[N][kWaves];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const ull below = (1ull << lane) - 1ull;
    ull b[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        b[k] = __ballot(flag[k]);
        if (lane == 0) ws[k][wave] = (uint32_t)__popcll(b[k]);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const uint32_t x = lane < kWaves ? ws[k][lane] : 0u;          // lane j holds wave j's count: at most 16, one row of lanes
        uint32_t p = lane < wave ? x : 0u, s = x;
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            p += (uint32_t)__shfl_xor((int)p, o, 64);
            s += (uint32_t)__shfl_xor((int)s, o, 64);
        }
        pre[k] = (uint32_t)__shfl((int)p, 0, 64) + (uint32_t)__popcll(b[k] & below);
        total[k] = (uint32_t)__shfl((int)s, 0, 64);
    }
    __syncthreads();
}

// the same for one flag: returns pre
template <uint32_t kThreads>
__device__ __forceinline__ uint32_t flag_scan(bool flag, uint32_t& total) {
    const bool f[1] = {flag};
    uint32_t pre[1], tot[1];
    flag_scan<1, kThreads>(f, pre, tot);
    total = tot[0];
    return pre[0];
}

// one workgroup: dst[j][c] = the sum of src[i][c] over i < j, for j < n, and total[c] = the sum over all n, in every lane.  src and
// dst may be the same array or two.  Each lane sums a contiguous chunk, lds_scan runs over the lane sums, the lanes write back.
template <int C, class T, uint32_t kThreads, class Src>
__device__ __forceinline__ void offsets(const Src* src, T* dst, uint64_t n, T (&total)[C]) {
    const uint64_t t = threadIdx.x, per = (n + kThreads - 1) / kThreads;
    const uint64_t j0 = t * per < n ? t * per : n, j1 = j0 + per < n ? j0 + per : n;
    T v[C], run[C];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = 0;
    for (uint64_t j = j0; j < j1; ++j)
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] += src[C * j + c];
    lds_scan<C, T, kThreads>(v, run, total);
    for (uint64_t j = j0; j < j1; ++j)
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const T own = src[C * j + c];
            dst[C * j + c] = run[c];
            run[c] += own;
        }
}

// `offsets` as a kernel of one workgroup; totals[C] (may be null) takes the grand totals
template <int C, class T, uint32_t kThreads>
__global__ __launch_bounds__(kThreads) void k_offsets(const T* src, T* dst, uint32_t nb, ull* totals) {
    T total[C];
    offsets<C, T, kThreads>(src, dst, nb, total);
    if (!totals) return;
#pragma unroll
    for (int c = 0; c < C; ++c)
        if (threadIdx.x == c) totals[c] = total[c];
}

// one workgroup: of part[nb][kSum + kOr], the first kSum columns added and the last kOr columns or-ed, into out[] in every lane
template <int kSum, int kOr, uint32_t kThreads>
__device__ __forceinline__ void block_totals(const uint32_t* __restrict__ part, uint32_t nb, ull (&out)[kSum + kOr]) {
    static_assert((kThreads & (kThreads - 1)) == 0, "the tree halves the workgroup");
    constexpr int N = kSum + kOr;
    __shared__ ull acc[N][kThreads];
    const uint32_t t = threadIdx.x;
    ull s[N];
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] = 0;
    for (uint32_t b = t; b < nb; b += kThreads) {
#pragma unroll
        for (int k = 0; k < kSum; ++k) s[k] += part[(ull)N * b + k];
#pragma unroll
        for (int k = kSum; k < N; ++k) s[k] |= part[(ull)N * b + k];
    }
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k][t] = s[k];
    __syncthreads();
    for (uint32_t o = kThreads / 2; o > 0; o >>= 1) {
        if (t < o) {
#pragma unroll
            for (int k = 0; k < kSum; ++k) acc[k][t] += acc[k][t + o];
#pragma unroll
            for (int k = kSum; k < N; ++k) acc[k][t] |= acc[k][t + o];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < N; ++k) out[k] = acc[k][0];
    __syncthreads();
}

}  // namespace scan
}  // namespace nsa
