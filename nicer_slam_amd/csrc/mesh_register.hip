// mesh_register.hip -- point-to-plane registration on the device (C ABI Section 27): moving the float64 source by a 4x4, and
// the thirty float64 sums and two counts of the 6x6 normal equations over the rows' correspondences.  The bodies live in
// register_passes.hpp, which also compiles as host C++.
//
// The order of every sum is a function of n alone.  A tile is 4096 consecutive rows and one workgroup of 256 lanes; lane l adds rows
// l, l + 256, ... of its tile in ascending order onto +0.0 (a row past n, without a correspondence or unused adds +0.0 in its place), a
// binary tree over the 256 lanes (s[i] = s[2 i] + s[2 i + 1], eight levels) gives the tile's total, and the totals go, zero-padded, in
// groups of 256 through the same tree until one value is left: one more launch per level, no counter of finished blocks and no
// floating-point atomic.  The tree runs as a butterfly: at level l every lane adds the value of the lane whose index differs in bit
// l - 1, so each lane holds the sum of its aligned group of 2^l lanes, lower half plus upper half (a + b and b + a are the same bits);
// six levels inside a wave, the last two over the four waves' values in LDS.  The counts are integers and go through block_scan.hpp.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/nicer_slam_amd.h"
#include "block_scan.hpp"
#include "grid_common.hpp"
#include "register_passes.hpp"

#pragma clang fp contract(off)

namespace nsa {
namespace reg {

typedef unsigned long long ull;

constexpr uint32_t kMaxRows = 0x7FFFFFFFu;
constexpr uint32_t kEntryWords = 32;                 // a tile's or a group's totals: 30 doubles, then 2 uint64 counts (256 bytes)

struct Mat4 {
    double m[16];
};

__global__ __launch_bounds__(256) void k_transform(double* __restrict__ cur, uint32_t n, Mat4 T, float* __restrict__ cur32) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double p[3] = {cur[3ull * i], cur[3ull * i + 1], cur[3ull * i + 2]};
    double y[3];
    transform_point(T.m, p, y);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        cur[3ull * i + k] = y[k];
        cur32[3ull * i + k] = (float)y[k];
    }
}

// the tree over the workgroup's 256 lane values of each of the thirty sums; lane i < 30 returns the total of sum i
__device__ __forceinline__ double tree_256(double (&v)[kSums]) {
    __shared__ double wave_total[kSums][4];
#pragma unroll
    for (int i = 0; i < kSums; ++i) {
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) v[i] = v[i] + __shfl_xor(v[i], o, 64);
    }
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < kSums; ++i) wave_total[i][wave] = v[i];
    }
    __syncthreads();
    double total = 0.0;
    if (threadIdx.x < kSums) {
        const double* w = wave_total[threadIdx.x];
        total = (w[0] + w[1]) + (w[2] + w[3]);
    }
    __syncthreads();
    return total;
}

// one workgroup per tile; sums_out / counts_out: the tile's entry, or the result itself when there is one tile
__global__ __launch_bounds__(256) void k_system(Rows a, double* __restrict__ sums_out, ull* __restrict__ counts_out) {
    const uint32_t lane = threadIdx.x;
    double acc[kSums];
#pragma unroll
    for (int i = 0; i < kSums; ++i) acc[i] = 0.0;
    ull cnt[2] = {0, 0};
    for (uint32_t j = 0; j < kRowsPerLane; ++j) {
        double t[kSums];
        bool corr, used;
        load_row(a, row_of(blockIdx.x, lane, j), t, corr, used);
#pragma unroll
        for (int i = 0; i < kSums; ++i) acc[i] = acc[i] + t[i];
        cnt[0] += corr ? 1u : 0u;
        cnt[1] += used ? 1u : 0u;
    }
    const double total = tree_256(acc);
    ull below[2], all[2];
    scan::lds_scan<2, ull, 256>(cnt, below, all);
    const uint64_t e = (uint64_t)blockIdx.x * kEntryWords;
    if (lane < kSums) sums_out[e + lane] = total;
    if (lane < 2) counts_out[e + lane] = all[lane];
}

// one workgroup per group of 256 entries of src (count of them; the rest of the last group is zeros)
__global__ __launch_bounds__(256) void k_reduce(const double* __restrict__ src, uint32_t count, double* __restrict__ sums_out,
                                                ull* __restrict__ counts_out) {
    const uint32_t lane = threadIdx.x;
    const uint64_t g = (uint64_t)blockIdx.x * kLanes + lane;
    double v[kSums];
    ull cnt[2] = {0, 0};
#pragma unroll
    for (int i = 0; i < kSums; ++i) v[i] = g < count ? src[g * kEntryWords + i] : 0.0;
    if (g < count) {
        const ull* c = reinterpret_cast<const ull*>(src) + g * kEntryWords + kSums;
        cnt[0] = c[0];
        cnt[1] = c[1];
    }
    const double total = tree_256(v);
    ull below[2], all[2];
    scan::lds_scan<2, ull, 256>(cnt, below, all);
    const uint64_t e = (uint64_t)blockIdx.x * kEntryWords;
    if (lane < kSums) sums_out[e + lane] = total;
    if (lane < 2) counts_out[e + lane] = all[lane];
}

inline uint64_t tiles_of(uint32_t n) { return ((uint64_t)n + kTile - 1) / kTile; }

}  // namespace reg
}  // namespace nsa

extern "C" {

int nsa_icp_transform(double* cur, uint32_t n, const double* upd, float* cur32, nsa_stream_t stream) {
    using namespace nsa;
    using namespace nsa::reg;
    if (n > kMaxRows) return NSA_EBADARG;
    if (n == 0) return NSA_OK;
    if (!cur || !upd || !cur32) return NSA_EBADARG;
    Mat4 T;
    for (int i = 0; i < 16; ++i) T.m[i] = upd[i];
    launch_begin();
    hipLaunchKernelGGL(k_transform, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, cur, n, T, cur32);
    return launch_end();
}

uint64_t nsa_icp_plane_system_workspace(uint32_t n) {
    using namespace nsa::reg;
    if (n == 0 || n > kMaxRows) return 0;
    const uint64_t tiles = tiles_of(n);
    return 8ull * kEntryWords * (tiles + groups_of(tiles));
}

int nsa_icp_plane_system(const double* cur, uint32_t n, int mode, const int32_t* corr, const float* dist, const float* targets,
                         const float* normals, uint32_t n_targets, const double* d2, const float* closest, const float* verts,
                         uint32_t n_verts, const int32_t* faces, uint32_t n_faces, int kernel, double k, void* workspace, double* sums,
                         uint64_t* counts, nsa_stream_t stream) {
    using namespace nsa;
    using namespace nsa::reg;
    if (n > kMaxRows) return NSA_EBADARG;
    if (mode != NSA_ICP_CLOUD && mode != NSA_ICP_SURFACE) return NSA_EBADARG;
    if (kernel != kL2 && kernel != kHuber && kernel != kTukey) return NSA_EBADARG;
    if (kernel != kL2 && !(k > 0.0 && finite_d(k))) return NSA_EBADARG;    // (a NaN fails too)
    if (n == 0) return NSA_OK;
    if (!cur || !corr || !workspace || !sums || !counts) return NSA_EBADARG;
    if (mode == NSA_ICP_CLOUD ? (!dist || !targets || !normals) : (!d2 || !closest || !verts || !faces)) return NSA_EBADARG;
    const Rows a = {cur, corr, dist, targets, normals, d2, closest, verts, faces, n, n_targets, n_verts, n_faces,
                    mode == NSA_ICP_SURFACE ? 1 : 0, kernel, k};
    hipStream_t s = (hipStream_t)stream;
    uint64_t count = tiles_of(n);
    double* level[2] = {static_cast<double*>(workspace), static_cast<double*>(workspace) + kEntryWords * count};
    ull* out_counts = reinterpret_cast<ull*>(counts);
    launch_begin();
    if (count == 1) {
        hipLaunchKernelGGL(k_system, dim3(1), dim3(256), 0, s, a, sums, out_counts);
        return launch_end();
    }
    hipLaunchKernelGGL(k_system, dim3((uint32_t)count), dim3(256), 0, s, a, level[0], reinterpret_cast<ull*>(level[0]) + kSums);
    int from = 0;
    while (count > 1) {
        const uint64_t next = groups_of(count);
        double* dst = next == 1 ? sums : level[from ^ 1];
        ull* dst_counts = next == 1 ? out_counts : reinterpret_cast<ull*>(level[from ^ 1]) + kSums;
        hipLaunchKernelGGL(k_reduce, dim3((uint32_t)next), dim3(256), 0, s, level[from], (uint32_t)count, dst, dst_counts);
        count = next;
        from ^= 1;
    }
    return launch_end();
}

}  // extern "C"
