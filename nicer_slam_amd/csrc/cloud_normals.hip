// cloud_normals.hip -- normals of a raw point cloud from its k-nearest-neighbour neighbourhoods (C ABI Section 28): per row the
// float64 mean and scatter of the neighbours in the order the query wrote them, the eigen-decomposition of the 3x3 by cyclic Jacobi, and
// the eigenvector of the smallest eigenvalue, oriented and rounded once to fp32.  One lane per row; the bodies live in normals_passes.hpp,
// which also compiles as host C++.  Nothing is summed across lanes, so nothing depends on the launch geometry.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/nicer_slam_amd.h"
#include "grid_common.hpp"
#include "normals_passes.hpp"

#pragma clang fp contract(off)

namespace nsa {
namespace cn {

constexpr uint32_t kMaxRows = 0x7FFFFFFFu;

__global__ __launch_bounds__(256) void k_cloud_normals(const float* __restrict__ points, uint32_t n, const int32_t* __restrict__ idx,
                                                       const uint32_t* __restrict__ count, uint32_t m, uint32_t k,
                                                       const float* __restrict__ origin, const float* __restrict__ viewpoint,
                                                       uint32_t viewpoint_rows, float* __restrict__ normals, double* __restrict__ eig,
                                                       uint8_t* __restrict__ valid) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const float* towards = viewpoint_rows == 0 ? nullptr : viewpoint + (viewpoint_rows == 1 ? 0ull : 3ull * i);
    normals_row(points, n, idx + (uint64_t)i * k, count[i], k, origin + 3ull * i, towards, normals + 3ull * i, eig ? eig + 3ull * i : nullptr,
                valid + i);
}

}  // namespace cn
}  // namespace nsa

extern "C" {

int nsa_cloud_normals(const float* points, uint32_t n, const int32_t* idx, const uint32_t* count, uint32_t m, uint32_t k, const float* origin,
                      const float* viewpoint, uint32_t viewpoint_rows, float* normals, double* eigenvalues, uint8_t* valid,
                      nsa_stream_t stream) {
    using namespace nsa;
    using namespace nsa::cn;
    if (n > kMaxRows || m > kMaxRows || k < 1 || k > kMaxK) return NSA_EBADARG;
    if (viewpoint_rows != 0 && viewpoint_rows != 1 && viewpoint_rows != m) return NSA_EBADARG;
    if (m == 0) return NSA_OK;
    if (!idx || !count || !origin || !normals || !valid || (n && !points) || (viewpoint_rows && !viewpoint)) return NSA_EBADARG;
    launch_begin();
    hipLaunchKernelGGL(k_cloud_normals, dim3((m + 255) / 256), dim3(256), 0, (hipStream_t)stream, points, n, idx, count, m, k, origin,
                       viewpoint, viewpoint_rows, normals, eigenvalues, valid);
    return launch_end();
}

}  // extern "C"
