// mesh_area.hpp -- the float64 face area of C ABI Section 8, shared by the surface sampler (mesh_eval.hip) and the per-component
// statistics (mesh_clean.hip): one definition, so both sum the very same values.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace nsa {

// area of face f in float64 (0 when an index is out of range): 0.5 * sqrt((cx*cx + cy*cy) + cz*cz), c = e1 x e2
__device__ inline double face_area(const float* __restrict__ v, uint32_t V, const int32_t* __restrict__ f, uint32_t i) {
#pragma clang fp contract(off)
    const int32_t a = f[3ull * i], b = f[3ull * i + 1], c = f[3ull * i + 2];
    if (a < 0 || b < 0 || c < 0 || (uint32_t)a >= V || (uint32_t)b >= V || (uint32_t)c >= V) return 0.0;
    const double x0 = v[3ull * a], y0 = v[3ull * a + 1], z0 = v[3ull * a + 2];
    const double e1x = v[3ull * b] - x0, e1y = v[3ull * b + 1] - y0, e1z = v[3ull * b + 2] - z0;
    const double e2x = v[3ull * c] - x0, e2y = v[3ull * c + 1] - y0, e2z = v[3ull * c + 2] - z0;
    const double cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
    return 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
}

}  // namespace nsa
