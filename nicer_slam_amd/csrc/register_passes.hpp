// register_passes.hpp -- the per-row bodies of point-to-plane registration (csrc/mesh_register.hip): moving one point by a
// 4x4, the normal of a face, one row's thirty terms with its weight, and the order in which 256 lane sums become one.  Like
// smooth_passes.hpp the bodies compile for the device and, unchanged, as host C++ (tests/register_host_check.cpp calls them one row at
// a time and is held to tests/register_ref.py bit for bit).  Every floating-point operation is rounded on its own: the pragma below
// keeps clang from contracting a * b + c, a host compiler that does not know it is given -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define NSA_RG_FN __host__ __device__ inline
#else
#define NSA_RG_FN static inline
#endif
#if defined(__clang__)
#define NSA_RG_EXACT _Pragma("clang fp contract(off)")
#else
#define NSA_RG_EXACT
#endif

namespace nsa {
namespace reg {

constexpr int kL2 = 0, kHuber = 1, kTukey = 2;      // NSA_ICP_KERNEL_*
constexpr int kSums = 30;                           // S[0..29] of header Section 27
constexpr uint32_t kLanes = 256;                    // the width of the tree
constexpr uint32_t kRowsPerLane = 16;
constexpr uint32_t kTile = kLanes * kRowsPerLane;   // 4096 consecutive rows

NSA_RG_FN bool finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; }      // false for a NaN

// row `j` of lane `lane` of tile `tile`: the lane adds its rows j = 0 .. 15 in this order
NSA_RG_FN uint64_t row_of(uint64_t tile, uint32_t lane, uint32_t j) { return tile * kTile + (uint64_t)j * kLanes + lane; }

// y = ((R_k0 x + R_k1 y) + R_k2 z) + t_k of the row-major 4x4 T
NSA_RG_FN void transform_point(const double* T, const double (&p)[3], double (&y)[3]) {
    NSA_RG_EXACT
    for (int k = 0; k < 3; ++k) y[k] = ((T[4 * k] * p[0] + T[4 * k + 1] * p[1]) + T[4 * k + 2] * p[2]) + T[4 * k + 3];
}

// c / sqrt((c_x c_x + c_y c_y) + c_z c_z), c = ab x ac in float64 from fp32 vertices; a face without area gives NaNs
NSA_RG_FN void face_normal(const float* a, const float* b, const float* c, double (&n)[3]) {
    NSA_RG_EXACT
    double ab[3], ac[3];
    for (int k = 0; k < 3; ++k) {
        ab[k] = (double)b[k] - (double)a[k];
        ac[k] = (double)c[k] - (double)a[k];
    }
    const double cx = ab[1] * ac[2] - ab[2] * ac[1];
    const double cy = ab[2] * ac[0] - ab[0] * ac[2];
    const double cz = ab[0] * ac[1] - ab[1] * ac[0];
    const double len = sqrt((cx * cx + cy * cy) + cz * cz);
    n[0] = cx / len;
    n[1] = cy / len;
    n[2] = cz / len;
}

// a row with a correspondence is used when its normal is finite and not (0, 0, 0)
NSA_RG_FN bool normal_usable(const double (&n)[3]) {
    return finite_d(n[0]) && finite_d(n[1]) && finite_d(n[2]) && !(n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0);
}

// the weight of residual r: open3d's L2Loss, HuberLoss(k) and TukeyLoss(k)
NSA_RG_FN double weight(int kernel, double k, double r) {
    NSA_RG_EXACT
    const double ar = fabs(r);
    if (kernel == kHuber) return ar <= k ? 1.0 : k / ar;
    if (kernel == kTukey) {
        const double u = r / k;
        const double v = 1.0 - u * u;
        return ar <= k ? v * v : 0.0;
    }
    return 1.0;
}

// the thirty terms of one row: `corr` it has a correspondence, `used` its normal is usable as well.  p the moved source point, q its
// correspondence, n the normal there, dd the squared correspondence distance the query reported.  A row that is not used gives
// +0.0 in S[0..28], one without a correspondence in S[29] too
NSA_RG_FN void row_terms(bool corr, bool used, const double (&p)[3], const double (&q)[3], const double (&n)[3], double dd, int kernel,
                         double k, double (&t)[kSums]) {
    NSA_RG_EXACT
    for (int i = 0; i < kSums; ++i) t[i] = 0.0;
    if (!corr) return;
    t[29] = dd;
    if (!used) return;
    const double d[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
    const double r = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2];
    const double J[6] = {p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0], n[0], n[1], n[2]};
    const double w = weight(kernel, k, r);
    double g[6];
    for (int i = 0; i < 6; ++i) g[i] = w * J[i];
    int s = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) t[s++] = g[i] * J[j];
    for (int i = 0; i < 6; ++i) t[21 + i] = g[i] * r;
    t[27] = r * r;
    t[28] = (w * r) * r;
}

struct Rows {                    // what a row reads; corr is idx (cloud) or face_idx (surface)
    const double* cur;
    const int32_t* corr;
    const float* dist;           // cloud: the query's fp32 distance
    const float* targets;        // cloud [n_targets, 3]
    const float* normals;        // cloud [n_targets, 3]
    const double* d2;            // surface: the query's float64 squared distance
    const float* closest;        // surface [n, 3]
    const float* verts;          // surface [n_verts, 3]
    const int32_t* faces;        // surface [n_faces, 3]
    uint32_t n, n_targets, n_verts, n_faces;
    int surface, kernel;
    double k;
};

// row i's terms; every index is checked before it is used
NSA_RG_FN void load_row(const Rows& a, uint64_t i, double (&t)[kSums], bool& corr, bool& used) {
    double p[3] = {0.0, 0.0, 0.0}, q[3] = {0.0, 0.0, 0.0}, nrm[3] = {0.0, 0.0, 0.0}, dd = 0.0;
    corr = used = false;
    if (i < a.n) {
        const int32_t c = a.corr[i];
        if (a.surface) {
            if (c >= 0 && (uint32_t)c < a.n_faces) {
                const uint32_t ia = (uint32_t)a.faces[3ull * c], ib = (uint32_t)a.faces[3ull * c + 1], ic = (uint32_t)a.faces[3ull * c + 2];
                if (ia < a.n_verts && ib < a.n_verts && ic < a.n_verts) {
                    corr = true;
                    face_normal(a.verts + 3ull * ia, a.verts + 3ull * ib, a.verts + 3ull * ic, nrm);
                    dd = a.d2[i];
                    for (int k = 0; k < 3; ++k) q[k] = (double)a.closest[3ull * i + k];
                }
            }
        } else if (c >= 0 && (uint32_t)c < a.n_targets) {
            corr = true;
            const double d = (double)a.dist[i];
            dd = d * d;
            for (int k = 0; k < 3; ++k) {
                q[k] = (double)a.targets[3ull * c + k];
                nrm[k] = (double)a.normals[3ull * c + k];
            }
        }
        if (corr) {
            for (int k = 0; k < 3; ++k) p[k] = a.cur[3ull * i + k];
            used = normal_usable(nrm);
        }
    }
    row_terms(corr, used, p, q, nrm, dd, a.kernel, a.k, t);
}

// the tree over 256 values in place: s[i] = s[2 i] + s[2 i + 1], eight levels; the total is s[0].  (The device kernels run the same
// tree as a butterfly over the lanes of a wave and then over the four waves: at level l lane i holds the sum of the aligned group
// of 2^l lanes it lies in, lower half plus upper half -- the same additions.)
NSA_RG_FN double tree256(double* s) {
    NSA_RG_EXACT
    for (uint32_t n = kLanes / 2; n > 0; n >>= 1)
        for (uint32_t i = 0; i < n; ++i) s[i] = s[2 * i] + s[2 * i + 1];
    return s[0];
}

// how many values one level of the tree leaves of `count`
NSA_RG_FN uint64_t groups_of(uint64_t count) { return (count + kLanes - 1) / kLanes; }

}  // namespace reg
}  // namespace nsa
