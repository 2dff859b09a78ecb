// normals_passes.hpp -- the per-lane bodies of k-nearest-neighbour search and of normal estimation from neighbourhoods (DESIGN 4za,
// csrc/mesh_eval.hip k_nn_query_k, csrc/cloud_normals.hip): the candidate list of one query, the mean and scatter of one neighbourhood,
// the cyclic Jacobi eigen-decomposition of a symmetric 3x3, and the normal with its orientation and validity.  Like register_passes.hpp
// the bodies compile for the device and, unchanged, as host C++ (tests/cloud_normals_host_check.cpp calls them one row at a time and is
// held to tests/normals_ref.py bit for bit).  Every floating-point operation is rounded on its own: the pragma below keeps clang from
// contracting a * b + c, a host compiler that does not know it is given -ffp-contract=off.  The operation set is + - * / sqrt and
// comparisons: those are the same bits on the device, on the host and in numpy.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define NSA_CN_FN __host__ __device__ inline
#else
#define NSA_CN_FN static inline
#endif
#if defined(__clang__)
#define NSA_CN_EXACT _Pragma("clang fp contract(off)")
#else
#define NSA_CN_EXACT
#endif

namespace nsa {
namespace cn {

constexpr uint32_t kMaxK = 64;                      // the largest k of nsa_nn_query_k and nsa_cloud_normals
constexpr int kMaxSweeps = 16;

// ---- the candidate list of one query ----------------------------------------------------------------------------------------------
// A candidate is the 64-bit key (bits of d2) << 32 | target index.  d2 is a sum of squares, so it is >= +0 or +inf and its bits order
// as the value does: keys order as the pairs (d2, index) do.  The list holds the `held` smallest keys seen, ascending, at
// keys[0], keys[stride], ...: slot-major, one column per lane on the device (stride 64), stride 1 on the host.

NSA_CN_FN uint32_t f32_bits(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
}

NSA_CN_FN float bits_f32(uint32_t u) {
    float x;
    memcpy(&x, &u, 4);
    return x;
}

NSA_CN_FN uint64_t knn_key(float d2, uint32_t idx) { return ((uint64_t)f32_bits(d2) << 32) | idx; }

// the bound a cell's box distance and the rings' lower bound are held against: the k-th best d2 once k are held, r2 before
NSA_CN_FN float knn_bound(uint32_t held, uint32_t k, uint64_t worst, float r2) { return held == k ? bits_f32((uint32_t)(worst >> 32)) : r2; }

// offer (d2, idx); `worst` is keys[(k - 1) * stride] once k are held.  With a radius (`strict`) only d2 < r2 counts
NSA_CN_FN void knn_offer(uint64_t* keys, uint32_t stride, uint32_t k, uint32_t& held, uint64_t& worst, float d2, uint32_t idx, float r2,
                         bool strict) {
    const uint64_t key = knn_key(d2, idx);
    if (held == k ? !(key < worst) : (strict && !(d2 < r2))) return;
    uint32_t pos = held == k ? k - 1 : held;                       // the slot that opens: behind the list, or the worst's
    while (pos > 0) {
        const uint64_t prev = keys[(uint64_t)(pos - 1) * stride];
        if (prev < key) break;
        keys[(uint64_t)pos * stride] = prev;
        --pos;
    }
    keys[(uint64_t)pos * stride] = key;
    if (held < k) ++held;
    if (held == k) worst = keys[(uint64_t)(k - 1) * stride];
}

// the correctly rounded fp32 root: the float64 root then one rounding (53 >= 2 * 24 + 2)
NSA_CN_FN float knn_root(float d2) { return (float)sqrt((double)d2); }

// ---- one neighbourhood --------------------------------------------------------------------------------------------------------------

NSA_CN_FN bool finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; }      // false for a NaN

// the first `count` slots of idx name the neighbours, in the order of the query.  mu = (((0 + p_0) + p_1) + ...) / count, d_j = p_j - mu,
// S = (S00, S01, S02, S11, S12, S22) with S_ab = ((0 + d_0a d_0b) + d_1a d_1b) + ...; false, with nothing read, when count is 0 or
// above k or an index is outside [0, n)
NSA_CN_FN bool scatter(const float* points, uint32_t n, const int32_t* idx, uint32_t count, uint32_t k, double (&S)[6]) {
    NSA_CN_EXACT
    if (count == 0 || count > k) return false;
    for (uint32_t j = 0; j < count; ++j)
        if (idx[j] < 0 || (uint32_t)idx[j] >= n) return false;
    double mu[3] = {0.0, 0.0, 0.0};
    for (uint32_t j = 0; j < count; ++j) {
        const float* p = points + 3ull * (uint32_t)idx[j];
        for (int a = 0; a < 3; ++a) mu[a] = mu[a] + (double)p[a];
    }
    const double c = (double)count;
    for (int a = 0; a < 3; ++a) mu[a] = mu[a] / c;
    for (int i = 0; i < 6; ++i) S[i] = 0.0;
    for (uint32_t j = 0; j < count; ++j) {
        const float* p = points + 3ull * (uint32_t)idx[j];
        const double d0 = (double)p[0] - mu[0], d1 = (double)p[1] - mu[1], d2 = (double)p[2] - mu[2];
        S[0] = S[0] + d0 * d0;
        S[1] = S[1] + d0 * d1;
        S[2] = S[2] + d0 * d2;
        S[3] = S[3] + d1 * d1;
        S[4] = S[4] + d1 * d2;
        S[5] = S[5] + d2 * d2;
    }
    return true;
}

// one pivot (p, q) of the symmetric A with r the third index: app, aqq the diagonal, g the pivot, arp, arq the other two off-diagonals;
// vp, vq the columns p and q of V.  Returns whether g was not zero on entry
NSA_CN_FN bool jacobi_pivot(double& app, double& aqq, double& g, double& arp, double& arq, double (&vp)[3], double (&vq)[3]) {
    NSA_CN_EXACT
    if (g == 0.0) return false;
    if (fabs(app) + fabs(g) == fabs(app) && fabs(aqq) + fabs(g) == fabs(aqq)) {
        g = 0.0;
        return true;
    }
    const double theta = (aqq - app) / (2.0 * g), at = fabs(theta);
    // theta * theta would overflow above 2^511: there sqrt(theta^2 + 1) rounds to |theta| anyway
    double t = at > 0x1p500 ? 1.0 / (at + at) : 1.0 / (at + sqrt(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, h = t * g;
    app = app - h;
    aqq = aqq + h;
    g = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp;
    arq = rq;
    for (int i = 0; i < 3; ++i) {
        const double a = c * vp[i] - s * vq[i], b = s * vp[i] + c * vq[i];
        vp[i] = a;
        vq[i] = b;
    }
    return true;
}

// eigenvalues w[3] ascending and their eigenvectors V[column][row] of the symmetric S by cyclic Jacobi: pivots (0, 1), (0, 2), (1, 2) per
// sweep, at most kMaxSweeps sweeps, stopping at the first sweep that finds the three off-diagonals zero.  Equal eigenvalues keep the
// order of their columns.  Returns the number of sweeps that found a non-zero off-diagonal
NSA_CN_FN int jacobi3(const double (&S)[6], double (&w)[3], double (&V)[3][3]) {
    NSA_CN_EXACT
    double a00 = S[0], a01 = S[1], a02 = S[2], a11 = S[3], a12 = S[4], a22 = S[5];
    double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};          // v[column][row]
    int sweeps = 0;
    for (; sweeps < kMaxSweeps; ++sweeps) {
        bool any = jacobi_pivot(a00, a11, a01, a02, a12, v[0], v[1]);
        any = jacobi_pivot(a00, a22, a02, a01, a12, v[0], v[2]) || any;
        any = jacobi_pivot(a11, a22, a12, a01, a02, v[1], v[2]) || any;
        if (!any) break;
    }
    double l[3] = {a00, a11, a22};
    int o[3] = {0, 1, 2};
    auto order = [&](int i, int j) {                                              // strict: a tie or a NaN leaves the pair as it is
        if (l[j] < l[i]) {
            const double x = l[i];
            l[i] = l[j];
            l[j] = x;
            const int y = o[i];
            o[i] = o[j];
            o[j] = y;
        }
    };
    order(0, 1);
    order(1, 2);
    order(0, 1);
    for (int c = 0; c < 3; ++c) {
        w[c] = l[c];
        for (int i = 0; i < 3; ++i) V[c][i] = v[o[c]][i];
    }
    return sweeps;
}

// the row's normal from its eigen-decomposition: V[0] renormalised, turned towards `towards` - origin when towards is given, else so that
// its component of largest magnitude (ties: the lowest axis) is positive; then one rounding to fp32.  valid = count >= 3, the three
// eigenvalues finite and w[1] > 0; a row that is not valid has the normal (0, 0, 0)
NSA_CN_FN bool normal_of(uint32_t count, const double (&w)[3], const double (&v)[3], const float* origin, const float* towards,
                         float (&out)[3]) {
    NSA_CN_EXACT
    out[0] = out[1] = out[2] = 0.0f;
    if (!(count >= 3 && finite_d(w[0]) && finite_d(w[1]) && finite_d(w[2]) && w[1] > 0.0)) return false;
    const double len = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    const double n[3] = {v[0] / len, v[1] / len, v[2] / len};
    bool flip;
    if (towards) {
        const double e0 = (double)towards[0] - (double)origin[0], e1 = (double)towards[1] - (double)origin[1],
                     e2 = (double)towards[2] - (double)origin[2];
        flip = (n[0] * e0 + n[1] * e1) + n[2] * e2 < 0.0;
    } else {
        int ax = 0;
        if (fabs(n[1]) > fabs(n[0])) ax = 1;
        if (fabs(n[2]) > fabs(n[ax])) ax = 2;
        flip = n[ax] < 0.0;
    }
    for (int a = 0; a < 3; ++a) out[a] = (float)(flip ? -n[a] : n[a]);
    return true;
}

// one row of nsa_cloud_normals; eig may be NULL.  An eigenvalue that is a NaN is written as the canonical quiet NaN
NSA_CN_FN void normals_row(const float* points, uint32_t n, const int32_t* idx, uint32_t count, uint32_t k, const float* origin,
                           const float* towards, float* normal, double* eig, uint8_t* valid) {
    double S[6], w[3] = {NAN, NAN, NAN}, V[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    float out[3] = {0.0f, 0.0f, 0.0f};
    bool ok = false;
    if (scatter(points, n, idx, count, k, S)) {
        jacobi3(S, w, V);
        ok = normal_of(count, w, V[0], origin, towards, out);
    }
    for (int a = 0; a < 3; ++a) {
        normal[a] = out[a];
        if (eig) eig[a] = w[a] != w[a] ? (double)NAN : w[a];
    }
    *valid = ok ? 1 : 0;
}

}  // namespace cn
}  // namespace nsa
