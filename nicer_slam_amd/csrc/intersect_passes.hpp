// intersect_passes.hpp -- the per-pair bodies of the self-intersection query (csrc/mesh_intersect.hip; header Section 25):
// the shared-position count, the float64 orientation filter and its error bound, a 256-bit integer on 32-bit limbs, the exact
// orientation determinants on it, and the closed-set decision of a pair of faces from their signs.  The bodies compile for the device
// and, unchanged, as host C++ (tests/intersect_host_check.cpp holds the integer to Python's and the decisions to tests/intersect_ref.py).
//
// The filter.  orient3d(a, b, c, d) = det[a - d; b - d; c - d], expanded along the first row, evaluated in float64 on fp32 inputs.
// With u = 2^-53: a difference of two fp32 numbers is a multiple of 2^-149, far above float64's subnormals, so every operation below
// obeys fl(x op y) = (x op y)(1 + e), |e| <= u, and no product of three differences (>= 2^-447 when non-zero, <= 2^387) under- or
// overflows.  A term adx * (bdy * cdz - bdz * cdy) carries the three differences (1 + u)^3, two products, one subtraction -- measured
// against |bdy cdz| + |bdz cdy|, not against their difference --, and two additions of terms: at most (1 + u)^8 in all.  Hence
//     |computed - exact| <= ((1 + u)^8 - 1) P,     P = the same expression with every product and difference in absolute value,
// the permanent.  The computed permanent Pc consists of positive terms through the same operations, so P <= Pc / (1 - u)^8 and
// |computed - exact| <= 8.0000001 u Pc < kFilter * Pc with kFilter = 2^-49 = 16 u (the product by a power of two is exact).  Shewchuk's
// A-filter has (7 + 56 u) u for a slightly different order; the factor of two here buys a derivation of five lines.  A sign is
// CERTAIN when |computed| > bound, or when bound == 0: then every product is exactly zero and so is the determinant.
//
// The width.  Per pair, with e(x) the exponent of the unit in the last place of a non-zero fp32 x (e = exponent field - 150, -149 for
// a subnormal), E = the least e over the pair's 18 coordinates and R = the greatest e - E: x = m 2^e with |m| < 2^24, so x / 2^E is an
// integer below 2^(24 + R) in magnitude.  A difference is below 2^(25 + R), a 2 x 2 minor below 2^(51 + 2 R), a term below
// 2^(76 + 3 R), the determinant below 3 * 2^(76 + 3 R) < 2^(78 + 3 R).  A two's-complement integer of 256 bits holds magnitudes below
// 2^255: R <= kMaxSpread = 59.  The collinearity of ONE face needs only the minors of its own 9 coordinates: 51 + 2 R <= 255 gives
// R <= kMaxFaceSpread = 102.  Sums, differences and products are taken modulo 2^256, which is exact whenever the true value fits.
//
// The decision, for non-degenerate closed triangles A, B sharing s vertex positions, I = A n B:
//   s = 3                           reported, proper, coplanar.
//   sb_k = sign orient3d(A, B_k), sa_k = sign orient3d(B, A_k).  All sb strictly of one sign, or all sa: I is empty.
//   sb = 0 0 0: coplanar, below.    Otherwise the planes meet in a line L; A n L is the segment between the two edges at A's APEX,
//   the vertex alone on its side (or on the plane with the two others strictly on one side: then the segment is that vertex).
//   For an edge (p, e) of A and an edge (q, f) of B that each meet L in one point X, Y:
//       orient3d(p, e, q, f) = k (Y - X) . D (dB(e) - dB(p)) (dA(f) - dA(q)),   D the direction of L, k a constant of the pair
//   (write the four points as X + a u, X + b u, Y + c w, Y + d w and expand), so c = sign(orient3d) sgn(sa_e - sa_p) sgn(sb_f - sb_q)
//   orders X against Y along L, consistently for the four combinations of the two edges at each apex, and is 0 iff X = Y.
//       I is empty             iff the four c are all > 0 or all < 0;
//       I is a segment         iff some c > 0 and some c < 0 and neither apex lies on the other plane;
//       proper                 iff some c > 0 and some c < 0 and both faces have vertices strictly on both sides.
//   s = 0: reported iff I is not empty.  s = 1: iff I is a segment (it contains the shared vertex).  s = 2: never, both cuts are the
//   shared edge.
//   Coplanar: drop an axis on which A's normal is not zero; ea[i][k] = the side of B_k of A's edge i, positive inside, eb alike.
//       proper    iff no edge of either has all three vertices of the other on its outer side or on its line (the separating axes
//                 of the two OPEN triangles are the edge normals: the edges of the Minkowski difference);
//       reported  iff a vertex of one that is no shared position lies in the other closed triangle, or an edge of A and an edge of
//                 B cross strictly -- the vertices of the polygon I are of these two kinds, and a vertex of a triangle lies in the
//                 hull of some of its vertices only if it is one of them.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define NSA_IS_FN __host__ __device__ inline
#define NSA_IS_SLOW static __host__ __device__ __attribute__((noinline))
#else
#define NSA_IS_FN static inline
#define NSA_IS_SLOW static __attribute__((noinline))
#endif

namespace nsa {
namespace isect {

constexpr uint32_t kProper = 1, kTouch = 2, kUnresolved = 3, kCoplanar = 4;        // the code of a pair; s in bits 4 and 5
constexpr int kStageFilter = 1, kStageExact = 2, kStageUnresolved = 3;
constexpr int kLimbs = 8;
constexpr int kMaxSpread = 59, kMaxFaceSpread = 102;
static_assert(78 + 3 * kMaxSpread <= 32 * kLimbs - 1 && 51 + 2 * kMaxFaceSpread <= 32 * kLimbs - 1, "see The width");
static_assert(kMaxSpread >= 40, "Section 25 promises at least 40");
constexpr double kFilter = 0x1p-49;
constexpr int kUncertain = 2;

NSA_IS_FN uint32_t code_of(uint32_t kind, bool coplanar, int s) { return kind | (coplanar ? kCoplanar : 0u) | ((uint32_t)s << 4); }

// ---- 256-bit two's-complement integers ------------------------------------------------------------------------------------------

struct Wide {
    uint32_t w[kLimbs];
};

NSA_IS_FN Wide wide_zero() {
    Wide r;
    for (int k = 0; k < kLimbs; ++k) r.w[k] = 0;
    return r;
}
NSA_IS_FN Wide wide_add(const Wide& a, const Wide& b) {
    Wide r;
    uint64_t c = 0;
    for (int k = 0; k < kLimbs; ++k) {
        c += (uint64_t)a.w[k] + (uint64_t)b.w[k];
        r.w[k] = (uint32_t)c;
        c >>= 32;
    }
    return r;
}
NSA_IS_FN Wide wide_sub(const Wide& a, const Wide& b) {           // a + ~b + 1
    Wide r;
    uint64_t c = 1;
    for (int k = 0; k < kLimbs; ++k) {
        c += (uint64_t)a.w[k] + (uint64_t)(~b.w[k]);
        r.w[k] = (uint32_t)c;
        c >>= 32;
    }
    return r;
}
NSA_IS_FN Wide wide_mul(const Wide& a, const Wide& b) {           // the low 256 bits: schoolbook, 36 products of 32 x 32 -> 64
    Wide r = wide_zero();
    for (int i = 0; i < kLimbs; ++i) {
        uint64_t carry = 0;
        for (int j = 0; i + j < kLimbs; ++j) {
            const uint64_t t = (uint64_t)a.w[i] * (uint64_t)b.w[j] + (uint64_t)r.w[i + j] + carry;     // <= 2^64 - 1
            r.w[i + j] = (uint32_t)t;
            carry = t >> 32;
        }
    }
    return r;
}
NSA_IS_FN int wide_sign(const Wide& a) {
    if (a.w[kLimbs - 1] >> 31) return -1;
    uint32_t any = 0;
    for (int k = 0; k < kLimbs; ++k) any |= a.w[k];
    return any ? 1 : 0;
}

// ---- fp32 coordinates as integers -------------------------------------------------------------------------------------------------

NSA_IS_FN uint32_t float_bits(float x) {
    uint32_t b;
    __builtin_memcpy(&b, &x, 4);
    return b;
}
// x = (-1)^neg * mant * 2^e for a finite x; mant = 0 for a zero
NSA_IS_FN void split(float x, uint32_t& mant, int& e, bool& neg) {
    const uint32_t b = float_bits(x), ef = (b >> 23) & 0xFFu, m = b & 0x7FFFFFu;
    neg = (b >> 31) != 0;
    mant = ef ? (m | 0x800000u) : m;
    e = ef ? (int)ef - 150 : -149;
}
// E and R of n coordinates (0, 0 when all are zero)
NSA_IS_FN void spread(const float* x, int n, int& E, int& R) {
    int lo = 1 << 20, hi = -(1 << 20);
    for (int k = 0; k < n; ++k) {
        uint32_t mant;
        int e;
        bool neg;
        split(x[k], mant, e, neg);
        if (mant == 0) continue;
        lo = e < lo ? e : lo;
        hi = e > hi ? e : hi;
    }
    E = hi < lo ? 0 : lo;
    R = hi < lo ? 0 : hi - lo;
}
// x / 2^E, for e(x) - E in [0, kMaxFaceSpread]
NSA_IS_FN Wide wide_of(float x, int E) {
    uint32_t mant;
    int e;
    bool neg;
    split(x, mant, e, neg);
    Wide r = wide_zero();
    if (mant == 0) return r;
    int sh = e - E;
    sh = sh < 0 ? 0 : (sh > 32 * (kLimbs - 2) ? 32 * (kLimbs - 2) : sh);            // (never clamps inside the stated range)
    const int limb = sh >> 5, off = sh & 31;
    r.w[limb] = mant << off;
    if (off) r.w[limb + 1] = mant >> (32 - off);
    return neg ? wide_sub(wide_zero(), r) : r;
}

struct Point {
    Wide x[3];
};
struct Face {
    Point p[3];
};
NSA_IS_FN void face_of(const float (&a)[3][3], int E, Face& out) {
    for (int v = 0; v < 3; ++v)
        for (int k = 0; k < 3; ++k) out.p[v].x[k] = wide_of(a[v][k], E);
}

NSA_IS_FN Wide minor2(const Wide& a, const Wide& b, const Wide& c, const Wide& d) { return wide_sub(wide_mul(a, b), wide_mul(c, d)); }

// the sign of det[a - d; b - d; c - d]
NSA_IS_SLOW int orient3d_exact(const Point& a, const Point& b, const Point& c, const Point& d) {
    Wide ad[3], bd[3], cd[3];
    for (int k = 0; k < 3; ++k) {
        ad[k] = wide_sub(a.x[k], d.x[k]);
        bd[k] = wide_sub(b.x[k], d.x[k]);
        cd[k] = wide_sub(c.x[k], d.x[k]);
    }
    Wide det = wide_zero();
    for (int k = 0; k < 3; ++k) {
        const int k1 = k == 2 ? 0 : k + 1, k2 = k1 == 2 ? 0 : k1 + 1;
        det = wide_add(det, wide_mul(ad[k], minor2(bd[k1], cd[k2], bd[k2], cd[k1])));
    }
    return wide_sign(det);
}

// the sign of (q - p) x (r - p) in the plane of the axes u, v
NSA_IS_SLOW int orient2d_exact(const Point& p, const Point& q, const Point& r, int u, int v) {
    return wide_sign(minor2(wide_sub(q.x[u], p.x[u]), wide_sub(r.x[v], p.x[v]), wide_sub(q.x[v], p.x[v]), wide_sub(r.x[u], p.x[u])));
}

// component k of (b - a) x (c - a)
NSA_IS_FN Wide normal_component(const Face& f, int k) {
    const int k1 = k == 2 ? 0 : k + 1, k2 = k1 == 2 ? 0 : k1 + 1;
    return minor2(wide_sub(f.p[1].x[k1], f.p[0].x[k1]), wide_sub(f.p[2].x[k2], f.p[0].x[k2]), wide_sub(f.p[1].x[k2], f.p[0].x[k2]),
                  wide_sub(f.p[2].x[k1], f.p[0].x[k1]));
}

// 1: the three vertices are exactly collinear, 0: they are not, -1: the face's exponents span more than kMaxFaceSpread
NSA_IS_SLOW int face_collinear(const float (&a)[3][3]) {
    int E, R;
    spread(&a[0][0], 9, E, R);
    if (R > kMaxFaceSpread) return -1;
    Face f;
    face_of(a, E, f);
    for (int k = 0; k < 3; ++k)
        if (wide_sign(normal_component(f, k)) != 0) return 0;
    return 1;
}

// ---- the float64 filter -----------------------------------------------------------------------------------------------------------

// the certain sign of orient3d(a, b, c, d), or kUncertain
NSA_IS_FN int orient3d_filter(const float* a, const float* b, const float* c, const float* d) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double adx = (double)a[0] - (double)d[0], ady = (double)a[1] - (double)d[1], adz = (double)a[2] - (double)d[2];
    const double bdx = (double)b[0] - (double)d[0], bdy = (double)b[1] - (double)d[1], bdz = (double)b[2] - (double)d[2];
    const double cdx = (double)c[0] - (double)d[0], cdy = (double)c[1] - (double)d[1], cdz = (double)c[2] - (double)d[2];
    const double m1 = bdy * cdz, m2 = bdz * cdy, m3 = bdz * cdx, m4 = bdx * cdz, m5 = bdx * cdy, m6 = bdy * cdx;
    const double det = (adx * (m1 - m2) + ady * (m3 - m4)) + adz * (m5 - m6);
    const double perm = (fabs(adx) * (fabs(m1) + fabs(m2)) + fabs(ady) * (fabs(m3) + fabs(m4))) + fabs(adz) * (fabs(m5) + fabs(m6));
    const double bound = kFilter * perm;
    if (det > bound) return 1;
    if (-det > bound) return -1;
    return bound == 0.0 ? 0 : kUncertain;
}

// ---- a pair -------------------------------------------------------------------------------------------------------------------------

NSA_IS_FN bool same_position(const float* p, const float* q) { return p[0] == q[0] && p[1] == q[1] && p[2] == q[2]; }

// which vertices of a are positions of b and the reverse; returns s
NSA_IS_FN int shared_positions(const float (&a)[3][3], const float (&b)[3][3], bool (&sha)[3], bool (&shb)[3]) {
    int s = 0;
    for (int k = 0; k < 3; ++k) sha[k] = shb[k] = false;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            if (same_position(a[i], b[j])) {
                sha[i] = true;
                shb[j] = true;
            }
    for (int k = 0; k < 3; ++k) s += sha[k] ? 1 : 0;
    return s;
}

NSA_IS_FN int sgn(int x) { return (x > 0) - (x < 0); }

NSA_IS_FN bool one_sided(const int (&s)[3]) { return (s[0] > 0 && s[1] > 0 && s[2] > 0) || (s[0] < 0 && s[1] < 0 && s[2] < 0); }

NSA_IS_FN int apex_of(const int (&s)[3]) {
    for (int i = 0; i < 3; ++i) {
        const int j = i == 2 ? 0 : i + 1, k = j == 2 ? 0 : j + 1;
        if (s[i] != 0 && s[j] * s[i] <= 0 && s[k] * s[i] <= 0) return i;
        if (s[i] == 0 && s[j] * s[k] > 0) return i;
    }
    return 0;                                                      // (unreachable after one_sided and the coplanar branch)
}

// from the four orders c of the ends along L
NSA_IS_FN uint32_t from_orders(const int (&c)[4], bool segment_possible, bool strict, int s) {
    bool pos = false, neg = false, zero = false;
    for (int k = 0; k < 4; ++k) {
        pos = pos || c[k] > 0;
        neg = neg || c[k] < 0;
        zero = zero || c[k] == 0;
    }
    if (!zero && pos != neg) return 0;                             // all on one side: I is empty
    const bool both = pos && neg;
    if (s == 1 && !(both && segment_possible)) return 0;
    return code_of(both && strict ? kProper : kTouch, false, s);
}

NSA_IS_FN bool strictly_both(const int (&s)[3]) {
    return (s[0] > 0 || s[1] > 0 || s[2] > 0) && (s[0] < 0 || s[1] < 0 || s[2] < 0);
}

NSA_IS_FN const Point& pick(const Face& f, int i) { return i == 0 ? f.p[0] : (i == 1 ? f.p[1] : f.p[2]); }
NSA_IS_FN int pick(const int (&s)[3], int i) { return i == 0 ? s[0] : (i == 1 ? s[1] : s[2]); }

NSA_IS_SLOW uint32_t coplanar_exact(const Face& A, const Face& B, const bool (&sha)[3], const bool (&shb)[3], int s) {
    int drop = 2;
    if (wide_sign(normal_component(A, 0)) != 0) drop = 0;
    else if (wide_sign(normal_component(A, 1)) != 0) drop = 1;
    const int u = drop == 2 ? 0 : drop + 1, v = u == 2 ? 0 : u + 1;
    const int oa = orient2d_exact(A.p[0], A.p[1], A.p[2], u, v), ob = orient2d_exact(B.p[0], B.p[1], B.p[2], u, v);
    int ea[3][3], eb[3][3];
    for (int i = 0; i < 3; ++i) {
        const int i1 = i == 2 ? 0 : i + 1;
        for (int k = 0; k < 3; ++k) {
            ea[i][k] = orient2d_exact(A.p[i], A.p[i1], B.p[k], u, v) * oa;
            eb[i][k] = orient2d_exact(B.p[i], B.p[i1], A.p[k], u, v) * ob;
        }
    }
    bool proper = true, reported = false;
    for (int i = 0; i < 3; ++i) {
        if (ea[i][0] <= 0 && ea[i][1] <= 0 && ea[i][2] <= 0) proper = false;
        if (eb[i][0] <= 0 && eb[i][1] <= 0 && eb[i][2] <= 0) proper = false;
    }
    for (int k = 0; k < 3; ++k) {
        if (!shb[k] && ea[0][k] >= 0 && ea[1][k] >= 0 && ea[2][k] >= 0) reported = true;
        if (!sha[k] && eb[0][k] >= 0 && eb[1][k] >= 0 && eb[2][k] >= 0) reported = true;
    }
    for (int i = 0; i < 3; ++i) {
        const int i1 = i == 2 ? 0 : i + 1;
        for (int j = 0; j < 3; ++j) {
            const int j1 = j == 2 ? 0 : j + 1;
            if (ea[i][j] * ea[i][j1] < 0 && eb[j][i] * eb[j][i1] < 0) reported = true;
        }
    }
    return reported ? code_of(proper ? kProper : kTouch, true, s) : 0u;
}

// stage 2: every sign exact.  stage becomes kStageExact, or kStageUnresolved with the code kUnresolved | s << 4
NSA_IS_SLOW uint32_t pair_exact(const float (&a)[3][3], const float (&b)[3][3], const bool (&sha)[3], const bool (&shb)[3], int s,
                                int& stage) {
    float all[18];
    for (int v = 0; v < 3; ++v)
        for (int k = 0; k < 3; ++k) {
            all[3 * v + k] = a[v][k];
            all[9 + 3 * v + k] = b[v][k];
        }
    int E, R;
    spread(all, 18, E, R);
    if (R > kMaxSpread) {
        stage = kStageUnresolved;
        return code_of(kUnresolved, false, s);
    }
    stage = kStageExact;
    Face A, B;
    face_of(a, E, A);
    face_of(b, E, B);
    int sa[3], sb[3];
    for (int k = 0; k < 3; ++k) {
        sb[k] = shb[k] ? 0 : orient3d_exact(A.p[0], A.p[1], A.p[2], B.p[k]);
        sa[k] = sha[k] ? 0 : orient3d_exact(B.p[0], B.p[1], B.p[2], A.p[k]);
    }
    if (sb[0] == 0 && sb[1] == 0 && sb[2] == 0) return coplanar_exact(A, B, sha, shb, s);
    if (one_sided(sa) || one_sided(sb) || s == 2) return 0;
    const int ia = apex_of(sa), ib = apex_of(sb);
    int c[4];
    for (int x = 1; x <= 2; ++x) {
        const int ja = (ia + x) % 3;
        for (int y = 1; y <= 2; ++y) {
            const int jb = (ib + y) % 3;
            c[2 * (x - 1) + (y - 1)] = orient3d_exact(pick(A, ia), pick(A, ja), pick(B, ib), pick(B, jb)) *
                                       sgn(pick(sa, ja) - pick(sa, ia)) * sgn(pick(sb, jb) - pick(sb, ib));
        }
    }
    return from_orders(c, pick(sa, ia) != 0 && pick(sb, ib) != 0, strictly_both(sa) && strictly_both(sb), s);
}

// The code of the pair of usable faces a, b (0: not reported), s, and the stage that decided it.  Stage 1 decides only from signs that
// are certain and not zero -- with one extension that needs no more: when every vertex of one face that is no shared position lies
// strictly on one side of the other's plane, that face meets the plane in the hull of the shared positions alone.
NSA_IS_FN uint32_t pair_code(const float (&a)[3][3], const float (&b)[3][3], int& s, int& stage) {
    bool sha[3], shb[3];
    s = shared_positions(a, b, sha, shb);
    stage = kStageFilter;
    if (s == 3) return code_of(kProper, true, 3);
    int sa[3], sb[3];
    bool generic = s == 0;
    for (int side = 0; side < 2; ++side) {
        int pos = 0, neg = 0, other = 0;
        for (int k = 0; k < 3; ++k) {
            int r = 0;
            if (side == 0) {
                if (!shb[k]) r = orient3d_filter(a[0], a[1], a[2], b[k]);
                sb[k] = r;
                if (shb[k]) continue;
            } else {
                if (!sha[k]) r = orient3d_filter(b[0], b[1], b[2], a[k]);
                sa[k] = r;
                if (sha[k]) continue;
            }
            pos += r == 1;
            neg += r == -1;
            other += (r == 0 || r == kUncertain);
        }
        if (other == 0 && (pos == 0 || neg == 0)) return 0;        // strictly on one side but for the shared positions
        generic = generic && other == 0;
    }
    if (generic) {
        const int ia = sa[0] == sa[1] ? 2 : (sa[0] == sa[2] ? 1 : 0), ib = sb[0] == sb[1] ? 2 : (sb[0] == sb[2] ? 1 : 0);
        int c[4];
        bool certain = true;
        for (int x = 1; x <= 2; ++x) {
            const int ja = (ia + x) % 3;
            for (int y = 1; y <= 2; ++y) {
                const int jb = (ib + y) % 3;
                const int r = orient3d_filter(a[ia], a[ja], b[ib], b[jb]);
                certain = certain && r != 0 && r != kUncertain;
                c[2 * (x - 1) + (y - 1)] = r * pick(sa, ia) * pick(sb, ib);         // sgn(-sa) sgn(-sb) = sa sb
            }
        }
        if (certain) return from_orders(c, true, true, 0);
    }
    return pair_exact(a, b, sha, shb, s, stage);
}

// whether the closed exact boxes of two faces overlap on all three axes
NSA_IS_FN bool boxes_overlap(const float (&a)[3][3], const float (&b)[3][3]) {
    for (int k = 0; k < 3; ++k) {
        const float alo = fminf(fminf(a[0][k], a[1][k]), a[2][k]), ahi = fmaxf(fmaxf(a[0][k], a[1][k]), a[2][k]);
        const float blo = fminf(fminf(b[0][k], b[1][k]), b[2][k]), bhi = fmaxf(fmaxf(b[0][k], b[1][k]), b[2][k]);
        if (!(alo <= bhi && blo <= ahi)) return false;
    }
    return true;
}

}  // namespace isect
}  // namespace nsa
