// mesh_raycast.hip -- rays against a triangle mesh (DESIGN 4p, C ABI Section 17): the closest hit (t, face, barycentrics) of each ray,
// or whether it hits anything at all, by the watertight test of Woop, Benthin & Wald ("Watertight Ray/Triangle Intersection", JCGT
// 2013) carried out in float64, over a box hierarchy on Section 16's scheme.  The statement in the header is the contract;
// tests/raycast_ref.py restates it in numpy float64 and the kernels are held to it bit for bit.
//
// Per ray (o, d fp32, taken to float64; inv_k = 1 / d_k):
//     kz = the index of the largest |d_k| (lowest on a tie), kx = kz + 1 mod 3, ky = kx + 1 mod 3, swapped when d_kz < 0
//     Sx = d_kx / d_kz, Sy = d_ky / d_kz, Sz = 1 / d_kz
// Per face (a, b, c):
//     A = a - o ;  Ax = A_kx - Sx A_kz ;  Ay = A_ky - Sy A_kz   (B, C alike)
//     U = Cx By - Cy Bx ;  V = Ax Cy - Ay Cx ;  W = Bx Ay - By Ax
//     miss if (U < 0 or V < 0 or W < 0) and (U > 0 or V > 0 or W > 0) ;  det = (U + V) + W ;  miss if det == 0
//     miss if det < 0 and back faces are culled (ab x ac points along d), if det > 0 and front faces are
//     T = (U (Sz A_kz) + V (Sz B_kz)) + W (Sz C_kz) ;  t = T / det ;  barycentrics (U, V, W) / det
//     miss unless enter <= t <= exit, the slab interval of the ray against the face's own padded box clipped to [tmin, tmax]
// Box of a face: s = the largest |coordinate| of its nine, pad = fp32(s * 2^-20); lo_k = the fp32 below fp32(min_k - pad), hi_k = the
// fp32 above fp32(max_k + pad).  Slab interval of a box: per axis with d_k != 0 the min and max of (lo_k - o_k) inv_k and
// (hi_k - o_k) inv_k; an axis with d_k == 0 passes iff lo_k <= o_k <= hi_k; enter = the largest of the mins and tmin, exit = the
// least of the maxes and tmax; empty when enter > exit.
//
// Why the tree never differs from the brute force.  A node's box is the fp32 min / max of its faces' boxes.  Subtraction and
// multiplication round monotonically, so the interval of a node contains the interval of every face below it: a node with an empty
// interval holds no hit, and one with enter > the best t so far holds none that wins or ties.  The box clause is part of the face
// test itself, so no error analysis of the pruning is needed -- only that the pad is wide enough for the clause never to reject
// what the edge functions accept (header Section 17 states when; tests/test_mesh_raycast_cpu.py asserts it on every case).
//
// Tree.  Section 16's, its topology built by octree_build.hpp: L, the cube, the Morton keys of the centroids, the stable radix argsort,
// a node per level and distinct key prefix, pre-order numbering with `skip`; no atomics.  This unit adds to each sorted face its box
// (inside the shared k_heads) and to each node its box and a table of its (up to eight) children by octant (cleared inside the shared
// k_nodes, filled by k_rc_children).
//
// Walk of one ray (m = 4 [d_x < 0] + 2 [d_y < 0] + [d_z < 0]), from the root:
//     visit(i):  nodes += 1 ;  the node's interval empty -> return ;  closest hit and enter > best t -> return
//                leaf:  for each of its faces in sorted order:  own interval empty, or (closest hit and enter > best t) -> next ;
//                       tested += 1 ;  the face test ;  a hit replaces the best when t < best t, or t == best t and its index is lower
//                       (any-hit: the walk ends at the first hit)
//                else:  for r = 0 .. 7:  the child of octant r xor m, when there is one:  visit(child)
// The children nearer along the ray come first, so the best t shrinks early and the far ones fail `enter > best t`.  Both counts are
// functions of the inputs.  The path (one node index per level, at most 11) lives in LDS, 2816 bytes a wave; the next rank of every
// level is a nibble of one 64-bit register.
//
// Worst cases, slow and never wrong: all centroids in one leaf (every ray through its box tests every face); a face as large as the
// mesh widens every box above it.
#include "ray_tree.hpp"

namespace nsa {
namespace rc {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kTile = 256;              // faces per LDS tile of k_ray_brute: 15 KiB a workgroup

// ---- build: the topology is octree_build.hpp's; the child tables and the boxes of its nodes ---------------------------------------

// one lane per sorted position: every node that begins there enters itself into its parent's table.  The parent of the first node
// of the position is the node of the level above whose range holds the position: it begins at the first position of that prefix
__global__ __launch_bounds__(256) void k_rc_children(uint32_t F, Tree t) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const Head h = *t.head;
    if (i >= F || i >= h.n_usable) return;
    const uint32_t first = t.base[i], cnt = t.base[i + 1] - first;
    if (cnt == 0 || cnt > h.L + 1) return;
    const uint32_t lmin = h.L + 1 - cnt, key = t.skey[i];
    for (uint32_t l = lmin > 0 ? lmin : 1; l <= h.L; ++l) {
        const uint32_t n = first + (l - lmin), sh = 3 * (h.L - l);
        uint32_t parent;
        if (l > lmin) {
            parent = n - 1;
        } else {                                                           // the first position whose key >> (sh + 3) is this one's
            const uint32_t p = key >> (sh + 3);
            uint32_t lo = 0, hi = i;
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if ((t.skey[mid] >> (sh + 3)) < p) lo = mid + 1;
                else hi = mid;
            }
            const uint32_t pf = t.base[lo], pc = t.base[lo + 1] - pf;
            if (pc == 0 || pc > h.L + 1 || l - 1 < h.L + 1 - pc) continue; // (a damaged buffer)
            parent = pf + ((l - 1) - (h.L + 1 - pc));
        }
        t.child[8ull * parent + ((key >> sh) & 7u)] = n;
    }
}

// one wave per node: the fp32 min / max of its faces' boxes
__global__ __launch_bounds__(256) void k_rc_boxes(uint32_t F, Tree t) {
    const uint32_t n = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x & 63;
    if (n >= t.head->n_nodes) return;
    const uint32_t s = t.node[n].begin, e = min(t.end[n], F);
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t pos = s + lane; pos < e; pos += 64) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lo[k] = fminf(lo[k], t.fbox[6ull * pos + k]);
            hi[k] = fmaxf(hi[k], t.fbox[6ull * pos + 3 + k]);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lo[k] = fminf(lo[k], __shfl_xor(lo[k], off));
            hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], off));
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            t.node[n].lo[k] = lo[k];
            t.node[n].hi[k] = hi[k];
        }
    }
}

// ---- query ----------------------------------------------------------------------------------------------------------------------

struct Ray {
    double o[3], inv[3];         // inv_k = 1 / d_k (unused where d_k == 0)
    double Sx, Sy, Sz, tmin, tmax;
    int kx, ky, kz;
    uint32_t zero;               // bit k: d_k == 0
    uint32_t m;                  // 4 [d_x < 0] + 2 [d_y < 0] + [d_z < 0]
};

struct Hit {
    double t, U, V, W, det;
    int32_t face;
};

__device__ __forceinline__ double pick(const double (&x)[3], int k) { return k == 0 ? x[0] : (k == 1 ? x[1] : x[2]); }

// false for a ray with a non-finite component or d == 0
__device__ __forceinline__ bool make_ray(const float* __restrict__ origins, const float* __restrict__ dirs, uint64_t j, double tmin,
                                         double tmax, Ray& r) {
#pragma clang fp contract(off)
    const float of[3] = {origins[3 * j], origins[3 * j + 1], origins[3 * j + 2]};
    const float df[3] = {dirs[3 * j], dirs[3 * j + 1], dirs[3 * j + 2]};
    if (!tri::finite3(of) || !tri::finite3(df) || (df[0] == 0.0f && df[1] == 0.0f && df[2] == 0.0f)) return false;
    const double d[3] = {df[0], df[1], df[2]};
    r.zero = 0;
    r.m = (d[0] < 0.0 ? 4u : 0u) | (d[1] < 0.0 ? 2u : 0u) | (d[2] < 0.0 ? 1u : 0u);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.o[k] = of[k];
        r.inv[k] = 1.0 / d[k];
        if (d[k] == 0.0) r.zero |= 1u << k;
    }
    int kz = 0;
    if (fabs(d[1]) > fabs(d[kz])) kz = 1;
    if (fabs(d[2]) > fabs(pick(d, kz))) kz = 2;
    int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
    const double dz = pick(d, kz);
    if (dz < 0.0) {
        const int s = kx;
        kx = ky;
        ky = s;
    }
    r.kx = kx; r.ky = ky; r.kz = kz;
    r.Sx = pick(d, kx) / dz;
    r.Sy = pick(d, ky) / dz;
    r.Sz = 1.0 / dz;
    r.tmin = tmin;
    r.tmax = tmax;
    return true;
}

// the slab interval of the ray against a box, clipped to [tmin, tmax]; false when it is empty
__device__ __forceinline__ bool slab(const Ray& r, const float* lo, const float* hi, double& enter, double& exit) {
#pragma clang fp contract(off)
    enter = r.tmin;
    exit = r.tmax;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double l = (double)lo[k], h = (double)hi[k];
        if (r.zero & (1u << k)) {
            ok = ok && l <= r.o[k] && r.o[k] <= h;
        } else {
            const double x = (l - r.o[k]) * r.inv[k], y = (h - r.o[k]) * r.inv[k];
            enter = fmax(enter, fmin(x, y));
            exit = fmin(exit, fmax(x, y));
        }
    }
    return ok && enter <= exit;
}

// the face test without its box clause; flags bit 1: cull back faces, bit 2: cull front faces
__device__ __forceinline__ bool woop(const Ray& r, const float (&a)[3], const float (&b)[3], const float (&c)[3], uint32_t flags,
                                     Hit& h) {
#pragma clang fp contract(off)
    const double A[3] = {(double)a[0] - r.o[0], (double)a[1] - r.o[1], (double)a[2] - r.o[2]};
    const double B[3] = {(double)b[0] - r.o[0], (double)b[1] - r.o[1], (double)b[2] - r.o[2]};
    const double C[3] = {(double)c[0] - r.o[0], (double)c[1] - r.o[1], (double)c[2] - r.o[2]};
    const double Az = pick(A, r.kz), Bz = pick(B, r.kz), Cz = pick(C, r.kz);
    const double Ax = pick(A, r.kx) - r.Sx * Az, Ay = pick(A, r.ky) - r.Sy * Az;
    const double Bx = pick(B, r.kx) - r.Sx * Bz, By = pick(B, r.ky) - r.Sy * Bz;
    const double Cx = pick(C, r.kx) - r.Sx * Cz, Cy = pick(C, r.ky) - r.Sy * Cz;
    const double U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    if ((U < 0.0 || V < 0.0 || W < 0.0) && (U > 0.0 || V > 0.0 || W > 0.0)) return false;
    const double det = (U + V) + W;
    if (det == 0.0) return false;
    if ((flags & NSA_RAY_CULL_BACK) && det < 0.0) return false;
    if ((flags & NSA_RAY_CULL_FRONT) && det > 0.0) return false;
    const double T = (U * (r.Sz * Az) + V * (r.Sz * Bz)) + W * (r.Sz * Cz);
    h.t = T / det;
    h.U = U; h.V = V; h.W = W; h.det = det;
    return true;
}

__device__ __forceinline__ bool load_index(const float* __restrict__ v, uint32_t V, const int32_t* __restrict__ f, uint32_t F,
                                           uint32_t g, float (&a)[3], float (&b)[3], float (&c)[3]) {
    if (g >= F) return false;                                              // (not the mesh the tree was built on)
    const int32_t i0 = f[3ull * g], i1 = f[3ull * g + 1], i2 = f[3ull * g + 2];
    if ((uint32_t)i0 >= V || (uint32_t)i1 >= V || (uint32_t)i2 >= V) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a[k] = v[3ull * i0 + k];
        b[k] = v[3ull * i1 + k];
        c[k] = v[3ull * i2 + k];
    }
    return true;
}

__device__ __forceinline__ void store_answer(uint64_t j, bool valid, const Hit& best, double* __restrict__ t, int32_t* __restrict__ face,
                                             double* __restrict__ bary, uint32_t nn, uint32_t nt, uint32_t* __restrict__ n_nodes,
                                             uint32_t* __restrict__ n_tested) {
#pragma clang fp contract(off)
    const double nan = __builtin_nan("");
    const bool hit = valid && best.face >= 0;
    t[j] = valid ? (hit ? best.t : (double)INFINITY) : nan;
    face[j] = hit ? best.face : -1;
    if (bary) {
        bary[3 * j] = hit ? best.U / best.det : nan;
        bary[3 * j + 1] = hit ? best.V / best.det : nan;
        bary[3 * j + 2] = hit ? best.W / best.det : nan;
    }
    if (n_nodes) n_nodes[j] = nn;
    if (n_tested) n_tested[j] = nt;
}

// one face against the ray and the best so far; true when it became the best
__device__ __forceinline__ bool try_face(const Ray& r, const float* box, const float (&a)[3], const float (&b)[3], const float (&c)[3],
                                         uint32_t g, uint32_t flags, bool any, Hit& best, uint32_t& n_tested) {
    double enter, exit;
    if (!slab(r, box, box + 3, enter, exit)) return false;
    if (!any && enter > best.t) return false;
    ++n_tested;
    Hit h;
    if (!woop(r, a, b, c, flags, h)) return false;
    if (!(enter <= h.t && h.t <= exit)) return false;
    if (h.t < best.t || (h.t == best.t && (int32_t)g < best.face)) {
        h.face = (int32_t)g;
        best = h;
        return true;
    }
    return false;
}

// one lane per ray: the ordered walk
__global__ __launch_bounds__(kBlock) void k_ray_tree(Tree t, const float* __restrict__ v, uint32_t V, const int32_t* __restrict__ f,
                                                     uint32_t F, const float* __restrict__ origins, const float* __restrict__ dirs,
                                                     uint32_t m, double tmin, double tmax, uint32_t flags, double* __restrict__ out_t,
                                                     int32_t* __restrict__ out_face, double* __restrict__ out_bary,
                                                     uint32_t* __restrict__ out_nodes, uint32_t* __restrict__ out_tested) {
    __shared__ uint32_t s_path[kMaxLevel + 1][kBlock];
    const uint32_t tid = threadIdx.x;
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + tid;
    if (j >= m) return;
    Ray r;
    Hit best;
    best.t = INFINITY;
    best.face = -1;
    best.U = best.V = best.W = best.det = 0.0;
    const bool valid = make_ray(origins, dirs, j, tmin, tmax, r);
    const bool any = (flags & NSA_RAY_ANY_HIT) != 0;
    uint32_t nn = 0, nt = 0;
    const Head* hd = t.head;
    const uint32_t n_nodes = hd->n_nodes, L = min(hd->L, kMaxLevel), n_usable = min(hd->n_usable, F);
    if (valid && n_nodes > 0) {
        uint32_t cur = 0;
        int l = 0;
        uint64_t ranks = 0;                                                // nibble l: the next rank of the node at level l
        for (;;) {
            ++nn;
            const Node nd = t.node[cur];
            double enter, exit;
            bool down = false;
            if (slab(r, nd.lo, nd.hi, enter, exit) && (any || !(enter > best.t))) {
                if ((nd.skip & kLeafBit) || l >= (int)L) {
                    const uint32_t e = min(t.end[cur], n_usable);
                    bool done = false;
                    for (uint32_t pos = nd.begin; pos < e && !done; ++pos) {
                        const uint32_t g = t.order[pos];
                        float a[3], b[3], c[3];
                        if (!load_index(v, V, f, F, g, a, b, c)) continue;
                        const bool won = try_face(r, t.fbox + 6ull * pos, a, b, c, g, flags, any, best, nt);
                        done = any && won;
                    }
                    if (done) break;
                } else {
                    s_path[l][tid] = cur;
                    ranks &= ~(0xFull << (4 * l));
                    down = true;
                }
            }
            if (!down) --l;
            bool found = false;
            while (l >= 0) {
                const uint32_t p = s_path[l][tid];
                uint32_t rank = (uint32_t)(ranks >> (4 * l)) & 0xFu, c = 0;
                while (rank < 8 && c == 0) {
                    c = t.child[8ull * p + (rank ^ r.m)];
                    ++rank;
                }
                ranks = (ranks & ~(0xFull << (4 * l))) | ((uint64_t)rank << (4 * l));
                if (c > p && c < n_nodes) {                                // (c <= p: a damaged buffer, never loop)
                    cur = c;
                    ++l;
                    found = true;
                    break;
                }
                --l;
            }
            if (!found) break;
        }
    }
    store_answer(j, valid, best, out_t, out_face, out_bary, nn, nt, out_nodes, out_tested);
}

// one lane per ray, every usable face in sorted order: tiles of kTile faces and their boxes through LDS
__global__ __launch_bounds__(kBlock) void k_ray_brute(Tree t, const float* __restrict__ v, uint32_t V, const int32_t* __restrict__ f,
                                                      uint32_t F, const float* __restrict__ origins, const float* __restrict__ dirs,
                                                      uint32_t m, double tmin, double tmax, uint32_t flags, double* __restrict__ out_t,
                                                      int32_t* __restrict__ out_face, double* __restrict__ out_bary,
                                                      uint32_t* __restrict__ out_nodes, uint32_t* __restrict__ out_tested) {
    __shared__ float s_face[kTile][15];
    __shared__ uint32_t s_index[kTile];
    const uint32_t tid = threadIdx.x;
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + tid;
    const bool live = j < m;
    Ray r;
    Hit best;
    best.t = INFINITY;
    best.face = -1;
    best.U = best.V = best.W = best.det = 0.0;
    const bool valid = live && make_ray(origins, dirs, j, tmin, tmax, r);
    const bool any = (flags & NSA_RAY_ANY_HIT) != 0;
    const uint32_t n_usable = min(t.head->n_usable, F);
    uint32_t nt = 0;
    bool done = false;
    for (uint32_t base = 0; base < n_usable; base += kTile) {
        const uint32_t count = min(kTile, n_usable - base);
        if (tid < count) {
            float a[3] = {0.0f, 0.0f, 0.0f}, b[3] = {0.0f, 0.0f, 0.0f}, c[3] = {0.0f, 0.0f, 0.0f};
            const uint32_t g = t.order[base + tid];
            const bool ok = load_index(v, V, f, F, g, a, b, c);
            s_index[tid] = ok ? g : 0xFFFFFFFFu;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                s_face[tid][k] = a[k];
                s_face[tid][3 + k] = b[k];
                s_face[tid][6 + k] = c[k];
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) s_face[tid][9 + k] = t.fbox[6ull * (base + tid) + k];
        }
        __syncthreads();
        if (valid && !done) {
            for (uint32_t s = 0; s < count && !done; ++s) {
                const uint32_t g = s_index[s];
                if (g == 0xFFFFFFFFu) continue;
                const float a[3] = {s_face[s][0], s_face[s][1], s_face[s][2]};
                const float b[3] = {s_face[s][3], s_face[s][4], s_face[s][5]};
                const float c[3] = {s_face[s][6], s_face[s][7], s_face[s][8]};
                const bool won = try_face(r, &s_face[s][9], a, b, c, g, flags, any, best, nt);
                done = any && won;
            }
        }
        __syncthreads();
    }
    if (!live) return;
    store_answer(j, valid, best, out_t, out_face, out_bary, 0, nt, out_nodes, out_tested);
}

}  // namespace rc
}  // namespace nsa

extern "C" {

uint64_t nsa_tri_ray_workspace(uint32_t n_faces) {
    using namespace nsa;
    if (n_faces == 0 || n_faces > tri::kMaxCount) return 0;
    return rc::carve(nullptr, n_faces, nullptr);
}

int nsa_tri_ray_build(const float* verts, uint32_t n_verts, const int32_t* faces, uint32_t n_faces, void* tree, uint32_t* info,
                      nsa_stream_t stream) {
    using namespace nsa;
    using namespace nsa::rc;
    if (n_verts > tri::kMaxCount || n_faces > tri::kMaxCount) return NSA_EBADARG;
    if (n_faces == 0) return NSA_OK;
    if (!verts || !faces || !tree || n_verts == 0) return NSA_EBADARG;
    Tree t;
    carve(tree, n_faces, &t);
    const uint32_t nb = (n_faces + 255) / 256;
    hipStream_t s = (hipStream_t)stream;
    launch_begin();
    octree::build(verts, n_verts, faces, n_faces, t, s);
    hipLaunchKernelGGL(k_rc_children, dim3(nb), dim3(256), 0, s, n_faces, t);
    hipLaunchKernelGGL(k_rc_boxes, dim3((uint32_t)((max_nodes(n_faces) + 3) / 4)), dim3(256), 0, s, n_faces, t);
    if (info) hipLaunchKernelGGL(octree::k_info<Tree>, dim3(1), dim3(1), 0, s, t, info);
    return launch_end();
}

int nsa_tri_ray_cast(const void* tree, const float* verts, uint32_t n_verts, const int32_t* faces, uint32_t n_faces,
                     const float* origins, const float* dirs, uint32_t n_rays, double tmin, double tmax, uint32_t flags, double* t,
                     int32_t* face, double* bary, uint32_t* n_nodes, uint32_t* n_tested, nsa_stream_t stream) {
    using namespace nsa;
    using namespace nsa::rc;
    const uint32_t known = NSA_RAY_ANY_HIT | NSA_RAY_CULL_BACK | NSA_RAY_CULL_FRONT | NSA_RAY_BRUTE;
    if (tmin != tmin || tmax != tmax || (flags & ~known) || ((flags & NSA_RAY_CULL_BACK) && (flags & NSA_RAY_CULL_FRONT)))
        return NSA_EBADARG;
    if (n_verts > tri::kMaxCount || n_faces > tri::kMaxCount || n_rays > tri::kMaxCount) return NSA_EBADARG;
    if (n_rays == 0 || n_faces == 0) return NSA_OK;
    if (!tree || !verts || !faces || n_verts == 0 || !origins || !dirs || !t || !face) return NSA_EBADARG;
    Tree tr;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((n_rays + kBlock - 1) / kBlock);
    launch_begin();
    carve(const_cast<void*>(tree), n_faces, &tr);
    if (flags & NSA_RAY_BRUTE)
        hipLaunchKernelGGL(k_ray_brute, grid, dim3(kBlock), 0, s, tr, verts, n_verts, faces, n_faces, origins, dirs, n_rays, tmin, tmax,
                           flags, t, face, bary, n_nodes, n_tested);
    else
        hipLaunchKernelGGL(k_ray_tree, grid, dim3(kBlock), 0, s, tr, verts, n_verts, faces, n_faces, origins, dirs, n_rays, tmin, tmax,
                           flags, t, face, bary, n_nodes, n_tested);
    return launch_end();
}

}  // extern "C"
