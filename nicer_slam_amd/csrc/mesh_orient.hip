// mesh_orient.hip -- a consistent winding for a triangle mesh, its orientability, and which of the two consistent windings of a closed
// component points outward, on the device (C ABI Section 20).  Input: the edge table of Section 18 for the same mesh.
//
// Winding: the union-find of uf_passes.hpp, unchanged, over the orientation double cover (2 F nodes: 2 f is face f as given, 2 f + 1
// is face f reversed).  One lane per edge; an edge with exactly two half-edges unites the matching sheets of its two faces, straight
// when they agree, crossed when they do not.  parent[x] <= x throughout, so a root is the smallest node of its tree whatever the
// interleaving: the label of a face is min(root(2 f), root(2 f + 1)) >> 1, its component is orientable when the two roots differ, and
// it is flipped when it lies on the sheet of its component's smallest face reversed.  Integers only; no atomics outside the union-find
// (and one atomicOr of its cap report).  The two pass bodies live in orient_passes.hpp, which also compiles as host C++.
//
// Outward by volume: the faces are sorted by label with the stable radix argsort, so a component is one run in ascending face order
// that starts at its smallest face.  Every face contributes (s det, perm, 1, open) -- float64 signed and absolute six-product sums about
// o, a face count and whether one of its edges is not of count 2.  A block of 1024 sorted positions adds them with a segmented
// Hillis-Steele scan whose shape depends on the position within the run alone; a run inside one block is final there, a run across
// blocks leaves one partial per block, which one workgroup (the block where the run ends) adds in a fixed strided order and a fixed
// tree.  No atomics: every sum is a function of the arguments alone and bit-reproducible.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/nicer_slam_amd.h"
#include "block_scan.hpp"
#include "grid_common.hpp"
#include "orient_passes.hpp"
#include "radix_sort.hpp"
#include "uf_passes.hpp"

namespace nsa {

constexpr uint32_t kOrMaxVerts = 0x7FFFFFFFu;
constexpr uint32_t kOrMaxFaces = 0x7FFFFFFFu / 3u;      // 2 F < 3 F < 2^31
constexpr uint32_t kOrBlock = 1024;                     // block of the partial counts and of the segmented scan
constexpr uint32_t kOrSpan = 256;                       // workgroup that adds the per-block partials of a run across blocks
constexpr uint32_t kOrBadOrder = 4u;                    // status: a sort order or a run start outside its range

using scan::ull;

__host__ __device__ inline uint64_t or_align(uint64_t b) { return (b + 255) & ~uint64_t(255); }
__host__ __device__ inline uint64_t or_blocks(uint64_t n) { return (n + kOrBlock - 1) / kOrBlock; }

// ---- consistent winding ---------------------------------------------------------------------------------------------------------------

struct OrientWork {
    int32_t* parent;             // [2 F]: union-find over the double cover
    uint32_t* part;              // [4 nbf]: components, non-orientable components, flipped faces and the status of a block of faces
    uint32_t* status;            // [1]: step caps of the unions
};

__host__ __device__ inline uint64_t orient_carve(void* ws, uint32_t F, OrientWork* out) {
    char* base = static_cast<char*>(ws);
    const uint64_t a = or_align(8ull * F), b = or_align(16 * or_blocks(F));
    if (out) {
        out->parent = reinterpret_cast<int32_t*>(base);
        out->part = reinterpret_cast<uint32_t*>(base ? base + a : nullptr);
        out->status = reinterpret_cast<uint32_t*>(base ? base + a + b : nullptr);
    }
    return a + b + or_align(4);
}

__global__ __launch_bounds__(256) void k_or_init(OrientWork w, uint32_t N) {
    const uint32_t x = blockIdx.x * 256 + threadIdx.x;
    if (x == 0) *w.status = 0;
    if (x < N) w.parent[x] = (int32_t)x;
}

// one lane per edge; E comes from the totals nsa_mesh_edges left on the device
__global__ __launch_bounds__(256) void k_or_unite(OrientWork w, uint32_t F, const int32_t* __restrict__ faces,
                                                  const int32_t* __restrict__ edge_start, const int32_t* __restrict__ edge_halfedges,
                                                  const ull* __restrict__ edge_totals) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    const uint32_t E = scan::capped(edge_totals[0], 3u * F);
    uint32_t status = 0;
    orient_pass_join(w.parent, F, faces, edge_start, edge_halfedges, e, E, &status);
    if (status) atomicOr(w.status, status);             // (the union-find's own cap report)
}

__global__ __launch_bounds__(kOrBlock) void k_or_label(OrientWork w, uint32_t F, const int32_t* __restrict__ face_edges,
                                                       int32_t* __restrict__ orient_label, uint8_t* __restrict__ orientable,
                                                       uint8_t* __restrict__ flip) {
    const uint32_t f = blockIdx.x * kOrBlock + threadIdx.x;
    bool flag[4] = {false, false, false, false};
    if (f < F) {
        uint32_t status = 0;
        uint8_t o, fl;
        const int32_t l = orient_pass_label(w.parent, F, face_edges, f, &o, &fl, &status);
        orient_label[f] = l;
        orientable[f] = o;
        flip[f] = fl;
        flag[0] = l == (int32_t)f;
        flag[1] = l == (int32_t)f && !o;
        flag[2] = fl != 0;
        flag[3] = status != 0;
    }
    uint32_t pre[4], out[4];
    scan::flag_scan<4, kOrBlock>(flag, pre, out);
    if (threadIdx.x == 0) {
        w.part[4ull * blockIdx.x] = out[0];
        w.part[4ull * blockIdx.x + 1] = out[1];
        w.part[4ull * blockIdx.x + 2] = out[2];
        w.part[4ull * blockIdx.x + 3] = out[3] ? kUfCapFind : 0u;
    }
}

__global__ __launch_bounds__(kOrBlock) void k_or_totals(OrientWork w, uint32_t nbf, ull* __restrict__ totals) {
    ull t[4];
    scan::block_totals<3, 1, kOrBlock>(w.part, nbf, t);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) totals[k] = t[k];
        totals[3] = t[3] | *w.status;
    }
}

// ---- outward by volume ----------------------------------------------------------------------------------------------------------------

struct Partial {                 // what a run of faces adds up to
    double s, p;                 // six times the signed volume about o and its absolute-value companion
    uint32_t n, open;            // faces; faces with an edge that is not of count 2
};

struct VolumeWork {
    uint32_t* keys[2];           // [F] each: radix ping-pong
    uint32_t* tmp;               // [F]
    uint32_t* order;             // [F]: faces sorted stably by label, the faces that do not contribute last
    uint32_t* counts;            // [256 * 256]
    uint32_t* pos;               // [F]: the sorted position of face f
    Partial* first;              // [nbf]: the piece of a block that continues a run from the block before
    Partial* last;               // [nbf]: the piece that starts in a block and goes on into the next
    uint32_t* part;              // [5 nbf]: closed, decided, toggled components, flipped faces and the status of a block of faces
};

__host__ __device__ inline uint64_t volume_carve(void* ws, uint32_t F, VolumeWork* out) {
    const uint64_t nbf = or_blocks(F);
    char* base = static_cast<char*>(ws);
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) { char* p = base ? base + o : nullptr; o += or_align(bytes ? bytes : 1); return p; };
    VolumeWork w;
    w.keys[0] = reinterpret_cast<uint32_t*>(take(4ull * F));
    w.keys[1] = reinterpret_cast<uint32_t*>(take(4ull * F));
    w.tmp = reinterpret_cast<uint32_t*>(take(4ull * F));
    w.order = reinterpret_cast<uint32_t*>(take(4ull * F));
    w.counts = reinterpret_cast<uint32_t*>(take(4ull * kRadixCountWords));
    w.pos = reinterpret_cast<uint32_t*>(take(4ull * F));
    w.first = reinterpret_cast<Partial*>(take(sizeof(Partial) * nbf));
    w.last = reinterpret_cast<Partial*>(take(sizeof(Partial) * nbf));
    w.part = reinterpret_cast<uint32_t*>(take(20 * nbf));
    if (out) *out = w;
    return o;
}

__device__ __forceinline__ uint32_t ov_key(const int32_t* __restrict__ orient_label, uint32_t f, uint32_t F) {
    const int32_t l = orient_label[f];
    return l >= 0 && (uint32_t)l < F ? (uint32_t)l : F;
}

// the key of sorted position i < F: the label of its face, F for a face that does not contribute or an order outside its range
__device__ __forceinline__ uint32_t ov_key_at(const VolumeWork& w, const int32_t* __restrict__ orient_label, uint32_t i, uint32_t F) {
    const uint32_t f = w.order[i];
    return f < F ? ov_key(orient_label, f, F) : F;
}

__global__ __launch_bounds__(256) void k_ov_keys(VolumeWork w, uint32_t F, const int32_t* __restrict__ orient_label) {
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    if (f < F) w.keys[0][f] = ov_key(orient_label, f, F);
}

__global__ __launch_bounds__(256) void k_ov_pos(VolumeWork w, uint32_t F) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= F) return;
    const uint32_t f = w.order[i];
    if (f < F) w.pos[f] = i;                            // (always: the order is a permutation of [0, F))
}

// six times the signed volume of the tetrahedron (o, a, b, c) and the same six products with absolute values; every operation is
// rounded on its own
__device__ __forceinline__ void ov_term(const float* __restrict__ verts, const int32_t v[3], const double o[3], double* det, double* perm) {
#pragma clang fp contract(off)
    double a[3], b[3], c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a[k] = (double)verts[3ull * v[0] + k] - o[k];
        b[k] = (double)verts[3ull * v[1] + k] - o[k];
        c[k] = (double)verts[3ull * v[2] + k] - o[k];
    }
    *det = (a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2])) + a[2] * (b[0] * c[1] - b[1] * c[0]);
    const double A[3] = {fabs(a[0]), fabs(a[1]), fabs(a[2])}, B[3] = {fabs(b[0]), fabs(b[1]), fabs(b[2])},
                 C[3] = {fabs(c[0]), fabs(c[1]), fabs(c[2])};
    *perm = (A[0] * (B[1] * C[2] + B[2] * C[1]) + A[1] * (B[2] * C[0] + B[0] * C[2])) + A[2] * (B[0] * C[1] + B[1] * C[0]);
}

// the sums of a whole component: S, P, the face count and the flags closed (1), decided (2), toggled (4)
__device__ __forceinline__ void ov_final(uint32_t l, const Partial& x, const uint8_t* __restrict__ orientable, double* __restrict__ comp_S,
                                         double* __restrict__ comp_P, int32_t* __restrict__ comp_n, uint8_t* __restrict__ comp_flags) {
    const double S = x.s / 6.0, P = x.p / 6.0;
    const bool closed = x.open == 0;
    const bool decided = closed && orientable[l] != 0 && fabs(S) > ((double)(x.n + 16u) * 0x1p-52) * P;
    comp_S[l] = S;
    comp_P[l] = P;
    comp_n[l] = (int32_t)x.n;
    comp_flags[l] = (uint8_t)((closed ? 1 : 0) | (decided ? 2 : 0) | (decided && S < 0.0 ? 4 : 0));
}

// a block of 1024 sorted positions: the terms, their segmented scan, and what each run piece in the block adds up to
__global__ __launch_bounds__(kOrBlock) void k_ov_block(VolumeWork w, uint32_t F, uint32_t V, const float* __restrict__ verts,
                                                       const int32_t* __restrict__ faces, const int32_t* __restrict__ face_edges,
                                                       const int32_t* __restrict__ edge_start, const int32_t* __restrict__ orient_label,
                                                       const uint8_t* __restrict__ orientable, const uint8_t* __restrict__ flip,
                                                       const float* __restrict__ origin, double* __restrict__ comp_S,
                                                       double* __restrict__ comp_P, int32_t* __restrict__ comp_n,
                                                       uint8_t* __restrict__ comp_flags) {
    __shared__ double ss[kOrBlock], sp[kOrBlock];
    __shared__ uint32_t sn[kOrBlock], so[kOrBlock], sk[kOrBlock];
    const uint32_t t = threadIdx.x, base = blockIdx.x * kOrBlock, i = base + t, H = 3u * F;
    uint32_t key = F, start = i;
    Partial x = {0.0, 0.0, 0u, 0u};
    if (i < F) {
        const uint32_t f = w.order[i];
        if (f < F) key = ov_key(orient_label, f, F);     // (always: the order is a permutation; k_ov_apply reports otherwise)
        if (key < F) {
            start = w.pos[key];
            if (start > i) start = i;                   // (never: a run starts at its smallest face; k_ov_apply reports it)
            int32_t v[3] = {faces[3ull * f], faces[3ull * f + 1], faces[3ull * f + 2]};
            x.n = 1;
            if (uf_valid_face(v[0], v[1], v[2], V)) {
                const double o[3] = {(double)origin[0], (double)origin[1], (double)origin[2]};
                double det, perm;
                ov_term(verts, v, o, &det, &perm);
                x.s = flip[f] ? -det : det;
                x.p = perm;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int32_t e = face_edges[3ull * f + k];
                if (e < 0 || (uint32_t)e >= H || edge_start[e + 1] - edge_start[e] != 2) x.open = 1;
            }
        }
    }
    const uint32_t lstart = (start > base ? start : base) - base;
    ss[t] = x.s;
    sp[t] = x.p;
    sn[t] = x.n;
    so[t] = x.open;
    sk[t] = key;
    __syncthreads();
    for (uint32_t d = 1; d < kOrBlock; d <<= 1) {
        const bool take = t >= d && t - d >= lstart;
        Partial y = {0.0, 0.0, 0u, 0u};
        if (take) y = Partial{ss[t - d], sp[t - d], sn[t - d], so[t - d]};
        __syncthreads();
        if (take) {
            x.s = y.s + x.s;
            x.p = y.p + x.p;
            x.n += y.n;
            x.open += y.open;
            ss[t] = x.s;
            sp[t] = x.p;
            sn[t] = x.n;
            so[t] = x.open;
        }
        __syncthreads();
    }
    if (key >= F) return;
    const bool last_lane = t + 1 == kOrBlock;
    const uint32_t next = i + 1 >= F ? F : last_lane ? ov_key_at(w, orient_label, i + 1, F) : sk[t + 1];
    const bool goes_on = next == key;
    if (goes_on && !last_lane) return;                  // inside its piece: the piece's last lane holds its sums
    if (start < base) w.first[blockIdx.x] = x;          // continues a run from the block before (and may go on)
    else if (goes_on) w.last[blockIdx.x] = x;           // starts here and goes on into the next block
    else ov_final(key, x, orientable, comp_S, comp_P, comp_n, comp_flags);
}

// one workgroup per block of sorted positions: where a run that started in an earlier block ends, its per-block partials -- last[b0],
// first[b0 + 1], ..., first[b] -- are added, thread t taking the terms t, t + 256, ... in order, then a fixed tree over the threads
__global__ __launch_bounds__(kOrSpan) void k_ov_span(VolumeWork w, uint32_t F, const int32_t* __restrict__ orient_label,
                                                     const uint8_t* __restrict__ orientable, double* __restrict__ comp_S,
                                                     double* __restrict__ comp_P, int32_t* __restrict__ comp_n,
                                                     uint8_t* __restrict__ comp_flags) {
    __shared__ double ss[kOrSpan], sp[kOrSpan];
    __shared__ uint32_t sn[kOrSpan], so[kOrSpan];
    const uint32_t t = threadIdx.x, b = blockIdx.x, i0 = b * kOrBlock;
    if (b == 0 || i0 >= F) return;                      // (every test up to the barrier is the same for the whole workgroup)
    const uint32_t key = ov_key_at(w, orient_label, i0, F);
    if (key >= F) return;
    const uint32_t start = w.pos[key];
    if (start >= i0) return;                            // a run starts here
    const uint64_t i1 = (uint64_t)i0 + kOrBlock;
    if (i1 < F && ov_key_at(w, orient_label, (uint32_t)i1, F) == key) return;    // the run goes on: a later block adds it
    const uint32_t b0 = start / kOrBlock, n = b - b0 + 1;
    Partial x = {0.0, 0.0, 0u, 0u};
    for (uint32_t j = t; j < n; j += kOrSpan) {
        const Partial y = j == 0 ? w.last[b0] : w.first[b0 + j];
        x.s += y.s;
        x.p += y.p;
        x.n += y.n;
        x.open += y.open;
    }
    ss[t] = x.s;
    sp[t] = x.p;
    sn[t] = x.n;
    so[t] = x.open;
    __syncthreads();
    for (uint32_t o = kOrSpan / 2; o > 0; o >>= 1) {
        if (t < o) {
            ss[t] += ss[t + o];
            sp[t] += sp[t + o];
            sn[t] += sn[t + o];
            so[t] += so[t + o];
        }
        __syncthreads();
    }
    if (t == 0) ov_final(key, Partial{ss[0], sp[0], sn[0], so[0]}, orientable, comp_S, comp_P, comp_n, comp_flags);
}

// one lane per face: the flip after its component's toggle; the counts over the components (at their smallest faces) and the faces;
// status when the sort order is not the permutation it must be or a run does not start at its label
__global__ __launch_bounds__(kOrBlock) void k_ov_apply(VolumeWork w, uint32_t F, const int32_t* __restrict__ orient_label,
                                                       const uint8_t* __restrict__ flip, const uint8_t* __restrict__ comp_flags,
                                                       uint8_t* __restrict__ flip_out) {
    const uint32_t f = blockIdx.x * kOrBlock + threadIdx.x;
    bool flag[5] = {false, false, false, false, false};
    if (f < F) {
        const uint32_t l = ov_key(orient_label, f, F), p = w.pos[f];
        flag[4] = p >= F || w.order[p] != f || (l < F && w.pos[l] > p);
        const uint8_t c = l < F ? comp_flags[l] : 0;
        const uint8_t out = (uint8_t)((flip[f] != 0) != ((c & 4) != 0));
        flip_out[f] = out;
        flag[0] = l == f && (c & 1);
        flag[1] = l == f && (c & 2);
        flag[2] = l == f && (c & 4);
        flag[3] = out != 0;
    }
    uint32_t pre[5], out[5];
    scan::flag_scan<5, kOrBlock>(flag, pre, out);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) w.part[5ull * blockIdx.x + k] = out[k];
        w.part[5ull * blockIdx.x + 4] = out[4] ? kOrBadOrder : 0u;
    }
}

__global__ __launch_bounds__(kOrBlock) void k_ov_totals(VolumeWork w, uint32_t nbf, ull* __restrict__ totals) {
    ull t[5];
    scan::block_totals<4, 1, kOrBlock>(w.part, nbf, t);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 5; ++k) totals[k] = t[k];
    }
}

}  // namespace nsa

extern "C" {

uint64_t nsa_mesh_orient_workspace(uint32_t n_faces) {
    if (n_faces == 0 || n_faces > nsa::kOrMaxFaces) return 0;
    return nsa::orient_carve(nullptr, n_faces, nullptr);
}

int nsa_mesh_orient(const int32_t* faces, uint32_t n_faces, const int32_t* face_edges, const int32_t* edge_start,
                    const int32_t* edge_halfedges, const uint64_t* edge_totals, void* workspace, int32_t* orient_label,
                    uint8_t* orientable, uint8_t* flip, uint64_t* totals, nsa_stream_t stream) {
    using namespace nsa;
    const uint32_t F = n_faces;
    if (F > kOrMaxFaces) return NSA_EBADARG;
    if (F == 0) return NSA_OK;
    if (!faces || !face_edges || !edge_start || !edge_halfedges || !edge_totals || !workspace || !orient_label || !orientable || !flip ||
        !totals)
        return NSA_EBADARG;
    OrientWork w;
    orient_carve(workspace, F, &w);
    const uint32_t H = 3u * F, nbf = (uint32_t)or_blocks(F);
    hipStream_t s = (hipStream_t)stream;
    launch_begin();
    hipLaunchKernelGGL(k_or_init, dim3((2u * F + 255) / 256), dim3(256), 0, s, w, 2u * F);
    hipLaunchKernelGGL(k_or_unite, dim3((H + 255) / 256), dim3(256), 0, s, w, F, faces, edge_start, edge_halfedges,
                       reinterpret_cast<const ull*>(edge_totals));
    hipLaunchKernelGGL(k_or_label, dim3(nbf), dim3(kOrBlock), 0, s, w, F, face_edges, orient_label, orientable, flip);
    hipLaunchKernelGGL(k_or_totals, dim3(1), dim3(kOrBlock), 0, s, w, nbf, reinterpret_cast<ull*>(totals));
    return launch_end();
}

uint64_t nsa_mesh_orient_volume_workspace(uint32_t n_faces) {
    if (n_faces == 0 || n_faces > nsa::kOrMaxFaces) return 0;
    return nsa::volume_carve(nullptr, n_faces, nullptr);
}

int nsa_mesh_orient_volume(const float* verts, uint32_t n_verts, const int32_t* faces, uint32_t n_faces, const int32_t* face_edges,
                           const int32_t* edge_start, const int32_t* orient_label, const uint8_t* orientable, const uint8_t* flip,
                           const float* origin, void* workspace, double* comp_S, double* comp_P, int32_t* comp_n, uint8_t* comp_flags,
                           uint8_t* flip_out, uint64_t* totals, nsa_stream_t stream) {
    using namespace nsa;
    const uint32_t F = n_faces, V = n_verts;
    if (F > kOrMaxFaces || V > kOrMaxVerts) return NSA_EBADARG;
    if (F == 0) return NSA_OK;
    if (!faces || !face_edges || !edge_start || !orient_label || !orientable || !flip || !origin || !workspace || !comp_S || !comp_P ||
        !comp_n || !comp_flags || !flip_out || !totals || (V && !verts))
        return NSA_EBADARG;
    VolumeWork w;
    volume_carve(workspace, F, &w);
    const uint32_t nbf = (uint32_t)or_blocks(F);
    uint32_t bits = 1;
    while ((1ull << bits) <= (uint64_t)F) ++bits;             // keys are <= F
    hipStream_t s = (hipStream_t)stream;
    launch_begin();
    hipLaunchKernelGGL(k_ov_keys, dim3((F + 255) / 256), dim3(256), 0, s, w, F, orient_label);
    radix_argsort(w.keys, w.tmp, w.order, w.counts, F, 0, (bits + 7) / 8, stream);
    hipLaunchKernelGGL(k_ov_pos, dim3((F + 255) / 256), dim3(256), 0, s, w, F);
    hipLaunchKernelGGL(k_ov_block, dim3(nbf), dim3(kOrBlock), 0, s, w, F, V, verts, faces, face_edges, edge_start, orient_label,
                       orientable, flip, origin, comp_S, comp_P, comp_n, comp_flags);
    hipLaunchKernelGGL(k_ov_span, dim3(nbf), dim3(kOrSpan), 0, s, w, F, orient_label, orientable, comp_S, comp_P, comp_n, comp_flags);
    hipLaunchKernelGGL(k_ov_apply, dim3(nbf), dim3(kOrBlock), 0, s, w, F, orient_label, flip, comp_flags, flip_out);
    hipLaunchKernelGGL(k_ov_totals, dim3(1), dim3(kOrBlock), 0, s, w, nbf, reinterpret_cast<ull*>(totals));
    return launch_end();
}

}  // extern "C"
