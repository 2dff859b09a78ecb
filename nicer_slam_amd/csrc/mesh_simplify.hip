// mesh_simplify.hip -- vertex clustering (Rossignac-Borrel) with error-quadric placement (Lindstrom's out-of-core form, with a
// Tikhonov pull towards the cluster mean in place of his truncated SVD) on the device (C ABI Section 19).  There is no
// reference program: the reference's users reach for open3d's simplify_vertex_clustering or Meshlab here.
//
// nsa_mesh_cluster, the combinatorial half (integers only once the cell of a vertex is known): a 63-bit cell key per vertex; the used
// vertices sorted by key with two stable radix argsorts (radix_sort.hpp), low word then high word, each with only the 8-bit passes
// the grid's width needs; run heads and one exclusive scan give the cluster numbers.  Faces map to cluster triples, rotate their
// smallest number to the front, and three chained argsorts (third, second, first number) bring equal triples together in ascending
// face index: the head of a run survives.  Two more scans compact the survivors in face order and number the clusters they name.
//
// nsa_mesh_cluster_place, the float half: the vertices sorted by cluster and the (face, corner) incidences sorted by the cluster of
// the corner vertex, both stable, so each cluster owns a run in ascending vertex index and a run in ascending 3 f + corner.  One lane
// per output vertex walks its two runs in that order: float64, every operation rounded on its own, no atomics -- the sums have one
// fixed order and the result is bit-reproducible.
//
// Counts are per-wave popcounts added with integer atomics (sums of integers: any order gives the same); no floating-point atomic
// exists in this file.  The three scans are block_scan.hpp's: flag_scan inside a block of kMsBlock, k_offsets over the block counts.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include "../../include/nicer_slam_amd.h"
#include "block_scan.hpp"
#include "grid_common.hpp"
#include "radix_sort.hpp"

namespace nsa {

constexpr uint32_t kMsMaxVerts = 0x7FFFFFFFu;
constexpr uint32_t kMsMaxFaces = 0x7FFFFFFFu / 3u;      // 3 F < 2^31
constexpr uint32_t kMsMaxCells = 1u << 21;              // cells per axis: three 21-bit fields in one 63-bit key
constexpr uint32_t kMsBlock = 1024;                     // block of the scans
constexpr uint64_t kMsNoKey = ~0ull;                    // a vertex that is not in the grid
constexpr uint32_t kMsBadOrder = 1u;                    // status: a sort order named an element outside its range

using scan::ull;

enum { kTotK = 0, kTotContrib, kTotUsed, kTotOutside, kTotCollapsed, kTotDuplicate, kTotVerts, kTotFaces, kTotStatus, kTotWords };

struct MsGrid {
    double o[3], h;
    uint32_t n;                  // cells per axis
};

__host__ __device__ inline uint64_t ms_align(uint64_t b) { return (b + 255) & ~uint64_t(255); }
__host__ __device__ inline uint64_t ms_blocks(uint64_t n) { return (n + kMsBlock - 1) / kMsBlock; }
__host__ __device__ inline uint32_t ms_bitlen(uint32_t x) {
    uint32_t b = 0;
    while (x) {
        ++b;
        x >>= 1;
    }
    return b;
}

struct ClusterWork {             // views into the caller's workspace (nsa_mesh_cluster_workspace bytes); P = max(V, F)
    uint64_t* key;               // [V]: the cell key, kMsNoKey outside the grid
    uint32_t* used;              // [V]: 1 for a vertex of a contributing face
    uint32_t* cmark;             // [V]: 1 for a cluster that a surviving face names
    uint32_t* keys[2];           // [P] each: radix ping-pong
    uint32_t* tmp;               // [P + 1]: radix payload ping-pong
    uint32_t* oa;                // [P]: first argsort of a chain
    uint32_t* ob;                // [P]: second (positions of the first)
    uint32_t* oc;                // [P]: third (positions of the second); the sorted vertices in the vertex stage
    uint32_t* pp;                // [P]: oa[ob[.]]
    uint32_t* t[3];              // [F] each: the rotated cluster triple of a face, V for a face that cannot survive
    uint32_t* flag;              // [P]: run heads of the sorted vertices, then the surviving faces
    uint32_t* counts;            // [256 * 256]
    uint32_t* bcount;            // [blocks(P)]: flags per block of 1024, then their exclusive scan
};

__host__ __device__ inline uint64_t cluster_carve(void* ws, uint32_t V, uint32_t F, ClusterWork* out) {
    const uint64_t P = V > F ? V : F;
    char* base = static_cast<char*>(ws);
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) { char* p = base ? base + o : nullptr; o += ms_align(bytes ? bytes : 1); return p; };
    ClusterWork w;
    w.key = reinterpret_cast<uint64_t*>(take(8ull * V));
    w.used = reinterpret_cast<uint32_t*>(take(4ull * V));
    w.cmark = reinterpret_cast<uint32_t*>(take(4ull * V));
    w.keys[0] = reinterpret_cast<uint32_t*>(take(4 * P));
    w.keys[1] = reinterpret_cast<uint32_t*>(take(4 * P));
    w.tmp = reinterpret_cast<uint32_t*>(take(4 * (P + 1)));
    w.oa = reinterpret_cast<uint32_t*>(take(4 * P));
    w.ob = reinterpret_cast<uint32_t*>(take(4 * P));
    w.oc = reinterpret_cast<uint32_t*>(take(4 * P));
    w.pp = reinterpret_cast<uint32_t*>(take(4 * P));
    for (int k = 0; k < 3; ++k) w.t[k] = reinterpret_cast<uint32_t*>(take(4ull * F));
    w.flag = reinterpret_cast<uint32_t*>(take(4 * P));
    w.counts = reinterpret_cast<uint32_t*>(take(4ull * kRadixCountWords));
    w.bcount = reinterpret_cast<uint32_t*>(take(4 * ms_blocks(P)));
    if (out) *out = w;
    return o;
}

struct PlaceWork {               // nsa_mesh_cluster_place_workspace bytes; P = max(V, 3 F)
    uint32_t* keys[2];           // [P] each
    uint32_t* tmp;               // [P + 1]
    uint32_t* vorder;            // [V]: the vertices sorted stably by cluster
    uint32_t* iorder;            // [3 F]: the incidences 3 f + corner sorted stably by the cluster of the corner vertex
    uint32_t* counts;            // [256 * 256]
    uint32_t* vstart;            // [V]: cluster k owns vorder[vstart[k], vend[k])
    uint32_t* vend;              // [V]
    uint32_t* istart;            // [V]: and iorder[istart[k], iend[k])
    uint32_t* iend;              // [V]
};

__host__ __device__ inline uint64_t place_carve(void* ws, uint32_t V, uint32_t F, PlaceWork* out) {
    const uint64_t H = 3ull * F, P = V > H ? V : H;
    char* base = static_cast<char*>(ws);
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) { char* p = base ? base + o : nullptr; o += ms_align(bytes ? bytes : 1); return p; };
    PlaceWork w;
    w.keys[0] = reinterpret_cast<uint32_t*>(take(4 * P));
    w.keys[1] = reinterpret_cast<uint32_t*>(take(4 * P));
    w.tmp = reinterpret_cast<uint32_t*>(take(4 * (P + 1)));
    w.vorder = reinterpret_cast<uint32_t*>(take(4ull * V));
    w.iorder = reinterpret_cast<uint32_t*>(take(4 * H));
    w.counts = reinterpret_cast<uint32_t*>(take(4ull * kRadixCountWords));
    w.vstart = reinterpret_cast<uint32_t*>(take(4ull * V));
    w.vend = reinterpret_cast<uint32_t*>(take(4ull * V));
    w.istart = reinterpret_cast<uint32_t*>(take(4ull * V));
    w.iend = reinterpret_cast<uint32_t*>(take(4ull * V));
    if (out) *out = w;
    return o;
}

// ---- shared pieces --------------------------------------------------------------------------------------------------------------------

// adds the lanes of this wave that hold `flag` to *dst; every lane of the wave must call it
__device__ __forceinline__ void ms_count(ull* dst, bool flag) {
    const ull b = __ballot(flag);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(dst, (ull)__popcll(b));
}

// the cell of vertex v: 0 in the grid (c filled), 1 finite but outside, 2 a non-finite coordinate
__device__ __forceinline__ int ms_cell(const float* __restrict__ verts, uint32_t v, const MsGrid& g, uint32_t (&c)[3]) {
#pragma clang fp contract(off)
    const float x[3] = {verts[3ull * v], verts[3ull * v + 1], verts[3ull * v + 2]};
    c[0] = c[1] = c[2] = 0;
    if (!(isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]))) return 2;
    bool in = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double q = floor(((double)x[k] - g.o[k]) / g.h);
        if (q >= 0.0 && q < (double)g.n) c[k] = (uint32_t)q;
        else in = false;
    }
    return in ? 0 : 1;
}

__device__ __forceinline__ bool ms_valid_face(const int32_t* __restrict__ faces, uint32_t f, uint32_t V, uint32_t (&v)[3]) {
    const int32_t a = faces[3ull * f], b = faces[3ull * f + 1], c = faces[3ull * f + 2];
    v[0] = (uint32_t)a;
    v[1] = (uint32_t)b;
    v[2] = (uint32_t)c;
    return a >= 0 && b >= 0 && c >= 0 && v[0] < V && v[1] < V && v[2] < V;
}

__global__ void k_ms_zero(ull* __restrict__ totals) {
    if (threadIdx.x < kTotWords) totals[threadIdx.x] = 0;
}

__global__ __launch_bounds__(kMsBlock) void k_ms_scan_count(const uint32_t* __restrict__ flag, uint32_t N, uint32_t* __restrict__ bcount) {
    const uint32_t i = blockIdx.x * kMsBlock + threadIdx.x;
    uint32_t tot;
    scan::flag_scan<kMsBlock>(i < N && flag[i] != 0, tot);
    if (threadIdx.x == 0) bcount[blockIdx.x] = tot;
}

// ---- clusters: keys, used marks, the two-word sort, numbers --------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_ms_vkeys(const float* __restrict__ verts, uint32_t V, MsGrid g, ClusterWork w,
                                                  ull* __restrict__ totals) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    bool outside = false;
    if (v < V) {
        uint32_t c[3];
        const int where = ms_cell(verts, v, g, c);
        outside = where == 1;
        w.key[v] = where == 0 ? ((uint64_t)c[0] << 42) | ((uint64_t)c[1] << 21) | c[2] : kMsNoKey;
        w.used[v] = 0;
        w.cmark[v] = 0;
    }
    ms_count(totals + kTotOutside, outside);
}

// one lane per face: a contributing face marks its vertices as used (the same value from every face)
__global__ __launch_bounds__(256) void k_ms_fmark(const int32_t* __restrict__ faces, uint32_t F, uint32_t V, ClusterWork w,
                                                  ull* __restrict__ totals) {
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    bool c = false;
    uint32_t v[3];
    if (f < F) c = ms_valid_face(faces, f, V, v) && w.key[v[0]] != kMsNoKey && w.key[v[1]] != kMsNoKey && w.key[v[2]] != kMsNoKey;
    if (c) w.used[v[0]] = w.used[v[1]] = w.used[v[2]] = 1;
    ms_count(totals + kTotContrib, c);
}

__global__ __launch_bounds__(256) void k_ms_keys_lo(uint32_t V, ClusterWork w) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v < V) w.keys[0][v] = w.used[v] ? (uint32_t)w.key[v] : 0u;
}

// position i of the order by the low word: the high word of its vertex; a vertex that is not used carries `last`, above every key
__global__ __launch_bounds__(256) void k_ms_keys_hi(uint32_t V, ClusterWork w, uint32_t last, ull* __restrict__ totals) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    const uint32_t v = w.oa[i];
    if (v >= V) {                                        // (never: the order is a permutation of [0, V))
        atomicOr(totals + kTotStatus, (ull)kMsBadOrder);
        w.keys[0][i] = last;
        return;
    }
    w.keys[0][i] = w.used[v] ? (uint32_t)(w.key[v] >> 32) : last;
}

__device__ __forceinline__ uint32_t ms_sorted_vertex(const ClusterWork& w, uint32_t i, uint32_t V) {
    const uint32_t p = w.ob[i];
    return p < V ? w.oa[p] : V;
}

// sorted position i: its vertex, and whether it opens a run of equal keys
__global__ __launch_bounds__(256) void k_ms_vsort(uint32_t V, ClusterWork w, ull* __restrict__ totals) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    bool used = false;
    if (i < V) {
        const uint32_t v = ms_sorted_vertex(w, i, V), u = i ? ms_sorted_vertex(w, i - 1, V) : V;
        bool head = false;
        if (v >= V || (i && u >= V)) atomicOr(totals + kTotStatus, (ull)kMsBadOrder);          // (never)
        else {
            used = w.used[v] != 0;
            head = used && (i == 0 || w.key[u] != w.key[v]);     // the used vertices sort first, so u is used as well
        }
        w.oc[i] = v;
        w.flag[i] = head ? 1u : 0u;
    }
    ms_count(totals + kTotUsed, used);
}

__global__ __launch_bounds__(kMsBlock) void k_ms_vrank(uint32_t V, ClusterWork w, int32_t* __restrict__ vertex_cluster) {
    const uint32_t i = blockIdx.x * kMsBlock + threadIdx.x;
    const bool head = i < V && w.flag[i] != 0;
    uint32_t tot;
    const uint32_t pre = scan::flag_scan<kMsBlock>(head, tot);
    if (i >= V) return;
    const uint32_t v = w.oc[i];
    if (v >= V) return;                                  // (never; reported by k_ms_vsort)
    vertex_cluster[v] = w.used[v] ? (int32_t)(w.bcount[blockIdx.x] + pre + (head ? 1u : 0u)) - 1 : -1;
}

// ---- faces: triples, the three-word sort, survivors ---------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_ms_triple(const int32_t* __restrict__ faces, uint32_t F, uint32_t V, ClusterWork w,
                                                   const int32_t* __restrict__ vertex_cluster, ull* __restrict__ totals) {
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    bool collapsed = false;
    if (f < F) {
        uint32_t v[3], a = V, b = V, c = V;
        if (ms_valid_face(faces, f, V, v)) {
            const int32_t c0 = vertex_cluster[v[0]], c1 = vertex_cluster[v[1]], c2 = vertex_cluster[v[2]];
            if (c0 >= 0 && c1 >= 0 && c2 >= 0) {        // all three used: all three in the grid, so the face contributes
                if (c0 != c1 && c1 != c2 && c2 != c0) {
                    const bool r0 = c0 < c1 && c0 < c2, r1 = !r0 && c1 < c2;
                    a = (uint32_t)(r0 ? c0 : r1 ? c1 : c2);
                    b = (uint32_t)(r0 ? c1 : r1 ? c2 : c0);
                    c = (uint32_t)(r0 ? c2 : r1 ? c0 : c1);
                } else
                    collapsed = true;
            }
        }
        w.t[0][f] = a;
        w.t[1][f] = b;
        w.t[2][f] = c;
        w.keys[0][f] = c;
    }
    ms_count(totals + kTotCollapsed, collapsed);
}

// keys of the next link of the chain: word `word` of the face at position i of the order so far
__global__ __launch_bounds__(256) void k_ms_chain(uint32_t F, uint32_t V, ClusterWork w, int word, ull* __restrict__ totals) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= F) return;
    uint32_t f = w.oa[i];
    if (word == 0) {
        const uint32_t p = w.ob[i];
        f = p < F ? w.oa[p] : F;
        w.pp[i] = f;
    }
    if (f >= F) {                                        // (never)
        atomicOr(totals + kTotStatus, (ull)kMsBadOrder);
        w.keys[0][i] = V;
        return;
    }
    w.keys[0][i] = w.t[word][f];
}

__device__ __forceinline__ uint32_t ms_sorted_face(const ClusterWork& w, uint32_t i, uint32_t F) {
    const uint32_t p = w.oc[i];
    return p < F ? w.pp[p] : F;
}

// sorted position i: the face there survives when it is a candidate and opens a run of equal triples
__global__ __launch_bounds__(256) void k_ms_fsort(uint32_t F, uint32_t V, ClusterWork w, ull* __restrict__ totals) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    bool dup = false;
    if (i < F) {
        const uint32_t f = ms_sorted_face(w, i, F), g = i ? ms_sorted_face(w, i - 1, F) : F;
        if (f >= F || (i && g >= F)) atomicOr(totals + kTotStatus, (ull)kMsBadOrder);          // (never)
        else {
            const bool cand = w.t[0][f] != V;
            const bool head = cand && (i == 0 || w.t[0][g] != w.t[0][f] || w.t[1][g] != w.t[1][f] || w.t[2][g] != w.t[2][f]);
            dup = cand && !head;
            w.flag[f] = head ? 1u : 0u;
        }
    }
    ms_count(totals + kTotDuplicate, dup);
}

// face f: its place among the survivors; the clusters it names are marked
__global__ __launch_bounds__(kMsBlock) void k_ms_fcompact(uint32_t F, uint32_t V, ClusterWork w, int32_t* __restrict__ out_faces,
                                                          int32_t* __restrict__ face_origin) {
    const uint32_t f = blockIdx.x * kMsBlock + threadIdx.x;
    const bool keep = f < F && w.flag[f] != 0;
    uint32_t tot;
    const uint32_t o = w.bcount[blockIdx.x] + scan::flag_scan<kMsBlock>(keep, tot);
    if (!keep || o >= F) return;
    face_origin[o] = (int32_t)f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t c = w.t[k][f];
        out_faces[3ull * o + k] = (int32_t)c;
        if (c < V) w.cmark[c] = 1;
    }
}

__global__ __launch_bounds__(kMsBlock) void k_ms_crank(uint32_t V, ClusterWork w, int32_t* __restrict__ cluster_vertex,
                                                       int32_t* __restrict__ out_cluster) {
    const uint32_t k = blockIdx.x * kMsBlock + threadIdx.x;
    const bool named = k < V && w.cmark[k] != 0;
    uint32_t tot;
    const uint32_t o = w.bcount[blockIdx.x] + scan::flag_scan<kMsBlock>(named, tot);
    if (k >= V) return;
    cluster_vertex[k] = named ? (int32_t)o : -1;
    if (named && o < V) out_cluster[o] = (int32_t)k;
}

__global__ __launch_bounds__(256) void k_ms_remap(uint32_t F, uint32_t V, const ull* __restrict__ totals,
                                                  const int32_t* __restrict__ cluster_vertex, int32_t* __restrict__ out_faces) {
    const uint32_t o = blockIdx.x * 256 + threadIdx.x;
    if (o >= F || (ull)o >= totals[kTotFaces]) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t c = (uint32_t)out_faces[3ull * o + k];
        out_faces[3ull * o + k] = c < V ? cluster_vertex[c] : -1;
    }
}

// ---- placement ----------------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t mp_cluster_of(const int32_t* __restrict__ vertex_cluster, uint32_t v, uint32_t V) {
    const int32_t c = vertex_cluster[v];
    return c >= 0 && (uint32_t)c < V ? (uint32_t)c : V;
}

__global__ __launch_bounds__(256) void k_mp_vkeys(uint32_t V, PlaceWork w, const int32_t* __restrict__ vertex_cluster) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    w.keys[0][v] = mp_cluster_of(vertex_cluster, v, V);
    w.vstart[v] = w.vend[v] = w.istart[v] = w.iend[v] = 0;
}

// the key of incidence e = 3 f + corner: the cluster of its corner vertex when the face contributes, else V
__device__ __forceinline__ uint32_t mp_incidence_key(const int32_t* __restrict__ faces, const int32_t* __restrict__ vertex_cluster,
                                                     uint32_t e, uint32_t V) {
    const uint32_t f = e / 3u, k = e - 3u * f;
    uint32_t v[3];
    if (!ms_valid_face(faces, f, V, v)) return V;
    const uint32_t c[3] = {mp_cluster_of(vertex_cluster, v[0], V), mp_cluster_of(vertex_cluster, v[1], V),
                           mp_cluster_of(vertex_cluster, v[2], V)};
    if (c[0] == V || c[1] == V || c[2] == V) return V;
    return k == 0 ? c[0] : k == 1 ? c[1] : c[2];
}

__global__ __launch_bounds__(256) void k_mp_ikeys(const int32_t* __restrict__ faces, uint32_t H, uint32_t V, PlaceWork w,
                                                  const int32_t* __restrict__ vertex_cluster) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e < H) w.keys[0][e] = mp_incidence_key(faces, vertex_cluster, e, V);
}

// sorted position i of N: where the run of its key starts and ends (keys below V only)
__global__ __launch_bounds__(256) void k_mp_vruns(uint32_t V, PlaceWork w, const int32_t* __restrict__ vertex_cluster) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    const uint32_t v = w.vorder[i];
    if (v >= V) return;                                  // (never)
    const uint32_t c = mp_cluster_of(vertex_cluster, v, V);
    if (c == V) return;
    const uint32_t u = i ? w.vorder[i - 1] : V, n = i + 1 < V ? w.vorder[i + 1] : V;
    if (i == 0 || u >= V || mp_cluster_of(vertex_cluster, u, V) != c) w.vstart[c] = i;
    if (i + 1 == V || n >= V || mp_cluster_of(vertex_cluster, n, V) != c) w.vend[c] = i + 1;
}

__global__ __launch_bounds__(256) void k_mp_iruns(const int32_t* __restrict__ faces, uint32_t H, uint32_t V, PlaceWork w,
                                                  const int32_t* __restrict__ vertex_cluster) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H) return;
    const uint32_t e = w.iorder[i];
    if (e >= H) return;                                  // (never)
    const uint32_t c = mp_incidence_key(faces, vertex_cluster, e, V);
    if (c == V) return;
    const uint32_t u = i ? w.iorder[i - 1] : H, n = i + 1 < H ? w.iorder[i + 1] : H;
    if (i == 0 || u >= H || mp_incidence_key(faces, vertex_cluster, u, V) != c) w.istart[c] = i;
    if (i + 1 == H || n >= H || mp_incidence_key(faces, vertex_cluster, n, V) != c) w.iend[c] = i + 1;
}

struct PlaceArgs {
    const float* verts;
    const int32_t* faces;
    const float* normals;
    const float* colours;
    const int32_t* cluster_vertex;
    float* out_verts;
    float* out_normals;
    float* out_colours;
    int32_t* out_cell;
    uint32_t V, H, n_out;
    int placement;
    double eps;
};

// (A + mu I) x = r by Cholesky, A symmetric as {00, 01, 02, 11, 12, 22}
__device__ __forceinline__ void mp_solve(const double (&A)[6], double mu, const double (&r)[3], double (&x)[3]) {
#pragma clang fp contract(off)
    const double l00 = sqrt(A[0] + mu);
    const double l10 = A[1] / l00, l20 = A[2] / l00;
    const double l11 = sqrt((A[3] + mu) - l10 * l10);
    const double l21 = (A[4] - l20 * l10) / l11;
    const double l22 = sqrt((A[5] + mu) - (l20 * l20 + l21 * l21));
    const double y0 = r[0] / l00;
    const double y1 = (r[1] - l10 * y0) / l11;
    const double y2 = (r[2] - (l20 * y0 + l21 * y1)) / l22;
    x[2] = y2 / l22;
    x[1] = (y1 - l21 * x[2]) / l11;
    x[0] = (y0 - (l10 * x[1] + l20 * x[2])) / l00;
}

// one lane per cluster that a surviving face names: its two runs in order
__global__ __launch_bounds__(256) void k_mp_place(PlaceArgs a, MsGrid g, PlaceWork w) {
#pragma clang fp contract(off)
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= a.V) return;
    const int32_t o = a.cluster_vertex[k];
    if (o < 0 || (uint32_t)o >= a.n_out) return;
    const uint32_t v0 = min(w.vstart[k], a.V), v1 = min(w.vend[k], a.V);
    const uint32_t i0 = min(w.istart[k], a.H), i1 = min(w.iend[k], a.H);
    double centre[3] = {0.0, 0.0, 0.0}, sum[3] = {0.0, 0.0, 0.0}, ns[3] = {0.0, 0.0, 0.0}, cs[3] = {0.0, 0.0, 0.0};
    uint32_t cell[3] = {0, 0, 0}, count = 0;
    for (uint32_t i = v0; i < v1; ++i) {
        const uint32_t v = w.vorder[i];
        if (v >= a.V) continue;                          // (never)
        if (count == 0) {
            ms_cell(a.verts, v, g, cell);
#pragma unroll
            for (int j = 0; j < 3; ++j) centre[j] = g.o[j] + ((double)cell[j] + 0.5) * g.h;
        }
        ++count;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            sum[j] = sum[j] + ((double)a.verts[3ull * v + j] - centre[j]);
            if (a.normals) ns[j] = ns[j] + (double)a.normals[3ull * v + j];
            if (a.colours) cs[j] = cs[j] + (double)a.colours[3ull * v + j];
        }
    }
    const double cnt = (double)count;
    double m[3], x[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) x[j] = m[j] = count ? sum[j] / cnt : 0.0;
    if (a.placement == 1) {
        double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
        for (uint32_t i = i0; i < i1; ++i) {
            const uint32_t e = w.iorder[i];
            if (e >= a.H) continue;                      // (never)
            const uint32_t f = e / 3u;
            uint32_t fv[3];
            if (!ms_valid_face(a.faces, f, a.V, fv)) continue;       // (never: the run holds contributing faces only)
            double p[3][3];
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int j = 0; j < 3; ++j) p[c][j] = (double)a.verts[3ull * fv[c] + j] - centre[j];
            const double u[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
            const double q[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
            const double n[3] = {u[1] * q[2] - u[2] * q[1], u[2] * q[0] - u[0] * q[2], u[0] * q[1] - u[1] * q[0]};
            const double d = -((n[0] * p[0][0] + n[1] * p[0][1]) + n[2] * p[0][2]);
            A[0] = A[0] + n[0] * n[0];
            A[1] = A[1] + n[0] * n[1];
            A[2] = A[2] + n[0] * n[2];
            A[3] = A[3] + n[1] * n[1];
            A[4] = A[4] + n[1] * n[2];
            A[5] = A[5] + n[2] * n[2];
#pragma unroll
            for (int j = 0; j < 3; ++j) b[j] = b[j] + n[j] * d;
        }
        const double tr = (A[0] + A[3]) + A[5];
        if (tr != 0.0) {
            const double mu = a.eps * tr, half = 0.5 * g.h;
            const double r[3] = {-b[0] + mu * m[0], -b[1] + mu * m[1], -b[2] + mu * m[2]};
            double s[3];
            mp_solve(A, mu, r, s);
            if (isfinite(s[0]) && isfinite(s[1]) && isfinite(s[2])) {
#pragma unroll
                for (int j = 0; j < 3; ++j) x[j] = s[j] < -half ? -half : (s[j] > half ? half : s[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        a.out_verts[3ull * o + j] = (float)(centre[j] + x[j]);
        if (a.out_cell) a.out_cell[3ull * o + j] = (int32_t)cell[j];
    }
    if (a.out_normals) {
        const double len = sqrt((ns[0] * ns[0] + ns[1] * ns[1]) + ns[2] * ns[2]);
        const bool ok = len > 0.0 && isfinite(len);
#pragma unroll
        for (int j = 0; j < 3; ++j) a.out_normals[3ull * o + j] = ok ? (float)(ns[j] / len) : 0.0f;
    }
    if (a.out_colours) {
#pragma unroll
        for (int j = 0; j < 3; ++j) a.out_colours[3ull * o + j] = count ? (float)(cs[j] / cnt) : 0.0f;
    }
}

constexpr auto k_ms_offsets = scan::k_offsets<1, uint32_t, kMsBlock>;

static bool ms_grid(const double* origin, double h, uint32_t n_cells, MsGrid* g) {
    if (!origin || !std::isfinite(h) || !(h > 0.0) || n_cells == 0 || n_cells > kMsMaxCells) return false;
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(origin[k])) return false;
        g->o[k] = origin[k];
    }
    g->h = h;
    g->n = n_cells;
    return true;
}

}  // namespace nsa

extern "C" {

uint64_t nsa_mesh_cluster_workspace(uint32_t n_verts, uint32_t n_faces) {
    if (n_verts == 0 || n_faces == 0 || n_faces > nsa::kMsMaxFaces || n_verts > nsa::kMsMaxVerts) return 0;
    return nsa::cluster_carve(nullptr, n_verts, n_faces, nullptr);
}

int nsa_mesh_cluster(const float* verts, uint32_t n_verts, const int32_t* faces, uint32_t n_faces, const double* origin, double h,
                     uint32_t n_cells, void* workspace, int32_t* vertex_cluster, int32_t* cluster_vertex, int32_t* out_cluster,
                     int32_t* out_faces, int32_t* face_origin, uint64_t* totals, nsa_stream_t stream) {
    using namespace nsa;
    const uint32_t V = n_verts, F = n_faces;
    MsGrid g;
    if (V > kMsMaxVerts || F > kMsMaxFaces || !ms_grid(origin, h, n_cells, &g)) return NSA_EBADARG;
    if (V == 0 || F == 0) return NSA_OK;
    if (!verts || !faces || !workspace || !vertex_cluster || !cluster_vertex || !out_cluster || !out_faces || !face_origin || !totals)
        return NSA_EBADARG;
    ClusterWork w;
    cluster_carve(workspace, V, F, &w);
    // the key's occupied width: c_z and c_y fill the low word up to bit 21 + bitlen(n - 1); the high word holds c_x << 10 and the
    // top of c_y, and n << 10 for a vertex that is not used
    const uint32_t lo_bits = 21 + ms_bitlen(n_cells - 1), hi_last = n_cells << 10;
    const uint32_t passes_lo = ((lo_bits > 32 ? 32 : lo_bits) + 7) / 8, passes_hi = (ms_bitlen(hi_last) + 7) / 8;
    const uint32_t passes_c = (ms_bitlen(V) + 7) / 8;         // cluster numbers and the V of a face that cannot survive
    const uint32_t nbv = (uint32_t)ms_blocks(V), nbf = (uint32_t)ms_blocks(F), gv = (V + 255) / 256, gf = (F + 255) / 256;
    ull* tot = reinterpret_cast<ull*>(totals);
    hipStream_t s = (hipStream_t)stream;
    launch_begin();
    hipLaunchKernelGGL(k_ms_zero, dim3(1), dim3(64), 0, s, tot);
    hipLaunchKernelGGL(k_ms_vkeys, dim3(gv), dim3(256), 0, s, verts, V, g, w, tot);
    hipLaunchKernelGGL(k_ms_fmark, dim3(gf), dim3(256), 0, s, faces, F, V, w, tot);
    hipLaunchKernelGGL(k_ms_keys_lo, dim3(gv), dim3(256), 0, s, V, w);
    radix_argsort(w.keys, w.tmp, w.oa, w.counts, V, 0, passes_lo, stream);
    hipLaunchKernelGGL(k_ms_keys_hi, dim3(gv), dim3(256), 0, s, V, w, hi_last, tot);
    radix_argsort(w.keys, w.tmp, w.ob, w.counts, V, 0, passes_hi, stream);
    hipLaunchKernelGGL(k_ms_vsort, dim3(gv), dim3(256), 0, s, V, w, tot);
    hipLaunchKernelGGL(k_ms_scan_count, dim3(nbv), dim3(kMsBlock), 0, s, w.flag, V, w.bcount);
    hipLaunchKernelGGL(k_ms_offsets, dim3(1), dim3(kMsBlock), 0, s, (const uint32_t*)w.bcount, w.bcount, nbv, tot + kTotK);
    hipLaunchKernelGGL(k_ms_vrank, dim3(nbv), dim3(kMsBlock), 0, s, V, w, vertex_cluster);
    hipLaunchKernelGGL(k_ms_triple, dim3(gf), dim3(256), 0, s, faces, F, V, w, vertex_cluster, tot);
    radix_argsort(w.keys, w.tmp, w.oa, w.counts, F, 0, passes_c, stream);
    hipLaunchKernelGGL(k_ms_chain, dim3(gf), dim3(256), 0, s, F, V, w, 1, tot);
    radix_argsort(w.keys, w.tmp, w.ob, w.counts, F, 0, passes_c, stream);
    hipLaunchKernelGGL(k_ms_chain, dim3(gf), dim3(256), 0, s, F, V, w, 0, tot);
    radix_argsort(w.keys, w.tmp, w.oc, w.counts, F, 0, passes_c, stream);
    hipLaunchKernelGGL(k_ms_fsort, dim3(gf), dim3(256), 0, s, F, V, w, tot);
    hipLaunchKernelGGL(k_ms_scan_count, dim3(nbf), dim3(kMsBlock), 0, s, w.flag, F, w.bcount);
    hipLaunchKernelGGL(k_ms_offsets, dim3(1), dim3(kMsBlock), 0, s, (const uint32_t*)w.bcount, w.bcount, nbf, tot + kTotFaces);
    hipLaunchKernelGGL(k_ms_fcompact, dim3(nbf), dim3(kMsBlock), 0, s, F, V, w, out_faces, face_origin);
    hipLaunchKernelGGL(k_ms_scan_count, dim3(nbv), dim3(kMsBlock), 0, s, w.cmark, V, w.bcount);
    hipLaunchKernelGGL(k_ms_offsets, dim3(1), dim3(kMsBlock), 0, s, (const uint32_t*)w.bcount, w.bcount, nbv, tot + kTotVerts);
    hipLaunchKernelGGL(k_ms_crank, dim3(nbv), dim3(kMsBlock), 0, s, V, w, cluster_vertex, out_cluster);
    hipLaunchKernelGGL(k_ms_remap, dim3(gf), dim3(256), 0, s, F, V, tot, cluster_vertex, out_faces);
    return launch_end();
}

uint64_t nsa_mesh_cluster_place_workspace(uint32_t n_verts, uint32_t n_faces) {
    if (n_verts == 0 || n_faces == 0 || n_faces > nsa::kMsMaxFaces || n_verts > nsa::kMsMaxVerts) return 0;
    return nsa::place_carve(nullptr, n_verts, n_faces, nullptr);
}

int nsa_mesh_cluster_place(const float* verts, uint32_t n_verts, const int32_t* faces, uint32_t n_faces, const float* normals,
                           const float* colours, const double* origin, double h, double eps, int placement,
                           const int32_t* vertex_cluster, const int32_t* cluster_vertex, uint32_t n_out, void* workspace,
                           float* out_verts, float* out_normals, float* out_colours, int32_t* out_cell, nsa_stream_t stream) {
    using namespace nsa;
    const uint32_t V = n_verts, F = n_faces;
    MsGrid g;
    if (V > kMsMaxVerts || F > kMsMaxFaces || !ms_grid(origin, h, kMsMaxCells, &g)) return NSA_EBADARG;
    if (!(eps >= 0.0) || !std::isfinite(eps) || (placement != 0 && placement != 1) || n_out > V) return NSA_EBADARG;
    if ((normals != nullptr) != (out_normals != nullptr) || (colours != nullptr) != (out_colours != nullptr)) return NSA_EBADARG;
    if (V == 0 || F == 0 || n_out == 0) return NSA_OK;
    if (!verts || !faces || !vertex_cluster || !cluster_vertex || !workspace || !out_verts) return NSA_EBADARG;
    PlaceWork w;
    place_carve(workspace, V, F, &w);
    const uint32_t H = 3u * F, passes = (ms_bitlen(V) + 7) / 8, gv = (V + 255) / 256, gh = (H + 255) / 256;
    const PlaceArgs a{verts, faces, normals, colours, cluster_vertex, out_verts, out_normals, out_colours, out_cell, V, H, n_out,
                      placement, eps};
    hipStream_t s = (hipStream_t)stream;
    launch_begin();
    hipLaunchKernelGGL(k_mp_vkeys, dim3(gv), dim3(256), 0, s, V, w, vertex_cluster);
    radix_argsort(w.keys, w.tmp, w.vorder, w.counts, V, 0, passes, stream);
    hipLaunchKernelGGL(k_mp_vruns, dim3(gv), dim3(256), 0, s, V, w, vertex_cluster);
    if (placement == 1) {
        hipLaunchKernelGGL(k_mp_ikeys, dim3(gh), dim3(256), 0, s, faces, H, V, w, vertex_cluster);
        radix_argsort(w.keys, w.tmp, w.iorder, w.counts, H, 0, passes, stream);
        hipLaunchKernelGGL(k_mp_iruns, dim3(gh), dim3(256), 0, s, faces, H, V, w, vertex_cluster);
    }
    hipLaunchKernelGGL(k_mp_place, dim3(gv), dim3(256), 0, s, a, g, w);
    return launch_end();
}

}  // extern "C"
