// mesh_intersect.hip -- which pairs of faces of a mesh meet, decided exactly (DESIGN 4x, C ABI Section 25).  The statement in the header
// is the contract; tests/intersect_ref.py restates it by constructing A n B in rationals, and the kernels are held to it element for
// element.  The per-pair bodies -- the float64 filter, its bound, the 256-bit integer, the decision -- are intersect_passes.hpp's.
//
// Broad phase.  The exact box of a face is the fp32 min / max of its nine coordinates; two usable faces are candidates iff these closed
// boxes overlap on all three axes.  The walk is over the ray-cast tree of Section 17 (ray_tree.hpp): the padded box of a face
// contains its exact box and a node's box contains its faces', so a node whose box misses the query face's exact box holds no
// candidate.  The exact-box clause is part of the pair test, so the tree and the brute force agree by construction.  One lane per
// sorted position p of the tree (neighbouring lanes are neighbouring faces), face i = order[p], partners g > i only.  The nodes are in
// pre-order with `skip`, so the walk needs no path at all: overlap and inner node -> the next index, else -> skip.
//
// No atomics.  The count pass writes per lane how many records it will emit and its share of the statistics; one workgroup scans the
// counts and sums the rest (block_scan.hpp); the emit pass repeats the walk and writes each record at its slot.  The records of one run are grouped
// by p in walk order; the caller sorts by (i, j).
#include "block_scan.hpp"
#include "intersect_passes.hpp"
#include "ray_tree.hpp"

namespace nsa {
namespace isect {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kTile = 256;              // faces per LDS tile of the brute force: 10 KiB a workgroup
constexpr int kStats = 8;                    // per lane: candidates with s = 0 .. 3, decided by stage 1, by stage 2, unresolved, 0
constexpr int kTotals = 16;
constexpr uint8_t kStateCollinear = 4, kStateUnresolved = 5;

struct Work {                    // views into the caller's workspace (nsa_tri_isect_workspace bytes)
    uint32_t* count;             // [F]: records of lane p
    uint64_t* offset;            // [F + 1]: exclusive prefix sum of count
    uint32_t* stats;             // [F][kStats]
};

__host__ __device__ inline uint64_t carve(void* ws, uint32_t F, Work* out) {
    char* base = static_cast<char*>(ws);
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) { char* p = base ? base + o : nullptr; o += bulk::up256(bytes); return p; };
    Work w;
    w.count = reinterpret_cast<uint32_t*>(take(4ull * F));
    w.offset = reinterpret_cast<uint64_t*>(take(8ull * ((uint64_t)F + 1)));
    w.stats = reinterpret_cast<uint32_t*>(take(4ull * kStats * F));
    if (out) *out = w;
    return o;
}

struct Mesh {
    const float* v;
    const int32_t* f;
    const uint8_t* state;
    const uint8_t* side;         // may be null
    uint32_t V, F;
};

struct Lane {                    // what one lane gathers, and where it emits
    uint32_t n, stats[kStats];
    uint64_t slot, slot_end;
    int64_t* pairs;
    uint8_t* code;
};

__device__ __forceinline__ bool load_vertices(const Mesh& m, uint32_t g, float (&a)[3][3]) {
    const int32_t i0 = m.f[3ull * g], i1 = m.f[3ull * g + 1], i2 = m.f[3ull * g + 2];
    if ((uint32_t)i0 >= m.V || (uint32_t)i1 >= m.V || (uint32_t)i2 >= m.V) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a[0][k] = m.v[3ull * i0 + k];
        a[1][k] = m.v[3ull * i1 + k];
        a[2][k] = m.v[3ull * i2 + k];
    }
    return true;
}

// one lane per face: 0 usable, 1 .. 3 Section 14's causes, 4 exactly collinear, 5 collinearity beyond the device's width
__global__ __launch_bounds__(kBlock) void k_isect_state(const float* __restrict__ v, uint32_t V, const int32_t* __restrict__ f, uint32_t F,
                                                        uint8_t* __restrict__ state) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= F) return;
    float a[3], b[3], c[3];
    int st = tri::load_face(v, V, f, i, a, b, c);
    if (st == 0) {
        const float t[3][3] = {{a[0], a[1], a[2]}, {b[0], b[1], b[2]}, {c[0], c[1], c[2]}};
        const int col = face_collinear(t);
        st = col < 0 ? kStateUnresolved : (col ? kStateCollinear : 0);
    }
    state[i] = (uint8_t)st;
}

// face i (vertices a) against face g > i (vertices b): the exact-box clause, the decision, the tallies, the record
template <bool kEmit>
__device__ __forceinline__ void test_pair(const Mesh& m, uint32_t i, const float (&a)[3][3], uint32_t g, const float (&b)[3][3],
                                          Lane& ln) {
    if (m.side && m.side[i] == m.side[g]) return;
    if (!boxes_overlap(a, b)) return;
    int s, stage;
    const uint32_t code = pair_code(a, b, s, stage);
    ln.stats[s & 3] += 1;
    ln.stats[3 + stage] += 1;                                      // stage 1 .. 3 -> stats[4 .. 6]
    if (code == 0) return;
    if (kEmit) {
        const uint64_t slot = ln.slot + ln.n;
        if (slot < ln.slot_end) {                                  // (always, on the arrays the count pass saw)
            ln.pairs[2 * slot] = (int64_t)i;
            ln.pairs[2 * slot + 1] = (int64_t)g;
            ln.code[slot] = (uint8_t)code;
        }
    }
    ln.n += 1;
}

template <bool kEmit>
__device__ __forceinline__ void begin_lane(Lane& ln, const Work& w, uint32_t p, uint64_t n_pairs, int64_t* pairs, uint8_t* code) {
    ln.n = 0;
#pragma unroll
    for (int k = 0; k < kStats; ++k) ln.stats[k] = 0;
    ln.slot = ln.slot_end = 0;
    ln.pairs = pairs;
    ln.code = code;
    if (kEmit) {
        ln.slot = w.offset[p];
        const uint64_t e = w.offset[p + 1];
        ln.slot_end = e < n_pairs ? e : n_pairs;
    }
}

template <bool kEmit>
__device__ __forceinline__ void end_lane(const Lane& ln, const Work& w, uint32_t p) {
    if (kEmit) return;
    w.count[p] = ln.n;
#pragma unroll
    for (int k = 0; k < kStats; ++k) w.stats[(uint64_t)kStats * p + k] = ln.stats[k];
}

// one lane per sorted position: the walk
template <bool kEmit>
__global__ __launch_bounds__(kBlock) void k_isect_tree(rc::Tree t, Mesh m, Work w, uint64_t n_pairs, int64_t* __restrict__ pairs,
                                                       uint8_t* __restrict__ code) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= m.F) return;
    Lane ln;
    begin_lane<kEmit>(ln, w, p, n_pairs, pairs, code);
    const octree::Head* hd = t.head;
    const uint32_t n_nodes = hd->n_nodes, n_usable = min(hd->n_usable, m.F);
    const uint32_t i = t.order[p];
    float a[3][3];
    if (p < n_usable && i < m.F && m.state[i] == 0 && load_vertices(m, i, a)) {
        float lo[3], hi[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lo[k] = fminf(fminf(a[0][k], a[1][k]), a[2][k]);
            hi[k] = fmaxf(fmaxf(a[0][k], a[1][k]), a[2][k]);
        }
        uint32_t cur = 0;
        while (cur < n_nodes) {
            const rc::Node nd = t.node[cur];
            const uint32_t behind = nd.skip & ~octree::kLeafBit;
            const bool hit = nd.lo[0] <= hi[0] && lo[0] <= nd.hi[0] && nd.lo[1] <= hi[1] && lo[1] <= nd.hi[1] && nd.lo[2] <= hi[2] &&
                             lo[2] <= nd.hi[2];
            uint32_t next = behind;
            if (hit) {
                if (nd.skip & octree::kLeafBit) {
                    const uint32_t e = min(t.end[cur], n_usable);
                    for (uint32_t pos = nd.begin; pos < e; ++pos) {
                        const uint32_t g = t.order[pos];
                        if (g <= i || g >= m.F || m.state[g] != 0) continue;
                        const float* bx = t.fbox + 6ull * pos;
                        if (!(bx[0] <= hi[0] && lo[0] <= bx[3] && bx[1] <= hi[1] && lo[1] <= bx[4] && bx[2] <= hi[2] && lo[2] <= bx[5]))
                            continue;
                        float b[3][3];
                        if (load_vertices(m, g, b)) test_pair<kEmit>(m, i, a, g, b, ln);
                    }
                } else {
                    next = cur + 1;                                // pre-order: the first child follows its parent
                }
            }
            if (next <= cur) break;                                // (a damaged buffer: never loop)
            cur = next;
        }
    }
    end_lane<kEmit>(ln, w, p);
}

// one lane per sorted position, every usable face through LDS: the cross-check of the walk
template <bool kEmit>
__global__ __launch_bounds__(kBlock) void k_isect_brute(rc::Tree t, Mesh m, Work w, uint64_t n_pairs, int64_t* __restrict__ pairs,
                                                        uint8_t* __restrict__ code) {
    __shared__ float s_face[kTile][9];
    __shared__ uint32_t s_index[kTile];
    const uint32_t tid = threadIdx.x, p = blockIdx.x * kBlock + tid;
    const bool live = p < m.F;
    Lane ln;
    begin_lane<kEmit>(ln, w, live ? p : 0, live ? n_pairs : 0, pairs, code);
    const uint32_t n_usable = min(t.head->n_usable, m.F);
    const uint32_t i = live ? t.order[p] : 0xFFFFFFFFu;
    float a[3][3];
    const bool valid = live && p < n_usable && i < m.F && m.state[i] == 0 && load_vertices(m, i, a);
    for (uint32_t base = 0; base < n_usable; base += kTile) {
        const uint32_t count = min(kTile, n_usable - base);
        if (tid < count) {
            const uint32_t g = t.order[base + tid];
            float b[3][3];
            const bool ok = g < m.F && m.state[g] == 0 && load_vertices(m, g, b);
            s_index[tid] = ok ? g : 0xFFFFFFFFu;
#pragma unroll
            for (int k = 0; k < 9; ++k) s_face[tid][k] = ok ? b[k / 3][k % 3] : 0.0f;
        }
        __syncthreads();
        if (valid) {
            for (uint32_t s = 0; s < count; ++s) {
                const uint32_t g = s_index[s];
                if (g == 0xFFFFFFFFu || g <= i) continue;
                float b[3][3];
#pragma unroll
                for (int k = 0; k < 9; ++k) b[k / 3][k % 3] = s_face[s][k];
                test_pair<kEmit>(m, i, a, g, b, ln);
            }
        }
        __syncthreads();
    }
    if (live) end_lane<kEmit>(ln, w, p);
}

// the sum of x over the workgroup of 1024
__device__ __forceinline__ uint64_t block_sum(uint64_t x) {
    const uint64_t v[1] = {x};
    uint64_t excl[1], total[1];
    scan::lds_scan<1, uint64_t, 1024>(v, excl, total);
    return total[0];
}

// one workgroup of 1024: offset = the exclusive prefix sum of count, and the totals
__global__ __launch_bounds__(1024) void k_isect_totals(uint32_t F, Work w, const uint8_t* __restrict__ state,
                                                       uint64_t* __restrict__ totals) {
    const uint32_t tid = threadIdx.x;
    const uint64_t n = F, chunk = (n + 1023) / 1024;
    const uint64_t lo = tid * chunk < n ? tid * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
    uint64_t n_emit[1];
    scan::offsets<1, uint64_t, 1024>(w.count, w.offset, n, n_emit);
    if (tid == 1023) w.offset[F] = n_emit[0];
    uint64_t part[kStats - 1 + 6];
    for (int k = 0; k < kStats - 1 + 6; ++k) part[k] = 0;
    for (uint64_t i = lo; i < hi; ++i) {
        for (int k = 0; k < kStats - 1; ++k) part[k] += w.stats[(uint64_t)kStats * i + k];
        const uint32_t st = state[i];
        for (uint32_t c = 0; c < 6; ++c) part[kStats - 1 + c] += st == c ? 1 : 0;
    }
    uint64_t out[kTotals];
    for (int k = 0; k < kTotals; ++k) out[k] = 0;
    out[0] = n_emit[0];
    for (int k = 0; k < kStats - 1; ++k) out[1 + k] = block_sum(part[k]);                        // 1 .. 4 candidates by s, 5 .. 7 stages
    for (int c = 1; c < 6; ++c) out[7 + c] = block_sum(part[kStats - 1 + c]);                    // 8 .. 12 faces by state 1 .. 5
    out[13] = block_sum(part[kStats - 1]);                                                       // usable faces
    if (tid == 0)
        for (int k = 0; k < kTotals; ++k) totals[k] = out[k];
}

static bool bad_mesh(const void* tree, const float* verts, uint32_t n_verts, const int32_t* faces, uint32_t n_faces, uint32_t flags) {
    return n_verts > tri::kMaxCount || n_faces > tri::kMaxCount || (flags & ~(uint32_t)NSA_ISECT_BRUTE) ||
           (n_faces > 0 && (!tree || !verts || !faces || n_verts == 0));
}

}  // namespace isect
}  // namespace nsa

extern "C" {

uint64_t nsa_tri_isect_workspace(uint32_t n_faces) {
    using namespace nsa;
    if (n_faces == 0 || n_faces > tri::kMaxCount) return 0;
    return isect::carve(nullptr, n_faces, nullptr);
}

int nsa_tri_isect_count(const void* tree, const float* verts, uint32_t n_verts, const int32_t* faces, uint32_t n_faces,
                        const uint8_t* side, uint32_t flags, void* workspace, uint8_t* state, uint64_t* totals, nsa_stream_t stream) {
    using namespace nsa;
    using namespace nsa::isect;
    if (bad_mesh(tree, verts, n_verts, faces, n_faces, flags)) return NSA_EBADARG;
    if (n_faces == 0) return NSA_OK;
    if (!workspace || !state || !totals) return NSA_EBADARG;
    rc::Tree t;
    Work w;
    rc::carve(const_cast<void*>(tree), n_faces, &t);
    carve(workspace, n_faces, &w);
    const Mesh m{verts, faces, state, side, n_verts, n_faces};
    const dim3 grid((n_faces + kBlock - 1) / kBlock);
    hipStream_t s = (hipStream_t)stream;
    launch_begin();
    hipLaunchKernelGGL(k_isect_state, grid, dim3(kBlock), 0, s, verts, n_verts, faces, n_faces, state);
    if (flags & NSA_ISECT_BRUTE)
        hipLaunchKernelGGL(k_isect_brute<false>, grid, dim3(kBlock), 0, s, t, m, w, (uint64_t)0, (int64_t*)nullptr, (uint8_t*)nullptr);
    else
        hipLaunchKernelGGL(k_isect_tree<false>, grid, dim3(kBlock), 0, s, t, m, w, (uint64_t)0, (int64_t*)nullptr, (uint8_t*)nullptr);
    hipLaunchKernelGGL(k_isect_totals, dim3(1), dim3(1024), 0, s, n_faces, w, (const uint8_t*)state, totals);
    return launch_end();
}

int nsa_tri_isect_emit(const void* tree, const float* verts, uint32_t n_verts, const int32_t* faces, uint32_t n_faces,
                       const uint8_t* side, uint32_t flags, const void* workspace, const uint8_t* state, uint64_t n_pairs,
                       int64_t* pairs, uint8_t* code, nsa_stream_t stream) {
    using namespace nsa;
    using namespace nsa::isect;
    if (bad_mesh(tree, verts, n_verts, faces, n_faces, flags)) return NSA_EBADARG;
    if (n_faces == 0 || n_pairs == 0) return NSA_OK;
    if (!workspace || !state || !pairs || !code) return NSA_EBADARG;
    rc::Tree t;
    Work w;
    rc::carve(const_cast<void*>(tree), n_faces, &t);
    carve(const_cast<void*>(workspace), n_faces, &w);
    const Mesh m{verts, faces, state, side, n_verts, n_faces};
    const dim3 grid((n_faces + kBlock - 1) / kBlock);
    hipStream_t s = (hipStream_t)stream;
    launch_begin();
    if (flags & NSA_ISECT_BRUTE)
        hipLaunchKernelGGL(k_isect_brute<true>, grid, dim3(kBlock), 0, s, t, m, w, n_pairs, pairs, code);
    else
        hipLaunchKernelGGL(k_isect_tree<true>, grid, dim3(kBlock), 0, s, t, m, w, n_pairs, pairs, code);
    return launch_end();
}

}  // extern "C"
