// mesh_raster.hip -- a z-buffered image of a triangle mesh (and of point sets) from a batch of cameras, its per-pixel attributes,
// and the visibility of the mesh's faces in those images.  include/nicer_slam_amd.h Section 12 states the rule operation
// by operation and is the contract; tests/raster_ref.py is its numpy restatement, and these kernels equal it bit for bit.
//
// The winner of a pixel is the smallest 64-bit key (bits of depth) << 32 | id, taken with one unsigned 64-bit atomic minimum per
// covered pixel (a single global_atomic_umin_x2, no compare-and-swap loop).  A minimum does not depend on arrival order, so the
// atomics decide nothing in the image, and the two face paths below give the same image by construction: both call rs_pixel().
//
// k_raster_faces.  One lane per face.  A lane loads its face and three vertices once and loops over the views of the batch: the view
// index is wave-uniform, so the pose rows and intrinsics come through scalar loads.  Per view: project, reject, bounding box, and a loop
// over the box's pixel centres.  A face whose box holds more than `large_threshold` pixel centres is not drawn by its lane: its box is
// cut into 64 x 64 screen tiles and one (face, view, tile) item per tile is appended to a queue -- one counter update per WAVE (a wave
// prefix sum of the lanes' tile counts), not one per lane.  A lane whose items do not fit the queue draws its face itself (slow, never
// wrong) and marks the slots it was given below the capacity as empty.
// k_raster_items.  One wave per queued item, grid-stride; lane = column of the tile, loop over the tile's rows: a wave-wide atomic
// touches 64 consecutive keys (512 bytes).  The face is set up again from its vertices -- a few dozen operations against 4096 pixels.
// k_raster_points, k_raster_resolve (one lane per pixel), k_mesh_visible (one lane per face, views in a loop), k_raster_clear.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include "../../include/nicer_slam_amd.h"
#include "grid_common.hpp"

namespace nsa {

constexpr float kRsGuard = (float)NSA_RASTER_GUARD_PIXELS;      // |x|, |y| of a drawn vertex, pixels
constexpr float kRsFar = NSA_RASTER_FAR;
constexpr int kRsTile = 64;                                      // screen tile of a queued item, pixels per side
constexpr uint32_t kRsNoItem = 0xFFFFFFFFu;
constexpr uint32_t kRsThreads = 256;
constexpr uint64_t kRsEmpty = ~0ull;

struct RsViews {
    const float* w2c;
    const float* K;
    uint32_t n, k_stride, H, W;
    float near;
};

struct RsSetup {
    int32_t ax, ay, bx, by, cx, cy;      // snapped, after the winding swap: orient(A, B, C) > 0
    long long area2;
    float fa, iza, izb, izc;
    bool own0, own1, own2;               // does edge B->C / C->A / A->B own the pixel centres that lie exactly on it
    bool swapped;                        // B and C were exchanged: the face's own winding has orient < 0 (front-facing)
};

enum { RS_OK = 0, RS_BAD_INDEX = 1, RS_DEPTH = 2, RS_GUARD = 3, RS_DEGENERATE = 4, RS_BACKFACE = 5 };

// Section 12 "Vertex".  RS_OK, RS_DEPTH or RS_GUARD.
__device__ __forceinline__ int rs_project(const float* __restrict__ M, const float* __restrict__ Kk, float near, float vx, float vy,
                                          float vz, float& x, float& y, float& p2) {
#pragma clang fp contract(off)
    const float p0 = ((M[0] * vx + M[1] * vy) + M[2] * vz) + M[3];
    const float p1 = ((M[4] * vx + M[5] * vy) + M[6] * vz) + M[7];
    p2 = ((M[8] * vx + M[9] * vy) + M[10] * vz) + M[11];
    if (!(p2 > near && p2 <= kRsFar)) return RS_DEPTH;
    x = (p0 * Kk[0]) / p2 + Kk[2];
    y = (p1 * Kk[1]) / p2 + Kk[3];
    if (!(fabsf(x) <= kRsGuard && fabsf(y) <= kRsGuard)) return RS_GUARD;
    return RS_OK;
}

__device__ __forceinline__ int32_t rs_snap(float x) {
#pragma clang fp contract(off)
    return (int32_t)rintf(x * 256.0f);
}

__device__ __forceinline__ bool rs_owns(long long dx, long long dy) { return dy < 0 || (dy == 0 && dx > 0); }

// Section 12 "Face validity" for one face (vertices in canonical rotation) and one view.
__device__ __forceinline__ int rs_setup(const float* __restrict__ M, const float* __restrict__ Kk, float near, const float* a,
                                        const float* b, const float* c, bool cull_backface, RsSetup& s) {
#pragma clang fp contract(off)
    float xa, ya, za, xb, yb, zb, xc, yc, zc;
    const int ra = rs_project(M, Kk, near, a[0], a[1], a[2], xa, ya, za);
    const int rb = rs_project(M, Kk, near, b[0], b[1], b[2], xb, yb, zb);
    const int rc = rs_project(M, Kk, near, c[0], c[1], c[2], xc, yc, zc);
    if (ra == RS_DEPTH || rb == RS_DEPTH || rc == RS_DEPTH) return RS_DEPTH;
    if (ra == RS_GUARD || rb == RS_GUARD || rc == RS_GUARD) return RS_GUARD;
    s.ax = rs_snap(xa);
    s.ay = rs_snap(ya);
    s.bx = rs_snap(xb);
    s.by = rs_snap(yb);
    s.cx = rs_snap(xc);
    s.cy = rs_snap(yc);
    s.iza = 1.0f / za;
    s.izb = 1.0f / zb;
    s.izc = 1.0f / zc;
    long long area2 = (long long)(s.bx - s.ax) * (s.cy - s.ay) - (long long)(s.by - s.ay) * (s.cx - s.ax);
    if (area2 == 0) return RS_DEGENERATE;
    s.swapped = area2 < 0;
    if (cull_backface && !s.swapped) return RS_BACKFACE;
    if (s.swapped) {
        int32_t t = s.bx; s.bx = s.cx; s.cx = t;
        t = s.by; s.by = s.cy; s.cy = t;
        const float z = s.izb; s.izb = s.izc; s.izc = z;
        area2 = -area2;
    }
    s.area2 = area2;
    s.fa = (float)area2;
    s.own0 = rs_owns(s.cx - s.bx, s.cy - s.by);
    s.own1 = rs_owns(s.ax - s.cx, s.ay - s.cy);
    s.own2 = rs_owns(s.bx - s.ax, s.by - s.ay);
    return RS_OK;
}

// Section 12 "Coverage" and "Depth" at pixel centre (i, j).  l0..l2: the barycentric weights of A, B, C.
__device__ __forceinline__ bool rs_pixel(const RsSetup& s, int i, int j, float& depth, float& l0, float& l1, float& l2) {
#pragma clang fp contract(off)
    const long long px = 256ll * i, py = 256ll * j;
    const long long w0 = (long long)(s.cx - s.bx) * (py - s.by) - (long long)(s.cy - s.by) * (px - s.bx);
    const long long w1 = (long long)(s.ax - s.cx) * (py - s.cy) - (long long)(s.ay - s.cy) * (px - s.cx);
    const long long w2 = (long long)(s.bx - s.ax) * (py - s.ay) - (long long)(s.by - s.ay) * (px - s.ax);
    if (!((w0 > 0 || (w0 == 0 && s.own0)) && (w1 > 0 || (w1 == 0 && s.own1)) && (w2 > 0 || (w2 == 0 && s.own2)))) return false;
    l0 = (float)w0 / s.fa;
    l1 = (float)w1 / s.fa;
    l2 = (float)w2 / s.fa;
    const float invz = (l0 * s.iza + l1 * s.izb) + l2 * s.izc;
    depth = 1.0f / invz;
    return true;
}

__device__ __forceinline__ void rs_box(const RsSetup& s, uint32_t H, uint32_t W, int& i0, int& i1, int& j0, int& j1) {
    const int32_t xmin = min(s.ax, min(s.bx, s.cx)), xmax = max(s.ax, max(s.bx, s.cx));
    const int32_t ymin = min(s.ay, min(s.by, s.cy)), ymax = max(s.ay, max(s.by, s.cy));
    i0 = max(0, (xmin + 255) >> 8);
    i1 = min((int)W - 1, xmax >> 8);
    j0 = max(0, (ymin + 255) >> 8);
    j1 = min((int)H - 1, ymax >> 8);
}

__device__ __forceinline__ void rs_put(unsigned long long* __restrict__ zb, float depth, uint32_t id) {
    atomicMin(zb, ((unsigned long long)__float_as_uint(depth) << 32) | id);
}

__device__ __forceinline__ unsigned long long rs_wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// (A, B, C): the face's indices rotated so that the smallest comes first (the winding is kept).  false: an index outside [0, V).
__device__ __forceinline__ bool rs_face(const int32_t* __restrict__ faces, uint32_t f, uint32_t V, int32_t& ia, int32_t& ib, int32_t& ic) {
    const int32_t i0 = faces[(size_t)f * 3], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];
    if ((uint32_t)i0 >= V || (uint32_t)i1 >= V || (uint32_t)i2 >= V) return false;
    if (i0 <= i1 && i0 <= i2) { ia = i0; ib = i1; ic = i2; }
    else if (i1 <= i2) { ia = i1; ib = i2; ic = i0; }       // i1 < i0, i1 <= i2
    else { ia = i2; ib = i0; ic = i1; }
    return true;
}

__global__ __launch_bounds__(kRsThreads) void k_raster_clear(unsigned long long* __restrict__ zbuf, uint64_t pixels, int clear,
                                                             unsigned long long* __restrict__ totals, unsigned long long* __restrict__ counter) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0 && counter) *counter = 0;
    if (!clear) return;
    if (t < NSA_RASTER_TOTALS) totals[t] = 0;
    for (uint64_t p = t; p < pixels; p += (uint64_t)gridDim.x * blockDim.x) zbuf[p] = kRsEmpty;
}

__global__ __launch_bounds__(kRsThreads) void k_raster_faces(const float* __restrict__ verts, uint32_t V, const int32_t* __restrict__ faces,
                                                             uint32_t F, RsViews vw, int cull_backface, uint32_t large_threshold,
                                                             unsigned long long* __restrict__ counter, uint4* __restrict__ queue,
                                                             uint32_t capacity, unsigned long long* __restrict__ zbuf,
                                                             unsigned long long* __restrict__ totals) {
    const uint32_t f = blockIdx.x * kRsThreads + threadIdx.x, lane = threadIdx.x & 63;
    const bool live = f < F;
    int32_t ia = 0, ib = 0, ic = 0;
    const bool indexed = live && rs_face(faces, f, V, ia, ib, ic);
    float a[3] = {0.f, 0.f, 0.f}, b[3] = {0.f, 0.f, 0.f}, c[3] = {0.f, 0.f, 0.f};
    if (indexed) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            a[k] = verts[(size_t)ia * 3 + k];
            b[k] = verts[(size_t)ib * 3 + k];
            c[k] = verts[(size_t)ic * 3 + k];
        }
    }
    uint32_t cnt[6] = {0, 0, 0, 0, 0, 0};
    unsigned long long n_atomics = 0, n_large = 0, n_items = 0;
    const size_t pixels = (size_t)vw.H * vw.W;
#pragma unroll 1
    for (uint32_t k = 0; k < vw.n; ++k) {
        const float* __restrict__ M = vw.w2c + (size_t)k * 12;
        const float* __restrict__ Kk = vw.K + (size_t)k * vw.k_stride;
        RsSetup s;
        int rc = RS_BAD_INDEX;
        if (indexed) rc = rs_setup(M, Kk, vw.near, a, b, c, cull_backface != 0, s);
#pragma unroll
        for (int r = 0; r < 6; ++r) cnt[r] += (live && rc == r) ? 1u : 0u;
        int i0 = 0, i1 = -1, j0 = 0, j1 = -1;
        if (rc == RS_OK) rs_box(s, vw.H, vw.W, i0, i1, j0, j1);
        bool draw = rc == RS_OK && i0 <= i1 && j0 <= j1;
        uint32_t tiles = 0;
        if (draw && (uint32_t)(i1 - i0 + 1) * (uint32_t)(j1 - j0 + 1) > large_threshold)
            tiles = (uint32_t)((i1 >> 6) - (i0 >> 6) + 1) * (uint32_t)((j1 >> 6) - (j0 >> 6) + 1);
        if (__ballot(tiles > 0)) {                          // wave-uniform: some lane of the wave has a large face in this view
            uint32_t incl = tiles;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t t = __shfl_up(incl, o);
                if (lane >= (uint32_t)o) incl += t;
            }
            const uint32_t total = __shfl(incl, 63);
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(counter, (unsigned long long)total);
            base = __shfl(base, 0);
            if (tiles > 0) {
                n_large++;
                const unsigned long long at = base + (incl - tiles);
                if (at + tiles <= capacity) {
                    n_items += tiles;
                    uint32_t q = (uint32_t)at;
                    for (int ty = j0 >> 6; ty <= (j1 >> 6); ++ty)
                        for (int tx = i0 >> 6; tx <= (i1 >> 6); ++tx) queue[q++] = make_uint4(f, k, (uint32_t)tx, (uint32_t)ty);
                    draw = false;
                } else {                                    // no room: the slots below the capacity are marked empty, the lane draws
                    for (unsigned long long q = at; q < at + tiles && q < capacity; ++q) queue[q] = make_uint4(kRsNoItem, 0, 0, 0);
                }
            }
        }
        if (draw) {
            unsigned long long* __restrict__ zb = zbuf + (size_t)k * pixels;
            for (int j = j0; j <= j1; ++j)
                for (int i = i0; i <= i1; ++i) {
                    float depth, l0, l1, l2;
                    if (rs_pixel(s, i, j, depth, l0, l1, l2)) {
                        rs_put(zb + (size_t)j * vw.W + i, depth, f);
                        n_atomics++;
                    }
                }
        }
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        const unsigned long long sum = rs_wave_sum(cnt[r]);
        if (lane == 0 && sum) atomicAdd(totals + r, sum);
    }
    const unsigned long long sa = rs_wave_sum(n_atomics), sl = rs_wave_sum(n_large), si = rs_wave_sum(n_items);
    if (lane == 0) {
        if (sa) atomicAdd(totals + 6, sa);
        if (sl) atomicAdd(totals + 7, sl);
        if (si) atomicAdd(totals + 8, si);
    }
}

__global__ __launch_bounds__(64) void k_raster_items(const float* __restrict__ verts, uint32_t V, const int32_t* __restrict__ faces,
                                                     uint32_t F, RsViews vw, int cull_backface,
                                                     const unsigned long long* __restrict__ counter, const uint4* __restrict__ queue,
                                                     uint32_t capacity, unsigned long long* __restrict__ zbuf,
                                                     unsigned long long* __restrict__ totals) {
    const unsigned long long asked = *counter;
    const uint32_t n = asked < capacity ? (uint32_t)asked : capacity;
    const uint32_t lane = threadIdx.x;
    const size_t pixels = (size_t)vw.H * vw.W;
    unsigned long long n_atomics = 0;
#pragma unroll 1
    for (uint32_t q = blockIdx.x; q < n; q += gridDim.x) {
        const uint4 it = queue[q];
        const uint32_t f = it.x, k = it.y;
        if (f >= F || k >= vw.n) continue;                   // an empty slot (wave-uniform)
        int32_t ia, ib, ic;
        if (!rs_face(faces, f, V, ia, ib, ic)) continue;
        float a[3], b[3], c[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            a[d] = verts[(size_t)ia * 3 + d];
            b[d] = verts[(size_t)ib * 3 + d];
            c[d] = verts[(size_t)ic * 3 + d];
        }
        RsSetup s;
        if (rs_setup(vw.w2c + (size_t)k * 12, vw.K + (size_t)k * vw.k_stride, vw.near, a, b, c, cull_backface != 0, s) != RS_OK) continue;
        int i0, i1, j0, j1;
        rs_box(s, vw.H, vw.W, i0, i1, j0, j1);
        const int i = (int)(it.z * kRsTile + lane);
        j0 = max(j0, (int)(it.w * kRsTile));
        j1 = min(j1, (int)(it.w * kRsTile) + kRsTile - 1);
        if (it.z > 0xFFFFu || it.w > 0xFFFFu || i < i0 || i > i1) continue;     // (i0 >= 0, i1 < W: i is inside the image)
        unsigned long long* __restrict__ zb = zbuf + (size_t)k * pixels;
        for (int j = j0; j <= j1; ++j) {
            float depth, l0, l1, l2;
            if (rs_pixel(s, i, j, depth, l0, l1, l2)) {
                rs_put(zb + (size_t)j * vw.W + i, depth, f);
                n_atomics++;
            }
        }
    }
    const unsigned long long sa = rs_wave_sum(n_atomics);
    if (lane == 0 && sa) atomicAdd(totals + 6, sa);
}

__global__ __launch_bounds__(kRsThreads) void k_raster_points(const float* __restrict__ points, uint32_t P, uint32_t id0, int32_t half,
                                                              RsViews vw, unsigned long long* __restrict__ zbuf,
                                                              unsigned long long* __restrict__ totals) {
    const uint32_t q = blockIdx.x * kRsThreads + threadIdx.x, lane = threadIdx.x & 63;
    const bool live = q < P;
    float v[3] = {0.f, 0.f, 0.f};
    if (live)
        for (int d = 0; d < 3; ++d) v[d] = points[(size_t)q * 3 + d];
    unsigned long long drawn = 0, skipped = 0, n_atomics = 0;
    const size_t pixels = (size_t)vw.H * vw.W;
#pragma unroll 1
    for (uint32_t k = 0; k < vw.n; ++k) {
        float x, y, p2;
        if (!live) continue;
        if (rs_project(vw.w2c + (size_t)k * 12, vw.K + (size_t)k * vw.k_stride, vw.near, v[0], v[1], v[2], x, y, p2) != RS_OK) {
            skipped++;
            continue;
        }
        drawn++;
        const int32_t X = rs_snap(x), Y = rs_snap(y);
        const int i0 = max(0, (X - half + 255) >> 8), i1 = min((int)vw.W - 1, ((X + half + 255) >> 8) - 1);
        const int j0 = max(0, (Y - half + 255) >> 8), j1 = min((int)vw.H - 1, ((Y + half + 255) >> 8) - 1);
        unsigned long long* __restrict__ zb = zbuf + (size_t)k * pixels;
        for (int j = j0; j <= j1; ++j)
            for (int i = i0; i <= i1; ++i) {
                rs_put(zb + (size_t)j * vw.W + i, p2, id0 + q);
                n_atomics++;
            }
    }
    const unsigned long long sd = rs_wave_sum(drawn), ss = rs_wave_sum(skipped), sa = rs_wave_sum(n_atomics);
    if (lane == 0) {
        if (sd) atomicAdd(totals + 9, sd);
        if (ss) atomicAdd(totals + 10, ss);
        if (sa) atomicAdd(totals + 6, sa);
    }
}

struct RsResolve {
    const float* colours;            // [V, 3] or NULL
    const int32_t* point_colour;     // [P] or NULL
    const float* palette;            // [n_palette, 3] or NULL
    uint32_t n_points, n_palette;
    int flip_to_camera;
    int32_t* face_id;
    float* depth;
    float* normal;
    float* colour;
    float* shade;
};

__global__ __launch_bounds__(kRsThreads) void k_raster_resolve(const float* __restrict__ verts, uint32_t V, const int32_t* __restrict__ faces,
                                                               uint32_t F, RsViews vw, const unsigned long long* __restrict__ zbuf,
                                                               RsResolve o, uint64_t total) {
#pragma clang fp contract(off)
    const uint64_t pixels = (uint64_t)vw.H * vw.W;
    for (uint64_t p = (uint64_t)blockIdx.x * kRsThreads + threadIdx.x; p < total; p += (uint64_t)gridDim.x * kRsThreads) {
        const unsigned long long key = zbuf[p];
        const uint32_t id = (uint32_t)key;
        const uint32_t k = (uint32_t)(p / pixels);
        const uint32_t pix = (uint32_t)(p - (uint64_t)k * pixels);
        const int j = (int)(pix / vw.W), i = (int)(pix - (uint32_t)j * vw.W);
        const bool hit = key != kRsEmpty && (uint64_t)id < (uint64_t)F + o.n_points;
        float n[3] = {0.f, 0.f, 0.f}, col[3] = {0.f, 0.f, 0.f}, sh = 0.f;
        if (hit && id >= F) {                                // a point: its palette colour, full shade, no normal
            sh = 1.0f;
            if (o.point_colour && o.palette) {
                const int32_t ci = o.point_colour[id - F];
                if ((uint32_t)ci < o.n_palette)
                    for (int d = 0; d < 3; ++d) col[d] = o.palette[(size_t)ci * 3 + d];
            }
        }
        int32_t ia, ib, ic;
        if (hit && id < F && (o.normal || o.colour || o.shade) && rs_face(faces, id, V, ia, ib, ic)) {
            const float* __restrict__ M = vw.w2c + (size_t)k * 12;
            const float* __restrict__ Kk = vw.K + (size_t)k * vw.k_stride;
            float a[3], b[3], c[3];
            for (int d = 0; d < 3; ++d) {
                a[d] = verts[(size_t)ia * 3 + d];
                b[d] = verts[(size_t)ib * 3 + d];
                c[d] = verts[(size_t)ic * 3 + d];
            }
            RsSetup s;
            float depth, l0, l1, l2;
            if (rs_setup(M, Kk, vw.near, a, b, c, false, s) == RS_OK && rs_pixel(s, i, j, depth, l0, l1, l2)) {
                if (o.colour && o.colours) {
                    const int32_t jb = s.swapped ? ic : ib, jc = s.swapped ? ib : ic;
                    const float q0 = l0 * s.iza, q1 = l1 * s.izb, q2 = l2 * s.izc;
                    const float invz = (q0 + q1) + q2;
                    for (int d = 0; d < 3; ++d)
                        col[d] = ((q0 * o.colours[(size_t)ia * 3 + d] + q1 * o.colours[(size_t)jb * 3 + d]) + q2 * o.colours[(size_t)jc * 3 + d]) / invz;
                }
                if (o.normal || o.shade) {
                    const float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
                    const float cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
                    const float len = sqrtf((cx * cx + cy * cy) + cz * cz);
                    if (len > 0.0f && len <= 3.0e38f) {
                        n[0] = cx / len;
                        n[1] = cy / len;
                        n[2] = cz / len;
                        const float nc0 = (M[0] * n[0] + M[1] * n[1]) + M[2] * n[2], nc1 = (M[4] * n[0] + M[5] * n[1]) + M[6] * n[2];
                        const float nc2 = (M[8] * n[0] + M[9] * n[1]) + M[10] * n[2];
                        const float dx = ((float)i - Kk[2]) / Kk[0], dy = ((float)j - Kk[3]) / Kk[1];
                        const float dl = sqrtf((dx * dx + dy * dy) + 1.0f);
                        sh = fabsf(((nc0 * dx + nc1 * dy) + nc2) / dl);
                        if (o.flip_to_camera && !s.swapped) {
                            n[0] = -n[0];
                            n[1] = -n[1];
                            n[2] = -n[2];
                        }
                    }
                }
            }
        }
        if (o.face_id) o.face_id[p] = hit ? (int32_t)id : -1;
        if (o.depth) o.depth[p] = hit ? __uint_as_float((uint32_t)(key >> 32)) : 0.0f;
        if (o.shade) o.shade[p] = sh;
        if (o.normal)
            for (int d = 0; d < 3; ++d) o.normal[p * 3 + d] = n[d];
        if (o.colour)
            for (int d = 0; d < 3; ++d) o.colour[p * 3 + d] = col[d];
    }
}

// Section 12 "Visibility" of one vertex in one finished view.
__device__ __forceinline__ bool rs_seen(const float* __restrict__ M, const float* __restrict__ Kk, const RsViews& vw,
                                        const unsigned long long* __restrict__ zb, const float* v, bool depth_test, float slack) {
#pragma clang fp contract(off)
    float x, y, p2;
    if (rs_project(M, Kk, vw.near, v[0], v[1], v[2], x, y, p2) != RS_OK) return false;
    if (!(x >= 0.0f && x <= (float)(vw.W - 1) && y >= 0.0f && y <= (float)(vw.H - 1))) return false;
    if (!depth_test) return true;
    const int i0 = (int)floorf(x), j0 = (int)floorf(y);
    const int i1 = min(i0 + 1, (int)vw.W - 1), j1 = min(j0 + 1, (int)vw.H - 1);
    const unsigned long long k00 = zb[(size_t)j0 * vw.W + i0], k01 = zb[(size_t)j0 * vw.W + i1];
    const unsigned long long k10 = zb[(size_t)j1 * vw.W + i0], k11 = zb[(size_t)j1 * vw.W + i1];
    const uint32_t top = (uint32_t)(max(max(k00, k01), max(k10, k11)) >> 32);       // positive floats order as their bits
    if (top == 0xFFFFFFFFu) return true;                   // an empty pixel: +inf
    return p2 <= slack * __uint_as_float(top);
}

__global__ __launch_bounds__(kRsThreads) void k_mesh_visible(const float* __restrict__ verts, uint32_t V, const int32_t* __restrict__ faces,
                                                             uint32_t F, RsViews vw, const unsigned long long* __restrict__ zbuf, int mode,
                                                             float slack, uint8_t* __restrict__ visible) {
    const uint32_t f = blockIdx.x * kRsThreads + threadIdx.x;
    if (f >= F) return;
    const int32_t i0 = faces[(size_t)f * 3], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];
    if ((uint32_t)i0 >= V || (uint32_t)i1 >= V || (uint32_t)i2 >= V) return;
    float a[3], b[3], c[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        a[d] = verts[(size_t)i0 * 3 + d];
        b[d] = verts[(size_t)i1 * 3 + d];
        c[d] = verts[(size_t)i2 * 3 + d];
    }
    const size_t pixels = (size_t)vw.H * vw.W;
    const bool depth_test = mode != NSA_VISIBLE_FRUSTUM;
    bool vis = false;
#pragma unroll 1
    for (uint32_t k = 0; k < vw.n; ++k) {
        if (vis) continue;
        const float* __restrict__ M = vw.w2c + (size_t)k * 12;
        const float* __restrict__ Kk = vw.K + (size_t)k * vw.k_stride;
        const unsigned long long* __restrict__ zb = zbuf + (size_t)k * pixels;
        const bool sa = rs_seen(M, Kk, vw, zb, a, depth_test, slack), sb = rs_seen(M, Kk, vw, zb, b, depth_test, slack);
        const bool sc = rs_seen(M, Kk, vw, zb, c, depth_test, slack);
        vis = mode == NSA_VISIBLE_ALL ? (sa && sb && sc) : (sa || sb || sc);
    }
    if (vis) visible[f] = 1;
}

inline bool rs_views(const nsa_raster_views_t* in, RsViews* v) {
    if (!in || in->n == 0 || !in->w2c || !in->K) return false;
    if (in->H == 0 || in->W == 0 || in->H > NSA_RASTER_GUARD_PIXELS || in->W > NSA_RASTER_GUARD_PIXELS) return false;
    if (in->n > (1u << 20) || (uint64_t)in->n * in->H * in->W >= (1ull << 40)) return false;
    if (!(in->near > 0.0f && in->near < NSA_RASTER_FAR)) return false;               // NaN included
    v->w2c = in->w2c;
    v->K = in->K;
    v->n = in->n;
    v->k_stride = in->K_per_view ? 4u : 0u;
    v->H = in->H;
    v->W = in->W;
    v->near = in->near;
    return true;
}

inline bool rs_mesh(const float* verts, uint32_t V, const int32_t* faces, uint32_t F) {
    if (V >= (1u << 31) || F >= (1u << 31)) return false;
    if ((V && !verts) || (F && !faces)) return false;
    return true;
}

}  // namespace nsa

extern "C" {

uint64_t nsa_mesh_raster_workspace(uint32_t queue_capacity) { return 16ull + 16ull * queue_capacity; }

int nsa_mesh_raster(const float* verts, uint32_t n_verts, const int32_t* faces, uint32_t n_faces, const float* points,
                    uint32_t n_points, uint32_t point_size, const nsa_raster_views_t* views, int cull_backface, int clear,
                    uint32_t large_threshold, void* workspace, uint32_t queue_capacity, uint64_t* zbuf, uint64_t* totals,
                    nsa_stream_t stream) {
    using namespace nsa;
    RsViews vw;
    if (!rs_views(views, &vw) || !rs_mesh(verts, n_verts, faces, n_faces)) return NSA_EBADARG;
    if (!zbuf || !totals || !workspace) return NSA_EBADARG;
    if ((uint64_t)n_faces + n_points >= (1ull << 31)) return NSA_EBADARG;
    if (n_points && (!points || point_size == 0 || point_size > NSA_RASTER_MAX_POINT_SIZE)) return NSA_EBADARG;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* counter = (unsigned long long*)workspace;
    uint4* queue = (uint4*)((char*)workspace + 16);
    unsigned long long* zb = (unsigned long long*)zbuf;
    unsigned long long* tot = (unsigned long long*)totals;
    const uint64_t total = (uint64_t)vw.n * vw.H * vw.W;
    launch_begin();
    {
        const uint64_t blocks = clear ? (total + kRsThreads - 1) / kRsThreads : 1;
        hipLaunchKernelGGL(k_raster_clear, dim3((uint32_t)(blocks < 65536 ? blocks : 65536)), dim3(kRsThreads), 0, st, zb, total, clear,
                           tot, counter);
    }
    if (n_faces) {
        hipLaunchKernelGGL(k_raster_faces, dim3((n_faces + kRsThreads - 1) / kRsThreads), dim3(kRsThreads), 0, st, verts, n_verts, faces,
                           n_faces, vw, cull_backface, large_threshold, counter, queue, queue_capacity, zb, tot);
        if (queue_capacity && large_threshold != 0xFFFFFFFFu)
            hipLaunchKernelGGL(k_raster_items, dim3(queue_capacity < 8192u ? queue_capacity : 8192u), dim3(64), 0, st, verts, n_verts,
                               faces, n_faces, vw, cull_backface, counter, queue, queue_capacity, zb, tot);
    }
    if (n_points)
        hipLaunchKernelGGL(k_raster_points, dim3((n_points + kRsThreads - 1) / kRsThreads), dim3(kRsThreads), 0, st, points, n_points,
                           n_faces, (int32_t)(128u * point_size), vw, zb, tot);
    return launch_end();
}

int nsa_mesh_raster_resolve(const float* verts, uint32_t n_verts, const int32_t* faces, uint32_t n_faces, const float* colours,
                            const int32_t* point_colour, uint32_t n_points, const float* palette, uint32_t n_palette,
                            const nsa_raster_views_t* views, const uint64_t* zbuf, int flip_to_camera, int32_t* face_id, float* depth,
                            float* normal, float* colour, float* shade, nsa_stream_t stream) {
    using namespace nsa;
    RsViews vw;
    if (!rs_views(views, &vw) || !rs_mesh(verts, n_verts, faces, n_faces) || !zbuf) return NSA_EBADARG;
    if ((uint64_t)n_faces + n_points >= (1ull << 31)) return NSA_EBADARG;
    if (!face_id && !depth && !normal && !colour && !shade) return NSA_EBADARG;
    if (n_palette && !palette) return NSA_EBADARG;
    RsResolve o{colours, point_colour, palette, n_points, n_palette, flip_to_camera, face_id, depth, normal, colour, shade};
    const uint64_t total = (uint64_t)vw.n * vw.H * vw.W;
    const uint64_t blocks = (total + kRsThreads - 1) / kRsThreads;
    launch_begin();
    hipLaunchKernelGGL(k_raster_resolve, dim3((uint32_t)(blocks < (1u << 20) ? blocks : (1u << 20))), dim3(kRsThreads), 0,
                       (hipStream_t)stream, verts, n_verts, faces, n_faces, vw, (const unsigned long long*)zbuf, o, total);
    return launch_end();
}

int nsa_mesh_visible(const float* verts, uint32_t n_verts, const int32_t* faces, uint32_t n_faces, const nsa_raster_views_t* views,
                     const uint64_t* zbuf, int mode, float rel, uint8_t* visible, nsa_stream_t stream) {
    using namespace nsa;
    RsViews vw;
    if (!rs_views(views, &vw) || !rs_mesh(verts, n_verts, faces, n_faces)) return NSA_EBADARG;
    if (mode != NSA_VISIBLE_ANY && mode != NSA_VISIBLE_ALL && mode != NSA_VISIBLE_FRUSTUM) return NSA_EBADARG;
    if (mode != NSA_VISIBLE_FRUSTUM && (!zbuf || !(rel >= 0.0f && rel <= 1.0f))) return NSA_EBADARG;
    if (n_faces == 0) return NSA_OK;
    if (!visible) return NSA_EBADARG;
    const float slack = mode == NSA_VISIBLE_FRUSTUM ? 1.0f : 1.0f + rel;
    launch_begin();
    hipLaunchKernelGGL(k_mesh_visible, dim3((n_faces + kRsThreads - 1) / kRsThreads), dim3(kRsThreads), 0, (hipStream_t)stream, verts,
                       n_verts, faces, n_faces, vw, (const unsigned long long*)zbuf, mode, slack, visible);
    return launch_end();
}

}  // extern "C"
