// flow_cues.hip -- optical-flow ground truth from depth and poses (C ABI section 13): what the reference gets offline from
// GMFlow plus a forward-backward consistency check (preprocess/extract_flows.py), and the per-iteration gather of the selected
// pixels (code/training/volsdf_train.py:348-361).  With depth and poses the flow between two frames is geometry.  Three kernels, each
// ONE launch over all edges / pairs, float64 per pixel, every output rounded once on its store:
//
//   k_flowcue_induced      pixel (u, v) of frame src[e] with z-depth d:  X = ((u - cx_i) / fx_i * d, (v - cy_i) / fy_i * d, d),
//                          Y = R_e X + t_e, flow = (fx_j Y_0 / Y_2 + cx_j - u, fy_j Y_1 / Y_2 + cy_j - v);
//                          valid = isfinite(d) and d > 0 and Y_2 > near, an invalid pixel gets flow (0, 0).
//   k_flowcue_consistency  the rule stated in the header, both directions of every pair (blockIdx: pixel blocks x pair).
//   k_flowcue_select       out[e, k] = flows[e, sampling_idx[idii[e], k]], an index outside the image gives 0 / false.
//
// Memory.  The first kernel is a stream: 4 B in, 9 B out per pixel and edge.  A lane owns four consecutive pixels of the flattened
// image when H * W is a multiple of four (every frame, flow and mask base is then 16-byte aligned with the tensor): one dwordx4 load,
// two dwordx4 stores and one dword store of four mask bytes per lane, consecutive lanes consecutive addresses.  Any other size takes
// the same code with one pixel per lane (dword load, dwordx2 store, byte store), which is as wide as an unaligned image base allows.
// The consistency kernel decides both directions of a pixel in one lane: the pixel's two flows are read once (a lane owns two
// consecutive pixels when H * W is even: one dwordx4 per flow; else one pixel, dwordx2) and share the threshold, 20 B per pixel and
// pair in all; each direction then gathers four float2 taps (8 B each) of the partner's flow at its landing point -- a 6.5 MB field
// at 680 x 1200 that stays in L2.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include "../../include/nicer_slam_amd.h"
#include "grid_common.hpp"

namespace nsa {

constexpr int kFcThreads = 256;

struct FcInducedArgs {
    const float* depth;       // [n, H, W]
    const double* K;          // [n or 1, 4]
    const double* rel;        // [E, 3, 4]
    const int32_t* src;       // [E]
    const int32_t* dst;       // [E]
    float* flow;              // [E, H, W, 2]
    uint8_t* valid;           // [E, H, W]
    uint32_t n, W, HW, E, blocks_per_edge;
    int K_per_frame;
    double near;
};

struct FcFlow {
    float x, y;
    uint8_t ok;
};

__device__ __forceinline__ FcFlow fc_induced_pixel(float df, uint32_t p, uint32_t W, const double* Ki, const double* Kj, const double* M,
                                                   double near) {
    const uint32_t v = p / W, u = p - v * W;
    const double d = (double)df, ud = (double)u, vd = (double)v;
    const double X0 = (ud - Ki[2]) / Ki[0] * d, X1 = (vd - Ki[3]) / Ki[1] * d;
    const double Y0 = M[0] * X0 + M[1] * X1 + M[2] * d + M[3];
    const double Y1 = M[4] * X0 + M[5] * X1 + M[6] * d + M[7];
    const double Y2 = M[8] * X0 + M[9] * X1 + M[10] * d + M[11];
    const bool ok = (df > 0.0f) && (df <= 3.4028234663852886e38f) && (Y2 > near);      // (NaN fails every comparison)
    FcFlow r;
    r.x = ok ? (float)(Kj[0] * Y0 / Y2 + Kj[2] - ud) : 0.0f;
    r.y = ok ? (float)(Kj[1] * Y1 / Y2 + Kj[3] - vd) : 0.0f;
    r.ok = ok ? 1 : 0;
    return r;
}

template <int VEC>
__global__ __launch_bounds__(kFcThreads) void k_flowcue_induced(FcInducedArgs a) {
    const uint32_t e = blockIdx.x / a.blocks_per_edge, blk = blockIdx.x - e * a.blocks_per_edge;
    const uint32_t p0 = (blk * kFcThreads + threadIdx.x) * VEC;
    if (p0 >= a.HW) return;
    const int32_t i = a.src[e], j = a.dst[e];
    float* flow = a.flow + ((uint64_t)e * a.HW + p0) * 2;
    uint8_t* valid = a.valid + (uint64_t)e * a.HW + p0;
    const bool frames_ok = i >= 0 && (uint32_t)i < a.n && j >= 0 && (uint32_t)j < a.n;      // a bad edge reads nothing: all invalid
    double Ki[4], Kj[4], M[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        Ki[k] = frames_ok ? a.K[(a.K_per_frame ? (uint64_t)i * 4 : 0) + k] : 1.0;
        Kj[k] = frames_ok ? a.K[(a.K_per_frame ? (uint64_t)j * 4 : 0) + k] : 1.0;
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) M[k] = a.rel[(uint64_t)e * 12 + k];
    const float* dp = a.depth + (uint64_t)(frames_ok ? i : 0) * a.HW + p0;
    if constexpr (VEC == 4) {
        float4 d = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (frames_ok) d = *reinterpret_cast<const float4*>(dp);
        const FcFlow r0 = fc_induced_pixel(d.x, p0, a.W, Ki, Kj, M, a.near), r1 = fc_induced_pixel(d.y, p0 + 1, a.W, Ki, Kj, M, a.near);
        const FcFlow r2 = fc_induced_pixel(d.z, p0 + 2, a.W, Ki, Kj, M, a.near), r3 = fc_induced_pixel(d.w, p0 + 3, a.W, Ki, Kj, M, a.near);
        reinterpret_cast<float4*>(flow)[0] = make_float4(r0.x, r0.y, r1.x, r1.y);
        reinterpret_cast<float4*>(flow)[1] = make_float4(r2.x, r2.y, r3.x, r3.y);
        *reinterpret_cast<uchar4*>(valid) = make_uchar4(r0.ok, r1.ok, r2.ok, r3.ok);
    } else {
        const float d = frames_ok ? dp[0] : 0.0f;
        const FcFlow r = fc_induced_pixel(d, p0, a.W, Ki, Kj, M, a.near);
        *reinterpret_cast<float2*>(flow) = make_float2(r.x, r.y);
        valid[0] = r.ok;
    }
}

struct FcConsArgs {
    const float* flow[2];         // fwd, bwd [P, H, W, 2]
    const uint8_t* valid[2];      // [P, H, W] or both NULL
    uint8_t* occ[2];              // [P, H, W]
    uint32_t P, H, W, HW, blocks_per_image;
    double alpha, beta;
};

// Bilinear sample at (x, y) in pixel coordinates of the partner's flow (and of 1 - valid), zeros outside the image.  The four taps are
// always loaded, from coordinates clamped into the image, and a tap outside it gets weight zero: no load sits under a branch, so all
// of a lane's taps are in flight together.  A non-finite coordinate passes no test: every weight is zero and pixel (0, 0) is read.
__device__ __forceinline__ void fc_sample(const float* f, const uint8_t* ok, uint32_t H, uint32_t W, double x, double y, double& sx,
                                          double& sy, double& sinv) {
    const double x0 = floor(x), y0 = floor(y);
    const bool near_image = x0 >= -1.0 && x0 <= (double)W - 1.0 && y0 >= -1.0 && y0 <= (double)H - 1.0;
    const int ix = near_image ? (int)x0 : 0, iy = near_image ? (int)y0 : 0;
    const double wx1 = x - x0, wy1 = y - y0, wx0 = 1.0 - wx1, wy0 = 1.0 - wy1;
    const bool cx0 = near_image && ix >= 0, cx1 = near_image && ix + 1 < (int)W, cy0 = iy >= 0, cy1 = iy + 1 < (int)H;
    const uint32_t ux0 = ix < 0 ? 0u : (uint32_t)ix, ux1 = ix + 1 < (int)W ? (uint32_t)(ix + 1) : W - 1;
    const uint32_t uy0 = iy < 0 ? 0u : (uint32_t)iy, uy1 = iy + 1 < (int)H ? (uint32_t)(iy + 1) : H - 1;
    const uint32_t q[4] = {uy0 * W + ux0, uy0 * W + ux1, uy1 * W + ux0, uy1 * W + ux1};
    const bool in[4] = {cx0 && cy0, cx1 && cy0, cx0 && cy1, cx1 && cy1};
    const double w[4] = {in[0] ? wx0 * wy0 : 0.0, in[1] ? wx1 * wy0 : 0.0, in[2] ? wx0 * wy1 : 0.0, in[3] ? wx1 * wy1 : 0.0};
    float2 t[4];
    uint8_t m[4] = {1, 1, 1, 1};
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = *reinterpret_cast<const float2*>(f + (uint64_t)q[k] * 2);
    if (ok) {
#pragma unroll
        for (int k = 0; k < 4; ++k) m[k] = ok[q[k]];
    }
    sx = 0.0;
    sy = 0.0;
    sinv = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        sx += w[k] * (in[k] ? (double)t[k].x : 0.0);          // (a clamped tap may hold anything: its value is dropped, not scaled by 0)
        sy += w[k] * (in[k] ? (double)t[k].y : 0.0);
        sinv += m[k] == 0 ? w[k] : 0.0;
    }
}

// Both directions of one pixel: its two flows f = fwd(p), g = bwd(p) are read once and share mag.
__device__ __forceinline__ void fc_occluded(const FcConsArgs& a, const float* fwd, const float* bwd, const uint8_t* fwd_ok,
                                            const uint8_t* bwd_ok, bool f_ok, bool g_ok, float fx, float fy, float gx, float gy,
                                            uint32_t p, uint8_t& f_occ, uint8_t& g_occ) {
    const uint32_t v = p / a.W, u = p - v * a.W;
    const double ax = (double)fx, ay = (double)fy, bx = (double)gx, by = (double)gy;
    const double thr = a.alpha * (sqrt(ax * ax + ay * ay) + sqrt(bx * bx + by * by)) + a.beta;      // >= 0: compared as squares
    double sx, sy, sinv, tx, ty, tinv;
    fc_sample(bwd, bwd_ok, a.H, a.W, (double)u + ax, (double)v + ay, sx, sy, sinv);
    fc_sample(fwd, fwd_ok, a.H, a.W, (double)u + bx, (double)v + by, tx, ty, tinv);
    const double ex = ax + sx, ey = ay + sy, hx = bx + tx, hy = by + ty;
    f_occ = (ex * ex + ey * ey > thr * thr || !f_ok || sinv > 1e-3) ? 1 : 0;
    g_occ = (hx * hx + hy * hy > thr * thr || !g_ok || tinv > 1e-3) ? 1 : 0;
}

template <int VEC>
__global__ __launch_bounds__(kFcThreads) void k_flowcue_consistency(FcConsArgs a) {
    const uint32_t pair = blockIdx.x / a.blocks_per_image, blk = blockIdx.x - pair * a.blocks_per_image;
    const uint32_t p0 = (blk * kFcThreads + threadIdx.x) * VEC;
    if (p0 >= a.HW) return;
    const uint64_t base = (uint64_t)pair * a.HW;
    const float* fwd = a.flow[0] + base * 2;
    const float* bwd = a.flow[1] + base * 2;
    const uint8_t* fwd_ok = a.valid[0] ? a.valid[0] + base : nullptr;
    const uint8_t* bwd_ok = a.valid[1] ? a.valid[1] + base : nullptr;
    uint8_t* f_occ = a.occ[0] + base + p0;
    uint8_t* g_occ = a.occ[1] + base + p0;
    if constexpr (VEC == 2) {
        const float4 f = *reinterpret_cast<const float4*>(fwd + (uint64_t)p0 * 2), g = *reinterpret_cast<const float4*>(bwd + (uint64_t)p0 * 2);
        uchar2 fo = make_uchar2(1, 1), go = make_uchar2(1, 1);
        if (fwd_ok) {
            fo = *reinterpret_cast<const uchar2*>(fwd_ok + p0);
            go = *reinterpret_cast<const uchar2*>(bwd_ok + p0);
        }
        uchar2 of, og;
        fc_occluded(a, fwd, bwd, fwd_ok, bwd_ok, fo.x != 0, go.x != 0, f.x, f.y, g.x, g.y, p0, of.x, og.x);
        fc_occluded(a, fwd, bwd, fwd_ok, bwd_ok, fo.y != 0, go.y != 0, f.z, f.w, g.z, g.w, p0 + 1, of.y, og.y);
        *reinterpret_cast<uchar2*>(f_occ) = of;
        *reinterpret_cast<uchar2*>(g_occ) = og;
    } else {
        const float2 f = *reinterpret_cast<const float2*>(fwd + (uint64_t)p0 * 2), g = *reinterpret_cast<const float2*>(bwd + (uint64_t)p0 * 2);
        const bool f_ok = fwd_ok ? fwd_ok[p0] != 0 : true, g_ok = bwd_ok ? bwd_ok[p0] != 0 : true;
        fc_occluded(a, fwd, bwd, fwd_ok, bwd_ok, f_ok, g_ok, f.x, f.y, g.x, g.y, p0, f_occ[0], g_occ[0]);
    }
}

struct FcSelectArgs {
    const float* flows;           // [E, HW, 2]
    const uint8_t* masks;         // [E, HW]
    const int64_t* sampling_idx;  // [b, n]
    const int64_t* idii;          // [E]
    float* out_flow;              // [E, n, 2]
    uint8_t* out_mask;            // [E, n]
    uint64_t HW;
    uint32_t E, b, n, blocks_per_edge;
};

__global__ __launch_bounds__(kFcThreads) void k_flowcue_select(FcSelectArgs a) {
    const uint32_t e = blockIdx.x / a.blocks_per_edge, blk = blockIdx.x - e * a.blocks_per_edge;
    const uint32_t k = blk * kFcThreads + threadIdx.x;
    if (k >= a.n) return;
    const int64_t row = a.idii[e];
    float2 f = make_float2(0.0f, 0.0f);
    uint8_t m = 0;
    if (row >= 0 && row < (int64_t)a.b) {
        const int64_t idx = a.sampling_idx[(uint64_t)row * a.n + k];
        if (idx >= 0 && (uint64_t)idx < a.HW) {
            const uint64_t q = (uint64_t)e * a.HW + (uint64_t)idx;
            f = *reinterpret_cast<const float2*>(a.flows + q * 2);
            m = a.masks[q] != 0 ? 1 : 0;
        }
    }
    const uint64_t o = (uint64_t)e * a.n + k;
    *reinterpret_cast<float2*>(a.out_flow + o * 2) = f;
    a.out_mask[o] = m;
}

static inline bool fc_aligned(const void* p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0; }

// blocks of kFcThreads lanes x vec pixels per image, and whether images * blocks fits a grid: HIP wants gridDim.x * blockDim.x
// below 2^32, i.e. fewer than 2^24 blocks of 256 lanes
static inline bool fc_grid(uint64_t hw, uint32_t vec, uint64_t images, uint32_t* per_image, uint32_t* total) {
    const uint64_t per = (hw + (uint64_t)kFcThreads * vec - 1) / ((uint64_t)kFcThreads * vec);
    if (per * images >= (1ull << 32) / kFcThreads) return false;
    *per_image = (uint32_t)per;
    *total = (uint32_t)(per * images);
    return true;
}

}  // namespace nsa

extern "C" {

int nsa_flowcue_induced(const float* depth, uint32_t n_frames, uint32_t H, uint32_t W, const double* K, int K_per_frame,
                        const double* rel, const int32_t* src, const int32_t* dst, uint32_t n_edges, double near, float* flow,
                        uint8_t* valid, nsa_stream_t stream) {
    using namespace nsa;
    if (!H || !W || (uint64_t)H * W >= (1ull << 31) || !(near >= 0.0) || !(near < INFINITY)) return NSA_EBADARG;
    if (!n_edges) return NSA_OK;
    if (!n_frames || !depth || !K || !rel || !src || !dst || !flow || !valid) return NSA_EBADARG;
    if (!fc_aligned(depth, 4) || !fc_aligned(flow, 8) || !fc_aligned(K, 8) || !fc_aligned(rel, 8) || !fc_aligned(src, 4) ||
        !fc_aligned(dst, 4))
        return NSA_EBADARG;
    FcInducedArgs a{};
    a.depth = depth;
    a.K = K;
    a.rel = rel;
    a.src = src;
    a.dst = dst;
    a.flow = flow;
    a.valid = valid;
    a.n = n_frames;
    a.W = W;
    a.HW = H * W;
    a.E = n_edges;
    a.K_per_frame = K_per_frame;
    a.near = near;
    const bool vec = (a.HW % 4 == 0) && fc_aligned(depth, 16) && fc_aligned(flow, 16) && fc_aligned(valid, 4);
    uint32_t total = 0;
    if (!fc_grid(a.HW, vec ? 4 : 1, n_edges, &a.blocks_per_edge, &total)) return NSA_EBADARG;
    launch_begin();
    if (vec)
        hipLaunchKernelGGL(k_flowcue_induced<4>, dim3(total), dim3(kFcThreads), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(k_flowcue_induced<1>, dim3(total), dim3(kFcThreads), 0, (hipStream_t)stream, a);
    return launch_end();
}

int nsa_flowcue_consistency(const float* fwd, const float* bwd, const uint8_t* fwd_valid, const uint8_t* bwd_valid, uint32_t n_pairs,
                            uint32_t H, uint32_t W, double alpha, double beta, uint8_t* fwd_occ, uint8_t* bwd_occ,
                            nsa_stream_t stream) {
    using namespace nsa;
    if (H < 2 || W < 2 || (uint64_t)H * W >= (1ull << 31)) return NSA_EBADARG;
    if (!(alpha >= 0.0) || !(alpha < INFINITY) || !(beta >= 0.0) || !(beta < INFINITY)) return NSA_EBADARG;
    if ((fwd_valid == nullptr) != (bwd_valid == nullptr)) return NSA_EBADARG;
    if (!n_pairs) return NSA_OK;
    if (!fwd || !bwd || !fwd_occ || !bwd_occ || !fc_aligned(fwd, 8) || !fc_aligned(bwd, 8)) return NSA_EBADARG;
    FcConsArgs a{};
    a.flow[0] = fwd;
    a.flow[1] = bwd;
    a.valid[0] = fwd_valid;
    a.valid[1] = bwd_valid;
    a.occ[0] = fwd_occ;
    a.occ[1] = bwd_occ;
    a.P = n_pairs;
    a.H = H;
    a.W = W;
    a.HW = H * W;
    a.alpha = alpha;
    a.beta = beta;
    const bool vec = (a.HW % 2 == 0) && fc_aligned(fwd, 16) && fc_aligned(bwd, 16) && fc_aligned(fwd_occ, 2) && fc_aligned(bwd_occ, 2) &&
                     fc_aligned(fwd_valid, 2) && fc_aligned(bwd_valid, 2);
    uint32_t total = 0;
    if (!fc_grid(a.HW, vec ? 2 : 1, n_pairs, &a.blocks_per_image, &total)) return NSA_EBADARG;
    launch_begin();
    if (vec)
        hipLaunchKernelGGL(k_flowcue_consistency<2>, dim3(total), dim3(kFcThreads), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(k_flowcue_consistency<1>, dim3(total), dim3(kFcThreads), 0, (hipStream_t)stream, a);
    return launch_end();
}

int nsa_flowcue_select(const float* flows, const uint8_t* masks, uint32_t n_edges, uint64_t n_pixels, const int64_t* sampling_idx,
                       uint32_t b, uint32_t n, const int64_t* idii, float* out_flow, uint8_t* out_mask, nsa_stream_t stream) {
    using namespace nsa;
    if (!n_pixels || n_pixels >= (1ull << 31)) return NSA_EBADARG;
    if (!n_edges || !n) return NSA_OK;
    if (!b || !flows || !masks || !sampling_idx || !idii || !out_flow || !out_mask) return NSA_EBADARG;
    if (!fc_aligned(flows, 8) || !fc_aligned(out_flow, 8) || !fc_aligned(sampling_idx, 8) || !fc_aligned(idii, 8)) return NSA_EBADARG;
    FcSelectArgs a{};
    a.flows = flows;
    a.masks = masks;
    a.sampling_idx = sampling_idx;
    a.idii = idii;
    a.out_flow = out_flow;
    a.out_mask = out_mask;
    a.HW = n_pixels;
    a.E = n_edges;
    a.b = b;
    a.n = n;
    uint32_t total = 0;
    if (!fc_grid(n, 1, n_edges, &a.blocks_per_edge, &total)) return NSA_EBADARG;
    launch_begin();
    hipLaunchKernelGGL(k_flowcue_select, dim3(total), dim3(kFcThreads), 0, (hipStream_t)stream, a);
    return launch_end();
}

}  // extern "C"
