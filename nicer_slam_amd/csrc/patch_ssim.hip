// patch_ssim.hip -- the SSIM form of the patch-warp term (C ABI section 5): warp_loss_type = "ssim" of the reference's
// SLAMLoss (code/model/loss.py:51-55,145-152), which scores every warped p x p patch against its source patch with pytorch_msssim's
// SSIM(data_range=1, win_size=p, size_average=True, channel=3).  The window is as large as the patch, so the separable valid
// convolution leaves ONE value per patch and channel; the package forms it from five grouped fp32 convolutions and
// sigma^2 = E[x^2] - mu^2, which cancels on flat patches.  Here: one pass, every moment, the SSIM value and the gradient in float64.
//
// Definition (pred = x, target = y, both [N, p^2, 3] fp32; mask [N, p^2] bytes or NULL):
//   x, y are taken as 0 where the mask is false (zeroed, not excluded: loss.py:146-147);
//   g_k = fp32 exp of the fp32 value -(k - p/2)^2 / 4.5, divided by the correctly rounded fp32 sum of the p values (sigma = 1.5);
//   w_ij = g_i * g_j exactly (a float64 product of two fp32 values), pixel i * p + j;
//   per patch and channel:  mu_x = sum w x, mu_y = sum w y, s_xx = sum w x^2 - mu_x^2, s_yy likewise, s_xy = sum w x y - mu_x mu_y,
//     A = (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1),  B = (2 s_xy + C2) / (s_xx + s_yy + C2),  SSIM = A B,  C1 = 1e-4, C2 = 9e-4;
//   loss = 1 - mean of SSIM over the 3 N values (a wholly masked patch counts with SSIM exactly 1: a reference quirk that is kept);
//   d SSIM / d x_k = w_k [ B (2 mu_y - 2 mu_x A) / (mu_x^2 + mu_y^2 + C1) + A (2 (y_k - mu_y) - 2 B (x_k - mu_x)) / (s_xx + s_yy + C2) ]
//   g_pred = -(1 / 3N) d SSIM / d x, rounded once to fp32; exactly 0 where the mask is false.
// The formulas are compiled without FMA contraction, so a patch scored against itself gives SSIM = 1 and loss = 0 exactly.
//
// Mapping.  16 lanes own one patch (4 patches per wave, 16 per workgroup); 15 of them work.  Step `it` of a group reads the 15
// consecutive floats [15 it, 15 it + 15) of the patch's run of 3 p^2, so lane l always holds channel l % 3 and five pixels per step
// are covered.  A lane keeps its elements in registers, reads their weights from a table in LDS (step `it`, lane l: pixel
// 5 it + l / 3), accumulates the five moments of its channel, and the group adds the five lanes of a channel in a fixed order
// (every lane the same order, so all lanes of a channel hold the same bits).
// Each lane then evaluates its channel's terms and writes the gradient of its elements.  The per-patch SSIM sums go, in a fixed
// order, to one float64 partial per workgroup; k_patch_ssim_final adds the partials in a fixed order.  No atomics: bit-identical
// from run to run, and a patch's gradient does not depend on where in the batch it sits.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include "../../include/nicer_slam_amd.h"
#include "grid_common.hpp"

namespace nsa {

constexpr int kPsThreads = 256;
constexpr int kPsGroup = 16;                         // lanes per patch
constexpr int kPsLanes = 15;                         // of which working: five pixels x three channels per step
constexpr int kPsPerBlock = kPsThreads / kPsGroup;   // patches per workgroup and pass
constexpr uint32_t kPsMaxBlocks = 1024;              // more patches than 1024 * 16: the workgroups stride
constexpr uint32_t kPsMaxPatch = 11;
constexpr double kPsC1 = 1e-4, kPsC2 = 9e-4;

struct PsArgs {
    const float* pred;
    const float* target;
    const uint8_t* mask;        // [n, p2] or NULL
    uint64_t n;                 // patches
    float* g_pred;              // [n, p2, 3] or NULL
    double* part;               // [blocks]
    float* loss;                // [1]
    uint32_t blocks;
    float g[kPsMaxPatch];       // the 1-D window
};

struct PsTerms {
    double ssim, B, t1, a2;     // t1 = B (2 mu_y - 2 mu_x A) / dA,  a2 = A / dB
};

// One channel of one patch from its five weighted sums: every operation rounded on its own.
__device__ __forceinline__ PsTerms ps_terms(double mx, double my, double exx, double eyy, double exy) {
#pragma clang fp contract(off)
    const double mxx = mx * mx, myy = my * my, mxy = mx * my;
    const double sxx = exx - mxx, syy = eyy - myy, sxy = exy - mxy;
    const double dA = mxx + myy + kPsC1, dB = sxx + syy + kPsC2;
    const double A = (2.0 * mxy + kPsC1) / dA, B = (2.0 * sxy + kPsC2) / dB;
    PsTerms t;
    t.ssim = A * B;
    t.B = B;
    t.t1 = B * (2.0 * my - 2.0 * mx * A) / dA;
    t.a2 = A / dB;
    return t;
}

__device__ __forceinline__ double ps_grad(const PsTerms& t, double w, double x, double y, double mx, double my) {
#pragma clang fp contract(off)
    return w * (t.t1 + t.a2 * (2.0 * (y - my) - 2.0 * t.B * (x - mx)));
}

template <int P>
__global__ __launch_bounds__(kPsThreads) void k_patch_ssim(PsArgs a) {
    constexpr int P2 = P * P, EL = 3 * P2, E = (EL + kPsLanes - 1) / kPsLanes;
    constexpr int WT = E * 5 + 1;                                     // pixels the steps reach (lane 15 included); zero past p^2
    __shared__ double sw[WT];                                         // w_ij, pixel i * p + j
    __shared__ double red[kPsPerBlock];
    const int t = threadIdx.x, l = t % kPsGroup, grp = t / kPsGroup, l3 = l / 3;
    const bool worker = l < kPsLanes;
    for (int k = t; k < WT; k += kPsThreads) sw[k] = k < P2 ? (double)a.g[k / P] * (double)a.g[k % P] : 0.0;
    __syncthreads();
    const int c0 = l % 3;                                             // the lanes c0, c0 + 3, .., c0 + 12 share this lane's channel
    const double inv = 1.0 / (3.0 * (double)a.n);
    double ssim_acc = 0.0;
    for (uint64_t base = (uint64_t)blockIdx.x * kPsPerBlock; base < a.n; base += (uint64_t)gridDim.x * kPsPerBlock) {
        const uint64_t patch = base + grp;
        const bool live = worker && patch < a.n;
        // every lane loads (idle lanes and the run's tail re-read a valid element and drop it): no load sits under a branch, so
        // all 2 E + E of them are in flight together
        const uint64_t pc = patch < a.n ? patch : a.n - 1;
        const float* px = a.pred + pc * EL;
        const float* py = a.target + pc * EL;
        float x[E], y[E];
        uint32_t valid = 0;
        int lw = l3;                                                  // opaque per pass: the weights are read where they are used,
        asm volatile("" : "+v"(lw));                                  // not hoisted into 2 E registers for the whole kernel
        if (a.mask) {
            const uint8_t* pm = a.mask + pc * P2;
            uint8_t mb[E];
#pragma unroll
            for (int it = 0; it < E; ++it) {
                const int e = it * kPsLanes + l, ec = e < EL ? e : EL - 1;
                x[it] = px[ec];
                y[it] = py[ec];
                mb[it] = pm[ec / 3];
            }
#pragma unroll
            for (int it = 0; it < E; ++it) valid |= ((live && it * kPsLanes + l < EL && mb[it] != 0) ? 1u : 0u) << it;
        } else {
#pragma unroll
            for (int it = 0; it < E; ++it) {
                const int e = it * kPsLanes + l, ec = e < EL ? e : EL - 1;
                x[it] = px[ec];
                y[it] = py[ec];
                valid |= ((live && e < EL) ? 1u : 0u) << it;
            }
        }
#pragma unroll
        for (int it = 0; it < E; ++it) {
            const bool m = (valid >> it) & 1u;
            x[it] = m ? x[it] : 0.0f;
            y[it] = m ? y[it] : 0.0f;
        }
        double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int it = 0; it < E; ++it) {
            const double xv = (double)x[it], yv = (double)y[it];
            const double wv = sw[it * 5 + lw];
            s[0] = fma(wv, xv, s[0]);
            s[1] = fma(wv, yv, s[1]);
            s[2] = fma(wv, xv * xv, s[2]);
            s[3] = fma(wv, yv * yv, s[3]);
            s[4] = fma(wv, xv * yv, s[4]);
        }
        double m5[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            double v = __shfl(s[q], c0, kPsGroup);
#pragma unroll
            for (int j = 1; j < 5; ++j) v += __shfl(s[q], c0 + 3 * j, kPsGroup);
            m5[q] = v;
        }
        const PsTerms tm = ps_terms(m5[0], m5[1], m5[2], m5[3], m5[4]);
        const double s0 = __shfl(tm.ssim, 0, kPsGroup), s1 = __shfl(tm.ssim, 1, kPsGroup), s2 = __shfl(tm.ssim, 2, kPsGroup);
        if (l == 0 && patch < a.n) ssim_acc += (s0 + s1) + s2;
        if (a.g_pred) {
            float* pg = a.g_pred + patch * EL;
#pragma unroll
            for (int it = 0; it < E; ++it) {
                const int e = it * kPsLanes + l;
                if (!(live && e < EL)) continue;
                float g = 0.0f;
                if ((valid >> it) & 1u) g = (float)(-(ps_grad(tm, sw[it * 5 + lw], (double)x[it], (double)y[it], m5[0], m5[1]) * inv));
                pg[e] = g;
            }
        }
    }
    if (l == 0) red[grp] = ssim_acc;
    __syncthreads();
    if (t == 0) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < kPsPerBlock; ++k) v += red[k];
        a.part[blockIdx.x] = v;
    }
}

__global__ __launch_bounds__(64) void k_patch_ssim_final(PsArgs a) {      // one wave, fixed order (deterministic)
    double s = 0.0;
    for (uint32_t k = threadIdx.x; k < a.blocks; k += 64) s += a.part[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (threadIdx.x != 0) return;
    a.loss[0] = (float)(1.0 - s / (3.0 * (double)a.n));      // no patches: NaN, like torch's mean of an empty tensor
}

// fp32 values of the Gaussian at the fp32 arguments, divided by their correctly rounded fp32 sum (the float64 sum of at most 11
// fp32 values of this range is exact): pytorch_msssim's _fspecial_gauss_1d(p, 1.5), with exp and the sum correctly rounded.
inline void ps_window(uint32_t patch, float* g) {
    const int half = (int)patch / 2;
    double sum = 0.0;
    for (int k = 0; k < (int)patch; ++k) {
        const float d = (float)(k - half);
        const float arg = -(d * d) / 4.5f;
        g[k] = (float)std::exp((double)arg);
        sum += (double)g[k];
    }
    const float fsum = (float)sum;
    for (int k = 0; k < (int)patch; ++k) g[k] = g[k] / fsum;
}

static inline uint32_t ps_blocks(uint64_t n_patches) {
    const uint64_t b = (n_patches + kPsPerBlock - 1) / kPsPerBlock;
    return (uint32_t)(b < 1 ? 1 : (b > kPsMaxBlocks ? kPsMaxBlocks : b));
}

}  // namespace nsa

extern "C" {

uint64_t nsa_patch_ssim_workspace(uint64_t n_patches) {
    return (uint64_t)nsa::ps_blocks(n_patches) * 2;          // doubles, counted in floats
}

int nsa_patch_ssim(const float* pred, const float* target, const uint8_t* mask, uint64_t n_patches, uint32_t patch, float* loss,
                   float* g_pred, float* workspace, nsa_stream_t stream) {
    using namespace nsa;
    if (!loss || !workspace || (n_patches && (!pred || !target))) return NSA_EBADARG;
    if (patch < 3 || !(patch & 1) || patch > kPsMaxPatch) return NSA_EBADARG;
    if (reinterpret_cast<uintptr_t>(workspace) & 7u) return NSA_EBADARG;
    if (n_patches > ((1ull << 31) - 1) / (3ull * patch * patch)) return NSA_EBADARG;      // 3 p^2 N stays below 2^31 elements
    PsArgs a{};
    a.pred = pred;
    a.target = target;
    a.mask = mask;
    a.n = n_patches;
    a.g_pred = g_pred;
    a.part = reinterpret_cast<double*>(workspace);
    a.loss = loss;
    a.blocks = n_patches ? ps_blocks(n_patches) : 0;
    ps_window(patch, a.g);
    launch_begin();
    if (n_patches) {
        const dim3 grid(a.blocks), block(kPsThreads);
        switch (patch) {
            case 3: hipLaunchKernelGGL(k_patch_ssim<3>, grid, block, 0, (hipStream_t)stream, a); break;
            case 5: hipLaunchKernelGGL(k_patch_ssim<5>, grid, block, 0, (hipStream_t)stream, a); break;
            case 7: hipLaunchKernelGGL(k_patch_ssim<7>, grid, block, 0, (hipStream_t)stream, a); break;
            case 9: hipLaunchKernelGGL(k_patch_ssim<9>, grid, block, 0, (hipStream_t)stream, a); break;
            default: hipLaunchKernelGGL(k_patch_ssim<11>, grid, block, 0, (hipStream_t)stream, a); break;
        }
    }
    hipLaunchKernelGGL(k_patch_ssim_final, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
    return launch_end();
}

}  // extern "C"
