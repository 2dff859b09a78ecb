// image_metrics.hip -- PSNR and SSIM of a batch of image pairs in one pass over the pixels, in float64.
// Reference: code/evaluation/eval_rendering.py scores each held-out view with rend_util.get_psnr and rend_util.get_ssim, the latter
// through code/utils/SSIM (size_average=True): five 11 x 11 grouped fp32 convolutions and sigma^2 = E[x^2] - mu^2, which cancels
// catastrophically on smooth images.  This restates the same definition with every moment and the per-pixel formula in float64.
//
// Window.  g_k = (float)exp(-(k - 5)^2 / (2 * 1.5^2)), k = 0..10, divided by their correctly rounded fp32 sum; the 2-D
// weight is the EXACT product w_ij = g_i * g_j (a float64 product of two fp32 values), so the window is separable.  The reference
// rounds w_ij to fp32 (its `mm`); that moves SSIM by < 4e-7, far below its own arithmetic error.  tests/ssim_ref.py
// uses the same window with a direct 2-D sum.
//
// Per channel, with x, y converted to float64 and zero padding of 5 on every side:
//   mu_x = sum w x, mu_y = sum w y, e_xx = sum w x^2, e_yy = sum w y^2, e_xy = sum w x y
//   s_xx = e_xx - mu_x^2, s_yy = e_yy - mu_y^2, s_xy = e_xy - mu_x mu_y
//   map = ((2 mu_x mu_y + C1)(2 s_xy + C2)) / ((mu_x^2 + mu_y^2 + C1)(s_xx + s_yy + C2)),  C1 = 1e-4, C2 = 9e-4
// The formula is compiled without FMA contraction, so an image scored against itself gives a map of exactly 1.
//
// Tiling.  k_ssim_tile: one workgroup of 256 lanes per 16 x 32 output tile of one image, all three channels.  It loads the tile with
// its 5-pixel halo of both images into LDS as fp32 (26 x 42 x 3 x 2 floats; rows read as contiguous RGB runs), then per channel a
// horizontal pass writes the five float64 moments of 26 x 32 positions to LDS and a vertical pass finishes two output pixels per
// lane.  Each lane keeps its pixels' channel sums, writes the optional map and adds its pixels' squared errors; the workgroup then
// reduces in a fixed tree to one (ssim sum, squared-error sum) partial per tile.  k_image_reduce sums an image's tile partials in a
// fixed order.  No atomics: results are bit-reproducible and independent of the other images in the batch.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include "../../include/nicer_slam_amd.h"
#include "grid_common.hpp"

namespace nsa {

constexpr int kImR = 5;                          // window radius (11 taps)
constexpr int kImTaps = 2 * kImR + 1;
constexpr int kImTH = 16, kImTW = 32;            // output tile
constexpr int kImIH = kImTH + 2 * kImR, kImIW = kImTW + 2 * kImR;
constexpr int kImThreads = 256;
constexpr uint32_t kImMaxGrid = 1u << 20;        // grid-stride beyond this many tiles
constexpr double kC1 = 0.01 * 0.01, kC2 = 0.03 * 0.03;

struct ImWindow {
    float g[kImTaps];
};

struct ImDims {
    uint32_t n, H, W, tiles_x, tiles;           // tiles per image
};

// The per-pixel SSIM value from the five windowed moments: every operation rounded on its own.
__device__ __forceinline__ double ssim_pixel(double mx, double my, double exx, double eyy, double exy) {
#pragma clang fp contract(off)
    const double mxx = mx * mx, myy = my * my, mxy = mx * my;
    const double sxx = exx - mxx, syy = eyy - myy, sxy = exy - mxy;
    return ((2.0 * mxy + kC1) * (2.0 * sxy + kC2)) / ((mxx + myy + kC1) * (sxx + syy + kC2));
}

__global__ __launch_bounds__(kImThreads) void k_ssim_tile(const float* __restrict__ pred, const float* __restrict__ gt, ImDims d,
                                                          ImWindow win, double2* __restrict__ partial, float* __restrict__ map) {
    __shared__ float sx[3][kImIH][kImIW], sy[3][kImIH][kImIW];
    __shared__ double hm[5][kImIH][kImTW];
    const int t = threadIdx.x;
    double g[kImTaps];
#pragma unroll
    for (int k = 0; k < kImTaps; ++k) g[k] = (double)win.g[k];
    const uint64_t total = (uint64_t)d.n * d.tiles;
    for (uint64_t blk = blockIdx.x; blk < total; blk += gridDim.x) {
        const uint32_t img = (uint32_t)(blk / d.tiles), tile = (uint32_t)(blk % d.tiles);
        const int r0 = (int)(tile / d.tiles_x) * kImTH, c0 = (int)(tile % d.tiles_x) * kImTW;
        const size_t base = (size_t)img * d.H * d.W * 3;
        __syncthreads();                                         // the previous tile's readers are done with LDS
        for (int e = t; e < kImIH * kImIW * 3; e += kImThreads) {
            const int ir = e / (kImIW * 3), k = e % (kImIW * 3), ic = k / 3, ch = k % 3;
            const int r = r0 - kImR + ir, c = c0 - kImR + ic;
            float xv = 0.f, yv = 0.f;
            if (r >= 0 && r < (int)d.H && c >= 0 && c < (int)d.W) {
                const size_t i = base + ((size_t)r * d.W + c) * 3 + ch;
                xv = pred[i];
                yv = gt[i];
            }
            sx[ch][ir][ic] = xv;
            sy[ch][ir][ic] = yv;
        }
        double pix[2] = {0.0, 0.0}, sse = 0.0;
        bool bad = false;
        for (int ch = 0; ch < 3; ++ch) {
            __syncthreads();                                     // inputs loaded / previous channel's vertical pass done
            for (int e = t; e < kImIH * kImTW; e += kImThreads) {
                const int ir = e / kImTW, oc = e % kImTW;
                double a = 0.0, b = 0.0, axx = 0.0, ayy = 0.0, axy = 0.0;
#pragma unroll
                for (int k = 0; k < kImTaps; ++k) {
                    const double xv = (double)sx[ch][ir][oc + k], yv = (double)sy[ch][ir][oc + k];
                    a = fma(g[k], xv, a);
                    b = fma(g[k], yv, b);
                    axx = fma(g[k], xv * xv, axx);
                    ayy = fma(g[k], yv * yv, ayy);
                    axy = fma(g[k], xv * yv, axy);
                }
                hm[0][ir][oc] = a;
                hm[1][ir][oc] = b;
                hm[2][ir][oc] = axx;
                hm[3][ir][oc] = ayy;
                hm[4][ir][oc] = axy;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int orow = t / kImTW + j * (kImTH / 2), oc = t % kImTW;
                const int r = r0 + orow, c = c0 + oc;
                if (r >= (int)d.H || c >= (int)d.W) continue;
                double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int k = 0; k < kImTaps; ++k)
#pragma unroll
                    for (int q = 0; q < 5; ++q) m[q] = fma(g[k], hm[q][orow + k][oc], m[q]);
                pix[j] += ssim_pixel(m[0], m[1], m[2], m[3], m[4]);
                const double xv = (double)sx[ch][orow + kImR][oc + kImR], yv = (double)sy[ch][orow + kImR][oc + kImR];
                const double dv = xv - yv;
                sse += dv * dv;
                bad |= !(__builtin_isfinite(xv) && __builtin_isfinite(yv));
            }
        }
        double ssim_sum = 0.0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int r = r0 + t / kImTW + j * (kImTH / 2), c = c0 + t % kImTW;
            if (r >= (int)d.H || c >= (int)d.W) continue;
            if (map) map[(size_t)img * d.H * d.W + (size_t)r * d.W + c] = (float)(pix[j] / 3.0);
            ssim_sum += pix[j];
        }
        if (bad) ssim_sum = sse = __builtin_nan("");
        // fixed-order tree over the 256 lanes (hm is free: every lane is past its vertical pass after this barrier)
        __syncthreads();
        double* red = &hm[0][0][0];
        red[t] = ssim_sum;
        red[kImThreads + t] = sse;
        for (int s = kImThreads / 2; s > 0; s >>= 1) {
            __syncthreads();
            if (t < s) {
                red[t] += red[t + s];
                red[kImThreads + t] += red[kImThreads + t + s];
            }
        }
        if (t == 0) partial[blk] = make_double2(red[0], red[kImThreads]);
    }
}

// One workgroup per image (grid-stride): the image's tile partials summed in a fixed order.
__global__ __launch_bounds__(kImThreads) void k_image_reduce(const double2* __restrict__ partial, ImDims d, double* __restrict__ ssim_mean,
                                                             double* __restrict__ sq_err_sum) {
    __shared__ double red[2][kImThreads];
    const int t = threadIdx.x;
    const double count = 3.0 * (double)d.H * (double)d.W;     // exact (< 2^31)
    for (uint32_t img = blockIdx.x; img < d.n; img += gridDim.x) {
        double s = 0.0, e = 0.0;
        for (uint32_t i = t; i < d.tiles; i += kImThreads) {
            const double2 p = partial[(size_t)img * d.tiles + i];
            s += p.x;
            e += p.y;
        }
        __syncthreads();
        red[0][t] = s;
        red[1][t] = e;
        for (int k = kImThreads / 2; k > 0; k >>= 1) {
            __syncthreads();
            if (t < k) {
                red[0][t] += red[0][t + k];
                red[1][t] += red[1][t + k];
            }
        }
        if (t == 0) {
            ssim_mean[img] = red[0][0] / count;
            sq_err_sum[img] = red[1][0];
        }
    }
}

inline bool im_dims(uint32_t n, uint32_t H, uint32_t W, ImDims* d) {
    if (n == 0 || H == 0 || W == 0 || (uint64_t)n * H * W * 3 >= (1ull << 31)) return false;
    d->n = n;
    d->H = H;
    d->W = W;
    d->tiles_x = (W + kImTW - 1) / kImTW;
    d->tiles = d->tiles_x * ((H + kImTH - 1) / kImTH);
    return true;
}

// The 1-D window as the reference builds it: fp32 values of the float64 Gaussian, divided by their fp32 sum.  The float64 sum of
// these 11 values is exact, so its fp32 rounding is the correctly rounded sum -- the value torch's sum gives in gaussian().
inline ImWindow im_window() {
    ImWindow w;
    double sum = 0.0;
    for (int k = 0; k < kImTaps; ++k) {
        w.g[k] = (float)std::exp(-(double)((k - kImR) * (k - kImR)) / (2.0 * 1.5 * 1.5));
        sum += (double)w.g[k];
    }
    const float fsum = (float)sum;
    for (int k = 0; k < kImTaps; ++k) w.g[k] = w.g[k] / fsum;
    return w;
}

}  // namespace nsa

extern "C" {

uint64_t nsa_image_metrics_workspace(uint32_t n_images, uint32_t height, uint32_t width) {
    nsa::ImDims d;
    if (!nsa::im_dims(n_images, height, width, &d)) return 0;
    return (uint64_t)d.n * d.tiles * sizeof(double2);
}

int nsa_image_metrics(const float* pred, const float* gt, uint32_t n_images, uint32_t height, uint32_t width, void* workspace,
                      double* ssim_mean, double* sq_err_sum, float* ssim_map, nsa_stream_t stream) {
    using namespace nsa;
    ImDims d;
    if (!pred || !gt || !workspace || !ssim_mean || !sq_err_sum || !im_dims(n_images, height, width, &d)) return NSA_EBADARG;
    const uint64_t total = (uint64_t)d.n * d.tiles;
    const uint32_t grid = (uint32_t)(total < kImMaxGrid ? total : kImMaxGrid);
    const uint32_t rgrid = d.n < kImMaxGrid ? d.n : kImMaxGrid;
    launch_begin();
    hipLaunchKernelGGL(k_ssim_tile, dim3(grid), dim3(kImThreads), 0, (hipStream_t)stream, pred, gt, d, im_window(),
                       (double2*)workspace, ssim_map);
    hipLaunchKernelGGL(k_image_reduce, dim3(rgrid), dim3(kImThreads), 0, (hipStream_t)stream, (const double2*)workspace, d,
                       ssim_mean, sq_err_sum);
    return launch_end();
}

}  // extern "C"
