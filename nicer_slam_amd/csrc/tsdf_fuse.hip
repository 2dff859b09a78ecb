// tsdf_fuse.hip -- depth frames fused into a dense truncated-signed-distance volume, and the volume's colour at points.
// Reference: preprocess/get_mesh_7scenes.py makes the ground-truth mesh of a 7-Scenes sequence by integrating its depth frames into
// open3d's ScalableTSDFVolume; include/nicer_slam_amd.h Section 10 restates the per-voxel rule and is the contract
// (tests/tsdf_ref.py is its numpy restatement, and the kernel equals it bit for bit).
//
// k_tsdf_integrate.  A workgroup of 256 lanes owns a brick of 4 x 8 x 32 voxels (x, y, z), four voxels per lane (y two apart), lanes
// along z: every wave-wide load or store of a state array is two runs of 128 bytes.  A lane loads its voxels' state once (twenty loads
// in flight), applies the frames of the batch in order from registers, and stores the state of the voxels that a frame touched.
// Four per lane because one per lane leaves too little in flight per workgroup: it reads the state at 2.0 instead of 4.5 TB/s on
// MI355X, while eight make the brick too coarse for the culling below (DESIGN 4i has the measurements).
//
// Culling.  Per chunk of 256 frames, lane j tests frame j against the brick: the brick's voxel centres lie in a box of half extents
// h = voxel_length * (2, 4, 16) about its centre, which the frame's rows map into a camera-frame box of half extents
// e_r = sum_j |R_rj| h_j (true for any matrix, rigid or not).  The frame is dropped when that box lies behind the camera, beyond
// the frame's largest accepted depth plus the truncation, or outside one of the four frustum planes that the pixel test
// 0 <= u_f < W, 0 <= v_f < H draws -- every one of them a condition under which the rule skips each voxel of the brick.  h is half a
// voxel larger per axis than the centres reach and every comparison carries a relative slack far above fp32 rounding, so the test is
// conservative; a NaN anywhere compares false and keeps the frame.  The wave ballots of the survivors go to LDS, and every lane then
// walks the set bits in ascending order: the frame index is wave-uniform, so the frame's rows and intrinsics come through scalar loads.
// A build with -DNSA_X_TSDF_NOCULL (side-by-side experiment builds only) keeps every frame, to price the test (tools/bench_tsdf.py).
//
// k_tsdf_frame_zmax_parts / k_tsdf_frame_zmax: the largest depth of each frame that the rule accepts (0 when there is none: the frame is
// dropped), 32 workgroups per frame and then one lane per frame -- two stages instead of an atomic maximum, so nothing needs zeroing.
// k_tsdf_sample_colour: one lane per point, the masked trilinear lookup of Section 10.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include "../../include/nicer_slam_amd.h"
#include "grid_common.hpp"

namespace nsa {

constexpr int kTsVPT = 4;                            // voxels per lane
constexpr int kTsBX = 4, kTsBY = 2 * kTsVPT, kTsBZ = 32;   // brick, voxels per axis
constexpr int kTsThreads = kTsBX * 2 * kTsBZ;        // kTsBX waves of 2 (y) * 32 (z) lanes
static_assert(kTsThreads == 256, "one wave per x of the brick");
constexpr int kTsZParts = 32;                        // workgroups per frame of the depth-range pass
constexpr int kTsWaves = kTsThreads / 64;
constexpr uint64_t kTsMaxGrid = 1ull << 23;       // workgroups per launch (grid * 256 lanes stays below 2^32); the rest by grid stride

struct TsdfVol {
    float* tsdf;
    float* weight;
    float* colour;
    uint32_t nx, ny, nz;
    float ox, oy, oz, vl, trunc, inv_trunc;
    uint32_t bricks_y, bricks_z;
};

struct TsdfFrames {
    const float* depth;
    const float* rgb;
    const float* w2c;
    const float* K;
    const float* zmax;
    uint32_t n, H, W;
    uint32_t k_stride;          // 4 with one K per frame, 0 with one for all
    float depth_trunc;
};

// The rule of Section 10 for one voxel and one frame.  Returns whether the frame touched the voxel.
template <bool COLOUR>
__device__ __forceinline__ bool tsdf_apply(const TsdfVol& v, const TsdfFrames& f, uint32_t k, float cx, float cy, float cz, float& ts,
                                           float& wt, float& c0, float& c1, float& c2) {
#pragma clang fp contract(off)
    const float* __restrict__ M = f.w2c + (size_t)k * 12;
    const float* __restrict__ Kk = f.K + (size_t)k * f.k_stride;
    const float p0 = ((M[0] * cx + M[1] * cy) + M[2] * cz) + M[3];
    const float p1 = ((M[4] * cx + M[5] * cy) + M[6] * cz) + M[7];
    const float p2 = ((M[8] * cx + M[9] * cy) + M[10] * cz) + M[11];
    if (!(p2 > 0.0f)) return false;
    const float uf = ((p0 * Kk[0]) / p2 + Kk[2]) + 0.5f;
    const float vf = ((p1 * Kk[1]) / p2 + Kk[3]) + 0.5f;
    if (!(uf >= 0.0f && uf < (float)f.W && vf >= 0.0f && vf < (float)f.H)) return false;
    const uint32_t pix = (uint32_t)(int)vf * f.W + (uint32_t)(int)uf;          // < H * W
    const size_t at = (size_t)k * f.H * f.W + pix;
    const float d = f.depth[at];
    if (!(d > 0.0f && d <= f.depth_trunc)) return false;
    const float sdf = d - p2;
    if (!(sdf > -v.trunc)) return false;
    const float x = sdf * v.inv_trunc;
    const float t = x < 1.0f ? x : 1.0f;
    const float den = wt + 1.0f;
    ts = (ts * wt + t) / den;
    if (COLOUR) {
        const float* __restrict__ px = f.rgb + at * 3;
        c0 = (c0 * wt + px[0]) / den;
        c1 = (c1 * wt + px[1]) / den;
        c2 = (c2 * wt + px[2]) / den;
    }
    wt = den;
    return true;
}

// Conservative: true only when the rule skips every voxel of the brick for frame k.  (bx, by, bz): the brick's centre.
__device__ __forceinline__ bool tsdf_cull(const TsdfVol& v, const TsdfFrames& f, uint32_t k, float bx, float by, float bz) {
#ifdef NSA_X_TSDF_NOCULL
    return false;
#else
    const float zm = f.zmax[k];
    if (zm == 0.0f) return true;                                   // no depth of this frame is accepted
    const float* __restrict__ M = f.w2c + (size_t)k * 12;
    const float* __restrict__ Kk = f.K + (size_t)k * f.k_stride;
    const float hx = v.vl * (0.5f * kTsBX), hy = v.vl * (0.5f * kTsBY), hz = v.vl * (0.5f * kTsBZ);
    constexpr float kRel = 1e-5f;                                  // >> the few ulp (6e-8 each) of either side's p_r
    float pc[3], e[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float a = M[4 * r] * bx, b = M[4 * r + 1] * by, c = M[4 * r + 2] * bz, t = M[4 * r + 3];
        pc[r] = a + b + c + t;
        e[r] = fabsf(M[4 * r]) * hx + fabsf(M[4 * r + 1]) * hy + fabsf(M[4 * r + 2]) * hz;
        e[r] += kRel * (fabsf(a) + fabsf(b) + fabsf(c) + fabsf(t) + e[r]);
    }
    if (pc[2] + e[2] <= 0.0f) return true;                         // p_2 <= 0 for every voxel
    if (pc[2] - e[2] > (zm + v.trunc) * (1.0f + kRel)) return true; // sdf = d - p_2 <= zmax - p_2 < -sdf_trunc for every voxel
    // 0 <= u_f  <=>  fx p_0 + (cx + 0.5) p_2 >= 0  and  u_f < W  <=>  fx p_0 + (cx + 0.5 - W) p_2 < 0  where p_2 > 0; v likewise.
    // u_f itself is off its exact value by a few ulp of max(|fx p_0 / p_2|, cx): in these units, a few 1e-7 of the magnitudes below.
    constexpr float kRelPix = 1e-4f;
#pragma unroll
    for (int ax = 0; ax < 2; ++ax) {
        const float fk = Kk[ax], lo = Kk[2 + ax] + 0.5f, hi = lo - (float)(ax == 0 ? f.W : f.H);
        const float fp = fk * pc[ax], fe = fabsf(fk) * e[ax];
        const float g_lo = fp + lo * pc[2], e_lo = fe + fabsf(lo) * e[2];
        if (g_lo + e_lo + kRelPix * (fabsf(fp) + fabsf(lo * pc[2]) + e_lo) < 0.0f) return true;
        const float g_hi = fp + hi * pc[2], e_hi = fe + fabsf(hi) * e[2];
        if (g_hi - e_hi - kRelPix * (fabsf(fp) + fabsf(hi * pc[2]) + e_hi) > 0.0f) return true;
    }
    return false;
#endif
}

template <bool COLOUR>
__global__ __launch_bounds__(kTsThreads) void k_tsdf_integrate(TsdfVol v, TsdfFrames f, uint64_t bricks) {
    __shared__ unsigned long long live[kTsWaves];
    const uint32_t t = threadIdx.x;
    const size_t cells = (size_t)v.nx * v.ny * v.nz;
    for (uint64_t brick = blockIdx.x; brick < bricks; brick += gridDim.x) {
        uint32_t b = (uint32_t)brick;
        const uint32_t bz = b % v.bricks_z;
        b /= v.bricks_z;
        const uint32_t by = b % v.bricks_y, bx = b / v.bricks_y;
        // lane -> voxels: x from the wave, z from the low five bits, and kTsVPT values of y two apart (each wave-wide access: two rows of 128 bytes)
        const uint32_t ix = bx * kTsBX + (t >> 6), iy0 = by * kTsBY + ((t >> 5) & 1), iz = bz * kTsBZ + (t & 31);
        const bool in_xz = ix < v.nx && iz < v.nz;
        bool valid[kTsVPT];
        size_t at[kTsVPT];
        float cx, cz, cy[kTsVPT];
        {
#pragma clang fp contract(off)
            cx = v.ox + v.vl * ((float)ix + 0.5f);
            cz = v.oz + v.vl * ((float)iz + 0.5f);
#pragma unroll
            for (int j = 0; j < kTsVPT; ++j) {
                const uint32_t iy = iy0 + 2 * j;
                valid[j] = in_xz && iy < v.ny;
                at[j] = ((size_t)ix * v.ny + iy) * v.nz + iz;
                cy[j] = v.oy + v.vl * ((float)iy + 0.5f);
            }
        }
        const float mx = v.ox + v.vl * ((float)(bx * kTsBX) + 0.5f * kTsBX);
        const float my = v.oy + v.vl * ((float)(by * kTsBY) + 0.5f * kTsBY);
        const float mz = v.oz + v.vl * ((float)(bz * kTsBZ) + 0.5f * kTsBZ);
        float ts[kTsVPT], wt[kTsVPT], c0[kTsVPT], c1[kTsVPT], c2[kTsVPT];
        bool touched[kTsVPT];
#pragma unroll
        for (int j = 0; j < kTsVPT; ++j) {
            ts[j] = wt[j] = c0[j] = c1[j] = c2[j] = 0.f;
            touched[j] = false;
            if (valid[j]) {
                ts[j] = v.tsdf[at[j]];
                wt[j] = v.weight[at[j]];
                if (COLOUR) {
                    c0[j] = v.colour[at[j]];
                    c1[j] = v.colour[cells + at[j]];
                    c2[j] = v.colour[2 * cells + at[j]];
                }
            }
        }
        for (uint32_t base = 0; base < f.n; base += kTsThreads) {
            const uint32_t mine = base + t;
            const bool keep = mine < f.n && !tsdf_cull(v, f, mine, mx, my, mz);
            const unsigned long long bal = __ballot(keep);
            __syncthreads();                                        // the previous chunk's readers are done
            if ((t & 63) == 0) live[t >> 6] = bal;
            __syncthreads();
#pragma unroll 1
            for (int w = 0; w < kTsWaves; ++w) {
                const unsigned long long m = live[w];
                const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)m), hi = __builtin_amdgcn_readfirstlane((uint32_t)(m >> 32));
#pragma unroll 1
                for (int half = 0; half < 2; ++half) {
                    uint32_t bits = half ? hi : lo;
                    while (bits) {                                  // ascending k: the frames are applied in order
                        const uint32_t k = base + (uint32_t)w * 64 + (uint32_t)half * 32 + (uint32_t)__builtin_ctz(bits);
                        bits &= bits - 1;
#pragma unroll
                        for (int j = 0; j < kTsVPT; ++j)
                            if (valid[j]) touched[j] |= tsdf_apply<COLOUR>(v, f, k, cx, cy[j], cz, ts[j], wt[j], c0[j], c1[j], c2[j]);
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kTsVPT; ++j)
            if (touched[j]) {
                v.tsdf[at[j]] = ts[j];
                v.weight[at[j]] = wt[j];
                if (COLOUR) {
                    v.colour[at[j]] = c0[j];
                    v.colour[cells + at[j]] = c1[j];
                    v.colour[2 * cells + at[j]] = c2[j];
                }
            }
    }
}

// Stage 1 of the frames' depth range: workgroup (j, k) takes the j-th of kTsZParts slices of frame k and writes the largest depth in it
// with d > 0 and d <= depth_trunc (0 when there is none) to part[k * kTsZParts + j].
__global__ __launch_bounds__(kTsThreads) void k_tsdf_frame_zmax_parts(const float* __restrict__ depth, uint32_t pixels, float depth_trunc,
                                                                      float* __restrict__ part) {
    __shared__ float red[kTsThreads];
    const uint32_t t = threadIdx.x, k = blockIdx.y;
    const float* __restrict__ d = depth + (size_t)k * pixels;
    const uint32_t per = (pixels + kTsZParts - 1) / kTsZParts;
    const uint32_t lo = blockIdx.x * per, hi = lo + per < pixels ? lo + per : pixels;
    float m = 0.f;
    for (uint32_t p = lo + t; p < hi; p += kTsThreads) {
        const float x = d[p];
        if (x > 0.0f && x <= depth_trunc && x > m) m = x;
    }
    red[t] = m;
    for (int s = kTsThreads / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (t < (uint32_t)s && red[t + s] > red[t]) red[t] = red[t + s];
    }
    if (t == 0) part[(size_t)k * kTsZParts + blockIdx.x] = red[0];
}

// Stage 2: zmax[k] = the largest of frame k's parts.
__global__ __launch_bounds__(kTsThreads) void k_tsdf_frame_zmax(const float* __restrict__ part, uint32_t n, float* __restrict__ zmax) {
    const uint32_t k = blockIdx.x * kTsThreads + threadIdx.x;
    if (k >= n) return;
    float m = 0.f;
    for (int j = 0; j < kTsZParts; ++j) {
        const float x = part[(size_t)k * kTsZParts + j];
        if (x > m) m = x;
    }
    zmax[k] = m;
}

__global__ __launch_bounds__(256) void k_tsdf_sample_colour(TsdfVol v, const float* __restrict__ points, uint64_t m,
                                                            float* __restrict__ out) {
#pragma clang fp contract(off)
    const size_t cells = (size_t)v.nx * v.ny * v.nz;
    const uint32_t dims[3] = {v.nx, v.ny, v.nz};
    const float org[3] = {v.ox, v.oy, v.oz};
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < m; q += (uint64_t)gridDim.x * blockDim.x) {
        int b[3];
        float fr[3];
        bool inside = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float g = (points[q * 3 + a] - org[a]) / v.vl - 0.5f;
            const float fl = floorf(g);
            inside = inside && fl >= -1.0f && fl < (float)dims[a];      // false for NaN / inf; past this, some corner may lie inside
            b[a] = inside ? (int)fl : 0;
            fr[a] = g - fl;
        }
        float s = 0.f, a0 = 0.f, a1 = 0.f, a2 = 0.f;
        if (inside) {
#pragma unroll
            for (int dx = 0; dx < 2; ++dx)
#pragma unroll
                for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                    for (int dz = 0; dz < 2; ++dz) {
                        const int x = b[0] + dx, y = b[1] + dy, z = b[2] + dz;
                        if (x < 0 || y < 0 || z < 0 || x >= (int)v.nx || y >= (int)v.ny || z >= (int)v.nz) continue;
                        const size_t i = ((size_t)x * v.ny + y) * v.nz + z;
                        if (!(v.weight[i] > 0.0f)) continue;
                        const float wx = dx ? fr[0] : 1.0f - fr[0], wy = dy ? fr[1] : 1.0f - fr[1], wz = dz ? fr[2] : 1.0f - fr[2];
                        const float w = (wx * wy) * wz;
                        s = s + w;
                        a0 = a0 + w * v.colour[i];
                        a1 = a1 + w * v.colour[cells + i];
                        a2 = a2 + w * v.colour[2 * cells + i];
                    }
        }
        const bool any = s > 0.0f;
        out[q * 3 + 0] = any ? a0 / s : 0.0f;
        out[q * 3 + 1] = any ? a1 / s : 0.0f;
        out[q * 3 + 2] = any ? a2 / s : 0.0f;
    }
}

inline bool finite_pos(float x) { return std::isfinite(x) && x > 0.0f; }

// Validates the descriptor (no device access) and fills the kernels' view of it.
inline bool tsdf_vol(const nsa_tsdf_volume_t* in, bool need_colour, TsdfVol* v) {
    if (!in || !in->tsdf || !in->weight || (need_colour && !in->colour)) return false;
    if (in->nx == 0 || in->ny == 0 || in->nz == 0) return false;
    if ((uint64_t)in->nx * in->ny > (1ull << 31) || (uint64_t)in->nx * in->ny * in->nz > (1ull << 31)) return false;
    if (!finite_pos(in->voxel_length) || !finite_pos(in->sdf_trunc) || !std::isfinite(1.0f / in->sdf_trunc)) return false;
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(in->origin[a])) return false;
    v->tsdf = in->tsdf;
    v->weight = in->weight;
    v->colour = in->colour;
    v->nx = in->nx;
    v->ny = in->ny;
    v->nz = in->nz;
    v->ox = in->origin[0];
    v->oy = in->origin[1];
    v->oz = in->origin[2];
    v->vl = in->voxel_length;
    v->trunc = in->sdf_trunc;
    v->inv_trunc = 1.0f / in->sdf_trunc;
    v->bricks_y = (in->ny + kTsBY - 1) / kTsBY;
    v->bricks_z = (in->nz + kTsBZ - 1) / kTsBZ;
    return true;
}

}  // namespace nsa

extern "C" {

int nsa_tsdf_integrate(const nsa_tsdf_volume_t* vol, const float* depth, const float* rgb, const float* w2c, const float* K,
                       int K_per_frame, uint32_t n, uint32_t H, uint32_t W, float depth_trunc, float* frame_zmax,
                       nsa_stream_t stream) {
    using namespace nsa;
    TsdfVol v;
    if (!tsdf_vol(vol, false, &v)) return NSA_EBADARG;
    if (n == 0) return NSA_OK;
    if (!depth || !w2c || !K || !frame_zmax || (v.colour && !rgb)) return NSA_EBADARG;
    if (H == 0 || W == 0 || H >= (1u << 24) || W >= (1u << 24) || (uint64_t)H * W >= (1ull << 31)) return NSA_EBADARG;
    if (!(depth_trunc > 0.0f)) return NSA_EBADARG;                  // NaN included
    TsdfFrames f{depth, rgb, w2c, K, frame_zmax, n, H, W, K_per_frame ? 4u : 0u, depth_trunc};
    const uint64_t bricks = (uint64_t)((v.nx + kTsBX - 1) / kTsBX) * v.bricks_y * v.bricks_z;   // <= the voxel count
    const uint32_t grid = (uint32_t)(bricks < kTsMaxGrid ? bricks : kTsMaxGrid);
    launch_begin();
    float* parts = frame_zmax + n;
    for (uint32_t lo = 0; lo < n; lo += 65535u) {                   // (grid y is limited to 65535)
        const uint32_t m = n - lo < 65535u ? n - lo : 65535u;
        hipLaunchKernelGGL(k_tsdf_frame_zmax_parts, dim3(kTsZParts, m), dim3(kTsThreads), 0, (hipStream_t)stream,
                           depth + (size_t)lo * H * W, H * W, depth_trunc, parts + (size_t)lo * kTsZParts);
    }
    hipLaunchKernelGGL(k_tsdf_frame_zmax, dim3((n + kTsThreads - 1) / kTsThreads), dim3(kTsThreads), 0, (hipStream_t)stream, parts, n,
                       frame_zmax);
    if (v.colour)
        hipLaunchKernelGGL(k_tsdf_integrate<true>, dim3(grid), dim3(kTsThreads), 0, (hipStream_t)stream, v, f, bricks);
    else
        hipLaunchKernelGGL(k_tsdf_integrate<false>, dim3(grid), dim3(kTsThreads), 0, (hipStream_t)stream, v, f, bricks);
    return launch_end();
}

int nsa_tsdf_sample_colour(const nsa_tsdf_volume_t* vol, const float* points, uint64_t m, float* out, nsa_stream_t stream) {
    using namespace nsa;
    TsdfVol v;
    if (!tsdf_vol(vol, true, &v)) return NSA_EBADARG;
    if (m == 0) return NSA_OK;
    if (!points || !out || m >= (1ull << 40)) return NSA_EBADARG;
    const uint64_t blocks = (m + 255) / 256;
    launch_begin();
    hipLaunchKernelGGL(k_tsdf_sample_colour, dim3((uint32_t)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, v,
                       points, m, out);
    return launch_end();
}

}  // extern "C"
