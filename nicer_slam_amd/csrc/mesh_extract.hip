// mesh_extract.hip -- marching cubes over a dense fp32 volume on the device.
// Reference: skimage.measure.marching_cubes on the host (code/utils/plots.py:128), fed by the grid of plots.py:117-127 (here
// inference.sdf_grid) and followed by the vertex colouring of plots.py:137-149 (here inference.extract_mesh).
//
// Volume vol[nx, ny, nz], C-contiguous, sample (x, y, z) at linear index s = (x * ny + y) * nz + z.
//   inside:   value < level (strict; a sample exactly at the level is outside).
//   vertex:   one per grid edge whose two samples are finite and on opposite sides, owned by the edge's lower sample s along
//             axis a.  With f0 = vol[s], f1 = vol[s + stride_a], all in fp32 with no FMA contraction:
//               t = (level - f0) / (f1 - f0)
//               p_k = origin_k + spacing_k * c_k,   c_k = (float)i_k for k != a,   c_a = (float)i_a + t
//   normal:   g(sample) per axis k: (f[i+1] - f[i-1]) / (2 spacing_k) inside, (f[1] - f[0]) / spacing_k and
//             (f[n-1] - f[n-2]) / spacing_k on the border; m = (1 - t) * g(s) + t * g(s + stride_a);
//             n = m / sqrt((m_x^2 + m_y^2) + m_z^2), or 0 when that length is zero or not finite.  It points towards increasing
//             value (outward for an SDF).  Not checked against skimage's normals (not available to compare).
//   faces:    a cell with a non-finite corner emits none; otherwise the triangles of csrc/mc_table.hpp for its case.  Vertices
//             next to non-finite samples may therefore be unreferenced.
//   order:    vertices by (owner sample s, axis x, y, z); faces by (cell = its lower corner's s, table order).  No atomics.
//
// Structure: a "chunk" is 64 consecutive samples, one wave; a block of 4 waves owns 64 consecutive chunks (4096 samples).
//   count:  k_mc_count classifies every sample (its up-to-3 owned edges: a ballot mask per axis; its cell: triangle count) and
//           writes per-chunk masks + counts and per-block sums; k_mc_scan (one workgroup) scans the block sums in order and
//           writes the two 64-bit totals.
//   emit:   k_mc_verts turns the block offsets into per-chunk offsets and writes the vertices; k_mc_faces maps each cell edge to
//           its vertex id (chunk offset + popcounts of the owner chunk's masks) and writes the faces.  Chunks without work exit
//           after one 8-byte read.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/nicer_slam_amd.h"
#include "block_scan.hpp"
#include "mc_table.hpp"

namespace nsa {

constexpr uint32_t kChunksPerBlock = 64;
constexpr uint32_t kSamplesPerBlock = kChunksPerBlock * 64;
constexpr uint32_t kMaxSamples = 1u << 31;

struct McDims {
    uint32_t nx, ny, nz, nynz, N;
};

struct McWork {                // views into the caller's workspace (nsa_marching_cubes_workspace bytes)
    uint64_t* masks;           // [n_chunks][3] crossing-edge ballots per axis
    uint2* cnt;                // [n_chunks] (vertices, triangles)
    uint2* off;                // [n_chunks] (first vertex, first face), written by k_mc_verts
    uint64_t* bsum;            // [n_blocks][2]
    uint64_t* boff;            // [n_blocks][2] exclusive
};

__host__ __device__ inline uint64_t align8(uint64_t b) { return (b + 7) & ~uint64_t(7); }

__host__ __device__ inline McWork carve(void* ws, uint32_t n_chunks, uint32_t n_blocks) {
    char* p = static_cast<char*>(ws);
    McWork w;
    w.masks = reinterpret_cast<uint64_t*>(p);
    p += align8(uint64_t(n_chunks) * 24);
    w.cnt = reinterpret_cast<uint2*>(p);
    p += align8(uint64_t(n_chunks) * 8);
    w.off = reinterpret_cast<uint2*>(p);
    p += align8(uint64_t(n_chunks) * 8);
    w.bsum = reinterpret_cast<uint64_t*>(p);
    p += uint64_t(n_blocks) * 16;
    w.boff = reinterpret_cast<uint64_t*>(p);
    return w;
}

__host__ __device__ inline uint64_t workspace_bytes(uint32_t n_chunks, uint32_t n_blocks) {
    return align8(uint64_t(n_chunks) * 24) + 2 * align8(uint64_t(n_chunks) * 8) + uint64_t(n_blocks) * 32;
}

__device__ __forceinline__ bool crosses(float f0, float f1, float level) {
    return __builtin_isfinite(f0) && __builtin_isfinite(f1) && ((f0 < level) != (f1 < level));
}

// case byte of the cell whose lower corner is s, or -1 when the cell has a non-finite corner
__device__ __forceinline__ int cell_case(const float* __restrict__ vol, const McDims& d, uint32_t s, float level) {
    int c = 0;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float f = vol[(size_t)s + (i & 1) * d.nynz + ((i >> 1) & 1) * d.nz + (i >> 2)];
        ok = ok && __builtin_isfinite(f);
        c |= (f < level) << i;
    }
    return ok ? c : -1;
}

__device__ __forceinline__ uint32_t wave_excl_scan(uint32_t v, uint32_t& total) {
    const int lane = threadIdx.x & 63;
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    total = __shfl(x, 63, 64);
    return x - v;
}

__global__ __launch_bounds__(256) void k_mc_count(const float* __restrict__ vol, McDims d, float level, McWork w,
                                                  uint32_t n_chunks) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t wv = 0, wt = 0;
    for (uint32_t k = 0; k < kChunksPerBlock / 4; ++k) {
        const uint32_t c = blockIdx.x * kChunksPerBlock + k * 4 + wave;    // the 4 waves read 256 consecutive samples
        if (c >= n_chunks) break;
        const uint32_t s = c * 64 + lane;
        bool ex = false, ey = false, ez = false;
        uint32_t ntri = 0;
        if (s < d.N) {
            const uint32_t z = s % d.nz, r = s / d.nz, y = r % d.ny, x = r / d.ny;
            const float f0 = vol[s];
            ex = x + 1 < d.nx && crosses(f0, vol[(size_t)s + d.nynz], level);
            ey = y + 1 < d.ny && crosses(f0, vol[(size_t)s + d.nz], level);
            ez = z + 1 < d.nz && crosses(f0, vol[(size_t)s + 1], level);
            if (x + 1 < d.nx && y + 1 < d.ny && z + 1 < d.nz) {
                const int cs = cell_case(vol, d, s, level);
                ntri = cs < 0 ? 0u : nsa_mc_tri_count[cs];
            }
        }
        const uint64_t mx = __ballot(ex), my = __ballot(ey), mz = __ballot(ez);
        uint32_t tsum;
        (void)wave_excl_scan(ntri, tsum);
        const uint32_t vsum = __popcll(mx) + __popcll(my) + __popcll(mz);
        if (lane < 3) w.masks[(size_t)c * 3 + lane] = lane == 0 ? mx : (lane == 1 ? my : mz);
        if (lane == 0) w.cnt[c] = make_uint2(vsum, tsum);
        wv += vsum;
        wt += tsum;
    }
    __shared__ uint32_t red[2][4];
    if (lane == 0) {
        red[0][wave] = wv;
        red[1][wave] = wt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        w.bsum[blockIdx.x * 2] = (uint64_t)red[0][0] + red[0][1] + red[0][2] + red[0][3];
        w.bsum[blockIdx.x * 2 + 1] = (uint64_t)red[1][0] + red[1][1] + red[1][2] + red[1][3];
    }
}

// one workgroup: boff = the exclusive scan of the per-block (vertex, triangle) sums bsum (block_scan.hpp), and the two totals
__global__ __launch_bounds__(1024) void k_mc_scan(McWork w, uint32_t n_blocks, uint64_t* __restrict__ totals) {
    uint64_t total[2];
    scan::offsets<2, uint64_t, 1024>(w.bsum, w.boff, n_blocks, total);
    if (threadIdx.x == 0) {
        totals[0] = total[0];
        totals[1] = total[1];
    }
}

// id of the vertex on edge (owner sample o, axis a): chunk offset + the owner chunk's crossing edges before it
__device__ __forceinline__ uint32_t vertex_id(const McWork& w, uint32_t o, int a) {
    const uint32_t c = o >> 6, l = o & 63;
    const uint64_t mx = w.masks[(size_t)c * 3], my = w.masks[(size_t)c * 3 + 1], mz = w.masks[(size_t)c * 3 + 2];
    const uint64_t below = l ? (~0ull >> (64 - l)) : 0ull;
    uint32_t id = w.off[c].x + __popcll(mx & below) + __popcll(my & below) + __popcll(mz & below);
    if (a > 0) id += (mx >> l) & 1;
    if (a > 1) id += (my >> l) & 1;
    return id;
}

struct McGeom {
    float origin[3], spacing[3], spacing2[3];   // spacing2 = 2 * spacing
};

// volume gradient at sample (i[0], i[1], i[2]) = linear index s
__device__ void gradient(const float* __restrict__ vol, const McDims& d, const McGeom& g, const uint32_t (&i)[3], uint32_t s,
                         float (&out)[3]) {
#pragma clang fp contract(off)
    const uint32_t n[3] = {d.nx, d.ny, d.nz}, stride[3] = {d.nynz, d.nz, 1u};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const bool lo = i[k] == 0, hi = i[k] + 1 == n[k];
        const float fp = vol[(size_t)s + (hi ? 0u : stride[k])];
        const float fm = vol[(size_t)s - (lo ? 0u : stride[k])];
        out[k] = (fp - fm) / ((lo || hi) ? g.spacing[k] : g.spacing2[k]);
    }
}

__global__ __launch_bounds__(256) void k_mc_verts(const float* __restrict__ vol, McDims d, float level, McGeom g, McWork w,
                                                  uint32_t n_chunks, uint32_t n_verts, float* __restrict__ verts,
                                                  float* __restrict__ normals) {
#pragma clang fp contract(off)      // every product and sum below rounded on its own: tests/mc_ref.py restates it bit for bit
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ uint2 cnt[kChunksPerBlock];
    if (wave == 0) {              // per-chunk offsets of this block: block offset + exclusive scan over its 64 chunks
        const uint32_t c = blockIdx.x * kChunksPerBlock + lane;
        const uint2 n = c < n_chunks ? w.cnt[c] : make_uint2(0u, 0u);
        uint32_t tv, tt;
        const uint32_t ev = wave_excl_scan(n.x, tv), et = wave_excl_scan(n.y, tt);
        const uint2 o = make_uint2((uint32_t)w.boff[blockIdx.x * 2] + ev, (uint32_t)w.boff[blockIdx.x * 2 + 1] + et);
        if (c < n_chunks) w.off[c] = o;
        cnt[lane] = make_uint2(n.x, o.x);
    }
    __syncthreads();
    for (uint32_t k = 0; k < kChunksPerBlock / 4; ++k) {
        const uint32_t ci = k * 4 + wave, c = blockIdx.x * kChunksPerBlock + ci;
        if (c >= n_chunks) break;
        if (cnt[ci].x == 0) continue;
        const uint32_t s = c * 64 + lane;
        const uint64_t m[3] = {w.masks[(size_t)c * 3], w.masks[(size_t)c * 3 + 1], w.masks[(size_t)c * 3 + 2]};
        const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
        uint32_t id = cnt[ci].y + __popcll(m[0] & below) + __popcll(m[1] & below) + __popcll(m[2] & below);
        const uint32_t stride[3] = {d.nynz, d.nz, 1u};
        uint32_t i0[3];
        i0[2] = s % d.nz;
        i0[1] = (s / d.nz) % d.ny;
        i0[0] = s / d.nynz;
        for (int a = 0; a < 3; ++a) {
            if (!((m[a] >> lane) & 1)) continue;
            const uint32_t s1 = s + stride[a];
            const float f0 = vol[s], f1 = vol[s1];
            const float t = (level - f0) / (f1 - f0);
            uint32_t i1[3] = {i0[0], i0[1], i0[2]};
            i1[a] += 1;
            float g0[3], g1[3], mm[3], p[3];
            gradient(vol, d, g, i0, s, g0);
            gradient(vol, d, g, i1, s1, g1);
            const float u = 1.0f - t;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const float cq = a == q ? (float)i0[q] + t : (float)i0[q];
                p[q] = g.origin[q] + g.spacing[q] * cq;
                mm[q] = u * g0[q] + t * g1[q];
            }
            const float len = __fsqrt_rn((mm[0] * mm[0] + mm[1] * mm[1]) + mm[2] * mm[2]);
            const bool unit = len > 0.0f && __builtin_isfinite(len);
            if (id < n_verts) {
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    verts[(size_t)id * 3 + q] = p[q];
                    normals[(size_t)id * 3 + q] = unit ? mm[q] / len : 0.0f;
                }
            }
            ++id;
        }
    }
}

__global__ __launch_bounds__(256) void k_mc_faces(const float* __restrict__ vol, McDims d, float level, McWork w,
                                                  uint32_t n_chunks, uint32_t n_faces, int32_t* __restrict__ faces) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t k = 0; k < kChunksPerBlock / 4; ++k) {
        const uint32_t c = blockIdx.x * kChunksPerBlock + k * 4 + wave;
        if (c >= n_chunks) break;
        if (w.cnt[c].y == 0) continue;
        const uint32_t s = c * 64 + lane;
        int cs = -1;
        if (s < d.N) {
            const uint32_t z = s % d.nz, r = s / d.nz, y = r % d.ny, x = r / d.ny;
            if (x + 1 < d.nx && y + 1 < d.ny && z + 1 < d.nz) cs = cell_case(vol, d, s, level);
        }
        const uint32_t ntri = cs < 0 ? 0u : nsa_mc_tri_count[cs];
        uint32_t total;
        const uint32_t f0 = w.off[c].y + wave_excl_scan(ntri, total);
        for (uint32_t j = 0; j < ntri; ++j) {
            int32_t v[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int e = nsa_mc_tri_edges[cs][j * 3 + q], a = e >> 2, lo = e & 1, hi = (e >> 1) & 1;
                // offsets of the edge's start corner on the two other axes, in increasing axis order
                const uint32_t ox = a == 0 ? 0 : lo, oy = a == 0 ? lo : (a == 1 ? 0 : hi), oz = a == 2 ? 0 : hi;
                v[q] = (int32_t)vertex_id(w, s + ox * d.nynz + oy * d.nz + oz, a);
            }
            const uint32_t f = f0 + j;
            if (f < n_faces) {
#pragma unroll
                for (int q = 0; q < 3; ++q) faces[(size_t)f * 3 + q] = v[q];
            }
        }
    }
}

static bool dims_of(uint32_t nx, uint32_t ny, uint32_t nz, McDims* d, uint32_t* n_chunks, uint32_t* n_blocks) {
    const uint64_t N = (uint64_t)nx * ny * nz;
    if (N > kMaxSamples) return false;
    *d = McDims{nx, ny, nz, ny * nz, (uint32_t)N};
    *n_chunks = (uint32_t)((N + 63) / 64);
    *n_blocks = (uint32_t)((N + kSamplesPerBlock - 1) / kSamplesPerBlock);
    return true;
}

}  // namespace nsa

extern "C" {

uint64_t nsa_marching_cubes_workspace(uint32_t nx, uint32_t ny, uint32_t nz) {
    nsa::McDims d;
    uint32_t nc, nb;
    if (!nsa::dims_of(nx, ny, nz, &d, &nc, &nb)) return 0;
    return nsa::workspace_bytes(nc, nb);
}

int nsa_marching_cubes_count(const float* vol, uint32_t nx, uint32_t ny, uint32_t nz, float level, void* workspace,
                             uint64_t* totals, nsa_stream_t stream) {
    if (!vol || !workspace || !totals || !__builtin_isfinite(level)) return NSA_EBADARG;
    nsa::McDims d;
    uint32_t nc, nb;
    if (!nsa::dims_of(nx, ny, nz, &d, &nc, &nb)) return NSA_EBADARG;
    (void)hipGetLastError();
    if (nx < 2 || ny < 2 || nz < 2) {       // no cells, no edges with both ends inside the volume along every axis: empty
        if (hipMemsetAsync(totals, 0, 2 * sizeof(uint64_t), (hipStream_t)stream) != hipSuccess) return NSA_ELAUNCH;
        return NSA_OK;
    }
    const nsa::McWork w = nsa::carve(workspace, nc, nb);
    nsa::k_mc_count<<<nb, 256, 0, (hipStream_t)stream>>>(vol, d, level, w, nc);
    nsa::k_mc_scan<<<1, 1024, 0, (hipStream_t)stream>>>(w, nb, totals);
    return hipGetLastError() == hipSuccess ? NSA_OK : NSA_ELAUNCH;
}

int nsa_marching_cubes_emit(const float* vol, uint32_t nx, uint32_t ny, uint32_t nz, float level, const float* origin_host,
                            const float* spacing_host, void* workspace, uint64_t n_verts, uint64_t n_faces, float* verts,
                            float* normals, int32_t* faces, nsa_stream_t stream) {
    if (!vol || !workspace || !origin_host || !spacing_host || !__builtin_isfinite(level)) return NSA_EBADARG;
    nsa::McGeom g;
    for (int k = 0; k < 3; ++k) {
        if (!__builtin_isfinite(origin_host[k]) || !__builtin_isfinite(spacing_host[k]) || !(spacing_host[k] > 0.0f))
            return NSA_EBADARG;
        g.origin[k] = origin_host[k];
        g.spacing[k] = spacing_host[k];
        g.spacing2[k] = 2.0f * spacing_host[k];
    }
    if ((n_verts && (!verts || !normals)) || (n_faces && !faces)) return NSA_EBADARG;
    if (n_verts > INT32_MAX || n_faces > INT32_MAX) return NSA_EMESH_TOO_LARGE;
    nsa::McDims d;
    uint32_t nc, nb;
    if (!nsa::dims_of(nx, ny, nz, &d, &nc, &nb)) return NSA_EBADARG;
    if (nx < 2 || ny < 2 || nz < 2 || n_verts == 0) return NSA_OK;      // (a face needs vertices)
    const nsa::McWork w = nsa::carve(workspace, nc, nb);
    (void)hipGetLastError();
    nsa::k_mc_verts<<<nb, 256, 0, (hipStream_t)stream>>>(vol, d, level, g, w, nc, (uint32_t)n_verts, verts, normals);
    if (n_faces) nsa::k_mc_faces<<<nb, 256, 0, (hipStream_t)stream>>>(vol, d, level, w, nc, (uint32_t)n_faces, faces);
    return hipGetLastError() == hipSuccess ? NSA_OK : NSA_ELAUNCH;
}

}  // extern "C"
