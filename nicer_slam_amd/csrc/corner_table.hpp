// corner_table.hpp -- the corners 3 g + k of a face list grouped by vertex: the 3 F corners keyed by a vertex name (V for a corner
// that takes no part), the stable radix argsort of radix_sort.hpp -- corners in index order, so ascending within a vertex -- and the
// start offsets by binary search.  No atomic takes part.  Shared by the adjacency of the signed distance (mesh_sdf.hip, DESIGN 4n,
// keyed by the adjacency faces of usable faces) and the vertex normals (mesh_smooth.hip, DESIGN 4t, keyed by the faces themselves);
// the unit supplies the key as a functor  uint32_t operator()(uint32_t corner) const  that returns a value in [0, V].
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "bulk_grid.hpp"
#include "radix_sort.hpp"

namespace nsa {
namespace corners {

struct Table {                   // views into the caller's buffer (carve() bytes)
    uint32_t* start;             // [V + 2]: first sorted position of key i; key V = the corners that take no part
    uint32_t* corner;            // [3 F]: corners 3 g + k sorted by key, ascending within a key
    uint32_t* skey;              // [3 F]: sorted keys
    uint32_t* keys[2];           // [3 F] each: radix ping-pong
    uint32_t* tmp;               // [3 F]
    uint32_t* counts;            // [256 * 256]
};

__host__ __device__ inline uint64_t carve(void* ws, uint32_t V, uint32_t F, Table* out) {
    char* base = static_cast<char*>(ws);
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) { char* p = base ? base + o : nullptr; o += bulk::up256(bytes); return p; };
    Table x;
    x.start = reinterpret_cast<uint32_t*>(take(4ull * ((uint64_t)V + 2)));
    x.corner = reinterpret_cast<uint32_t*>(take(12ull * F));
    x.skey = reinterpret_cast<uint32_t*>(take(12ull * F));
    x.keys[0] = reinterpret_cast<uint32_t*>(take(12ull * F));
    x.keys[1] = reinterpret_cast<uint32_t*>(take(12ull * F));
    x.tmp = reinterpret_cast<uint32_t*>(take(12ull * F));
    x.counts = reinterpret_cast<uint32_t*>(take(4ull * kRadixCountWords));
    if (out) *out = x;
    return o;
}

template <typename Key>
__global__ __launch_bounds__(256) void k_keys(Key key, uint32_t n_corners, Table t) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_corners) return;
    t.keys[0][i] = key(i);
}

template <typename Key>
__global__ __launch_bounds__(256) void k_gather(Key key, uint32_t n_corners, Table t) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_corners) return;
    t.skey[i] = key(t.corner[i]);
}

// one lane per key i in [0, V + 1]
template <typename Key>
__global__ __launch_bounds__(256) void k_start(uint32_t V, uint32_t n_corners, Table t) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i > V + 1) return;
    t.start[i] = bulk::lower_bound(t.skey, n_corners, i);
}

// the four steps on `stream`, between the caller's launch_begin() and launch_end().  V >= 1, 1 <= 3 F < 2^31
template <typename Key>
inline void build(Key key, uint32_t V, uint32_t F, const Table& t, nsa_stream_t stream) {
    const uint32_t P = 3 * F, nb = (P + 255) / 256;
    uint32_t bits = 1;
    while ((1ull << bits) <= (uint64_t)V) ++bits;                          // keys are <= V
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_keys<Key>, dim3(nb), dim3(256), 0, s, key, P, t);
    radix_argsort(t.keys, t.tmp, t.corner, t.counts, P, 0, (bits + 7) / 8, stream);
    hipLaunchKernelGGL(k_gather<Key>, dim3(nb), dim3(256), 0, s, key, P, t);
    hipLaunchKernelGGL(k_start<Key>, dim3((V + 2 + 255) / 256), dim3(256), 0, s, V, P, t);
}

}  // namespace corners
}  // namespace nsa
