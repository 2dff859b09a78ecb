// Host rehearsal of mesh smoothing: the bodies of nicer_slam_amd/csrc/smooth_passes.hpp -- the ring's offsets, fill and row lookup, the
// state and neighbour passes, one vertex's step, one vertex's area normal -- compiled as host C++ and called one item at a time, the
// way the kernels of csrc/mesh_smooth.hip call them, on an edge table and two stable sorts made here with the standard library.
// Built and run by tests/test_mesh_smooth_host_cpu.py:
//     c++ -O2 -std=c++17 -ffp-contract=off [-fsanitize=address,undefined -fno-sanitize-recover=all] smooth_host_check.cpp
//     ./a.out CASE > RESULT
// CASE (text): V F n_steps boundary clamp max_move_bits / 3 V vertex words (fp32 bits) / 3 F indices / V fixed flags / n_steps factor
// words (float64 bits).  RESULT: one line each of ring_start, ring, ring_edge, the output's fp32 bits, the state bytes and the area
// normals' fp32 bits, which the test compares with tests/smooth_ref.py element for element.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "../nicer_slam_amd/csrc/smooth_passes.hpp"

using namespace nsa::smooth;

template <typename T>
static bool read_all(FILE* fh, const char* fmt, std::vector<T>& out) {
    for (auto& x : out)
        if (fscanf(fh, fmt, &x) != 1) return false;
    return true;
}

template <typename T>
static void print_line(const char* fmt, const T* p, size_t n) {
    for (size_t i = 0; i < n; ++i) printf(fmt, p[i]);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* fh = fopen(argv[1], "r");
    if (!fh) return 2;
    unsigned V, F, n_steps, clamp;
    int boundary;
    unsigned long long mm_bits;
    if (fscanf(fh, "%u %u %u %d %u %llu", &V, &F, &n_steps, &boundary, &clamp, &mm_bits) != 6) return 2;
    std::vector<unsigned> vbits(3 * (size_t)V), fixed_in(V);
    std::vector<int> faces(3 * (size_t)F);
    std::vector<unsigned long long> fbits(n_steps);
    if (!read_all(fh, "%u", vbits) || !read_all(fh, "%d", faces) || !read_all(fh, "%u", fixed_in) || !read_all(fh, "%llu", fbits)) return 2;
    fclose(fh);
    std::vector<float> verts(vbits.size());
    if (!verts.empty()) memcpy(verts.data(), vbits.data(), 4 * vbits.size());
    std::vector<double> factors(n_steps);
    if (n_steps) memcpy(factors.data(), fbits.data(), 8 * (size_t)n_steps);
    double max_move;
    memcpy(&max_move, &mm_bits, 8);
    std::vector<uint8_t> fixed(V);
    for (unsigned v = 0; v < V; ++v) fixed[v] = (uint8_t)(fixed_in[v] != 0);

    // header Section 18, sequentially: the distinct edges in (lo, hi) order and the half-edges on each
    const uint32_t H = 3 * F, cap = 6 * F;
    std::vector<uint64_t> keys;
    for (uint32_t f = 0; f < F; ++f) {
        const int32_t* v = &faces[3 * (size_t)f];
        if (v[0] < 0 || v[1] < 0 || v[2] < 0 || (uint32_t)v[0] >= V || (uint32_t)v[1] >= V || (uint32_t)v[2] >= V || v[0] == v[1] ||
            v[1] == v[2] || v[2] == v[0])
            continue;
        for (int k = 0; k < 3; ++k) {
            const uint64_t a = (uint64_t)v[k], b = (uint64_t)v[(k + 1) % 3];
            keys.push_back((std::min(a, b) << 32) | std::max(a, b));
        }
    }
    std::sort(keys.begin(), keys.end());
    std::vector<int32_t> edges(2 * (size_t)H + 2, -1), edge_count(H + 1, 0);
    uint32_t E = 0;
    for (size_t i = 0; i < keys.size(); ++i) {
        if (i == 0 || keys[i] != keys[i - 1]) {
            edges[2 * (size_t)E] = (int32_t)(keys[i] >> 32);
            edges[2 * (size_t)E + 1] = (int32_t)(keys[i] & 0xFFFFFFFFu);
            ++E;
        }
        ++edge_count[E - 1];
    }

    // the ring: keys, the stable sort by hi (the device's radix argsort), offsets, fill
    std::vector<uint32_t> lo(H), hi(H), order(H), hs(H);
    for (uint32_t i = 0; i < H; ++i) {
        lo[i] = ring_key(edges.data(), E, V, i, 0);
        hi[i] = ring_key(edges.data(), E, V, i, 1);
    }
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return hi[a] < hi[b]; });
    for (uint32_t i = 0; i < H; ++i) hs[i] = hi[order[i]];
    std::vector<int32_t> below_lo((size_t)V + 1), below_hi((size_t)V + 1), ring_start((size_t)V + 1), ring(cap, -7), ring_edge(cap, -7);
    for (uint32_t v = 0; v <= V; ++v) ring_pass_start(lo.data(), hs.data(), H, v, below_lo.data(), below_hi.data(), ring_start.data());
    for (uint32_t i = 0; i < H; ++i)
        ring_pass_fill(edges.data(), E, hs.data(), order.data(), below_lo.data(), below_hi.data(), H, V, cap, i, ring.data(), ring_edge.data());
    if (ring_start[V] != (int32_t)(2 * E)) return 3;
    print_line("%d ", ring_start.data(), ring_start.size());
    print_line("%d ", ring.data(), 2 * (size_t)E);
    print_line("%d ", ring_edge.data(), 2 * (size_t)E);

    // smoothing: state, neighbour lists, the steps over ping-pong positions, the final rounding
    std::vector<double> pos[2] = {std::vector<double>(3 * (size_t)V), std::vector<double>(3 * (size_t)V)};
    std::vector<int32_t> member(cap), count(V);
    std::vector<uint8_t> state(V), state_out(V);
    for (uint32_t v = 0; v < V; ++v)
        state[v] = smooth_pass_state(verts.data(), ring_start.data(), ring_edge.data(), edge_count.data(), fixed.data(), V, cap, H, boundary, v,
                                     pos[0].data());
    for (uint32_t v = 0; v < V; ++v)
        state_out[v] = smooth_pass_members(ring_start.data(), ring.data(), ring_edge.data(), edge_count.data(), state.data(), V, cap, H, boundary,
                                           v, member.data(), count.data());
    std::vector<unsigned> out(vbits);
    for (unsigned i = 0; i < n_steps; ++i) {
        const int from = (int)(i & 1u);
        for (uint32_t v = 0; v < V; ++v) {
            double y[3];
            const bool stepped = smooth_pass_step(pos[from].data(), verts.data(), ring_start.data(), member.data(), count.data(), V, cap, v,
                                                  factors[i], max_move, clamp != 0, y);
            for (int k = 0; k < 3; ++k) {
                pos[from ^ 1][3 * (size_t)v + k] = y[k];
                if (i + 1 == n_steps && stepped) {
                    const float r = (float)y[k];
                    memcpy(&out[3 * (size_t)v + k], &r, 4);
                }
            }
        }
    }
    print_line("%u ", out.data(), out.size());
    std::vector<unsigned> st(state_out.begin(), state_out.end());
    print_line("%u ", st.data(), st.size());

    // area normals over the corner-by-vertex order (the device's stable radix argsort of the corner keys)
    std::vector<uint32_t> ckey(H), corner(H), start((size_t)V + 2);
    for (uint32_t c = 0; c < H; ++c) ckey[c] = normal_corner_key(verts.data(), V, faces.data(), F, c);
    std::iota(corner.begin(), corner.end(), 0u);
    std::stable_sort(corner.begin(), corner.end(), [&](uint32_t a, uint32_t b) { return ckey[a] < ckey[b]; });
    std::vector<uint32_t> skey(H);
    for (uint32_t i = 0; i < H; ++i) skey[i] = ckey[corner[i]];
    for (uint32_t v = 0; v <= V + 1; ++v) start[v] = nsa::bulk::lower_bound(skey.data(), H, v);
    std::vector<unsigned> nbits(3 * (size_t)V);
    for (uint32_t v = 0; v < V; ++v) {
        float n[3];
        normal_pass_vertex(verts.data(), V, faces.data(), F, corner.data(), start[v], start[v + 1], kArea, n);
        memcpy(&nbits[3 * (size_t)v], n, 12);
    }
    print_line("%u ", nbits.data(), nbits.size());
    return 0;
}
