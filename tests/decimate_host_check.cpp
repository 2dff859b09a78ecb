// Host rehearsal of mesh decimation: the bodies of nicer_slam_amd/csrc/decimate_passes.hpp -- the quadric sums and locks, one edge's
// placement, cost, link count and fold test, m1 / m2 / select, the prefix rule, apply, rename and compose -- compiled as host C++ and
// called one item at a time, the way the kernels of csrc/mesh_decimate.hip call them, on an edge table, rings and stable sorts made
// here with the standard library.  Built and run by tests/test_mesh_decimate_host_cpu.py:
//     c++ -O2 -std=c++17 -ffp-contract=off [-fsanitize=address,undefined -fno-sanitize-recover=all] decimate_host_check.cpp
//     ./a.out CASE > RESULT
// CASE (text): V F has_target target has_limit max_error2_bits min_cos2_bits eps_bits boundary weight_bits max_rounds has_colors /
// 3 V vertex words (fp32 bits) / 3 F indices / V fixed flags / 3 V colour words when has_colors.  RESULT: one line each of the totals
// (rounds, collapses, the last round's candidates, four rejections and selected), the log, the working faces, vertex_map, the
// output's fp32 bits, the colours' fp32 bits, the lock bytes and the initial quadrics' float64 bits, which the test compares with
// tests/decimate_ref.py element for element.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "../nicer_slam_amd/csrc/decimate_passes.hpp"

using namespace nsa::decimate;

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

static double from_bits(unsigned long long b) {
    double x;
    memcpy(&x, &b, 8);
    return x;
}

struct Tables {
    std::vector<int32_t> edges, edge_count, edge_start, edge_halfedges, ring_start, ring, ring_edge;
    uint32_t E = 0, Fc = 0;
};

// header Sections 18 and 21, sequentially
static void build_tables(const std::vector<int32_t>& faces, uint32_t V, uint32_t F, Tables& t) {
    const uint32_t H = 3 * F, cap = 6 * F;
    std::vector<std::pair<uint64_t, uint32_t>> keys;
    t.Fc = 0;
    for (uint32_t f = 0; f < F; ++f) {
        const int32_t* v = &faces[3 * (size_t)f];
        if (v[0] < 0 || v[1] < 0 || v[2] < 0 || (uint32_t)v[0] >= V || (uint32_t)v[1] >= V || (uint32_t)v[2] >= V || v[0] == v[1] ||
            v[1] == v[2] || v[2] == v[0])
            continue;
        ++t.Fc;
        for (int k = 0; k < 3; ++k) {
            const uint64_t a = (uint64_t)v[k], b = (uint64_t)v[(k + 1) % 3];
            keys.push_back({(std::min(a, b) << 32) | std::max(a, b), 3 * f + (uint32_t)k});
        }
    }
    std::sort(keys.begin(), keys.end());
    t.edges.assign(2 * (size_t)H + 2, -1);
    t.edge_count.assign(H + 1, 0);
    t.edge_start.assign(H + 2, 0);
    t.edge_halfedges.assign(H + 1, -1);
    uint32_t E = 0;
    for (size_t i = 0; i < keys.size(); ++i) {
        if (i == 0 || keys[i].first != keys[i - 1].first) {
            t.edges[2 * (size_t)E] = (int32_t)(keys[i].first >> 32);
            t.edges[2 * (size_t)E + 1] = (int32_t)(keys[i].first & 0xFFFFFFFFu);
            t.edge_start[E] = (int32_t)i;
            ++E;
        }
        ++t.edge_count[E - 1];
        t.edge_halfedges[i] = (int32_t)keys[i].second;
    }
    t.edge_start[E] = (int32_t)keys.size();
    t.E = E;
    std::vector<uint32_t> lo(H), hi(H), order(H), hs(H);
    for (uint32_t i = 0; i < H; ++i) {
        lo[i] = nsa::smooth::ring_key(t.edges.data(), E, V, i, 0);
        hi[i] = nsa::smooth::ring_key(t.edges.data(), E, V, i, 1);
    }
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return hi[a] < hi[b]; });
    for (uint32_t i = 0; i < H; ++i) hs[i] = hi[order[i]];
    std::vector<int32_t> below_lo((size_t)V + 1), below_hi((size_t)V + 1);
    t.ring_start.assign((size_t)V + 1, 0);
    t.ring.assign(cap + 1, -7);
    t.ring_edge.assign(cap + 1, -7);
    for (uint32_t v = 0; v <= V; ++v)
        nsa::smooth::ring_pass_start(lo.data(), hs.data(), H, v, below_lo.data(), below_hi.data(), t.ring_start.data());
    for (uint32_t i = 0; i < H; ++i)
        nsa::smooth::ring_pass_fill(t.edges.data(), E, hs.data(), order.data(), below_lo.data(), below_hi.data(), H, V, cap, i,
                                    t.ring.data(), t.ring_edge.data());
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* fh = fopen(argv[1], "r");
    if (!fh) return 2;
    unsigned V, F, has_target, has_limit, max_rounds, has_colors;
    int boundary;
    unsigned long long target, me2_bits, mc2_bits, eps_bits, bw_bits;
    if (fscanf(fh, "%u %u %u %llu %u %llu %llu %llu %d %llu %u %u", &V, &F, &has_target, &target, &has_limit, &me2_bits, &mc2_bits,
               &eps_bits, &boundary, &bw_bits, &max_rounds, &has_colors) != 12)
        return 2;
    std::vector<unsigned> vbits(3 * (size_t)V), fixed_in(V), cbits(has_colors ? 3 * (size_t)V : 0);
    std::vector<int32_t> faces(3 * (size_t)F);
    if (!read_all(fh, "%u", vbits) || !read_all(fh, "%d", faces) || !read_all(fh, "%u", fixed_in) || !read_all(fh, "%u", cbits)) return 2;
    fclose(fh);
    std::vector<float> verts(vbits.size() + 1), colors(cbits.size() + 1);
    if (!vbits.empty()) memcpy(verts.data(), vbits.data(), 4 * vbits.size());
    if (!cbits.empty()) memcpy(colors.data(), cbits.data(), 4 * cbits.size());
    std::vector<uint8_t> fixed(V + 1);
    for (unsigned v = 0; v < V; ++v) fixed[v] = (uint8_t)(fixed_in[v] != 0);
    const double me2 = from_bits(me2_bits), mc2 = from_bits(mc2_bits), eps = from_bits(eps_bits), bw = from_bits(bw_bits);
    const uint32_t H = 3 * F;

    // the state
    std::vector<double> pos(3 * (size_t)V + 1), quad((size_t)kQ * V + 1), col(3 * (size_t)V + 1);
    std::vector<int32_t> vmap(V + 1);
    std::vector<uint8_t> locked(V + 1), moved(V + 1);
    Tables t;
    build_tables(faces, V, F, t);
    for (uint32_t v = 0; v < V; ++v)
        init_pass_position(verts.data(), has_colors ? colors.data() : nullptr, v, pos.data(), col.data(), vmap.data(), moved.data());
    {   // the corner-by-vertex order (the device's stable radix argsort of the corner keys)
        std::vector<uint32_t> ckey(H), corner(H), skey(H), start((size_t)V + 2);
        for (uint32_t c = 0; c < H; ++c) ckey[c] = nsa::smooth::normal_corner_key(verts.data(), V, faces.data(), F, c);
        std::iota(corner.begin(), corner.end(), 0u);
        std::stable_sort(corner.begin(), corner.end(), [&](uint32_t a, uint32_t b) { return ckey[a] < ckey[b]; });
        for (uint32_t i = 0; i < H; ++i) skey[i] = ckey[corner[i]];
        for (uint32_t v = 0; v <= V + 1; ++v) start[v] = nsa::bulk::lower_bound(skey.data(), H, v);
        for (uint32_t v = 0; v < V; ++v)
            init_pass_vertex(pos.data(), V, faces.data(), F, corner.data(), start[v], start[v + 1], t.ring_start.data(), t.ring.data(),
                             t.ring_edge.data(), t.edge_count.data(), t.edge_start.data(), t.edge_halfedges.data(), fixed.data(), boundary,
                             bw, v, locked.data(), quad.data());
    }
    std::vector<unsigned long long> quad0((size_t)kQ * V);
    if (V) memcpy(quad0.data(), quad.data(), 8 * quad0.size());

    // the rounds, as the driver of nicer_slam_amd/mesh_decimate.py runs them
    std::vector<unsigned long long> log;
    unsigned long long last[6] = {0, 0, 0, 0, 0, 0};
    uint64_t n_faces = t.Fc;
    unsigned rounds = 0;
    std::vector<uint64_t> cost_bits(H + 1), skey(H + 1), m1c(V + 1), m1w(V + 1);
    std::vector<double> place(3 * (size_t)H + 1);
    std::vector<uint8_t> code(H + 1);
    std::vector<uint32_t> m1e(V + 1), m2e(V + 1), sorted(H + 1);
    while (rounds < max_rounds && n_faces > 0 && V > 0) {
        if (has_target && n_faces <= target) break;
        if (rounds) build_tables(faces, V, F, t);
        EdgeTables et{faces.data(), t.edges.data(), t.edge_count.data(), t.edge_start.data(), t.edge_halfedges.data(), t.ring_start.data(),
                      t.ring.data(), t.ring_edge.data(), pos.data(), quad.data(), locked.data(), V, F, t.E};
        for (uint32_t i = 0; i < H; ++i) code[i] = edge_pass(et, i, eps, has_limit != 0, me2, mc2, cost_bits.data(), place.data());
        for (uint32_t v = 0; v < V; ++v)
            min1_pass(t.ring_start.data(), t.ring_edge.data(), t.edges.data(), code.data(), cost_bits.data(), V, F, v, m1c.data(),
                      m1w.data(), m1e.data());
        for (uint32_t v = 0; v < V; ++v)
            min2_pass(t.ring_start.data(), t.ring.data(), m1c.data(), m1w.data(), m1e.data(), V, F, v, m2e.data());
        for (uint32_t i = 0; i < H; ++i) skey[i] = select_pass(t.edges.data(), code.data(), cost_bits.data(), m2e.data(), V, i);
        std::iota(sorted.begin(), sorted.begin() + H, 0u);
        for (int k = 0; k < 4; ++k)                                       // the device's four stable argsorts, least significant word first
            std::stable_sort(sorted.begin(), sorted.begin() + H, [&](uint32_t a, uint32_t b) {
                return sort_word(t.edges.data(), skey.data(), a, k) < sort_word(t.edges.data(), skey.data(), b, k);
            });
        unsigned long long cnt[6] = {0, 0, 0, 0, 0, 0};
        for (uint32_t i = 0; i < H; ++i) {
            if (code[i] < 5) ++cnt[code[i]];
            cnt[5] += skey[i] != kNoKey;
        }
        uint64_t before = 0, n_take = 0;
        for (uint32_t p = 0; p < cnt[5]; ++p) {
            const uint32_t i = sorted[p];
            if (!prefix_take(has_target != 0, n_faces, before, target)) break;
            uint32_t lo, hi;
            apply_pass(t.edges.data(), place.data(), V, i, pos.data(), quad.data(), has_colors ? col.data() : nullptr, vmap.data(),
                       moved.data(), &lo, &hi);
            const unsigned long long row[4] = {rounds, lo, hi, cost_bits[i]};
            log.insert(log.end(), row, row + 4);
            before += (uint64_t)t.edge_count[i];
            ++n_take;
        }
        for (uint64_t c = 0; c < H; ++c) rename_pass(vmap.data(), V, c, faces.data());
        for (uint32_t v = 0; v < V; ++v) compose_pass(V, v, vmap.data());
        ++rounds;
        n_faces -= before;
        for (int k = 0; k < 6; ++k) last[k] = cnt[k];
        if (n_take == 0) break;
    }
    const unsigned long long totals[8] = {rounds, log.size() / 4, last[0], last[1], last[2], last[3], last[4], last[5]};
    print_line("%llu ", totals, 8);
    print_line("%llu ", log.data(), log.size());
    print_line("%d ", faces.data(), faces.size());
    print_line("%d ", vmap.data(), (size_t)V);
    std::vector<unsigned> out(vbits), cout_(cbits);
    for (uint32_t v = 0; v < V; ++v)
        for (int k = 0; k < 3 && moved[v]; ++k) {
            const float r = (float)pos[3 * (size_t)v + k];
            memcpy(&out[3 * (size_t)v + k], &r, 4);
            if (has_colors) {
                const float c = (float)col[3 * (size_t)v + k];
                memcpy(&cout_[3 * (size_t)v + k], &c, 4);
            }
        }
    print_line("%u ", out.data(), out.size());
    print_line("%u ", cout_.data(), cout_.size());
    std::vector<unsigned> lk(locked.begin(), locked.begin() + V);
    print_line("%u ", lk.data(), lk.size());
    print_line("%llu ", quad0.data(), quad0.size());
    return 0;
}
