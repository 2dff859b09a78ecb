// Host rehearsal of hole filling: the bodies of nicer_slam_amd/csrc/fill_passes.hpp -- the boundary test, the successor by rotation,
// the pinch mark, the rounds of pointer jumping and list ranking, the row of a loop and the faces and vertices of the patch --
// compiled as host C++ and called one item at a time, the way the kernels of csrc/mesh_fill.hip call them, on an edge table, a stable
// sort and scans made here with the standard library.  Built and run by tests/test_mesh_fill_host_cpu.py:
//     c++ -O2 -std=c++17 -ffp-contract=off [-fsanitize=address,undefined -fno-sanitize-recover=all] fill_host_check.cpp
//     ./a.out CASE > RESULT
// CASE (text): V F has_colors has_max_edges max_edges has_max_size max_size2_bits rings max_rings skip_folded / 3 V vertex words (fp32
// bits) / 3 F indices / 3 V colour words when has_colors.  RESULT: one line each of the totals, halfedges, next, flags, leader, rank,
// order, the loops' integers, the bits of their reals, the new vertices' and colours' fp32 bits and the new faces, which the test
// compares with tests/fill_ref.py element for element.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "../nicer_slam_amd/csrc/fill_passes.hpp"

using namespace nsa::fill;

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

struct Tables {
    std::vector<int32_t> edge_count, edge_forward, edge_start, edge_halfedges, face_edges;
    uint32_t E = 0;
};

// header Section 18, sequentially
static void build_tables(const std::vector<int32_t>& faces, uint32_t V, uint32_t F, Tables& t) {
    const uint32_t H = 3 * F;
    std::vector<std::pair<uint64_t, uint32_t>> keys;
    for (uint32_t f = 0; f < F; ++f) {
        const int32_t* v = &faces[3 * (size_t)f];
        if (v[0] < 0 || v[1] < 0 || v[2] < 0 || (uint32_t)v[0] >= V || (uint32_t)v[1] >= V || (uint32_t)v[2] >= V || v[0] == v[1] ||
            v[1] == v[2] || v[2] == v[0])
            continue;
        for (int k = 0; k < 3; ++k) {
            const uint64_t a = (uint64_t)v[k], b = (uint64_t)v[(k + 1) % 3];
            keys.push_back({(std::min(a, b) << 32) | std::max(a, b), 3 * f + (uint32_t)k});
        }
    }
    std::sort(keys.begin(), keys.end());
    t.edge_count.assign(H + 1, 0);
    t.edge_forward.assign(H + 1, 0);
    t.edge_start.assign(H + 2, 0);
    t.edge_halfedges.assign(H + 1, -1);
    t.face_edges.assign(H + 1, -1);
    uint32_t E = 0;
    for (size_t i = 0; i < keys.size(); ++i) {
        if (i == 0 || keys[i].first != keys[i - 1].first) t.edge_start[E++] = (int32_t)i;
        const uint32_t h = keys[i].second;
        ++t.edge_count[E - 1];
        t.edge_forward[E - 1] += faces[h] < faces[3 * (h / 3) + (h % 3 + 1) % 3];
        t.edge_halfedges[i] = (int32_t)h;
        t.face_edges[h] = (int32_t)(E - 1);
    }
    t.edge_start[E] = (int32_t)keys.size();
    t.E = E;
}

static uint32_t rounds_of(uint32_t B) {
    uint32_t r = 1, n = B < 2 ? 2 : B;
    while ((1ull << r) < n) ++r;
    return r + 1;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* fh = fopen(argv[1], "r");
    if (!fh) return 2;
    unsigned V, F, has_colors, has_max_edges, has_max_size, rings, max_rings, skip_folded;
    unsigned long long max_edges, ms2_bits;
    if (fscanf(fh, "%u %u %u %u %llu %u %llu %u %u %u", &V, &F, &has_colors, &has_max_edges, &max_edges, &has_max_size, &ms2_bits, &rings,
               &max_rings, &skip_folded) != 10)
        return 2;
    std::vector<unsigned> vbits(3 * (size_t)V), cbits(has_colors ? 3 * (size_t)V : 0);
    std::vector<int32_t> faces(3 * (size_t)F);
    if (!read_all(fh, "%u", vbits) || !read_all(fh, "%d", faces) || !read_all(fh, "%u", cbits)) return 2;
    fclose(fh);
    std::vector<float> verts(vbits.size() + 1), colors(cbits.size() + 1);
    if (!vbits.empty()) memcpy(verts.data(), vbits.data(), 4 * vbits.size());
    if (!cbits.empty()) memcpy(colors.data(), cbits.data(), 4 * cbits.size());
    double ms2;
    memcpy(&ms2, &ms2_bits, 8);
    const uint32_t H = 3 * F;

    Tables tb;
    build_tables(faces, V, F, tb);
    faces.push_back(-1);
    const Topo t{faces.data(), tb.face_edges.data(), tb.edge_count.data(), tb.edge_forward.data(), tb.edge_start.data(),
                 tb.edge_halfedges.data(), V, F, tb.E};
    const Shape m{verts.data(), has_colors ? colors.data() : nullptr, faces.data(), V, F};
    const Limits lim{has_max_edges != 0, max_edges, has_max_size != 0, ms2, rings, max_rings, skip_folded != 0};

    // the items: an exclusive scan of the boundary flags
    std::vector<int32_t> hslot(H + 1, -1);
    std::vector<uint32_t> bh;
    for (uint32_t h = 0; h < H; ++h)
        if (boundary_halfedge(t, h)) {
            hslot[h] = (int32_t)bh.size();
            bh.push_back(h);
        }
    const uint32_t B = (uint32_t)bh.size();
    bh.push_back(kNone);
    std::vector<uint32_t> next(B + 1), a[2], b[2], leader(B + 1), item_start(B + 1), order_item(B + 1, kNone), sorder(B + 1);
    std::vector<uint8_t> tm[2], blk(B + 1), pinch(B + 1);
    for (int k = 0; k < 2; ++k) {
        a[k].assign(B + 1, 0);
        b[k].assign(B + 1, 0);
        tm[k].assign(B + 1, 0);
    }
    for (uint32_t i = 0; i < B; ++i) {
        blk[i] = next_pass(t, bh.data(), hslot.data(), B, i, next.data());
        a[0][i] = i;
        b[0][i] = next[i];
        tm[0][i] = blk[i] & kBlocked;
    }
    std::iota(sorder.begin(), sorder.begin() + B, 0u);
    std::stable_sort(sorder.begin(), sorder.begin() + B,
                     [&](uint32_t x, uint32_t y) { return start_key(t, bh.data(), B, x) < start_key(t, bh.data(), B, y); });
    for (uint32_t p = 0; p < B; ++p) pinch_pass(t, bh.data(), sorder.data(), B, p, pinch.data());
    const uint32_t R = rounds_of(B);
    int cur = 0;
    for (uint32_t r = 0; r < R; ++r, cur ^= 1)
        for (uint32_t i = 0; i < B; ++i)
            jump_pass(a[cur].data(), b[cur].data(), tm[cur].data(), B, i, a[cur ^ 1].data(), b[cur ^ 1].data(), tm[cur ^ 1].data());
    const int term = cur;
    for (uint32_t i = 0; i < B; ++i)
        rank_init_pass(a[cur].data(), tm[cur].data(), next.data(), B, i, leader.data(), a[cur ^ 1].data(), b[cur ^ 1].data());
    cur ^= 1;
    for (uint32_t r = 0; r < R; ++r, cur ^= 1)
        for (uint32_t i = 0; i < B; ++i) rank_pass(a[cur].data(), b[cur].data(), B, i, a[cur ^ 1].data(), b[cur ^ 1].data());
    const std::vector<uint32_t>& dist = a[cur];

    // the loops: an exclusive scan of (leader, length) over the items
    std::vector<long long> ints((size_t)kLoopInts * B + 1, 0);
    std::vector<double> reals((size_t)kLoopReals * B + 1, 0.0);
    unsigned long long L = 0, at = 0, open = 0, cap = 0;
    for (uint32_t i = 0; i < B; ++i) {
        item_start[i] = (uint32_t)at;
        open += tm[term][i] != 0;
        cap += (blk[i] & kCapHit) != 0;
        if (!is_leader(leader.data(), i)) continue;
        long long* row = &ints[(size_t)kLoopInts * L];
        row[0] = bh[i];
        row[1] = (long long)dist[i] + 1;
        row[2] = (long long)at;
        at += dist[i] + 1;
        ++L;
    }
    std::vector<int32_t> rank(B + 1), order(B + 1, -1), lead_out(B + 1);
    std::vector<unsigned> flags(B + 1);
    for (uint32_t i = 0; i < B; ++i) {
        order_pass(bh.data(), leader.data(), dist.data(), item_start.data(), B, i, rank.data(), order_item.data(), order.data());
        lead_out[i] = leader[i] < B ? (int32_t)leader[i] : -1;
        flags[i] = (unsigned)((blk[i] & (kBlocked | kCapHit)) | pinch[i] | (tm[term][i] ? kOpenChain : 0));
    }
    static_assert(sizeof(long long) == sizeof(int64_t), "int64");
    int64_t* ip = reinterpret_cast<int64_t*>(ints.data());
    for (uint32_t l = 0; l < L; ++l) loop_pass(m, bh.data(), order_item.data(), pinch.data(), B, lim, l, ip, reals.data());
    unsigned long long nv = 0, nf = 0, cls[kClasses] = {0, 0, 0, 0, 0, 0};
    for (uint32_t l = 0; l < L; ++l) {
        long long* row = &ints[(size_t)kLoopInts * l];
        row[7] = (long long)nv;
        row[8] = (long long)nf;
        nv += (unsigned long long)row[5];
        nf += (unsigned long long)row[6];
        if (row[3] >= 0 && row[3] < kClasses) ++cls[row[3]];
    }
    const unsigned long long totals[kTotals] = {B, L, cls[0], cls[1], cls[2], cls[3], cls[4], cls[5], open, nv, nf, cap ? 1ull : 0ull};

    std::vector<float> new_verts(3 * (size_t)nv + 1), new_colors(3 * (size_t)nv + 1);
    std::vector<int32_t> new_faces(3 * (size_t)nf + 1);
    for (unsigned long long x = 0; x < nf; ++x)
        emit_pass(m, order.data(), B, ip, reals.data(), (uint32_t)L, nv, nf, x, new_verts.data(), has_colors ? new_colors.data() : nullptr,
                  new_faces.data());

    print_line("%llu ", totals, (size_t)kTotals);
    print_line("%u ", bh.data(), (size_t)B);
    print_line("%u ", next.data(), (size_t)B);
    print_line("%u ", flags.data(), (size_t)B);
    print_line("%d ", lead_out.data(), (size_t)B);
    print_line("%d ", rank.data(), (size_t)B);
    print_line("%d ", order.data(), (size_t)(B - open));
    print_line("%lld ", ints.data(), (size_t)kLoopInts * L);
    std::vector<unsigned long long> rb((size_t)kLoopReals * L);
    if (!rb.empty()) memcpy(rb.data(), reals.data(), 8 * rb.size());
    print_line("%llu ", rb.data(), rb.size());
    std::vector<unsigned> vb(3 * (size_t)nv), cb(has_colors ? 3 * (size_t)nv : 0);
    if (!vb.empty()) memcpy(vb.data(), new_verts.data(), 4 * vb.size());
    if (!cb.empty()) memcpy(cb.data(), new_colors.data(), 4 * cb.size());
    print_line("%u ", vb.data(), vb.size());
    print_line("%u ", cb.data(), cb.size());
    print_line("%d ", new_faces.data(), 3 * (size_t)nf);
    return 0;
}
