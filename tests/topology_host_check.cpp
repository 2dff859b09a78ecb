// Host rehearsal of the union-find passes of the mesh topology: the pass bodies of nicer_slam_amd/csrc/topo_passes.hpp, compiled as host
// C++ and run by many threads on an edge table built here with std::sort, against a sequential union-find (smaller root wins).
// Built and run by tests/test_mesh_topology_cpu.py:   c++ -O2 -std=c++17 -pthread [-fsanitize=thread] topology_host_check.cpp && ./a.out
// [threads] [n].  Prints one line per case; exit status 1 on any mismatch or tripped step cap.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../nicer_slam_amd/csrc/topo_passes.hpp"

struct Case {
    std::string name;
    uint32_t V;
    std::vector<int32_t> faces;
};

struct Table {                   // header Section 18, built sequentially
    std::vector<int32_t> edges, count, start, halfedges, face_edges;
    uint32_t E = 0;
};

static Table build(const Case& c) {
    const uint32_t F = (uint32_t)(c.faces.size() / 3), H = 3 * F;
    Table t;
    t.face_edges.assign(H, -1);
    t.halfedges.assign(H, -1);
    std::vector<std::pair<uint64_t, int32_t>> keys;
    for (uint32_t f = 0; f < F; ++f) {
        const int32_t* v = &c.faces[3 * f];
        const bool ok = v[0] >= 0 && v[1] >= 0 && v[2] >= 0 && (uint32_t)v[0] < c.V && (uint32_t)v[1] < c.V && (uint32_t)v[2] < c.V &&
                        v[0] != v[1] && v[1] != v[2] && v[2] != v[0];
        if (!ok) continue;
        for (int k = 0; k < 3; ++k) {
            const uint64_t a = (uint64_t)v[k], b = (uint64_t)v[(k + 1) % 3];
            keys.push_back({(std::min(a, b) << 32) | std::max(a, b), (int32_t)(3 * f + k)});
        }
    }
    std::sort(keys.begin(), keys.end());
    t.edges.assign(2 * (size_t)H, 0);
    t.count.assign(H, 0);
    t.start.assign((size_t)H + 1, 0);
    for (size_t i = 0; i < keys.size(); ++i) {
        if (i == 0 || keys[i].first != keys[i - 1].first) {
            t.edges[2 * t.E] = (int32_t)(keys[i].first >> 32);
            t.edges[2 * t.E + 1] = (int32_t)(keys[i].first & 0xFFFFFFFFu);
            t.start[t.E++] = (int32_t)i;
        }
        t.count[t.E - 1]++;
        t.halfedges[i] = keys[i].second;
        t.face_edges[keys[i].second] = (int32_t)(t.E - 1);
    }
    t.start[t.E] = (int32_t)keys.size();
    return t;
}

struct Seq {                     // sequential union-find, smaller root wins
    std::vector<int32_t> p;
    explicit Seq(uint32_t n) : p(n) { std::iota(p.begin(), p.end(), 0); }
    int32_t find(int32_t x) {
        while (p[x] != x) x = p[x] = p[p[x]];
        return x;
    }
    void unite(int32_t a, int32_t b) {
        a = find(a), b = find(b);
        if (a != b) p[std::max(a, b)] = std::min(a, b);
    }
};

template <typename Fn>
static void parallel(uint32_t n, unsigned threads, Fn fn) {      // interleaved items: neighbours run on different threads
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < threads; ++t)
        pool.emplace_back([=] {
            for (uint32_t i = t; i < n; i += threads) fn(i);
        });
    for (auto& th : pool) th.join();
}

static bool run(const Case& c, unsigned threads) {
    const uint32_t V = c.V, F = (uint32_t)(c.faces.size() / 3), H = 3 * F;
    const Table t = build(c);
    std::vector<uint32_t> status(threads * 16, 0);                // one padded word per thread
    uint32_t* sp = status.data();
    // face components
    std::vector<int32_t> parent(F), label(F);
    int32_t *pp = parent.data(), *lp = label.data();
    const int32_t *fe = t.face_edges.data(), *es = t.start.data(), *he = t.halfedges.data();
    parallel(F, threads, [=](uint32_t f) { pp[f] = (int32_t)f; });
    parallel(H, threads, [=](uint32_t i) { nsa::topo_pass_join(pp, F, fe, es, he, i, sp + 16 * (i % threads)); });
    parallel(F, threads, [=](uint32_t f) { lp[f] = nsa::topo_pass_label(pp, F, fe, f, sp + 16 * (f % threads)); });
    Seq sf(F);
    for (uint32_t e = 0; e < t.E; ++e)
        for (int32_t i = t.start[e] + 1; i < t.start[e + 1]; ++i) sf.unite(t.halfedges[i] / 3, t.halfedges[i - 1] / 3);
    size_t bad = 0, comps = 0;
    for (uint32_t f = 0; f < F; ++f) {
        const int32_t ref = t.face_edges[3 * f] >= 0 ? sf.find((int32_t)f) : -1;
        bad += ref != label[f];
        comps += ref == (int32_t)f;
    }
    // boundary loops
    std::vector<int32_t> vparent(V), mark(V);
    int32_t *vp = vparent.data(), *mp = mark.data();
    const int32_t *ed = t.edges.data(), *cn = t.count.data();
    parallel(V, threads, [=](uint32_t v) { nsa::uf_pass_init(vp, mp, v); });
    parallel(t.E, threads, [=](uint32_t e) { nsa::topo_pass_boundary(vp, mp, V, ed, e, cn[e], sp + 16 * (e % threads)); });
    Seq sv(V);
    std::vector<char> on(V, 0);
    for (uint32_t e = 0; e < t.E; ++e)
        if (t.count[e] == 1) {
            on[t.edges[2 * e]] = on[t.edges[2 * e + 1]] = 1;
            sv.unite(t.edges[2 * e], t.edges[2 * e + 1]);
        }
    size_t loops = 0, loops_ref = 0;
    for (uint32_t v = 0; v < V; ++v) {
        bad += (mark[v] == 0) != (on[v] != 0);
        loops += mark[v] == 0 && vparent[v] == (int32_t)v;
        loops_ref += on[v] && sv.find((int32_t)v) == (int32_t)v;
        uint32_t st = 0;
        if (on[v]) bad += nsa::uf_find(vp, (int32_t)v, V, &st) != sv.find((int32_t)v);
    }
    bad += loops != loops_ref;
    uint32_t st = 0;
    for (unsigned k = 0; k < threads; ++k) st |= status[16 * k];
    std::printf("%-28s V %8u F %8u E %8u components %7zu loops %6zu status %u mismatches %zu\n", c.name.c_str(), V, F, t.E, comps, loops,
                st, bad);
    return bad == 0 && st == 0;
}

int main(int argc, char** argv) {
    const unsigned threads = argc > 1 ? (unsigned)std::atoi(argv[1]) : 8;
    const uint32_t n = argc > 2 ? (uint32_t)std::atoi(argv[2]) : 100000;
    std::mt19937 g(4321);
    std::vector<Case> cases;
    auto strip = [&](uint32_t m, int32_t base) {
        std::vector<int32_t> f;
        for (uint32_t i = 0; i + 2 < m; ++i) f.insert(f.end(), {base + (int32_t)i, base + (int32_t)i + 1, base + (int32_t)i + 2});
        return f;
    };
    cases.push_back({"strip", n, strip(n, 0)});
    {
        Case c{"strip permuted names", n, strip(n, 0)};
        std::vector<int32_t> perm(n);
        std::iota(perm.begin(), perm.end(), 0);
        std::shuffle(perm.begin(), perm.end(), g);
        for (auto& x : c.faces) x = perm[x];
        cases.push_back(c);
    }
    {
        Case c{"fan on one edge", n + 2, {}};                     // one run of n half-edges: every union meets at one root
        for (uint32_t i = 0; i < n; ++i) c.faces.insert(c.faces.end(), {0, 1, (int32_t)i + 2});
        cases.push_back(c);
    }
    {
        Case c{"star around a vertex", n + 1, {}};
        for (uint32_t i = 0; i + 1 < n; ++i) c.faces.insert(c.faces.end(), {(int32_t)(n / 2), (int32_t)i, (int32_t)i + 1});
        cases.push_back(c);
    }
    for (uint32_t V : {3 * n, n / 8}) {
        Case c{V > n ? "random sparse" : "random dense", V, {}};
        std::uniform_int_distribution<int32_t> d(0, (int32_t)V - 1);
        for (uint32_t i = 0; i < 3 * n; ++i) c.faces.push_back(d(g));
        cases.push_back(c);
    }
    {
        Case c{"soup", 3 * (n / 2), {}};
        for (uint32_t i = 0; i < 3 * (n / 2); ++i) c.faces.push_back((int32_t)i);
        cases.push_back(c);
    }
    {
        Case c{"two strips alternating", 2 * n, {}};
        const std::vector<int32_t> a = strip(n, 0), b = strip(n, (int32_t)n);
        for (size_t f = 0; f < a.size() / 3; ++f) {
            c.faces.insert(c.faces.end(), a.begin() + 3 * f, a.begin() + 3 * f + 3);
            c.faces.insert(c.faces.end(), b.begin() + 3 * f, b.begin() + 3 * f + 3);
        }
        cases.push_back(c);
    }
    cases.push_back({"invalid and degenerate", 12, {0, 1, 2, -1, 3, 4, 5, 12, 6, 7, 7, 8, 2, 8, 8, 5, 6, 5, 2, 1, 9}});
    cases.push_back({"no faces", 5, {}});
    bool ok = true;
    for (const Case& c : cases) ok = run(c, threads) && ok;
    std::printf("%s\n", ok ? "ok" : "FAILED");
    return ok ? 0 : 1;
}
