// Host rehearsal of the union-find passes of the mesh orientation: the pass bodies of nicer_slam_amd/csrc/orient_passes.hpp, compiled as
// host C++ and run by many threads on an edge table built here with std::sort, against a sequential breadth-first two-colouring in
// which the smallest face of a component keeps its winding.
// Built and run by tests/test_mesh_orient_cpu.py:   c++ -O2 -std=c++17 -pthread [-fsanitize=thread] orient_host_check.cpp && ./a.out
// [threads] [n].  Prints one line per case; exit status 1 on any mismatch or tripped step cap.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../nicer_slam_amd/csrc/orient_passes.hpp"

struct Case {
    std::string name;
    uint32_t V;
    std::vector<int32_t> faces;
};

struct Table {                   // header Section 18, built sequentially
    std::vector<int32_t> start, halfedges, face_edges;
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
    t.start.assign((size_t)H + 1, 0);
    for (size_t i = 0; i < keys.size(); ++i) {
        if (i == 0 || keys[i].first != keys[i - 1].first) t.start[t.E++] = (int32_t)i;
        t.halfedges[i] = keys[i].second;
        t.face_edges[keys[i].second] = (int32_t)(t.E - 1);
    }
    t.start[t.E] = (int32_t)keys.size();
    return t;
}

template <typename Fn>
static void parallel(uint32_t n, unsigned threads, Fn fn) {      // interleaved items: neighbours run on different threads
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < threads; ++t)
        pool.emplace_back([=] {
            for (uint32_t i = t; i < n; i += threads) fn(i);
        });
    for (auto& th : pool) th.join();
}

struct Ref {
    std::vector<int32_t> label;
    std::vector<uint8_t> orientable, flip;
};

// sequential two-colouring over the edges with exactly two half-edges; faces visited in ascending order
static Ref colour(const Case& c, const Table& t) {
    const uint32_t F = (uint32_t)(c.faces.size() / 3);
    std::vector<std::vector<std::pair<int32_t, int>>> nbr(F);
    for (uint32_t e = 0; e < t.E; ++e) {
        if (t.start[e + 1] - t.start[e] != 2) continue;
        const int32_t h0 = t.halfedges[t.start[e]], h1 = t.halfedges[t.start[e] + 1];
        const int par = c.faces[h0] != c.faces[h1] ? 0 : 1;
        nbr[h0 / 3].push_back({h1 / 3, par});
        nbr[h1 / 3].push_back({h0 / 3, par});
    }
    Ref r;
    r.label.assign(F, -1);
    r.orientable.assign(F, 0);
    r.flip.assign(F, 0);
    std::vector<int> col(F, 0);
    for (uint32_t s = 0; s < F; ++s) {
        if (t.face_edges[3 * s] < 0 || r.label[s] >= 0) continue;
        std::vector<int32_t> members{(int32_t)s};
        r.label[s] = (int32_t)s;
        bool ok = true;
        for (size_t q = 0; q < members.size(); ++q) {
            const int32_t a = members[q];
            for (auto [b, par] : nbr[a]) {
                if (r.label[b] < 0) {
                    r.label[b] = (int32_t)s;
                    col[b] = col[a] ^ par;
                    members.push_back(b);
                } else if (col[b] != (col[a] ^ par)) {
                    ok = false;
                }
            }
        }
        for (int32_t m : members) {
            r.orientable[m] = ok;
            r.flip[m] = ok && col[m] == 1;
        }
    }
    return r;
}

static bool run(const Case& c, unsigned threads) {
    const uint32_t F = (uint32_t)(c.faces.size() / 3), H = 3 * F;
    const Table t = build(c);
    std::vector<uint32_t> status(threads * 16, 0);                // one padded word per thread
    uint32_t* sp = status.data();
    std::vector<int32_t> parent(2 * (size_t)F), label(F);
    std::vector<uint8_t> orientable(F), flip(F);
    int32_t *pp = parent.data(), *lp = label.data();
    uint8_t *op = orientable.data(), *fp = flip.data();
    const int32_t *fc = c.faces.data(), *fe = t.face_edges.data(), *es = t.start.data(), *he = t.halfedges.data();
    const uint32_t E = t.E;
    parallel(2 * F, threads, [=](uint32_t x) { pp[x] = (int32_t)x; });
    parallel(H, threads, [=](uint32_t e) { nsa::orient_pass_join(pp, F, fc, es, he, e, E, sp + 16 * (e % threads)); });
    parallel(F, threads, [=](uint32_t f) { lp[f] = nsa::orient_pass_label(pp, F, fe, f, op + f, fp + f, sp + 16 * (f % threads)); });
    const Ref r = colour(c, t);
    size_t bad = 0, comps = 0, nonor = 0, flips = 0;
    for (uint32_t f = 0; f < F; ++f) {
        bad += r.label[f] != label[f] || r.orientable[f] != orientable[f] || r.flip[f] != flip[f];
        comps += label[f] == (int32_t)f;
        nonor += label[f] == (int32_t)f && !orientable[f];
        flips += flip[f];
    }
    uint32_t st = 0;
    for (unsigned k = 0; k < threads; ++k) st |= status[16 * k];
    std::printf("%-30s V %8u F %8u E %8u components %7zu not orientable %5zu flipped %7zu status %u mismatches %zu\n", c.name.c_str(), c.V,
                F, t.E, comps, nonor, flips, st, bad);
    return bad == 0 && st == 0;
}

int main(int argc, char** argv) {
    const unsigned threads = argc > 1 ? (unsigned)std::atoi(argv[1]) : 8;
    const uint32_t n = argc > 2 ? (uint32_t)std::atoi(argv[2]) : 100000;
    std::mt19937 g(4321);
    std::vector<Case> cases;
    auto strip = [&](uint32_t m, uint32_t every) {               // consistently wound, then every `every`-th face reversed
        std::vector<int32_t> f;
        for (uint32_t i = 0; i + 2 < m; ++i) {
            int32_t a = (int32_t)i, b = (int32_t)i + 1, c = (int32_t)i + 2;
            if (i & 1) std::swap(a, b);
            if (every && i % every == 0) std::swap(b, c);
            f.insert(f.end(), {a, b, c});
        }
        return f;
    };
    cases.push_back({"strip", n, strip(n, 0)});
    cases.push_back({"strip, every 2nd reversed", n, strip(n, 2)});
    cases.push_back({"strip, every 7th reversed", n, strip(n, 7)});
    {
        Case c{"strip permuted, every 3rd", n, strip(n, 3)};
        std::vector<int32_t> perm(n);
        std::iota(perm.begin(), perm.end(), 0);
        std::shuffle(perm.begin(), perm.end(), g);
        for (auto& x : c.faces) x = perm[x];
        cases.push_back(c);
    }
    {
        const int32_t q = 8;                                      // the 8-quad Moebius strip of tests/topology_ref.py
        auto top = [&](int32_t i) { return 2 * (i % q) + ((i / q) % 2 ? 1 : 0); };
        auto bot = [&](int32_t i) { return 2 * (i % q) + ((i / q) % 2 ? 0 : 1); };
        Case c{"moebius strip", 2 * q, {}};
        for (int32_t i = 0; i < q; ++i) {
            const int32_t a = top(i), b = bot(i), cc = top(i + 1), d = bot(i + 1);
            c.faces.insert(c.faces.end(), {a, b, cc, cc, b, d});
        }
        cases.push_back(c);
    }
    {
        const uint32_t q = n / 2;                                 // a long Moebius strip: the two sheets meet at the far end
        Case c{"long moebius strip", 2 * q, {}};
        for (uint32_t i = 0; i < q; ++i) {
            const bool wrap = i + 1 == q;
            const int32_t a = 2 * (int32_t)i, b = a + 1, cc = wrap ? 1 : a + 2, d = wrap ? 0 : a + 3;
            c.faces.insert(c.faces.end(), {a, b, cc, cc, b, d});
        }
        cases.push_back(c);
    }
    {
        Case c{"fan on one edge", 100002, {}};                    // one edge with 10^5 half-edges: joins nothing
        for (uint32_t i = 0; i < 100000; ++i) c.faces.insert(c.faces.end(), {0, 1, (int32_t)i + 2});
        cases.push_back(c);
    }
    for (uint32_t V : {3 * n, n / 8}) {
        Case c{V > n ? "random sparse" : "random dense", V, {}};
        std::uniform_int_distribution<int32_t> d(0, (int32_t)V - 1);
        for (uint32_t i = 0; i < 3 * n; ++i) c.faces.push_back(d(g));
        cases.push_back(c);
    }
    {
        Case c{"random strips, random reversals", n, strip(n, 0)};
        std::bernoulli_distribution coin(0.3);
        for (size_t f = 0; f < c.faces.size() / 3; ++f)
            if (coin(g)) std::swap(c.faces[3 * f + 1], c.faces[3 * f + 2]);
        cases.push_back(c);
    }
    cases.push_back({"invalid and degenerate", 12, {0, 1, 2, -1, 3, 4, 5, 12, 6, 7, 7, 8, 2, 8, 8, 5, 6, 5, 2, 1, 9}});
    cases.push_back({"no faces", 5, {}});
    bool ok = true;
    for (const Case& c : cases) ok = run(c, threads) && ok;
    std::printf("%s\n", ok ? "ok" : "FAILED");
    return ok ? 0 : 1;
}
