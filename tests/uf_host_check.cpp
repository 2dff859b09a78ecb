// Host rehearsal of the component labelling: the pass bodies of nicer_slam_amd/csrc/uf_passes.hpp, compiled as host C++ and run
// by many threads on adversarial face lists, against a sequential union-find (smaller root wins).  Built and run by
// tests/test_mesh_clean_cpu.py:   c++ -O2 -std=c++17 -pthread [-fsanitize=thread] uf_host_check.cpp && ./a.out [threads]
// Prints one line per case; exit status 1 on any mismatch or tripped step cap.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../nicer_slam_amd/csrc/uf_passes.hpp"

using nsa::uf_pass_face;
using nsa::uf_pass_init;
using nsa::uf_pass_label;

struct Case {
    std::string name;
    uint32_t V;
    std::vector<int32_t> faces;
};

static std::vector<int32_t> sequential(const Case& c) {
    std::vector<int32_t> p(c.V), out(c.V, -1);
    std::vector<char> used(c.V, 0);
    std::iota(p.begin(), p.end(), 0);
    auto find = [&](int32_t x) {
        while (p[x] != x) x = p[x] = p[p[x]];
        return x;
    };
    auto unite = [&](int32_t a, int32_t b) {
        a = find(a), b = find(b);
        if (a != b) p[std::max(a, b)] = std::min(a, b);
    };
    for (size_t f = 0; f < c.faces.size() / 3; ++f) {
        const int32_t a = c.faces[3 * f], b = c.faces[3 * f + 1], d = c.faces[3 * f + 2];
        if (a < 0 || b < 0 || d < 0 || (uint32_t)a >= c.V || (uint32_t)b >= c.V || (uint32_t)d >= c.V) continue;
        used[a] = used[b] = used[d] = 1;
        unite(a, b);
        unite(b, d);
    }
    for (uint32_t v = 0; v < c.V; ++v)
        if (used[v]) out[v] = find((int32_t)v);
    return out;
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

static bool run(const Case& c, unsigned threads) {
    const uint32_t V = c.V, F = (uint32_t)(c.faces.size() / 3);
    std::vector<int32_t> parent(V), label(V);
    std::vector<uint32_t> status(threads * 16, 0);                // one padded word per thread
    int32_t *pp = parent.data(), *lp = label.data();
    const int32_t* fp = c.faces.data();
    uint32_t* sp = status.data();
    parallel(V, threads, [=](uint32_t v) { uf_pass_init(pp, lp, v); });
    parallel(F, threads, [=](uint32_t f) { uf_pass_face(pp, lp, fp, f, V, sp + 16 * (f % threads)); });
    parallel(V, threads, [=](uint32_t v) { uf_pass_label(pp, lp, v, V, sp + 16 * (v % threads)); });
    uint32_t st = 0;
    for (unsigned t = 0; t < threads; ++t) st |= status[16 * t];
    const std::vector<int32_t> ref = sequential(c);
    size_t bad = 0, comps = 0;
    for (uint32_t v = 0; v < V; ++v) {
        bad += ref[v] != label[v];
        comps += ref[v] == (int32_t)v;
    }
    std::printf("%-28s V %8u F %8u components %7zu status %u mismatches %zu\n", c.name.c_str(), V, F, comps, st, bad);
    return bad == 0 && st == 0;
}

int main(int argc, char** argv) {
    const unsigned threads = argc > 1 ? (unsigned)std::atoi(argv[1]) : 8;
    const uint32_t n = argc > 2 ? (uint32_t)std::atoi(argv[2]) : 100000;
    std::mt19937 g(1234);
    std::vector<Case> cases;
    auto strip = [&](uint32_t m) {
        std::vector<int32_t> f;
        for (uint32_t i = 0; i + 2 < m; ++i) f.insert(f.end(), {(int32_t)i, (int32_t)i + 1, (int32_t)i + 2});
        return f;
    };
    cases.push_back({"strip", n, strip(n)});
    {
        Case c{"strip reversed", n, strip(n)};
        const size_t F = c.faces.size() / 3;
        for (size_t i = 0; i < F / 2; ++i)
            for (int k = 0; k < 3; ++k) std::swap(c.faces[3 * i + k], c.faces[3 * (F - 1 - i) + k]);
        cases.push_back(c);
    }
    {
        Case c{"strip permuted names", n, strip(n)};
        std::vector<int32_t> perm(n);
        std::iota(perm.begin(), perm.end(), 0);
        std::shuffle(perm.begin(), perm.end(), g);
        for (auto& x : c.faces) x = perm[x];
        cases.push_back(c);
    }
    {
        Case c{"star", n + 1, {}};
        for (uint32_t i = 0; i + 1 < n; ++i) c.faces.insert(c.faces.end(), {(int32_t)(n / 2), (int32_t)i, (int32_t)i + 1});
        cases.push_back(c);
    }
    for (uint32_t V : {3 * n, n / 2}) {
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
        for (uint32_t i = 0; i + 2 < n; ++i) {
            c.faces.insert(c.faces.end(), {(int32_t)i, (int32_t)i + 1, (int32_t)i + 2});
            c.faces.insert(c.faces.end(), {(int32_t)(n + i), (int32_t)(n + i) + 1, (int32_t)(n + i) + 2});
        }
        cases.push_back(c);
    }
    cases.push_back({"invalid and degenerate", 12, {0, 1, 2, -1, 3, 4, 5, 12, 6, 7, 7, 8, 2, 8, 8, 5, 6, 5}});
    cases.push_back({"no faces", 5, {}});
    bool ok = true;
    for (const Case& c : cases) ok = run(c, threads) && ok;
    std::printf("%s\n", ok ? "ok" : "FAILED");
    return ok ? 0 : 1;
}
