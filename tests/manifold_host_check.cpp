// Host rehearsal of the fan split: the pass bodies of nicer_slam_amd/csrc/manifold_passes.hpp, compiled as host C++ and run by many
// threads on an edge table built here with std::sort, against the outputs of the sequential oracle tests/manifold_ref.py, element for
// element.  Built and run by tests/test_mesh_repair_host_cpu.py:
//   c++ -O2 -std=c++17 -pthread [-fsanitize=address,undefined | -fsanitize=thread] manifold_host_check.cpp && ./a.out CASES [threads]
// CASES is the text file the test writes: per case  name V F flags has_labels has_mask, the 3 F face indices, the labels, the mask,
// then the expected corner_fan [3 F], vertex_fans [V], faces_out [3 F], n_new, new_source [n_new] and totals [8].
// Prints one line per case; exit status 1 on any mismatch or tripped step cap.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "../nicer_slam_amd/csrc/manifold_passes.hpp"

struct Case {
    std::string name;
    uint32_t V = 0, F = 0, flags = 0;
    std::vector<int32_t> faces, labels, corner_fan, vertex_fans, faces_out, new_source;
    std::vector<uint8_t> mask;
    bool has_labels = false, has_mask = false;
    uint64_t totals[8] = {};
};

struct Table {                   // header Section 18, built sequentially
    std::vector<int32_t> edges, count, forward, start, halfedges, face_edges;
    uint32_t E = 0;
};

static Table build(const Case& c) {
    const uint32_t F = c.F, H = 3 * F;
    Table t;
    t.face_edges.assign(H, -1);
    t.halfedges.assign(H, -1);
    std::vector<std::pair<uint64_t, int32_t>> keys;
    for (uint32_t f = 0; f < F; ++f) {
        const int32_t* v = &c.faces[3 * f];
        const bool ok = v[0] >= 0 && v[1] >= 0 && v[2] >= 0 && (uint32_t)v[0] < c.V && (uint32_t)v[1] < c.V && (uint32_t)v[2] < c.V &&
                        v[0] != v[1] && v[1] != v[2] && v[2] != v[0] && (!c.has_mask || c.mask[f]);
        if (!ok) continue;
        for (int k = 0; k < 3; ++k) {
            const uint64_t a = (uint64_t)v[k], b = (uint64_t)v[(k + 1) % 3];
            keys.push_back({(std::min(a, b) << 32) | std::max(a, b), (int32_t)(3 * f + k)});
        }
    }
    std::sort(keys.begin(), keys.end());
    t.edges.assign(2 * (size_t)H, 0);
    t.count.assign(H, 0);
    t.forward.assign(H, 0);
    t.start.assign((size_t)H + 1, 0);
    for (size_t i = 0; i < keys.size(); ++i) {
        if (i == 0 || keys[i].first != keys[i - 1].first) {
            t.edges[2 * t.E] = (int32_t)(keys[i].first >> 32);
            t.edges[2 * t.E + 1] = (int32_t)(keys[i].first & 0xFFFFFFFFu);
            t.start[t.E++] = (int32_t)i;
        }
        const int32_t h = keys[i].second;
        t.count[t.E - 1]++;
        t.forward[t.E - 1] += c.faces[h] < c.faces[3 * (h / 3) + (h % 3 + 1) % 3];
        t.halfedges[i] = h;
        t.face_edges[h] = (int32_t)(t.E - 1);
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

template <typename A, typename B>
static size_t differ(const std::vector<A>& a, const std::vector<B>& b, size_t n) {
    size_t bad = 0;
    for (size_t i = 0; i < n; ++i) bad += (int64_t)a[i] != (int64_t)b[i];
    return bad;
}

static bool run(const Case& c, unsigned threads) {
    const uint32_t V = c.V, F = c.F, H = 3 * F;
    const Table t = build(c);
    std::vector<uint32_t> status(threads * 16, 0);                // one padded word per thread
    uint32_t* sp = status.data();
    std::vector<int32_t> parent(H), fan_name(H, -1), corner_fan(H), on_cut(V, 0), first_r(V, -1), last_r(V, -1), vertex_fans(V),
        faces_out(H), new_source(H, -7);
    std::vector<uint32_t> key(H), order(H), r(H, 0);
    std::vector<char> cut(H, 0);
    int32_t *pp = parent.data(), *fn = fan_name.data(), *cf = corner_fan.data(), *oc = on_cut.data(), *fr = first_r.data(),
            *lr = last_r.data(), *vf = vertex_fans.data(), *fo = faces_out.data(), *ns = new_source.data();
    uint32_t *kp = key.data(), *op = order.data(), *rp = r.data();
    char* cp = cut.data();
    const int32_t *fa = c.faces.data(), *lab = c.has_labels ? c.labels.data() : nullptr, *ed = t.edges.data(), *cn = t.count.data(),
                  *fw = t.forward.data(), *es = t.start.data(), *he = t.halfedges.data(), *fe = t.face_edges.data();
    const uint32_t flags = c.flags;
    parallel(H, threads, [=](uint32_t i) { pp[i] = (int32_t)i; });
    parallel(t.E, threads, [=](uint32_t e) {
        cp[e] = nsa::mf_pass_join(pp, oc, fa, F, V, lab, flags, ed, cn, fw, es, he, fe, e, sp + 16 * (e % threads));
    });
    parallel(H, threads, [=](uint32_t i) { cf[i] = nsa::mf_pass_leader(pp, fa, fe, F, V, i, kp + i, sp + 16 * (i % threads)); });
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    uint32_t n_new = 0, n_fans = 0;
    for (uint32_t i = 0; i < H; ++i) {                            // the exclusive scan of the "not head of its run" flags
        uint32_t cc, vv;
        const int kind = nsa::mf_run_head(cf, fa, fe, op, H, V, i, &cc, &vv);
        r[i] = n_new;
        n_new += kind == 2;
        n_fans += kind != 0;
    }
    parallel(H, threads, [=](uint32_t i) { nsa::mf_pass_name(cf, fa, fe, op, F, V, i, rp[i], fn, ns, fr, lr); });
    parallel(V, threads, [=](uint32_t v) { vf[v] = nsa::mf_vertex_fans(fr, lr, v); });
    parallel(H, threads, [=](uint32_t i) { fo[i] = nsa::mf_pass_face(fa, cf, fn, F, V, i); });
    uint64_t tot[8] = {0, n_fans, 0, 0, 0, n_new, 0, 0};
    for (uint32_t f = 0; f < F; ++f) tot[0] += corner_fan[3 * f] >= 0;
    for (uint32_t v = 0; v < V; ++v) {
        tot[2] += vertex_fans[v] > 1;
        tot[3] += vertex_fans[v] > 1 && !on_cut[v];
        tot[6] = std::max<uint64_t>(tot[6], (uint64_t)vertex_fans[v]);
    }
    for (uint32_t e = 0; e < t.E; ++e) tot[4] += cut[e] != 0;
    for (unsigned k = 0; k < threads; ++k) tot[7] |= status[16 * k];
    size_t bad = differ(corner_fan, c.corner_fan, H) + differ(vertex_fans, c.vertex_fans, V) + differ(faces_out, c.faces_out, H);
    bad += n_new != c.new_source.size() ? 1 : differ(new_source, c.new_source, n_new);
    for (int k = 0; k < 8; ++k) bad += tot[k] != c.totals[k];
    std::printf("%-32s V %7u F %7u E %7u fans %7u new %7u cut %6llu status %llu mismatches %zu\n", c.name.c_str(), V, F, t.E, n_fans, n_new,
                (unsigned long long)tot[4], (unsigned long long)tot[7], bad);
    return bad == 0 && tot[7] == 0;
}

template <typename T>
static bool read_n(std::ifstream& in, std::vector<T>& out, size_t n) {
    out.resize(n);
    for (size_t i = 0; i < n; ++i) {
        long long x;
        if (!(in >> x)) return false;
        out[i] = (T)x;
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: manifold_host_check CASES [threads]\n");
        return 2;
    }
    const unsigned threads = argc > 2 ? (unsigned)std::max(1, std::atoi(argv[2])) : 8;
    std::ifstream in(argv[1]);
    bool ok = true;
    size_t n_cases = 0;
    Case c;
    while (in >> c.name) {
        int hl = 0, hm = 0;
        size_t n_new = 0;
        std::vector<uint64_t> tot;
        bool good = bool(in >> c.V >> c.F >> c.flags >> hl >> hm);
        c.has_labels = hl != 0;
        c.has_mask = hm != 0;
        good = good && (uint64_t)c.V + 3ull * c.F < 0x80000000ull && read_n(in, c.faces, 3 * (size_t)c.F);
        good = good && read_n(in, c.labels, c.has_labels ? c.F : 0) && read_n(in, c.mask, c.has_mask ? c.F : 0);
        good = good && read_n(in, c.corner_fan, 3 * (size_t)c.F) && read_n(in, c.vertex_fans, c.V) && read_n(in, c.faces_out, 3 * (size_t)c.F);
        good = good && bool(in >> n_new) && n_new <= 3 * (size_t)c.F && read_n(in, c.new_source, n_new) && read_n(in, tot, 8);
        if (!good) {
            std::fprintf(stderr, "manifold_host_check: case %s is malformed\n", c.name.c_str());
            return 2;
        }
        std::copy(tot.begin(), tot.end(), c.totals);
        ok = run(c, threads) && ok;
        ++n_cases;
    }
    std::printf("%zu cases\n%s\n", n_cases, ok && n_cases ? "ok" : "FAILED");
    return ok && n_cases ? 0 : 1;
}
