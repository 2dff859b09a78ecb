// Host rehearsal of k nearest neighbours and normal estimation: the bodies of nicer_slam_amd/csrc/normals_passes.hpp -- the candidate list
// of a query, a neighbourhood's mean and scatter, the cyclic Jacobi, the normal's orientation and validity -- compiled as host C++ and
// called one row at a time, the way k_nn_query_k (csrc/mesh_eval.hip) and k_cloud_normals (csrc/cloud_normals.hip) call them.
// Built and run by tests/test_cloud_normals_host_cpu.py:
//     c++ -O2 -std=c++17 -ffp-contract=off [-fsanitize=address,undefined -fno-sanitize-recover=all] cloud_normals_host_check.cpp
//     ./a.out knn CASE > RESULT       ./a.out normals CASE > RESULT
// knn CASE (text): nq nt k strict r2_bits / 3 nt target words (fp32 bits) / 3 nq query words / nt numbers: the order the targets are
// offered in.  The d2 is the kernel's (sq_dist), the list is strided as on the device.  RESULT: nq k indices / nq k dist words / nq counts.
// normals CASE: n m k vrows want_eig / 3 n point words / m k indices / m counts / 3 m origin words / 3 vrows viewpoint words.
// RESULT: 3 m normal words (fp32 bits) / 3 m eigenvalue words (float64 bits; absent without want_eig) / m valid / m sweep counts.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../nicer_slam_amd/csrc/normals_passes.hpp"

using namespace nsa::cn;
typedef unsigned long long ull;

template <typename T>
static bool read_all(FILE* fh, const char* fmt, std::vector<T>& out) {
    for (auto& x : out)
        if (fscanf(fh, fmt, &x) != 1) return false;
    return true;
}

static std::vector<float> floats(const std::vector<unsigned>& bits) {
    std::vector<float> out(bits.size());
    if (!bits.empty()) memcpy(out.data(), bits.data(), 4 * bits.size());
    return out;
}

static bool finite3(const float* p) { return fabsf(p[0]) <= 3.4028234e38f && fabsf(p[1]) <= 3.4028234e38f && fabsf(p[2]) <= 3.4028234e38f; }

static float sq_dist(const float* a, const float* q) {
    const float dx = a[0] - q[0], dy = a[1] - q[1], dz = a[2] - q[2];
    return (dx * dx + dy * dy) + dz * dz;
}

static int run_knn(FILE* fh) {
    unsigned nq, nt, k, strict, r2_bits;
    if (fscanf(fh, "%u %u %u %u %u", &nq, &nt, &k, &strict, &r2_bits) != 5 || k < 1 || k > kMaxK) return 2;
    std::vector<unsigned> t_bits(3 * (size_t)nt), q_bits(3 * (size_t)nq), order(nt);
    if (!read_all(fh, "%u", t_bits) || !read_all(fh, "%u", q_bits) || !read_all(fh, "%u", order)) return 2;
    const std::vector<float> t = floats(t_bits), q = floats(q_bits);
    const float r2 = bits_f32(r2_bits);
    const uint32_t stride = 5;                                    // any stride: the device's is 64
    std::vector<int> idx((size_t)nq * k);
    std::vector<unsigned> dist((size_t)nq * k), count(nq);
    for (size_t j = 0; j < nq; ++j) {
        std::vector<uint64_t> keys((size_t)k * stride);
        uint32_t held = 0;
        uint64_t worst = 0;
        const bool ok = finite3(&q[3 * j]);
        if (ok)
            for (unsigned o : order) {
                if (o >= nt) return 2;
                if (finite3(&t[3 * (size_t)o])) knn_offer(keys.data(), stride, k, held, worst, sq_dist(&t[3 * (size_t)o], &q[3 * j]), o, r2, strict != 0);
            }
        for (uint32_t s = 0; s < k; ++s) {
            const uint64_t key = s < held ? keys[(size_t)s * stride] : 0;
            idx[j * k + s] = s < held ? (int)(uint32_t)key : -1;
            const float d = !ok ? NAN : (s < held ? knn_root(bits_f32((uint32_t)(key >> 32))) : INFINITY);
            dist[j * k + s] = f32_bits(d);
        }
        count[j] = held;
    }
    for (int i : idx) printf("%d ", i);
    printf("\n");
    for (unsigned d : dist) printf("%u ", d);
    printf("\n");
    for (unsigned c : count) printf("%u ", c);
    printf("\n");
    return 0;
}

static int run_normals(FILE* fh) {
    unsigned n, m, k, vrows, want_eig;
    if (fscanf(fh, "%u %u %u %u %u", &n, &m, &k, &vrows, &want_eig) != 5 || k < 1 || k > kMaxK) return 2;
    if (vrows != 0 && vrows != 1 && vrows != m) return 2;
    std::vector<unsigned> p_bits(3 * (size_t)n), count(m), o_bits(3 * (size_t)m), v_bits(3 * (size_t)vrows);
    std::vector<int> idx((size_t)m * k);
    if (!read_all(fh, "%u", p_bits) || !read_all(fh, "%d", idx) || !read_all(fh, "%u", count) || !read_all(fh, "%u", o_bits) ||
        !read_all(fh, "%u", v_bits))
        return 2;
    const std::vector<float> p = floats(p_bits), origin = floats(o_bits), view = floats(v_bits);
    std::vector<float> normals(3 * (size_t)m);
    std::vector<double> eig(3 * (size_t)m);
    std::vector<uint8_t> valid(m);
    std::vector<int> sweeps(m);
    for (size_t i = 0; i < m; ++i) {
        const float* towards = vrows == 0 ? nullptr : view.data() + (vrows == 1 ? 0 : 3 * i);
        normals_row(p.data(), n, idx.data() + i * k, count[i], k, origin.data() + 3 * i, towards, normals.data() + 3 * i,
                    want_eig ? eig.data() + 3 * i : nullptr, valid.data() + i);
        double S[6], w[3], V[3][3];
        sweeps[i] = scatter(p.data(), n, idx.data() + i * k, count[i], k, S) ? jacobi3(S, w, V) : -1;
    }
    for (float x : normals) printf("%u ", f32_bits(x));
    printf("\n");
    if (want_eig) {
        for (double x : eig) {
            ull b;
            memcpy(&b, &x, 8);
            printf("%llu ", b);
        }
        printf("\n");
    }
    for (uint8_t v : valid) printf("%u ", (unsigned)v);
    printf("\n");
    for (int s : sweeps) printf("%d ", s);
    printf("\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fh = fopen(argv[2], "r");
    if (!fh) return 2;
    const int rc = strcmp(argv[1], "knn") == 0 ? run_knn(fh) : (strcmp(argv[1], "normals") == 0 ? run_normals(fh) : 2);
    fclose(fh);
    return rc;
}
