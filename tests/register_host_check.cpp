// Host rehearsal of point-to-plane registration: the bodies of nicer_slam_amd/csrc/register_passes.hpp -- moving a point, a face's normal,
// a row's terms and weight, the rows a lane adds and the tree over the lanes -- compiled as host C++ and called one row at a time, the
// way the kernels of csrc/mesh_register.hip call them: a loop over the tiles, the 256 lanes and each lane's 16 rows, the tree per tile,
// then the tree over groups of 256 totals until one value is left.
// Built and run by tests/test_mesh_register_host_cpu.py:
//     c++ -O2 -std=c++17 -ffp-contract=off [-fsanitize=address,undefined -fno-sanitize-recover=all] register_host_check.cpp
//     ./a.out CASE > RESULT
// CASE (text): n surface kernel k_bits m V F / 16 words of the 4x4 (float64 bits) / 3 n words of cur (float64 bits) / n correspondences /
// cloud: n dist words (fp32 bits), 3 m target words, 3 m normal words / surface: n d2 words (float64 bits), 3 n closest words (fp32 bits),
// 3 V vertex words, 3 F indices.  RESULT: one line each of the sums' float64 bits, the two counts, the moved points' float64 bits and
// their fp32 roundings' bits, which the test compares with tests/register_ref.py element for element.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../nicer_slam_amd/csrc/register_passes.hpp"

using namespace nsa::reg;
typedef unsigned long long ull;

template <typename T>
static bool read_all(FILE* fh, const char* fmt, std::vector<T>& out) {
    for (auto& x : out)
        if (fscanf(fh, fmt, &x) != 1) return false;
    return true;
}

template <typename T, typename B>
static std::vector<T> from_bits(const std::vector<B>& bits) {
    static_assert(sizeof(T) == sizeof(B), "same width");
    std::vector<T> out(bits.size());
    if (!bits.empty()) memcpy(out.data(), bits.data(), sizeof(T) * bits.size());
    return out;
}

struct Entry {
    double s[kSums];
    ull c[2];
};

// the tree over up to 256 entries, the rest zeros
static Entry tree_of(const Entry* e, size_t count) {
    Entry out;
    for (int i = 0; i < kSums; ++i) {
        double lanes[kLanes];
        for (uint32_t l = 0; l < kLanes; ++l) lanes[l] = l < count ? e[l].s[i] : 0.0;
        out.s[i] = tree256(lanes);
    }
    for (int c = 0; c < 2; ++c) {
        out.c[c] = 0;
        for (size_t l = 0; l < count; ++l) out.c[c] += e[l].c[c];
    }
    return out;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* fh = fopen(argv[1], "r");
    if (!fh) return 2;
    unsigned n, surface, m, V, F;
    int kernel;
    ull k_bits;
    if (fscanf(fh, "%u %u %d %llu %u %u %u", &n, &surface, &kernel, &k_bits, &m, &V, &F) != 7) return 2;
    std::vector<ull> T_bits(16), cur_bits(3 * (size_t)n);
    std::vector<int> corr(n);
    if (!read_all(fh, "%llu", T_bits) || !read_all(fh, "%llu", cur_bits) || !read_all(fh, "%d", corr)) return 2;
    std::vector<unsigned> dist_bits, tgt_bits, nrm_bits, closest_bits, vert_bits;
    std::vector<ull> d2_bits;
    std::vector<int> faces;
    if (surface) {
        d2_bits.resize(n), closest_bits.resize(3 * (size_t)n), vert_bits.resize(3 * (size_t)V), faces.resize(3 * (size_t)F);
        if (!read_all(fh, "%llu", d2_bits) || !read_all(fh, "%u", closest_bits) || !read_all(fh, "%u", vert_bits) || !read_all(fh, "%d", faces))
            return 2;
    } else {
        dist_bits.resize(n), tgt_bits.resize(3 * (size_t)m), nrm_bits.resize(3 * (size_t)m);
        if (!read_all(fh, "%u", dist_bits) || !read_all(fh, "%u", tgt_bits) || !read_all(fh, "%u", nrm_bits)) return 2;
    }
    fclose(fh);
    const std::vector<double> T = from_bits<double>(T_bits), d2 = from_bits<double>(d2_bits);
    std::vector<double> cur = from_bits<double>(cur_bits);
    const std::vector<float> dist = from_bits<float>(dist_bits), targets = from_bits<float>(tgt_bits), normals = from_bits<float>(nrm_bits),
                             closest = from_bits<float>(closest_bits), verts = from_bits<float>(vert_bits);
    double k;
    memcpy(&k, &k_bits, 8);

    // the system on the points as given
    const Rows a = {cur.data(), corr.data(), dist.data(), targets.data(), normals.data(), d2.data(), closest.data(), verts.data(), faces.data(),
                    n, m, V, F, (int)surface, kernel, k};
    const uint64_t tiles = n ? ((uint64_t)n + kTile - 1) / kTile : 1;
    std::vector<Entry> level(tiles);
    for (uint64_t tile = 0; tile < tiles; ++tile) {
        std::vector<Entry> lanes(kLanes);
        for (uint32_t lane = 0; lane < kLanes; ++lane) {
            Entry& e = lanes[lane];
            for (int i = 0; i < kSums; ++i) e.s[i] = 0.0;
            e.c[0] = e.c[1] = 0;
            for (uint32_t j = 0; j < kRowsPerLane; ++j) {
                double t[kSums];
                bool has, used;
                load_row(a, row_of(tile, lane, j), t, has, used);
                for (int i = 0; i < kSums; ++i) e.s[i] = e.s[i] + t[i];
                e.c[0] += has;
                e.c[1] += used;
            }
        }
        level[tile] = tree_of(lanes.data(), kLanes);
    }
    while (level.size() > 1) {
        std::vector<Entry> next(groups_of(level.size()));
        for (size_t g = 0; g < next.size(); ++g) {
            const size_t lo = g * kLanes, cnt = level.size() - lo < kLanes ? level.size() - lo : kLanes;
            next[g] = tree_of(level.data() + lo, cnt);
        }
        level.swap(next);
    }
    for (int i = 0; i < kSums; ++i) {
        ull b;
        memcpy(&b, &level[0].s[i], 8);
        printf("%llu ", b);
    }
    printf("\n%llu %llu\n", level[0].c[0], level[0].c[1]);

    // the move
    std::vector<ull> moved(3 * (size_t)n);
    std::vector<unsigned> moved32(3 * (size_t)n);
    for (size_t i = 0; i < n; ++i) {
        const double p[3] = {cur[3 * i], cur[3 * i + 1], cur[3 * i + 2]};
        double y[3];
        transform_point(T.data(), p, y);
        for (int c = 0; c < 3; ++c) {
            const float r = (float)y[c];
            memcpy(&moved[3 * i + c], &y[c], 8);
            memcpy(&moved32[3 * i + c], &r, 4);
        }
    }
    for (ull b : moved) printf("%llu ", b);
    printf("\n");
    for (unsigned b : moved32) printf("%u ", b);
    printf("\n");
    return 0;
}
