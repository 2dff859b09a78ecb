// grid_index_host_check.cpp -- the pure index arithmetic of csrc/grid_common.hpp (make_grid_geom, level_row, generic_corner_terms /
// generic_corner_row, corner_offsets: the very functions the kernels call) compiled by the host compiler and swept, as a stand-alone
// program for tests/test_grid_index_cpu.py (which also runs it under the address and undefined-behaviour sanitizers).
//     grid_index_host_check C S H off_0 ... off_L
// For every level it sweeps cells inside the level, on its upper face (cell + 1 == res where the scale is an integer), and far outside
// (the cell the device's saturating float -> uint32 conversion makes of unit coordinates up to 1e6, of negative ones and of NaN), and
// prints one line per level:
//     level flags rows res  n_in  in_disagree  n_far  far_generic_over far_generic_max  far_offsets_over  far_level_row_over  far_offsets_out_of_table
// in_disagree: in-range cells where a path's row differs from the reference rule (get_grid_index restated below) or is >= rows;
// far_*_over: far-outside cells where the path forms a row >= rows of the LEVEL (far_generic_max: the largest such row);
// far_offsets_out_of_table: those of corner_offsets whose byte offset does not even lie inside the table.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../nicer_slam_amd/csrc/grid_common.hpp"

using namespace nsa;

// the reference's rule: stride loop with uint32 wrap, xor-prime hash when the stride passes the row count, true modulo
static uint32_t ref_row(uint32_t rows, uint32_t res, const uint32_t (&q)[3]) {
    static const uint32_t primes[3] = {1u, 2654435761u, 805459861u};
    uint32_t stride = 1u, idx = 0u;
    for (int d = 0; d < 3 && stride <= rows; ++d) {
        idx += q[d] * stride;
        stride *= res;
    }
    if (stride > rows) {
        idx = 0u;
        for (int d = 0; d < 3; ++d) idx ^= q[d] * primes[d];
    }
    return idx % rows;
}

// v_cvt_u32_f32: saturating, NaN -> 0 (the C++ conversion of such a value is undefined on the host)
static uint32_t sat_u32(float p) {
    if (!(p > 0.0f)) return 0u;
    if (p >= 4294967296.0f) return 0xFFFFFFFFu;
    return (uint32_t)p;
}

template <int C>
static void rows_of_paths(const LevelGeom& g, const uint32_t (&cell)[3], uint32_t (&gen)[8], uint32_t (&fast)[8], uint32_t (&lr)[8],
                          uint32_t (&off)[8]) {
    uint32_t term[3][2];
    generic_corner_terms<3>(g, cell, term);
    corner_offsets<C>(g, cell, off);
    for (int corner = 0; corner < 8; ++corner) {
        gen[corner] = generic_corner_row<3, false>(g, term, corner);
        fast[corner] = (off[corner] - g.row0B) / (C * 4u);          // (an offset below row0B wraps to a huge row: counted as over)
        const uint32_t q[3] = {cell[0] + (corner & 1u), cell[1] + ((corner >> 1) & 1u), cell[2] + ((corner >> 2) & 1u)};
        lr[corner] = level_row<3>(g, q);
    }
}

template <int C>
static int sweep(const std::vector<int32_t>& off, float S, uint32_t H) {
    const uint32_t L = (uint32_t)off.size() - 1;
    GridGeom geom;
    if (make_grid_geom(off.data(), L, 3, S, H, &geom, C) != NSA_OK) return 3;
    int bad = 0;
    for (uint32_t l = 0; l < L; ++l) {
        const LevelGeom& g = geom.lv[l];
        const uint32_t res = (uint32_t)std::ceil(g.scale) + 1u, top = sat_u32(1.0f * g.scale);
        std::vector<uint32_t> in = {0u, 1u, 2u, top / 3u, top / 2u, top > 2u ? top - 2u : 0u, top > 1u ? top - 1u : 0u, top};
        uint64_t n_in = 0, disagree = 0, n_far = 0, gen_over = 0, gen_max = 0, fast_over = 0, lr_over = 0;
        uint32_t gen[8], fast[8], lr[8], offs[8];
        uint64_t fast_out = 0;
        const uint64_t table_bytes = (uint64_t)(uint32_t)off[L] * C * 4;
        for (uint32_t x : in) for (uint32_t y : in) for (uint32_t z : in) {
            const uint32_t cell[3] = {x, y, z};
            rows_of_paths<C>(g, cell, gen, fast, lr, offs);
            for (int corner = 0; corner < 8; ++corner) {
                const uint32_t q[3] = {x + (corner & 1u), y + ((corner >> 1) & 1u), z + ((corner >> 2) & 1u)};
                const uint32_t want = ref_row(g.rows, res, q);
                ++n_in;
                if (gen[corner] != want || fast[corner] != want || lr[corner] != want || want >= g.rows) ++disagree;
            }
        }
        const float far_u[] = {1.0000001f, 1.5f, 2.0f, 10.0f, 1e3f, 1e6f, 3e9f, -1e-6f, -0.5f, -10.0f, -1e6f, NAN};
        std::vector<uint32_t> far;
        for (float u : far_u) far.push_back(sat_u32(u * g.scale));
        far.push_back(0xFFFFFFFFu);
        std::vector<uint32_t> all = far;
        all.insert(all.end(), in.begin(), in.end());
        for (uint32_t x : all) for (uint32_t y : all) for (uint32_t z : all) {
            const uint32_t cell[3] = {x, y, z};
            if (x <= top && y <= top && z <= top) continue;          // in range: covered above
            rows_of_paths<C>(g, cell, gen, fast, lr, offs);
            for (int corner = 0; corner < 8; ++corner) {
                ++n_far;
                if (gen[corner] >= g.rows) { ++gen_over; if (gen[corner] > gen_max) gen_max = gen[corner]; }
                if (fast[corner] >= g.rows) ++fast_over;
                if ((uint64_t)offs[corner] + C * 4 > table_bytes) ++fast_out;
                if (lr[corner] >= g.rows) ++lr_over;
            }
        }
        printf("%u %u %u %u %llu %llu %llu %llu %llu %llu %llu %llu\n", l, g.flags, g.rows, res, (unsigned long long)n_in,
               (unsigned long long)disagree, (unsigned long long)n_far, (unsigned long long)gen_over, (unsigned long long)gen_max,
               (unsigned long long)fast_over, (unsigned long long)lr_over, (unsigned long long)fast_out);
        if (disagree) bad = 1;
    }
    return bad;
}

int main(int argc, char** argv) {
    if (argc < 6) return 2;
    const int C = atoi(argv[1]);
    const float S = strtof(argv[2], nullptr);
    const uint32_t H = (uint32_t)atoi(argv[3]);
    std::vector<int32_t> off;
    for (int i = 4; i < argc; ++i) off.push_back((int32_t)strtol(argv[i], nullptr, 10));
    switch (C) {
        case 2: return sweep<2>(off, S, H);
        case 4: return sweep<4>(off, S, H);
        case 8: return sweep<8>(off, S, H);
        default: return 2;
    }
}
