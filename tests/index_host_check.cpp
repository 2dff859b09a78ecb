// index_host_check.cpp -- the host-compilable parts of csrc/octree_build.hpp and csrc/bulk_grid.hpp, the very functions the kernels
// call, as a stand-alone program for tests/test_index_host_cpu.py (which also runs it under the address and undefined-behaviour
// sanitizers).  It prints; the test compares with the numpy oracles.
//     index_host_check level F ...                               -> "F level_of(F) max_nodes(F)" per F
//     index_host_check morton x y z [x y z ...]                  -> the Morton code of each cell
//     index_host_check solve lo_x lo_y lo_z hi_x hi_y hi_z m b   -> "Rx Ry Rz ncells hx hy hz" of the grid over that bulk of m points, budget b
//     index_host_check search x v0 v1 ...                        -> lower_bound of x in the sorted v, and up256(x)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../nicer_slam_amd/csrc/bulk_grid.hpp"
#include "../nicer_slam_amd/csrc/octree_build.hpp"

int main(int argc, char** argv) {
    using namespace nsa;
    if (argc < 3) return 2;
    const char* what = argv[1];
    if (!strcmp(what, "level")) {
        for (int i = 2; i < argc; ++i) {
            const uint32_t F = (uint32_t)strtoull(argv[i], nullptr, 10);
            printf("%u %u %llu\n", F, octree::level_of(F), (unsigned long long)octree::max_nodes(F));
        }
    } else if (!strcmp(what, "morton") && (argc - 2) % 3 == 0) {
        for (int i = 2; i < argc; i += 3) {
            const uint32_t cell[3] = {(uint32_t)atoi(argv[i]), (uint32_t)atoi(argv[i + 1]), (uint32_t)atoi(argv[i + 2])};
            printf("%u\n", octree::morton3(cell));
        }
    } else if (!strcmp(what, "solve") && argc == 10) {
        float lo[3], hi[3];
        for (int k = 0; k < 3; ++k) {
            lo[k] = strtof(argv[2 + k], nullptr);
            hi[k] = strtof(argv[5 + k], nullptr);
        }
        bulk::Grid g;
        bulk::solve(lo, hi, (uint32_t)atoi(argv[8]), (uint32_t)atoi(argv[9]), g);
        printf("%u %u %u %u %.9g %.9g %.9g\n", g.R[0], g.R[1], g.R[2], g.ncells, g.h[0], g.h[1], g.h[2]);
    } else if (!strcmp(what, "search")) {
        std::vector<uint32_t> v;
        for (int i = 3; i < argc; ++i) v.push_back((uint32_t)strtoul(argv[i], nullptr, 10));
        const uint32_t x = (uint32_t)strtoul(argv[2], nullptr, 10);
        printf("%u %llu\n", bulk::lower_bound(v.data(), (uint32_t)v.size(), x), (unsigned long long)bulk::up256(x));
    } else {
        return 2;
    }
    return 0;
}
