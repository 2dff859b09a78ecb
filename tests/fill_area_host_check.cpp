// Host rehearsal of the minimum-area patches: the bodies of nicer_slam_amd/csrc/fill_area_passes.hpp -- the plan row, the row of a
// loop vertex, the chord mask with the start values, the cell minimum in both of the kernels' forms (one lane over all candidates;
// 64 lanes striding j and merging their pairs along the xor butterfly) and the store, the final class and one face by descent --
// compiled as host C++ and called one item at a time, the way the kernels of csrc/mesh_fill_area.hip call them, on the loops, the
// order and the sorted edges that the test hands over, with the scans made here.  Built and run by
// tests/test_mesh_fill_area_host_cpu.py:
//     c++ -O2 -std=c++17 -ffp-contract=off [-fsanitize=address,undefined -fno-sanitize-recover=all] fill_area_host_check.cpp
//     ./a.out CASE > RESULT
// CASE (text): V F B L E class_mask max_area_edges min_sin2_bits has_names / 3 V vertex words (fp32 bits) / 3 F indices / 3 F names
// when has_names / 2 E edge ends / B entries of order / 9 L loop integers.  RESULT: one line each of the plan totals, the final
// totals, the loops' area integers, the bits of their areas, the mask, the bits of W, J and the new faces in the plan's numbering,
// which the test compares with tests/fill_area_ref.py element for element.  Exit status 3: the two forms of a cell disagree.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../nicer_slam_amd/csrc/fill_area_passes.hpp"

using namespace nsa::fill_area;

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

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* fh = fopen(argv[1], "r");
    if (!fh) return 2;
    unsigned V, F, B, L, E, class_mask, cap, has_names;
    unsigned long long ms2_bits;
    if (fscanf(fh, "%u %u %u %u %u %u %u %llu %u", &V, &F, &B, &L, &E, &class_mask, &cap, &ms2_bits, &has_names) != 9) return 2;
    std::vector<unsigned> vbits(3 * (size_t)V);
    std::vector<int32_t> faces(3 * (size_t)F), names(has_names ? 3 * (size_t)F : 0), edges(2 * (size_t)E), order(B);
    std::vector<long long> lints((size_t)nsa::fill::kLoopInts * L);
    if (!read_all(fh, "%u", vbits) || !read_all(fh, "%d", faces) || !read_all(fh, "%d", names) || !read_all(fh, "%d", edges) ||
        !read_all(fh, "%d", order) || !read_all(fh, "%lld", lints))
        return 2;
    fclose(fh);
    std::vector<float> verts(vbits.size() + 1);
    if (!vbits.empty()) memcpy(verts.data(), vbits.data(), 4 * vbits.size());
    double min_sin2;
    memcpy(&min_sin2, &ms2_bits, 8);
    faces.push_back(-1);
    names.push_back(-1);
    edges.push_back(-1);
    order.push_back(-1);
    lints.push_back(0);
    static_assert(sizeof(long long) == sizeof(int64_t), "int64");
    const int64_t* loop_ints = reinterpret_cast<const int64_t*>(lints.data());
    const Shape m{verts.data(), nullptr, faces.data(), V, F};

    // the plan: one row per loop and the exclusive scans
    std::vector<int64_t> area_ints((size_t)kAreaInts * L + 1, 0);
    unsigned long long cells = 0, faces_plan = 0, rows = 0, selected = 0, tabled = 0, too_many = 0, max_n = 0;
    for (uint32_t l = 0; l < L; ++l) {
        uint64_t n = 0;
        const int64_t cls = plan_class(loop_ints, l, class_mask, cap, B, &n);
        int64_t* a = &area_ints[(size_t)kAreaInts * l];
        a[0] = cls;
        a[1] = loop_ints[(size_t)nsa::fill::kLoopInts * l + 1];
        a[2] = (int64_t)cells;
        a[3] = (int64_t)faces_plan;
        a[4] = (int64_t)rows;
        cells += n * n;
        faces_plan += n >= 3 ? n - 2 : 0;
        rows += n;
        selected += cls != kNotSelected;
        tabled += n != 0;
        too_many += cls == kAreaTooManyEdges;
        if (n > max_n) max_n = n;
    }
    const unsigned long long plan_totals[kPlanTotals] = {selected, tabled, too_many, cells, max_n, faces_plan, rows, 0};

    std::vector<double> W(cells + 1), WT(cells + 1), pos(3 * rows + 1), area(L + 1, 0.0);
    std::vector<int32_t> J(cells + 1), row_name(rows + 1), new_faces(3 * faces_plan + 1);
    std::vector<uint32_t> row_loop(rows + 1);
    std::vector<uint8_t> mask(cells + 1);
    const int32_t* nm = has_names ? names.data() : faces.data();
    for (uint64_t r = 0; r < rows; ++r)
        row_pass(m, nm, order.data(), B, loop_ints, area_ints.data(), L, cells, rows, r, row_loop.data(), row_name.data(), pos.data());
    for (uint64_t x = 0; x < cells; ++x)
        mask_pass(edges.data(), E, loop_ints, area_ints.data(), L, B, cells, rows, row_name.data(), x, mask.data(), W.data(), WT.data(),
                  J.data());
    for (uint32_t d = 2; d < max_n; ++d)
        for (uint64_t r = 0; r < rows; ++r) {
            Table t;
            uint64_t i;
            if (!cell_of(loop_ints, area_ints.data(), L, B, cells, rows, row_loop.data(), r, d, &t, &i)) continue;
            double best;
            uint32_t bj;
            cell_scan(W.data(), WT.data(), pos.data(), t, i, i + d, i + 1, 1, min_sin2, &best, &bj);
            double lb[64], nb[64];
            uint32_t lj[64], nj[64];
            for (uint32_t lane = 0; lane < 64; ++lane)
                cell_scan(W.data(), WT.data(), pos.data(), t, i, i + d, i + 1 + lane, 64, min_sin2, &lb[lane], &lj[lane]);
            for (uint32_t s = 32; s >= 1; s >>= 1) {
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    const bool take = beats(lb[lane ^ s], lj[lane ^ s], lb[lane], lj[lane]);
                    nb[lane] = take ? lb[lane ^ s] : lb[lane];
                    nj[lane] = take ? lj[lane ^ s] : lj[lane];
                }
                memcpy(lb, nb, sizeof lb);
                memcpy(lj, nj, sizeof lj);
            }
            if (memcmp(&lb[0], &best, 8) != 0 || lj[0] != bj) return 3;
            if (d - 1 >= kWaveCandidates) {
                best = lb[0];
                bj = lj[0];
            }
            cell_store(t, i, i + d, best, bj, mask.data(), W.data(), WT.data(), J.data());
        }
    unsigned long long fin[kFinalTotals] = {0, 0, 0, 0};
    for (uint32_t l = 0; l < L; ++l) {
        const int64_t cls = final_class(loop_ints, area_ints.data(), L, B, cells, rows, W.data(), l, &area[l]);
        area_ints[(size_t)kAreaInts * l + 5] = (int64_t)fin[3];
        if (cls == kAreaFilled) {
            ++fin[0];
            fin[3] += (unsigned long long)area_ints[(size_t)kAreaInts * l + 1] - 2;
        }
        fin[1] += cls == kAreaTooManyEdges;
        fin[2] += cls == kNoTriangulation;
    }
    for (uint32_t l = 0; l < L; ++l) {                          // (the classes change after every loop has read its own)
        double unused;
        area_ints[(size_t)kAreaInts * l] = final_class(loop_ints, area_ints.data(), L, B, cells, rows, W.data(), l, &unused);
    }
    for (uint64_t x = 0; x < faces_plan; ++x)
        emit_pass(m, order.data(), B, loop_ints, area_ints.data(), L, cells, rows, J.data(), faces_plan, x, new_faces.data());

    print_line("%llu ", plan_totals, (size_t)kPlanTotals);
    print_line("%llu ", fin, (size_t)kFinalTotals);
    std::vector<long long> ai(area_ints.begin(), area_ints.begin() + (size_t)kAreaInts * L);
    print_line("%lld ", ai.data(), ai.size());
    std::vector<unsigned long long> bits(L);
    if (L) memcpy(bits.data(), area.data(), 8 * (size_t)L);
    print_line("%llu ", bits.data(), bits.size());
    std::vector<unsigned> mk(mask.begin(), mask.begin() + cells);
    print_line("%u ", mk.data(), mk.size());
    bits.resize(cells);
    if (cells) memcpy(bits.data(), W.data(), 8 * (size_t)cells);
    print_line("%llu ", bits.data(), bits.size());
    print_line("%d ", J.data(), (size_t)cells);
    print_line("%d ", new_faces.data(), 3 * (size_t)faces_plan);
    return 0;
}
