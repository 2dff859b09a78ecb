// intersect_host_check.cpp -- csrc/intersect_passes.hpp as host C++, one item a line (tests/test_mesh_intersect_host_cpu.py).
//   w OP A B      A, B: 64 hex digits (256 bits, two's complement); OP add | sub | mul  ->  the result in hex and its sign
//   c BITS E      the fp32 with these bits over 2^E                                      ->  hex
//   f 9 WORDS     a face as fp32 bit patterns                                            ->  face_collinear
//   p 18 WORDS    two faces                                                              ->  code s stage, and the code of stage 2 alone
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../nicer_slam_amd/csrc/intersect_passes.hpp"

using namespace nsa::isect;

static Wide parse(const char* hex) {
    Wide r = wide_zero();
    const size_t n = strlen(hex);
    for (size_t i = 0; i < n && i < 64; ++i) {
        const char ch = hex[n - 1 - i];
        const uint32_t d = ch <= '9' ? ch - '0' : (ch | 32) - 'a' + 10;
        r.w[i / 8] |= (d & 15u) << (4 * (i % 8));
    }
    return r;
}

static void show(const Wide& a) {
    for (int k = kLimbs - 1; k >= 0; --k) printf("%08x", a.w[k]);
}

static float of_bits(uint32_t b) {
    float x;
    memcpy(&x, &b, 4);
    return x;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* fh = fopen(argv[1], "r");
    if (!fh) return 2;
    char kind[8], op[8], x[80], y[80];
    while (fscanf(fh, "%7s", kind) == 1) {
        if (kind[0] == 'w') {
            if (fscanf(fh, "%7s %79s %79s", op, x, y) != 3) return 3;
            const Wide a = parse(x), b = parse(y);
            const Wide r = op[0] == 'a' ? wide_add(a, b) : (op[0] == 's' ? wide_sub(a, b) : wide_mul(a, b));
            show(r);
            printf(" %d\n", wide_sign(r));
        } else if (kind[0] == 'c') {
            unsigned bits;
            int E;
            if (fscanf(fh, "%u %d", &bits, &E) != 2) return 3;
            show(wide_of(of_bits(bits), E));
            printf("\n");
        } else if (kind[0] == 'f') {
            float a[3][3];
            for (int k = 0; k < 9; ++k) {
                unsigned bits;
                if (fscanf(fh, "%u", &bits) != 1) return 3;
                a[k / 3][k % 3] = of_bits(bits);
            }
            printf("%d\n", face_collinear(a));
        } else if (kind[0] == 'p') {
            float a[3][3], b[3][3];
            for (int k = 0; k < 18; ++k) {
                unsigned bits;
                if (fscanf(fh, "%u", &bits) != 1) return 3;
                if (k < 9) a[k / 3][k % 3] = of_bits(bits);
                else b[(k - 9) / 3][k % 3] = of_bits(bits);
            }
            int s, stage, stage2;
            const uint32_t code = pair_code(a, b, s, stage);
            bool sha[3], shb[3];
            const int s2 = shared_positions(a, b, sha, shb);
            const uint32_t code2 = s2 == 3 ? code_of(kProper, true, 3) : pair_exact(a, b, sha, shb, s2, stage2);
            printf("%u %d %d %u\n", code, s, stage, code2);
        } else {
            return 3;
        }
    }
    fclose(fh);
    return 0;
}
