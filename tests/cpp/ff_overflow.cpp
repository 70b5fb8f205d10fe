// The column accumulators of snarkvm_amd/csrc/ff.hip.h on the host, over operands chosen as internal 29-bit limb patterns, in a program of its
// own so that it can be built with -fsanitize=signed-integer-overflow,shift -fno-sanitize-recover.  What the sanitizer ends the run for: a
// column sum of diff_of_products that leaves its SIGNED 64-bit accumulator, and any shift that loses a sign.  operator*, sqr and
// sum_of_products accumulate in uint64_t, whose wrap-around the sanitizer does not report: for those three only the comparisons below stand
// guard (a wrapped column gives a wrong limb).  The comparisons hold the header's routines against EACH OTHER (sqr against *, diff_of_products
// against * and -, sum_of_products<6> against six sum_of_products<1>), so an error common to both sides passes here; the exact references
// are the Python-integer tests of tests/test_field_limb_edges_host.py.
//   ff_overflow <file>    file: u32 n_fr, n_fr * 8 words, u32 n_fq, n_fq * 12 words - memory images (tests/test_field_overflow_host.py writes it)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "ff.hip.h"

using namespace sv;

template <class F>
static std::vector<F> read_list(FILE* f) {
    uint32_t n = 0;
    if (fread(&n, 4, 1, f) != 1 || n == 0 || n > 4096) exit(2);
    std::vector<F> v(n);
    for (uint32_t i = 0; i < n; i++) {
        uint32_t w[F::WORDS];
        if (fread(w, 4, F::WORDS, f) != (size_t)F::WORDS) exit(2);
        v[i] = F::from_raw_words(w);
    }
    return v;
}
static int fail(const char* what, size_t i, size_t j) {
    fprintf(stderr, "FAIL %s at pair (%zu, %zu)\n", what, i, j);
    return 1;
}
template <class F>
static int pairs(const std::vector<F>& v, const char* name) {
    const size_t n = v.size();
    for (size_t i = 0; i < n; i++) {
        if (v[i].sqr() != v[i] * v[i]) return fail("sqr", i, i);
        for (size_t j = 0; j < n; j++) {
            const F &a = v[i], &b = v[j], &c = v[(i + 3 * j + 1) % n], &d = v[(7 * i + j + 2) % n];
            const F ab = a * b;
            if (ab != b * a) return fail("mul", i, j);
            if (F::diff_of_products(a, b, c, d) != ab - c * d) return fail("diff_of_products", i, j);
            if (!F::diff_of_products(a, b, b, a).is_zero()) return fail("diff_of_products = 0", i, j);
            if (F::diff_of_products(F::zero(), F::zero(), a, b) != ab.neg()) return fail("diff_of_products < 0", i, j);
        }
    }
    printf("%s: %zu elements, %zu pairs\n", name, n, n * n);
    return 0;
}
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<fr_t> fr = read_list<fr_t>(f);
    const std::vector<fq_t> fq = read_list<fq_t>(f);
    fclose(f);
    if (pairs(fr, "fr") || pairs(fq, "fq")) return 1;
    // Fr sum_of_products<6>: six canonical a against six b, canonical ones and the largest the routine admits (2^256 - 1: every limb full, 24 bits on top)
    fr_t big;
    for (int i = 0; i < 9; i++) big.v[i] = (i == 8) ? 0x00ffffffu : LIMB_MASK;
    const size_t n = fr.size();
    for (size_t i = 0; i < n; i++)
        for (size_t j = 0; j < n; j++) {
            fr_t a[6], b[6], want = fr_t::zero();
            for (int g = 0; g < 6; g++) {
                a[g] = fr[(i + g * (j + 1)) % n];
                b[g] = (j % 3 == 2) ? big : fr[(j + g * (i + 1)) % n];
                want = want + fr_t::sum_of_products<1>(&a[g], &b[g]);
            }
            if (fr_t::sum_of_products<6>(a, b) != want) return fail("sum_of_products<6>", i, j);
        }
    {  // the extreme column: six times the largest canonical value against the largest admitted one
        fr_t a[6], b[6], want = fr_t::zero();
        fr_t pm1 = fr_t::from_table(FrP::MOD);
        pm1.v[0] -= 1;
        for (int k = 0; k < 6; k++) a[k] = pm1, b[k] = big, want = want + fr_t::sum_of_products<1>(&a[k], &b[k]);
        if (fr_t::sum_of_products<6>(a, b) != want) return fail("sum_of_products<6> extreme", 0, 0);
    }
    printf("fr: sum_of_products<6> on %zu operand sets\nOK\n", n * n + 1);
    return 0;
}
