// warp_hostcheck.cpp -- the per-pixel WarpRectilinear arithmetic of csrc/warp_dev.h under a host compiler and its sanitizers
// (tests/test_warp_cpu.py builds this with -fsanitize=address,undefined -ffp-contract=off and runs it; it never runs on a GPU).
//
//   warp_hostcheck cases.bin
//
// cases.bin (written by the test, little-endian): uint32 ncases; per case uint32 Hm, Wm; one EldWarp record (184 bytes); 3 x Hm x Wm float32,
// the planes; 3 x Hm x Wm float32, the expected resampled planes (tests/warp_ref.py).
// 1. every pixel of every plane of every case evaluates to the expected bits;
// 2. 4000 single-field corruptions of the cases' valid records from a fixed seed (nsets, one of the 18 coefficients, cxp, cyp, m, m2 set
//    to NaN, +-inf, +-1e300, a denormal, a centre far outside the image, ...): a handful of pixels of each plane are evaluated; every result
//    must be finite and within the Catmull-Rom bound of the plane's values (sum |w| <= 1.25 per axis), and a NaN in a field the pixel's set
//    uses must give the plane's first pixel (both coordinates become -1: the replicated corner).
// Every plane is a heap allocation of its exact size, so any read outside it stops the program under AddressSanitizer.
// Prints one line per stage and "hostcheck OK"; exit status 0 only then.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../eld_amd/csrc/warp_dev.h"

namespace {

struct Case {
    uint32_t Hm, Wm;
    EldWarp w;
    std::vector<float> in, expect;
};

bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

uint32_t bits(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}

// plane c of the case as an exact-size heap copy
float* plane_copy(const Case& c, int ch) {
    const size_t n = (size_t)c.Hm * c.Wm;
    float* p = (float*)malloc(n * sizeof(float));
    memcpy(p, c.in.data() + (size_t)ch * n, n * sizeof(float));
    return p;
}

uint32_t rng_state = 2018u;
uint32_t rnd() {                                                     // xorshift32
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return rng_state;
}

double nasty_double(const Case& c) {
    static const double v[] = {0.0, -0.0, 1e300, -1e300, 1e-300, 4.9406564584124654e-324, -2.2250738585072009e-308,
                               std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(),
                               -std::numeric_limits<double>::infinity(), 0.5, -3.0, 1e9, -1e9, 1e18, 2147483648.0, -2147483649.0};
    const uint32_t n = sizeof(v) / sizeof(v[0]);
    const uint32_t k = rnd() % (n + 2u);
    if (k < n) return v[k];
    if (k == n) return (double)c.Wm * 1e6 * ((rnd() & 1u) ? 1.0 : -1.0);                          // a centre far outside the image
    return ((double)(rnd() % 2001u) - 1000.0) * 0.01;
}

}  // namespace

int main(int argc, char** argv) {
    static_assert(sizeof(EldWarp) == 184, "the record the test writes");
    if (argc != 2) {
        fprintf(stderr, "usage: warp_hostcheck cases.bin\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    uint32_t ncases = 0;
    if (!read_exact(f, &ncases, 4) || ncases < 1 || ncases > 64) return 2;
    std::vector<Case> cases(ncases);
    for (auto& c : cases) {
        if (!read_exact(f, &c.Hm, 4) || !read_exact(f, &c.Wm, 4) || c.Hm < 1 || c.Wm < 1 || c.Hm > 4096 || c.Wm > 4096) return 2;
        const size_t n = 3 * (size_t)c.Hm * c.Wm;
        c.in.resize(n);
        c.expect.resize(n);
        if (!read_exact(f, &c.w, sizeof(EldWarp)) || !read_exact(f, c.in.data(), n * 4) || !read_exact(f, c.expect.data(), n * 4)) return 2;
    }
    fclose(f);
    // 1. the expected values
    size_t npix = 0;
    for (size_t i = 0; i < cases.size(); ++i) {
        const Case& c = cases[i];
        if (!warp_record_ok(c.w)) {
            printf("case %zu: the test's own record is refused\n", i);
            return 1;
        }
        for (int ch = 0; ch < 3; ++ch) {
            float* p = plane_copy(c, ch);
            for (int y = 0; y < (int)c.Hm; ++y)
                for (int x = 0; x < (int)c.Wm; ++x) {
                    const float r = warp_eval(c.w, p, ch, (int)c.Hm, (int)c.Wm, y, x);
                    const float e = c.expect[((size_t)ch * c.Hm + y) * c.Wm + x];
                    if (bits(r) != bits(e)) {
                        printf("case %zu plane %d pixel (%d, %d): %.9g (%08x), expected %.9g (%08x)\n", i, ch, y, x, (double)r, bits(r), (double)e,
                               bits(e));
                        return 1;
                    }
                    ++npix;
                }
            free(p);
        }
    }
    printf("%zu pixels of %zu cases: the expected bits\n", npix, cases.size());
    // 2. single-field corruptions
    const int trials = 4000;
    int refused = 0, corner = 0;
    for (int t = 0; t < trials; ++t) {
        const Case& c = cases[rnd() % cases.size()];
        EldWarp w = c.w;
        const uint32_t field = rnd() % 23u;                           // nsets, 18 coefficients, cxp, cyp, m, m2
        double put = 0.0;
        if (field == 0u) {
            static const int32_t ns[] = {0, -1, 2, 4, 1, 3, std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::min()};
            w.nsets = ns[rnd() % 8u];
        } else {
            put = nasty_double(c);
            if (field <= 18u) w.k[(field - 1u) / 6u][(field - 1u) % 6u] = put;
            else (field == 19u ? w.cxp : field == 20u ? w.cyp : field == 21u ? w.m : w.m2) = put;
        }
        refused += !warp_record_ok(w);
        for (int ch = 0; ch < 3; ++ch) {
            float* p = plane_copy(c, ch);
            const size_t n = (size_t)c.Hm * c.Wm;
            float big = 0.f;
            for (size_t i = 0; i < n; ++i) big = fabsf(p[i]) > big ? fabsf(p[i]) : big;
            const int set = w.nsets == 3 ? ch : 0;
            const bool used = field >= 19u || (field >= 1u && (int)((field - 1u) / 6u) == set);
            for (int k = 0; k < 6; ++k) {
                int y, x;
                if (k == 0) { y = 0; x = 0; }
                else if (k == 1) { y = (int)c.Hm - 1; x = (int)c.Wm - 1; }
                else { y = (int)(rnd() % c.Hm); x = (int)(rnd() % c.Wm); }
                const float r = warp_eval(w, p, ch, (int)c.Hm, (int)c.Wm, y, x);
                if (!(fabsf(r) <= 1.5626f * big)) {                   // 1.25 * 1.25 and the roundings of 20 operations; false for NaN and inf
                    printf("corruption %d (field %u = %g): plane %d pixel (%d, %d) gives %.9g, the plane's values are within %.9g\n", t, field, put,
                           ch, y, x, (double)r, (double)big);
                    return 1;
                }
                if (used && put != put) {
                    if (bits(r) != bits(p[0])) {
                        printf("corruption %d (field %u = NaN): plane %d pixel (%d, %d) gives %.9g, not the first pixel %.9g\n", t, field, ch, y, x,
                               (double)r, (double)p[0]);
                        return 1;
                    }
                    ++corner;
                }
            }
            free(p);
        }
    }
    printf("%d single-field corruptions: %d refused by warp_record_ok, every result finite and bounded, %d NaN results at the corner\n", trials, refused,
           corner);
    printf("hostcheck OK\n");
    return 0;
}
