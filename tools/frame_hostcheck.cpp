// frame_hostcheck.cpp -- the per-output arithmetic of the frame (csrc/frame_dev.h) under a host compiler and its sanitizers
// (tests/test_frame_cpu.py builds this with -fsanitize=address,undefined -ffp-contract=off and runs it; it never runs on a GPU).
//
//   frame_hostcheck cases.bin
//
// cases.bin (written by the test, little-endian): uint32 ncases; per case int32 Hs, Ws, Hc, Wc, Ty, Tx, orientation; the tables ystart[Hc],
// ycount[Hc] (int32), yw[Hc * Ty] (float32), xstart[Wc], xcount[Wc], xw[Tx * Wc] (tap-major, as the entry point takes it); 3 x Hs x Ws float32, the planes; 3 x Ho x Wo float32, the
// expected UPRIGHT resampled planes (tests/frame_ref.py; Ho x Wo is Hc x Wc, swapped for orientation >= 5).
// 1. every output of every plane of every case evaluates to the expected bits at the place the orientation gives it;
// 2. 6000 single-field corruptions of the cases' valid tables from a fixed seed (a start far outside the plane, a negative or huge count, a
//    NaN, infinite or huge weight): the corrupted output and a few others are evaluated.  With a start or a count corrupted the result
//    must be finite and within 4 times the plane's largest value (the clamps keep the taps inside the plane resp. the workspace column and the weights inside their
//    row: sum |w| of a row is below 2 per axis); with a weight corrupted only the accesses are checked.
// Every plane and every table is a heap allocation of its exact size, so any access outside one stops the program under AddressSanitizer.
// Prints one line per stage and "hostcheck OK"; exit status 0 only then.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../eld_amd/csrc/frame_dev.h"

namespace {

struct Case {
    int32_t Hs, Ws, Hc, Wc, Ty, Tx, o;
    int row0, rows;                                                  // the source rows the valid vertical table uses, as the caller of the kernels takes them
    std::vector<int32_t> ystart, ycount, xstart, xcount;
    std::vector<float> yw, xw, in, expect;
};

bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

template <class T>
bool read_vec(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return read_exact(f, v.data(), n * sizeof(T));
}

uint32_t bits(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}

// an exact-size heap copy
template <class T>
T* heap_copy(const T* src, size_t n) {
    T* p = (T*)malloc(n * sizeof(T));
    memcpy(p, src, n * sizeof(T));
    return p;
}

struct Tables {                                                      // exact-size heap copies of a case's six tables
    int32_t *ystart, *ycount, *xstart, *xcount;
    float *yw, *xw;
    explicit Tables(const Case& c)
        : ystart(heap_copy(c.ystart.data(), c.ystart.size())), ycount(heap_copy(c.ycount.data(), c.ycount.size())),
          xstart(heap_copy(c.xstart.data(), c.xstart.size())), xcount(heap_copy(c.xcount.data(), c.xcount.size())),
          yw(heap_copy(c.yw.data(), c.yw.size())), xw(heap_copy(c.xw.data(), c.xw.size())) {}
    ~Tables() {
        free(ystart); free(ycount); free(xstart); free(xcount); free(yw); free(xw);
    }
    Tables(const Tables&) = delete;
    Tables& operator=(const Tables&) = delete;
};

float eval(const Case& c, const Tables& t, const float* plane, int i, int j) {
    return frame_eval(plane, c.Hs, c.Ws, i, j, t.ystart, t.ycount, t.yw, c.Ty, t.xstart, t.xcount, t.xw, c.Tx, c.Wc, c.row0, c.rows);
}

uint32_t rng_state = 2018u;
uint32_t rnd() {                                                     // xorshift32
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return rng_state;
}

int32_t nasty_int() {
    static const int32_t v[] = {-1, 0, -4096, 4097, 1 << 20, -(1 << 20), std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::min(),
                                std::numeric_limits<int32_t>::max() - 3, std::numeric_limits<int32_t>::min() + 5, 65536, -65537};
    const uint32_t n = sizeof(v) / sizeof(v[0]);
    const uint32_t k = rnd() % (n + 1u);
    return k < n ? v[k] : (int32_t)rnd();
}

float nasty_float() {
    static const float v[] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(),
                              3e38f, -3e38f, 1e-45f, -0.0f, 1e20f};
    return v[rnd() % (sizeof(v) / sizeof(v[0]))];
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: frame_hostcheck cases.bin\n");
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
        int32_t h[7];
        if (!read_exact(f, h, sizeof(h))) return 2;
        c.Hs = h[0]; c.Ws = h[1]; c.Hc = h[2]; c.Wc = h[3]; c.Ty = h[4]; c.Tx = h[5]; c.o = h[6];
        for (int k = 0; k < 4; ++k)
            if (h[k] < 1 || h[k] > 4096) return 2;
        if (c.Ty < 1 || c.Ty > FRAME_MAX_TAPS || c.Tx < 1 || c.Tx > FRAME_MAX_TAPS || c.o < 1 || c.o > 8) return 2;
        const size_t nin = 3 * (size_t)c.Hs * c.Ws, nout = 3 * (size_t)c.Hc * c.Wc;
        if (!read_vec(f, c.ystart, c.Hc) || !read_vec(f, c.ycount, c.Hc) || !read_vec(f, c.yw, (size_t)c.Hc * c.Ty) || !read_vec(f, c.xstart, c.Wc) ||
            !read_vec(f, c.xcount, c.Wc) || !read_vec(f, c.xw, (size_t)c.Wc * c.Tx) || !read_vec(f, c.in, nin) || !read_vec(f, c.expect, nout))
            return 2;
        int lo = c.ystart[0], hi = c.ystart[0] + c.ycount[0];
        for (int i = 1; i < c.Hc; ++i) {
            lo = c.ystart[i] < lo ? c.ystart[i] : lo;
            hi = c.ystart[i] + c.ycount[i] > hi ? c.ystart[i] + c.ycount[i] : hi;
        }
        if (lo < 0 || hi > c.Hs || hi <= lo) return 2;
        c.row0 = lo;
        c.rows = hi - lo;
    }
    fclose(f);
    // 1. the expected values, at the place the orientation gives them
    size_t nvals = 0;
    for (size_t ci = 0; ci < cases.size(); ++ci) {
        const Case& c = cases[ci];
        const Tables t(c);
        const int Ho = frame_transposed(c.o) ? c.Wc : c.Hc, Wo = frame_transposed(c.o) ? c.Hc : c.Wc;
        std::vector<char> seen((size_t)Ho * Wo, 0);
        for (int ch = 0; ch < 3; ++ch) {
            float* p = heap_copy(c.in.data() + (size_t)ch * c.Hs * c.Ws, (size_t)c.Hs * c.Ws);
            for (int i = 0; i < c.Hc; ++i)
                for (int j = 0; j < c.Wc; ++j) {
                    int Y = -1, X = -1;
                    frame_upright(c.o, i, j, c.Hc, c.Wc, &Y, &X);
                    if (Y < 0 || Y >= Ho || X < 0 || X >= Wo) {
                        printf("case %zu: orientation %d sends (%d, %d) to (%d, %d), outside %d x %d\n", ci, c.o, i, j, Y, X, Ho, Wo);
                        return 1;
                    }
                    if (ch == 0 && seen[(size_t)Y * Wo + X]++) {
                        printf("case %zu: orientation %d sends two pixels to (%d, %d)\n", ci, c.o, Y, X);
                        return 1;
                    }
                    const float r = eval(c, t, p, i, j);
                    const float e = c.expect[((size_t)ch * Ho + Y) * Wo + X];
                    if (bits(r) != bits(e)) {
                        printf("case %zu plane %d output (%d, %d) -> upright (%d, %d): %.9g (%08x), expected %.9g (%08x)\n", ci, ch, i, j, Y, X, (double)r,
                               bits(r), (double)e, bits(e));
                        return 1;
                    }
                    ++nvals;
                }
            free(p);
        }
    }
    printf("%zu outputs of %zu cases: the expected bits\n", nvals, cases.size());
    // 2. single-field corruptions
    const int trials = 6000;
    int bounded = 0, weights = 0;
    for (int tr = 0; tr < trials; ++tr) {
        const Case& c = cases[rnd() % cases.size()];
        Tables t(c);
        const uint32_t field = rnd() % 6u;                            // ystart, ycount, yw, xstart, xcount, xw
        const int i = (int)(rnd() % (uint32_t)c.Hc), j = (int)(rnd() % (uint32_t)c.Wc);
        long long put_i = 0;
        float put_f = 0.f;
        switch (field) {
        case 0: t.ystart[i] = (int32_t)(put_i = nasty_int()); break;
        case 1: t.ycount[i] = (int32_t)(put_i = nasty_int()); break;
        case 2: t.yw[(size_t)i * c.Ty + rnd() % (uint32_t)c.Ty] = put_f = nasty_float(); break;
        case 3: t.xstart[j] = (int32_t)(put_i = nasty_int()); break;
        case 4: t.xcount[j] = (int32_t)(put_i = nasty_int()); break;
        default: t.xw[(size_t)j * c.Tx + rnd() % (uint32_t)c.Tx] = put_f = nasty_float(); break;
        }
        const bool weight = field == 2u || field == 5u;
        for (int ch = 0; ch < 3; ++ch) {
            const size_t n = (size_t)c.Hs * c.Ws;
            float* p = heap_copy(c.in.data() + (size_t)ch * n, n);
            float big = 0.f;
            for (size_t q = 0; q < n; ++q) big = fabsf(p[q]) > big ? fabsf(p[q]) : big;
            for (int k = 0; k < 4; ++k) {
                const int ii = k == 0 ? i : (k == 1 ? 0 : (k == 2 ? c.Hc - 1 : (int)(rnd() % (uint32_t)c.Hc)));
                const int jj = k == 0 ? j : (k == 1 ? 0 : (k == 2 ? c.Wc - 1 : (int)(rnd() % (uint32_t)c.Wc)));
                const float r = eval(c, t, p, ii, jj);
                if (weight) {
                    ++weights;
                    continue;
                }
                if (!(fabsf(r) <= 4.f * big)) {                      // false for NaN and inf
                    printf("corruption %d (field %u = %lld) of output (%d, %d): plane %d output (%d, %d) gives %.9g, the plane's values are within %.9g\n",
                           tr, field, put_i, i, j, ch, ii, jj, (double)r, (double)big);
                    return 1;
                }
                ++bounded;
            }
            free(p);
        }
        (void)put_f;
    }
    printf("%d single-field corruptions: %d results with a corrupt start or count finite and bounded, %d evaluated through a corrupt weight\n", trials,
           bounded, weights);
    printf("hostcheck OK\n");
    return 0;
}
