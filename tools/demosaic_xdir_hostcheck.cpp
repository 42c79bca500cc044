// demosaic_xdir_hostcheck.cpp -- the per-site arithmetic of csrc/demosaic_xdir_dev.h under a host compiler and its sanitizers
// (tests/test_demosaic_xdir_cpu.py builds this with -fsanitize=address,undefined -ffp-contract=off and runs it; it never runs on a GPU).
//
//   demosaic_xdir_hostcheck cases.bin
//
// cases.bin (written by the test, little-endian): uint32 ncases; per case uint32 H, W (mosaic sides, multiples of 6, >= 6);
// H x W float32, the X-Trans mosaic v after gain and clamp; 3 x H x W float32, the expected camera RGB (tests/demosaic_xdir_ref.py).
// 1. xdir_ext_row / xdir_ext_col for every side 6 .. 30 and every index -6 .. side + 5: inside, and the site's phase colour is kept;
// 2. every case goes through the four stages the way the kernel's tile does -- v on the frame + 6 through the extension, G0 on the frame + 5,
//    d_h and d_v on the frame + 3, G^ written over G0 at the R and B sites of the frame + 2, the output on the frame -- and every value must
//    have the expected bits, sampled values included;
// 3. the first case's output is printed as hexadecimal words, plane by plane, one row per line, for a comparison outside this program.
// Every image is a heap allocation of its exact size, so any read outside it stops the program under AddressSanitizer.
// Prints one line per stage and "hostcheck OK"; exit status 0 only then.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../eld_amd/csrc/demosaic_xdir_dev.h"

namespace {

struct Case {
    uint32_t H, W;
    std::vector<float> v, expect;
};

bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

uint32_t bits(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}

float* image(size_t rows, size_t cols, float fill) {              // an exact-size heap allocation
    float* p = (float*)malloc(rows * cols * sizeof(float));
    for (size_t i = 0; i < rows * cols; ++i) p[i] = fill;
    return p;
}

int phase(int y, int x) { return 6 * ((y + 6) % 6) + (x + 6) % 6; }           // y, x >= -6: the extension keeps the periodic colour map

// the four stages over one frame; out: 3 x H x W
void demosaic(const Case& c, std::vector<float>& out) {
    const int H = (int)c.H, W = (int)c.W;
    const int vp = W + 2 * XDIR_HALO, gp = W + 10, dp = W + 6;
    const float nan = std::numeric_limits<float>::quiet_NaN();
    float* V = image(H + 2 * XDIR_HALO, vp, nan);
    float* G = image(H + 10, gp, nan);
    float* DH = image(H + 6, dp, nan);
    float* DV = image(H + 6, dp, nan);
    for (int y = -6; y < H + 6; ++y)
        for (int x = -6; x < W + 6; ++x) V[(y + 6) * vp + x + 6] = c.v[(size_t)xdir_ext_row(y, H) * W + xdir_ext_col(x, W)];
    for (int y = -5; y < H + 5; ++y)
        for (int x = -5; x < W + 5; ++x) {
            const float* s = V + (y + 6) * vp + x + 6;
            const int ph = phase(y, x);
            G[(y + 5) * gp + x + 5] = XT.colour[ph] == 1 ? s[0] : xdir_green0(s, vp, ph);
        }
    for (int y = -3; y < H + 3; ++y)
        for (int x = -3; x < W + 3; ++x) xdir_grad(G + (y + 5) * gp + x + 5, gp, DH[(y + 3) * dp + x + 3], DV[(y + 3) * dp + x + 3]);
    for (int y = -2; y < H + 2; ++y)
        for (int x = -2; x < W + 2; ++x) {
            const int ph = phase(y, x);
            if (XT.colour[ph] != 1)
                G[(y + 5) * gp + x + 5] = xdir_green(V + (y + 6) * vp + x + 6, vp, DH + (y + 3) * dp + x + 3, DV + (y + 3) * dp + x + 3, dp, ph);
        }
    out.assign((size_t)3 * H * W, nan);
    const size_t hw = (size_t)H * W;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const float* s = V + (y + 6) * vp + x + 6;
            const float* g = G + (y + 5) * gp + x + 5;
            const int ph = phase(y, x), col = XT.colour[ph];
            const float gg = col == 1 ? s[0] : g[0];
            out[(size_t)y * W + x] = col == 0 ? s[0] : gg + xdir_chroma(s, vp, g, gp, ph, 0);
            out[hw + (size_t)y * W + x] = gg;
            out[2 * hw + (size_t)y * W + x] = col == 2 ? s[0] : gg + xdir_chroma(s, vp, g, gp, ph, 1);
        }
    free(V); free(G); free(DH); free(DV);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: demosaic_xdir_hostcheck cases.bin\n");
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
        if (!read_exact(f, &c.H, 4) || !read_exact(f, &c.W, 4)) return 2;
        if (c.H < 6 || c.W < 6 || c.H > 4096 || c.W > 4096 || c.H % 6 || c.W % 6) return 2;
        const size_t n = (size_t)c.H * c.W;
        c.v.resize(n);
        c.expect.resize(3 * n);
        if (!read_exact(f, c.v.data(), n * 4) || !read_exact(f, c.expect.data(), 3 * n * 4)) return 2;
    }
    fclose(f);
    // 1. the extension's index map
    int nidx = 0;
    for (int L = 6; L <= 30; L += 6)
        for (int i = -6; i < L + 6; ++i) {
            const int y = xdir_ext_row(i, L), x = xdir_ext_col(i, L);
            if (y < 0 || y >= L || x < 0 || x >= L) {
                printf("extension of index %d of %d sites: row %d, column %d\n", i, L, y, x);
                return 1;
            }
            for (int k = 0; k < 6; ++k)
                if (XT.colour[phase(y, k)] != XT.colour[phase(i, k)] || XT.colour[phase(k, x)] != XT.colour[phase(k, i)]) {
                    printf("extension of index %d of %d sites changes the colour: row %d, column %d\n", i, L, y, x);
                    return 1;
                }
            nidx += 2;
        }
    printf("%d extended indices: inside, colour kept\n", nidx);
    // 2. the expected values
    size_t nval = 0;
    std::vector<float> first;
    for (size_t i = 0; i < cases.size(); ++i) {
        const Case& c = cases[i];
        std::vector<float> out;
        demosaic(c, out);
        for (size_t k = 0; k < out.size(); ++k) {
            if (bits(out[k]) != bits(c.expect[k])) {
                const size_t hw = (size_t)c.H * c.W;
                printf("case %zu plane %zu site (%zu, %zu): %.9g (%08x), expected %.9g (%08x)\n", i, k / hw, (k % hw) / c.W, (k % hw) % c.W,
                       (double)out[k], bits(out[k]), (double)c.expect[k], bits(c.expect[k]));
                return 1;
            }
            ++nval;
        }
        if (i == 0) first = out;
    }
    printf("%zu values of %zu cases: the expected bits\n", nval, cases.size());
    // 3. the first case, for a comparison outside this program
    printf("frame %u %u\n", cases[0].H, cases[0].W);
    for (size_t k = 0; k < first.size(); ++k) printf("%08x%c", bits(first[k]), (k + 1) % cases[0].W == 0 ? '\n' : ' ');
    printf("hostcheck OK\n");
    return 0;
}
