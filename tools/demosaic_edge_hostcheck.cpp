// demosaic_edge_hostcheck.cpp -- the per-site arithmetic of csrc/demosaic_edge_dev.h under a host compiler and its sanitizers
// (tests/test_demosaic_edge_cpu.py builds this with -fsanitize=address,undefined -ffp-contract=off and runs it; it never runs on a GPU).
//
//   demosaic_edge_hostcheck cases.bin
//
// cases.bin (written by the test, little-endian): uint32 ncases; per case uint32 H, W (mosaic sides, even, >= 2); int32 raw_pattern[4];
// H x W float32, the mosaic v after gain and clamp; 3 x H x W float32, the expected camera RGB (tests/demosaic_edge_ref.py).
// 1. edge_reflect against a walk of the reflected sequence, for every length 2 .. 9 and every index -40 .. 40: inside, parity kept;
// 2. every case goes through the four stages the way the kernel's tile does -- v on the frame + 4 through edge_reflect, d_h and d_v on the
//    frame + 2, G^ at the R and B sites of the frame + 1 (the other sites hold NaN: a read of one shows in the bits), the output on the frame --
//    and every value must have the expected bits, sampled values included;
// 3. the first case's output is printed as hexadecimal words, plane by plane, one row per line, for a comparison outside this program.
// Every image is a heap allocation of its exact size, so any read outside it stops the program under AddressSanitizer.
// Prints one line per stage and "hostcheck OK"; exit status 0 only then.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../eld_amd/csrc/demosaic_edge_dev.h"

namespace {

struct Case {
    uint32_t H, W;
    int32_t pat[4];
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

// the four stages over one frame; out: 3 x H x W
void demosaic(const Case& c, std::vector<float>& out) {
    const int H = (int)c.H, W = (int)c.W;
    const int vp = W + 2 * EDGE_HALO, dp = W + 4, gp = W + 2;
    const float nan = std::numeric_limits<float>::quiet_NaN();
    float* V = image(H + 2 * EDGE_HALO, vp, nan);
    float* DH = image(H + 4, dp, nan);
    float* DV = image(H + 4, dp, nan);
    float* G = image(H + 2, gp, nan);
    for (int y = -EDGE_HALO; y < H + EDGE_HALO; ++y)
        for (int x = -EDGE_HALO; x < W + EDGE_HALO; ++x)
            V[(y + EDGE_HALO) * vp + x + EDGE_HALO] = c.v[(size_t)edge_reflect(y, H) * W + edge_reflect(x, W)];
    for (int y = -2; y < H + 2; ++y)
        for (int x = -2; x < W + 2; ++x)
            edge_grad(V + (y + EDGE_HALO) * vp + x + EDGE_HALO, vp, DH[(y + 2) * dp + x + 2], DV[(y + 2) * dp + x + 2]);
    const bool g00 = (c.pat[0] & 1) != 0;
    int r_row = 0;
    for (int k = 0; k < 4; ++k)
        if (c.pat[k] == 0) r_row = k >> 1;
    auto is_g = [&](int y, int x) { return ((((y ^ x) & 1) == 0) == g00); };      // the extension keeps parity: also outside the frame
    for (int y = -1; y < H + 1; ++y)
        for (int x = -1; x < W + 1; ++x)
            if (!is_g(y, x))
                G[(y + 1) * gp + x + 1] = edge_green(V + (y + EDGE_HALO) * vp + x + EDGE_HALO, vp, DH + (y + 2) * dp + x + 2, DV + (y + 2) * dp + x + 2, dp);
    out.assign((size_t)3 * H * W, nan);
    const size_t hw = (size_t)H * W;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const float* cc = V + (y + EDGE_HALO) * vp + x + EDGE_HALO;
            const float* g = G + (y + 1) * gp + x + 1;
            const bool r_in_row = r_row == (y & 1);
            float r, gg, b;
            if (is_g(y, x)) {
                float hor, ver;
                edge_rb_at_g(cc, vp, g, gp, hor, ver);
                gg = cc[0];
                r = r_in_row ? hor : ver;
                b = r_in_row ? ver : hor;
            } else {
                const float other = edge_other_at_rb(cc, vp, g, gp);
                gg = g[0];
                r = r_in_row ? cc[0] : other;
                b = r_in_row ? other : cc[0];
            }
            out[(size_t)y * W + x] = r;
            out[hw + (size_t)y * W + x] = gg;
            out[2 * hw + (size_t)y * W + x] = b;
        }
    free(V); free(DH); free(DV); free(G);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: demosaic_edge_hostcheck cases.bin\n");
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
        if (!read_exact(f, &c.H, 4) || !read_exact(f, &c.W, 4) || !read_exact(f, c.pat, 16)) return 2;
        if (c.H < 2 || c.W < 2 || c.H > 4096 || c.W > 4096 || (c.H & 1) || (c.W & 1)) return 2;
        int seen = 0;
        for (int k = 0; k < 4; ++k) {
            if (c.pat[k] < 0 || c.pat[k] > 3) return 2;
            seen |= 1 << c.pat[k];
        }
        if (seen != 15 || (c.pat[0] & 1) != (c.pat[3] & 1)) return 2;
        const size_t n = (size_t)c.H * c.W;
        c.v.resize(n);
        c.expect.resize(3 * n);
        if (!read_exact(f, c.v.data(), n * 4) || !read_exact(f, c.expect.data(), 3 * n * 4)) return 2;
    }
    fclose(f);
    // 1. the mirrored index
    int nidx = 0;
    for (int L = 2; L <= 9; ++L)
        for (int x = -40; x <= 40; ++x) {
            int pos = 0, dir = 1;                                      // walk |x| steps from 0, turning at both ends
            for (int s = 0; s < (x < 0 ? -x : x); ++s) {
                if (pos + dir < 0 || pos + dir >= L) dir = -dir;
                pos += dir;
            }
            const int r = edge_reflect(x, L);
            if (r != pos || r < 0 || r >= L || ((r ^ x) & 1)) {
                printf("edge_reflect(%d, %d) = %d, the walk gives %d\n", x, L, r, pos);
                return 1;
            }
            ++nidx;
        }
    printf("%d mirrored indices: inside, parity kept\n", nidx);
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
