// xtrans.h -- the X-Trans index map and plane colours (RawPacker.pack_raw_xtrans's layout, noise.py:22-64), shared by the pack /
// unpack kernels and the sampler (noise.hip) and the X-Trans ISP (eval.hip).  constexpr, so kernels that unroll over the 6x6 cell
// fold every entry into an immediate; kernels that index with run-time values read the constant-memory copy the compiler emits.
// The per-phase tables of the cell (XT, below) are derived from the map here, once, for the X-Trans renders (demosaic.hip, demosaic_xdir_dev.h)
// and the defect maps (defect.hip).  A plain host compiler takes this header too (tools/demosaic_xdir_hostcheck.cpp): the one place where
// __host__ __device__ are defined away for it.
#pragma once
#include <stdint.h>
#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

// The 6x6 colour cell <-> 9 planes at 1/3 resolution.  Planes 0..4: packed (2a + pi, 2b + pj) <-> cell (a, b), position
// XT_RC[c][pi][pj] = (row, col) in the cell; planes 5..8: packed (i, j) <-> 3x3 block (i, j), position XT_RC3[c - 5].
constexpr unsigned char XT_RC[5][2][2][2] = {
    {{{0, 0}, {0, 4}}, {{3, 1}, {3, 3}}},
    {{{0, 2}, {0, 5}}, {{3, 2}, {3, 5}}},
    {{{0, 1}, {0, 3}}, {{3, 0}, {3, 4}}},
    {{{1, 2}, {2, 5}}, {{5, 2}, {4, 5}}},
    {{{2, 2}, {1, 5}}, {{4, 2}, {5, 5}}},
};
constexpr unsigned char XT_RC3[4][2] = {{1, 0}, {1, 1}, {2, 0}, {2, 1}};

// CFA colour of plane c: (XT_COLOUR >> 2c) & 3 (R 0, G 1, B 2): planes {0, 3} R, {1, 5, 6, 7, 8} G, {2, 4} B
constexpr uint32_t XT_COLOUR = 0x15624u;
__host__ __device__ constexpr uint32_t xt_colour(uint32_t c) { return (XT_COLOUR >> (2u * c)) & 3u; }

// Per-phase tables of the 6 x 6 cell, derived from the map above at compile time (phase = 6 * row + col): the site's colour (R 0, G 1, B 2)
// and packed plane; the G taps of its 3x3 window and the R / B taps of its 5x5 window (bit = raster index of the tap) with the sums of their
// weights ([1 2 1] x [1 2 1], [1 2 3 2 1] x [1 2 3 2 1]) in the interior; and, for a non-G site, its two axes: 0 = solitary (both neighbours
// and both second neighbours are G), -1 / +1 = paired, the side a of the G neighbour (then 2a has the site's colour, -a the other colour,
// -2a is G).  eld_debug_xtrans_demosaic_tables exports colour .. csum.
struct XtTables {
    unsigned char colour[36], plane[36];
    unsigned gmask[36], gsum[36];
    unsigned cmask[2][36], csum[2][36];          // [0] R, [1] B
    signed char ah[36], av[36];
};
constexpr int XT_W3[3] = {1, 2, 1}, XT_W5[5] = {1, 2, 3, 2, 1};

constexpr XtTables make_xt_tables() {
    XtTables t{};
    for (int i = 0; i < 36; ++i) t.plane[i] = 255;
    for (int k = 0; k < 5; ++k)
        for (int pi = 0; pi < 2; ++pi)
            for (int pj = 0; pj < 2; ++pj) t.plane[6 * XT_RC[k][pi][pj][0] + XT_RC[k][pi][pj][1]] = (unsigned char)k;
    for (int k = 5; k < 9; ++k)
        for (int bi = 0; bi < 2; ++bi)
            for (int bj = 0; bj < 2; ++bj) t.plane[6 * (3 * bi + XT_RC3[k - 5][0]) + 3 * bj + XT_RC3[k - 5][1]] = (unsigned char)k;
    for (int i = 0; i < 36; ++i) t.colour[i] = (unsigned char)xt_colour(t.plane[i]);
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) {
            const int ph = 6 * r + c;
            for (int dy = -2; dy <= 2; ++dy)
                for (int dx = -2; dx <= 2; ++dx) {
                    const int col = t.colour[6 * ((r + dy + 6) % 6) + (c + dx + 6) % 6];
                    if (col == 1) {
                        if (dy >= -1 && dy <= 1 && dx >= -1 && dx <= 1) {
                            t.gmask[ph] |= 1u << (3 * (dy + 1) + dx + 1);
                            t.gsum[ph] += XT_W3[dy + 1] * XT_W3[dx + 1];
                        }
                    } else {
                        t.cmask[col >> 1][ph] |= 1u << (5 * (dy + 2) + dx + 2);
                        t.csum[col >> 1][ph] += XT_W5[dy + 2] * XT_W5[dx + 2];
                    }
                }
            if (t.colour[ph] != 1) {
                const bool gw = t.colour[6 * r + (c + 5) % 6] == 1, ge = t.colour[6 * r + (c + 1) % 6] == 1;
                const bool gn = t.colour[6 * ((r + 5) % 6) + c] == 1, gs = t.colour[6 * ((r + 1) % 6) + c] == 1;
                t.ah[ph] = (signed char)(gw && ge ? 0 : gw ? -1 : 1);
                t.av[ph] = (signed char)(gn && gs ? 0 : gn ? -1 : 1);
            }
        }
    return t;
}
constexpr XtTables XT = make_xt_tables();

// every plane fills its places, and a mosaic site (Y, X) is packed pixel (Y / 3, X / 3) of plane XT.plane[phase]: the block parity of
// XT_RC's [pi][pj] is the 3x3 block the position lies in
constexpr bool xt_map_ok() {
    for (int i = 0; i < 36; ++i)
        if (XT.plane[i] > 8) return false;
    for (int k = 0; k < 5; ++k)
        for (int pi = 0; pi < 2; ++pi)
            for (int pj = 0; pj < 2; ++pj)
                if (XT_RC[k][pi][pj][0] / 3 != pi || XT_RC[k][pi][pj][1] / 3 != pj) return false;
    return true;
}
static_assert(xt_map_ok(), "X-Trans index map: site (Y, X) must be packed pixel (Y / 3, X / 3)");

constexpr bool xt_cell_complete() {
    int n[3] = {0, 0, 0};
    for (int i = 0; i < 36; ++i) {
        if (XT.colour[i] > 2) return false;
        ++n[XT.colour[i]];
    }
    return n[0] == 8 && n[1] == 20 && n[2] == 8;
}
static_assert(xt_cell_complete(), "the map must colour every site of the 6x6 cell: 8 R, 20 G, 8 B");

// window coverage on frames of ch x cw whole cells: every clipped 3x3 window holds a G site, every clipped 5x5 window an R and a B site
constexpr bool xt_covered(int ch, int cw) {
    const int H = 6 * ch, W = 6 * cw;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            bool g = false, r = false, b = false;
            for (int dy = -2; dy <= 2; ++dy)
                for (int dx = -2; dx <= 2; ++dx) {
                    const int yy = y + dy, xx = x + dx;
                    if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
                    const int col = XT.colour[6 * (yy % 6) + xx % 6];
                    if (col == 1) g = g || (dy >= -1 && dy <= 1 && dx >= -1 && dx <= 1);
                    else if (col == 0) r = true;
                    else b = true;
                }
            if (!g || !r || !b) return false;
        }
    return true;
}
static_assert(xt_covered(1, 1) && xt_covered(1, 3) && xt_covered(3, 1) && xt_covered(3, 3), "X-Trans window coverage");

// the pattern facts the directional demosaic's stage C stands on, for every non-G phase, and the two mirrors of its extension
constexpr bool xdir_pattern_ok() {
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) {
            const int ph = 6 * r + c, own = XT.colour[ph];
            // row y and row -y, column x and column 4 - x have one colour; with the period 6 so have the mirrors about row 3 and column 5
            if (XT.colour[6 * ((6 - r) % 6) + c] != own || XT.colour[6 * r + (10 - c) % 6] != own) return false;
            if (own == 1) continue;
            if ((XT.ah[ph] == 0) == (XT.av[ph] == 0)) return false;          // exactly one solitary axis
            for (int axis = 0; axis < 2; ++axis) {
                const int a = axis ? XT.av[ph] : XT.ah[ph];
                int col[5] = {};
                for (int k = -2; k <= 2; ++k) col[k + 2] = axis ? XT.colour[6 * ((r + k + 6) % 6) + c] : XT.colour[6 * r + (c + k + 6) % 6];
                if (a == 0) {
                    if (col[0] != 1 || col[1] != 1 || col[3] != 1 || col[4] != 1) return false;
                } else {
                    if (col[2 + a] != 1 || col[2 + 2 * a] != own || col[2 - a] != 2 - own || col[2 - 2 * a] != 1) return false;
                }
            }
        }
    return true;
}
static_assert(xdir_pattern_ok(), "X-Trans pattern facts: one solitary and one paired axis at every R and B site; the cell's mirrors");
