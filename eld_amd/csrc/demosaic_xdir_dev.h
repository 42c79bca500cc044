// demosaic_xdir_dev.h -- the per-site arithmetic of the directional X-Trans demosaic (demosaic_xdir.hip eld_render_xtrans_dir):
// the colour-preserving extension index, the per-phase tables of the 6 x 6 cell and the four stages, as functions a plain host compiler accepts
// too: tools/demosaic_xdir_hostcheck.cpp runs them under AddressSanitizer over small frames, borders included.  Nothing here is HIP-only; under
// hipcc the functions are __host__ __device__.
//
// Every stage function takes a pointer AT its site into a row-major image of float32 with the given pitch and reads a fixed neighbourhood of it
// (stated per function); the caller owns that neighbourhood.  `ph` is the site's phase, 6 * (row % 6) + col % 6: where it is a compile-time
// constant (the kernel unrolls over the cell) every table entry folds into the code.  The images are the mosaic v after gain and clamp,
// extended by one cell with xdir_ext_row / xdir_ext_col, and what the earlier stages wrote.  Arithmetic: float32, the plain operators, every
// operation rounded on its own (the build passes -ffp-contract=off, the division is correctly rounded) -- the contract
// tests/demosaic_xdir_ref.py restates bit for bit.  delta = v - G^ is recomputed by stage D instead of stored: the same instruction on the
// same operands gives the same bits.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define XDIR_HD __host__ __device__ __forceinline__
#else
#define XDIR_HD inline
#ifndef __host__
#define __host__
#define __device__
#endif
#endif
#include "xtrans.h"

constexpr int XDIR_HALO = 6;             // sites of the extension the four stages reach: A 1, B 2 + 1, C 2 (with B's sums), D 2 -- one cell

// The 6 x 6 cell is mirror-symmetric about the rows = 0 (mod 3) and about the columns = 2 (mod 3), and about no other line.  So the extension
// of [0, L) that keeps every site's colour mirrors rows about row 0 and row L - 3, columns about column 2 and column L - 1 (L a multiple of 6),
// repeated until the index is inside: one round for |overhang| <= L - 6, two for a 6-site side extended by 6.
XDIR_HD int xdir_ext_row(int y, int H) {
    while (y < 0 || y >= H) y = y < 0 ? -y : 2 * (H - 3) - y;
    return y;
}
XDIR_HD int xdir_ext_col(int x, int W) {
    while (x < 0 || x >= W) x = x < 0 ? 4 - x : 2 * (W - 1) - x;
    return x;
}

// Per-phase tables, derived from xtrans.h at compile time: the site's colour (R 0, G 1, B 2) and packed plane; the G taps of its 3x3 window and
// the R / B taps of its 5x5 window (bit = raster index of the tap) with the sums of their weights ([1 2 1] x [1 2 1],
// [1 2 3 2 1] x [1 2 3 2 1]); and, for a non-G site, its two axes: 0 = solitary (both neighbours and both second neighbours are G), -1 / +1 =
// paired, the side a of the G neighbour (then 2a has the site's colour, -a the other colour, -2a is G).
struct XdirTables {
    unsigned char colour[36], plane[36];
    unsigned gmask[36], gsum[36];
    unsigned cmask[2][36], csum[2][36];          // [0] R, [1] B
    signed char ah[36], av[36];
};
constexpr int XDIR_W3[3] = {1, 2, 1}, XDIR_W5[5] = {1, 2, 3, 2, 1};

constexpr XdirTables make_xdir_tables() {
    XdirTables t{};
    for (int i = 0; i < 36; ++i) t.plane[i] = 255;
    for (int k = 0; k < 5; ++k)
        for (int pi = 0; pi < 2; ++pi)
            for (int pj = 0; pj < 2; ++pj) t.plane[6 * XT_RC[k][pi][pj][0] + XT_RC[k][pi][pj][1]] = (unsigned char)k;
    for (int k = 5; k < 9; ++k)
        for (int bi = 0; bi < 2; ++bi)
            for (int bj = 0; bj < 2; ++bj) t.plane[6 * (3 * bi + XT_RC3[k - 5][0]) + 3 * bj + XT_RC3[k - 5][1]] = (unsigned char)k;
    for (int i = 0; i < 36; ++i) t.colour[i] = (unsigned char)((XT_COLOUR >> (2u * t.plane[i])) & 3u);
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) {
            const int ph = 6 * r + c;
            for (int dy = -2; dy <= 2; ++dy)
                for (int dx = -2; dx <= 2; ++dx) {
                    const int col = t.colour[6 * ((r + dy + 6) % 6) + (c + dx + 6) % 6];
                    if (col == 1) {
                        if (dy >= -1 && dy <= 1 && dx >= -1 && dx <= 1) {
                            t.gmask[ph] |= 1u << (3 * (dy + 1) + dx + 1);
                            t.gsum[ph] += XDIR_W3[dy + 1] * XDIR_W3[dx + 1];
                        }
                    } else {
                        t.cmask[col >> 1][ph] |= 1u << (5 * (dy + 2) + dx + 2);
                        t.csum[col >> 1][ph] += XDIR_W5[dy + 2] * XDIR_W5[dx + 2];
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
constexpr XdirTables XDIR = make_xdir_tables();

// the pattern facts stage C stands on, for every non-G phase, and the two mirrors of the extension
constexpr bool xdir_pattern_ok() {
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) {
            const int ph = 6 * r + c, own = XDIR.colour[ph];
            if (XDIR.plane[ph] > 8) return false;
            // row y and row -y, column x and column 4 - x have one colour; with the period 6 so have the mirrors about row 3 and column 5
            if (XDIR.colour[6 * ((6 - r) % 6) + c] != own || XDIR.colour[6 * r + (10 - c) % 6] != own) return false;
            if (own == 1) continue;
            if ((XDIR.ah[ph] == 0) == (XDIR.av[ph] == 0)) return false;          // exactly one solitary axis
            for (int axis = 0; axis < 2; ++axis) {
                const int a = axis ? XDIR.av[ph] : XDIR.ah[ph];
                int col[5] = {};
                for (int k = -2; k <= 2; ++k) col[k + 2] = axis ? XDIR.colour[6 * ((r + k + 6) % 6) + c] : XDIR.colour[6 * r + (c + k + 6) % 6];
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

// stage A at a non-G site: the provisional green.  s into v (pitch vp); reads the G sites of the 3x3 window
XDIR_HD float xdir_green0(const float* s, int vp, int ph) {
    float acc = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx)
            if ((XDIR.gmask[ph] >> (3 * (dy + 1) + dx + 1)) & 1u) acc = acc + (float)(XDIR_W3[dy + 1] * XDIR_W3[dx + 1]) * s[dy * vp + dx];
    return acc / (float)XDIR.gsum[ph];
}

// stage B at any site: d_h = |W - E| + |(2c - WW) - EE| on G0, d_v likewise.  g into G0 (pitch p); reads g[-2 .. 2] and g[-2p .. 2p]
XDIR_HD void xdir_grad(const float* g, int p, float& d_h, float& d_v) {
    d_h = fabsf(g[-1] - g[1]) + fabsf((2.f * g[0] - g[-2]) - g[2]);
    d_v = fabsf(g[-p] - g[p]) + fabsf((2.f * g[0] - g[-2 * p]) - g[2 * p]);
}

// the nine terms of the 3x3 window added to a zero in raster order
XDIR_HD float xdir_sum9(const float* d, int p) {
    float s = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) s = s + d[dy * p + dx];
    return s;
}

// stage C, one axis of an R or B site: c into v, `step` the distance of a neighbour along the axis (1 or the pitch), a the table's entry.
// Reads c[-2 step .. 2 step].  Markesteijn's weights (174, -46) / 256 and (223, 33, 92) / 256 as a mean plus differences.
XDIR_HD float xdir_axis(const float* c, int step, int a) {
    if (a == 0) {
        const float s1 = c[-step] + c[step], s2 = c[-2 * step] + c[2 * step];
        return s1 * 0.5f + (s1 - s2) * (46.f / 256.f);
    }
    const float ga = c[a * step];
    return (ga + (c[-2 * a * step] - ga) * (33.f / 256.f)) + (c[0] - c[2 * a * step]) * (92.f / 256.f);
}

// stage C at an R or B site: G^.  c into v (pitch vp; reads c[-2 .. 2], c[-2vp .. 2vp]), d_h and d_v into the stage B images (pitch dp; 3x3)
XDIR_HD float xdir_green(const float* c, int vp, const float* d_h, const float* d_v, int dp, int ph) {
    const float S_h = xdir_sum9(d_h, dp), S_v = xdir_sum9(d_v, dp);
    const float g_h = xdir_axis(c, 1, XDIR.ah[ph]), g_v = xdir_axis(c, vp, XDIR.av[ph]);
    const float w_h = S_v * S_v + 1e-6f, w_v = S_h * S_h + 1e-6f;
    return g_h + (g_v - g_h) * (w_v / (w_h + w_v));
}

// stage D at a site that is not of colour k (0 R, 1 B): the weighted mean of delta = v - G^ over the k sites of the 5x5 window.  c into v
// (pitch vp), g into the image of G^ (pitch gp), which holds G^ at the R and B sites only; reads both at the k sites of the window.
XDIR_HD float xdir_chroma(const float* c, int vp, const float* g, int gp, int ph, int k) {
    float acc = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx)
            if ((XDIR.cmask[k][ph] >> (5 * (dy + 2) + dx + 2)) & 1u)
                acc = acc + (float)(XDIR_W5[dy + 2] * XDIR_W5[dx + 2]) * (c[dy * vp + dx] - g[dy * gp + dx]);
    return acc / (float)XDIR.csum[k][ph];
}
