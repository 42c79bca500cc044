// demosaic_xdir_dev.h -- the per-site arithmetic of the directional X-Trans demosaic (demosaic_xdir.hip eld_render_xtrans_dir):
// the colour-preserving extension index and the four stages over the per-phase tables of the 6 x 6 cell (xtrans.h), as functions a plain host
// compiler accepts too: tools/demosaic_xdir_hostcheck.cpp runs them under AddressSanitizer over small frames, borders included.  Nothing here is
// HIP-only; under hipcc the functions are __host__ __device__.
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
#endif
#include "xtrans.h"                      // the per-phase tables XT, and the pattern facts stage C and the extension stand on (xdir_pattern_ok)

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

// stage A at a non-G site: the provisional green.  s into v (pitch vp); reads the G sites of the 3x3 window
XDIR_HD float xdir_green0(const float* s, int vp, int ph) {
    float acc = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx)
            if ((XT.gmask[ph] >> (3 * (dy + 1) + dx + 1)) & 1u) acc = acc + (float)(XT_W3[dy + 1] * XT_W3[dx + 1]) * s[dy * vp + dx];
    return acc / (float)XT.gsum[ph];
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
    const float g_h = xdir_axis(c, 1, XT.ah[ph]), g_v = xdir_axis(c, vp, XT.av[ph]);
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
            if ((XT.cmask[k][ph] >> (5 * (dy + 2) + dx + 2)) & 1u)
                acc = acc + (float)(XT_W5[dy + 2] * XT_W5[dx + 2]) * (c[dy * vp + dx] - g[dy * gp + dx]);
    return acc / (float)XT.csum[k][ph];
}
