// demosaic_edge_dev.h -- the per-site arithmetic of the edge-directed Bayer demosaic (demosaic_edge.hip eld_render_bayer_edge):
// the mirrored index and the four stages, as functions a plain host compiler accepts too: tools/demosaic_edge_hostcheck.cpp runs them under
// AddressSanitizer over small frames, borders included.  Nothing here is HIP-only; under hipcc the functions are __host__ __device__.
//
// Every function takes a pointer AT its site into a row-major image of float32 with the given pitch and reads a fixed neighbourhood of it
// (stated per function); the caller owns that neighbourhood.  The images are the mosaic v after gain and clamp, extended by mirroring, and what
// the earlier stages wrote.  Arithmetic: float32, the plain operators, every operation rounded on its own (the build passes
// -ffp-contract=off, the division is correctly rounded) -- the contract tests/demosaic_edge_ref.py restates bit for bit.  A value may be
// recomputed by a later stage instead of stored (a_h, a_v, delta): the same instructions on the same operands give the same bits.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define EDGE_HD __host__ __device__ __forceinline__
#else
#define EDGE_HD inline
#endif

constexpr int EDGE_HALO = 4;             // sites of the extension the four stages reach: A 2, B 1, D 1

// index x of the extension of [0, L), L >= 2, into [0, L): np.pad(mode='reflect'), period 2 (L - 1), the edge not repeated.  Any x gives an
// index inside; the parity of x is kept (the period is even).
EDGE_HD int edge_reflect(int x, int L) {
    const int p = 2 * (L - 1);
    x = x < 0 ? -x : x;
    if (x >= p) x %= p;
    return x >= L ? p - x : x;
}

// the second differences of stage A: reads c[-2 .. 2] and c[-2p .. 2p]
EDGE_HD void edge_second(const float* c, int p, float& a_h, float& a_v) {
    a_h = (2.f * c[0] - c[-2]) - c[2];
    a_v = (2.f * c[0] - c[-2 * p]) - c[2 * p];
}

// stage A at any site: d_h = |W - E| + |a_h|, d_v = |N - S| + |a_v|
EDGE_HD void edge_grad(const float* c, int p, float& d_h, float& d_v) {
    float a_h, a_v;
    edge_second(c, p, a_h, a_v);
    d_h = fabsf(c[-1] - c[1]) + fabsf(a_h);
    d_v = fabsf(c[-p] - c[p]) + fabsf(a_v);
}

// stage B: the nine terms of the 3x3 window added to a zero in raster order
EDGE_HD float edge_sum9(const float* d, int p) {
    float s = 0.f;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) s = s + d[dy * p + dx];
    return s;
}

// stage C at an R or B site: G^.  c into v (pitch vp; reads what edge_second reads), d_h and d_v into the stage A images (pitch dp; 3x3)
EDGE_HD float edge_green(const float* c, int vp, const float* d_h, const float* d_v, int dp) {
    const float S_h = edge_sum9(d_h, dp), S_v = edge_sum9(d_v, dp);
    float a_h, a_v;
    edge_second(c, vp, a_h, a_v);
    const float g_h = (c[-1] + c[1]) * 0.5f + a_h * 0.25f;
    const float g_v = (c[-vp] + c[vp]) * 0.5f + a_v * 0.25f;
    const float w_h = S_v * S_v + 1e-6f, w_v = S_h * S_h + 1e-6f;
    return g_h + (g_v - g_h) * (w_v / (w_h + w_v));
}

// stage D.  c into v (pitch vp), g into the image of G^ (pitch gp), which holds G^ at the R and B sites only: at a G site G^ is c, and
// delta = c - G^ is only ever taken at an R or B site.
// At a G site: the colour to its left and right (hor) and the colour above and below (ver)
EDGE_HD void edge_rb_at_g(const float* c, int vp, const float* g, int gp, float& hor, float& ver) {
    hor = c[0] + ((c[-1] - g[-1]) + (c[1] - g[1])) * 0.5f;
    ver = c[0] + ((c[-vp] - g[-gp]) + (c[vp] - g[gp])) * 0.5f;
}

// At an R or B site: the other of the two colours, from the four diagonal neighbours
EDGE_HD float edge_other_at_rb(const float* c, int vp, const float* g, int gp) {
    const float nw = c[-vp - 1] - g[-gp - 1], ne = c[-vp + 1] - g[-gp + 1];
    const float sw = c[vp - 1] - g[gp - 1], se = c[vp + 1] - g[gp + 1];
    return g[0] + ((nw + ne) + (sw + se)) * 0.25f;
}
