// warp_dev.h -- the per-pixel arithmetic of DNG WarpRectilinear (warp.hip, eld_amd/dng_opcodes.py Warp): the float64 map, the
// clamp of its result, the tap indices and the 16-tap Catmull-Rom sum, as functions a plain host compiler accepts too:
// tools/warp_hostcheck.cpp runs them under AddressSanitizer on corrupted records.  Nothing here is HIP-only; under hipcc the functions are
// __host__ __device__.
//
// The rule of the file is dng_dev.h's and dng_opcodes_dev.h's: no address is formed from a coordinate before it has been clamped.  The map's
// result is a float64 that a record's fields can make anything, NaN included; warp_site clamps it to [-1, L] (NaN -> -1) before the floor, and
// warp_tap clamps every tap to [0, L - 1] before it indexes a row or a column.  Whatever the record holds, every read lies inside the plane.
//
// Arithmetic (the contract tests/warp_ref.py restates bit for bit): the map in float64 with the plain operators, every operation rounded on
// its own (the build passes -ffp-contract=off); the weights and sums in float32 through WARP_MUL / WARP_ADD / WARP_SUB, which are __fmul_rn and
// friends on the device and the plain operators elsewhere.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/eld_amd.h"

#if defined(__HIPCC__)
#define WARP_HD __host__ __device__ __forceinline__
#else
#define WARP_HD inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define WARP_MUL(a, b) __fmul_rn((a), (b))
#define WARP_ADD(a, b) __fadd_rn((a), (b))
#define WARP_SUB(a, b) __fsub_rn((a), (b))
#else
#define WARP_MUL(a, b) ((float)(a) * (float)(b))
#define WARP_ADD(a, b) ((float)(a) + (float)(b))
#define WARP_SUB(a, b) ((float)(a) - (float)(b))
#endif

// where one destination pixel samples one plane: the cell (i0, j0) of the clamped source coordinate and the fractions inside it
struct WarpSite {
    int i0, j0;                          // floor(v), floor(u): -1 .. Hm resp. -1 .. Wm
    float ty, tx;                        // float32(v - i0), float32(u - j0)
};

// what the entry point refuses: the record's fields, before anything is computed from them
WARP_HD bool warp_record_ok(const EldWarp& w) {
    if (w.nsets != 1 && w.nsets != 3) return false;
    for (int s = 0; s < w.nsets; ++s)
        for (int i = 0; i < 6; ++i)
            if (!isfinite(w.k[s][i])) return false;
    if (!isfinite(w.cxp) || !isfinite(w.cyp) || !isfinite(w.m) || !isfinite(w.m2)) return false;
    return w.m2 > 0.0;
}

// a float64 coordinate -> its cell and fraction along an axis of L pixels; NaN and everything below -1 become -1, everything above L becomes L
WARP_HD void warp_cell(double c, int L, int* i0, float* t) {
    if (!(c >= -1.0)) c = -1.0;
    if (c > (double)L) c = (double)L;
    const double f = floor(c);
    *i0 = (int)f;                                                    // -1 <= f <= L < 2^31
    *t = (float)(c - f);
}

// the map of coefficient set k (kr0 - 1, kr1, kr2, kr3, kt0, kt1) at destination pixel (x, y), then the clamp
WARP_HD WarpSite warp_site(const double* k, double cxp, double cyp, double m, double m2, int x, int y, int Hm, int Wm) {
    const double px = (double)x + 0.5, py = (double)y + 0.5;
    const double dx = px - cxp, dy = py - cyp;
    const double r2 = (dx * dx + dy * dy) / m2;
    const double g = k[0] + r2 * (k[1] + r2 * (k[2] + r2 * k[3]));
    const double nx = dx / m, ny = dy / m;
    const double nxy2 = (2.0 * nx) * ny;
    const double tx = k[4] * nxy2 + k[5] * (r2 + (2.0 * nx) * nx);
    const double ty = k[5] * nxy2 + k[4] * (r2 + (2.0 * ny) * ny);
    const double u = (px + (g * dx + m * tx)) - 0.5;
    const double v = (py + (g * dy + m * ty)) - 0.5;
    WarpSite s;
    warp_cell(u, Wm, &s.j0, &s.tx);
    warp_cell(v, Hm, &s.i0, &s.ty);
    return s;
}

// tap q (0 .. 3) of cell i0 along an axis of L pixels: i0 - 1 + q clamped to the image (the edge is replicated)
WARP_HD int warp_tap(int i0, int q, int L) {
    const int64_t i = (int64_t)i0 - 1 + q;                           // i0 may be anything when a caller skipped warp_cell: no overflow here
    return i < 0 ? 0 : (i > (int64_t)L - 1 ? L - 1 : (int)i);
}

// the four Catmull-Rom weights of fraction t
WARP_HD void warp_weights(float t, float (&w)[4]) {
    const float tt = WARP_MUL(t, t);
    w[0] = WARP_MUL(t, WARP_SUB(WARP_MUL(t, WARP_ADD(WARP_MUL(-0.5f, t), 1.f)), 0.5f));
    w[1] = WARP_ADD(WARP_MUL(tt, WARP_SUB(WARP_MUL(1.5f, t), 2.5f)), 1.f);
    w[2] = WARP_MUL(t, WARP_ADD(WARP_MUL(t, WARP_ADD(WARP_MUL(-1.5f, t), 2.f)), 0.5f));
    w[3] = WARP_MUL(tt, WARP_SUB(WARP_MUL(0.5f, t), 0.5f));
}

WARP_HD float warp_dot4(const float (&w)[4], float p0, float p1, float p2, float p3) {
    return WARP_ADD(WARP_ADD(WARP_ADD(WARP_MUL(w[0], p0), WARP_MUL(w[1], p1)), WARP_MUL(w[2], p2)), WARP_MUL(w[3], p3));
}

// the 16-tap sum: the four row sums, then their column.  p[i][j]: the tap of row i0 - 1 + i, column j0 - 1 + j, each clamped to the image
WARP_HD float warp_sum16(const float (&p)[4][4], const float (&wx)[4], const float (&wy)[4]) {
    float h[4];
    for (int i = 0; i < 4; ++i) h[i] = warp_dot4(wx, p[i][0], p[i][1], p[i][2], p[i][3]);
    return warp_dot4(wy, h[0], h[1], h[2], h[3]);
}

// One plane at one site, taps read from the Hm x Wm plane itself through the clamp: what the kernel's direct path computes, and what its LDS
// path must equal.
WARP_HD float warp_sample(const float* plane, int Hm, int Wm, const WarpSite& s) {
    float wx[4], wy[4];
    warp_weights(s.tx, wx);
    warp_weights(s.ty, wy);
    int cols[4];
    for (int q = 0; q < 4; ++q) cols[q] = warp_tap(s.j0, q, Wm);
    float p[4][4];
    for (int i = 0; i < 4; ++i) {
        const float* row = plane + (size_t)warp_tap(s.i0, i, Hm) * (size_t)Wm;
        for (int j = 0; j < 4; ++j) p[i][j] = row[cols[j]];
    }
    return warp_sum16(p, wx, wy);
}

// A record at one pixel of one plane, nothing cached: for the host check.  A record the entry point would refuse is still evaluated here (the
// kernel never sees one); the clamps alone keep it inside the plane.
WARP_HD float warp_eval(const EldWarp& w, const float* plane, int c, int Hm, int Wm, int y, int x) {
    const int s = w.nsets == 3 ? (c < 0 ? 0 : (c > 2 ? 2 : c)) : 0;
    return warp_sample(plane, Hm, Wm, warp_site(w.k[s], w.cxp, w.cyp, w.m, w.m2, x, y, Hm, Wm));
}
