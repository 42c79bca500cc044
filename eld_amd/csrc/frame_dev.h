// frame_dev.h -- the per-output arithmetic of the frame (frame.hip, eld_amd/isp.py Frame): the clamps of the tap tables, the
// two float32 tap sums and the orientation index, as functions a plain host compiler accepts too: tools/frame_hostcheck.cpp runs them under
// AddressSanitizer on corrupted tables.  Nothing here is HIP-only; under hipcc the functions are __host__ __device__.
//
// The rule of the file is dng_dev.h's and warp_dev.h's: no address is formed from a table value before it has been clamped.  A table holds,
// per output index, a first tap `start`, a `count` and `count` weights in a dense row of T floats.  frame_count clamps every count to [1, T]
// (the weights' row is never left), frame_tap clamps every tap start + k to [0, L - 1] (the plane is never left); the weights are only ever
// multiplied.  Whatever the tables hold, every read lies inside the plane and inside the table.
//
// Arithmetic (the contract tests/frame_ref.py restates bit for bit): float32, strictly ascending tap order, every product and sum rounded on
// its own through FRAME_MUL / FRAME_ADD (__fmul_rn / __fadd_rn on the device, the plain operators elsewhere: the build passes
// -ffp-contract=off).  No initial zero: the first product starts the sum, so -0.0 and NaN pass through a single tap of weight 1.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#if defined(__HIPCC__)
#define FRAME_HD __host__ __device__ __forceinline__
#else
#define FRAME_HD inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define FRAME_MUL(a, b) __fmul_rn((a), (b))
#define FRAME_ADD(a, b) __fadd_rn((a), (b))
#else
#define FRAME_MUL(a, b) ((float)(a) * (float)(b))
#define FRAME_ADD(a, b) ((float)(a) + (float)(b))
#endif

constexpr int FRAME_MAX_TAPS = 4096;                                 // the widest table row the entry point takes

// a table's count -> the taps that are read: 1 .. T
FRAME_HD int frame_count(int count, int T) { return count < 1 ? 1 : (count > T ? T : count); }

// tap k of a run that starts at `start`, along an axis of L elements: start + k clamped to [0, L - 1]
FRAME_HD int frame_tap(int64_t start, int k, int L) {
    const int64_t i = start + (int64_t)k;                            // start: an int table value, or one minus a row offset: no overflow here
    return i < 0 ? 0 : (i > (int64_t)L - 1 ? L - 1 : (int)i);
}

// Taps k0 .. k1 - 1 of the sums of M outputs that share their taps, added to v in ascending order (tap 0 starts the sums: no initial zero).
// Tap k reads element frame_tap(start, k, L) of M lines of L elements `stride` apart and weight w[k * wstride].  This is the tap loop of both
// kernels and of frame_eval below: the row pass runs it on M source rows of one column (stride 1; the x weights are stored tap-major, so
// wstride = Wc) -- on the rows themselves, or chunk by chunk on a staged piece of them, which is why it takes a range of taps -- and the
// column pass on the three planes' workspace columns (stride Wc, start relative to the workspace's first row, wstride 1).
template <int M>
FRAME_HD void frame_sums_part(const float* const (&line)[M], size_t stride, int L, int64_t start, int k0, int k1, const float* w, size_t wstride,
                              float (&v)[M]) {
    for (int k = k0; k < k1; ++k) {
        const size_t e = (size_t)frame_tap(start, k, L) * stride;
        const float wk = w[(size_t)k * wstride];
        for (int m = 0; m < M; ++m) v[m] = k == 0 ? FRAME_MUL(wk, line[m][e]) : FRAME_ADD(v[m], FRAME_MUL(wk, line[m][e]));
    }
}

// all taps of a table entry: count clamped to 1 .. T
template <int M>
FRAME_HD void frame_sums(const float* const (&line)[M], size_t stride, int L, int64_t start, int count, const float* w, size_t wstride, int T,
                         float (&v)[M]) {
    frame_sums_part<M>(line, stride, L, start, 0, frame_count(count, T), w, wstride, v);
}

// The orientation: unoriented pixel (i, j) of the Hc x Wc grid -> the upright pixel (Y, X) a TIFF Orientation o = 1 .. 8 puts it at (the
// inverse of the contract's table, which gives (i, j) for (Y, X)).  o >= 5 transposes: the upright picture is Wc x Hc.  Any other o is 1.
FRAME_HD bool frame_transposed(int o) { return o >= 5 && o <= 8; }
FRAME_HD void frame_upright(int o, int i, int j, int Hc, int Wc, int* Y, int* X) {
    const bool flip_i = o == 3 || o == 4 || o == 6 || o == 7, flip_j = o == 2 || o == 3 || o == 7 || o == 8;
    const int ii = flip_i ? Hc - 1 - i : i, jj = flip_j ? Wc - 1 - j : j;
    if (frame_transposed(o)) { *Y = jj; *X = ii; }
    else { *Y = ii; *X = jj; }
}

// where the workspace's row r lies in the source: row0 + r clamped to the plane (the entry point keeps row0 + rows <= Hs)
FRAME_HD int frame_source_row(int row0, int r, int Hs) { return frame_tap((int64_t)row0, r, Hs); }

#if !defined(__HIP_DEVICE_COMPILE__)
// One output of one plane on the host, for tools/frame_hostcheck.cpp: what the two kernels compute between them, through the same
// frame_sums with the same arguments.  Column j of the workspace (the horizontal sums of the source rows row0 .. row0 + rows - 1) is built
// in a heap buffer of exactly `rows` floats as the row pass builds it, then summed as the column pass sums it: from the row
// ystart[i] - row0, clamped into the workspace.  xw is tap-major, Tx x Wc, as the entry point takes it.  plane: Hs x Ws; the caller keeps 0 <= i < Hc, 0 <= j < Wc (the tables' lengths) and rows >= 1.
inline float frame_eval(const float* plane, int Hs, int Ws, int i, int j, const int* ystart, const int* ycount, const float* yw, int Ty,
                        const int* xstart, const int* xcount, const float* xw, int Tx, int Wc, int row0, int rows) {
    float* h = (float*)malloc((size_t)rows * sizeof(float));
    for (int r = 0; r < rows; ++r) {
        const float* const line[1] = {plane + (size_t)frame_source_row(row0, r, Hs) * (size_t)Ws};
        float s[1];
        frame_sums<1>(line, 1, Ws, xstart[j], xcount[j], xw + (size_t)j, (size_t)Wc, Tx, s);
        h[r] = s[0];
    }
    const float* const col[1] = {h};
    float v[1];
    frame_sums<1>(col, 1, rows, (int64_t)ystart[i] - (int64_t)row0, ycount[i], yw + (size_t)i * (size_t)Ty, 1, Ty, v);
    free(h);
    return v[0];
}
#endif
