// xtrans.h -- the X-Trans index map and plane colours (RawPacker.pack_raw_xtrans's layout, noise.py:22-64), shared by the pack /
// unpack kernels and the sampler (noise.hip) and the X-Trans ISP (eval.hip).  constexpr, so kernels that unroll over the 6x6 cell
// fold every entry into an immediate; kernels that index with run-time values read the constant-memory copy the compiler emits.
#pragma once
#include <stdint.h>

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
