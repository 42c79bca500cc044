// render_args.h -- what the four full-resolution demosaic renders share in front of the tail (demosaic.hip, demosaic_edge.hip, demosaic_xdir.hip):
// the argument record and what every entry point refuses, the Bayer cell read from raw_pattern, gain and clamp, and the store of adjacent
// sites.  Include inside the translation unit's anonymous namespace, after common.h; this includes render_tail.h.
#pragma once
#include "render_tail.h"

struct RenderArgs {
    const float* packed;
    const float* wbs;
    TailArgs t;
    void* out;
    int h, w;                          // packed sides
};

// what the four entry points refuse before any launch, beside their own limits on the sides and the grid
inline int render_args_bad(const void* packed, const void* wbs, const void* ccms, const void* out, int out_mode, int N, float gamma,
                           const float* crf_E, const float* crf_f, int crf_n) {
    if (!packed || !wbs || !out) return 1;
    if (((uintptr_t)packed & 15) || ((uintptr_t)out & 15) || ((uintptr_t)wbs & 3)) return 1;
    if (N < 1 || N > 65535) return 1;
    return tail_args_bad(ccms, out_mode, gamma, crf_E, crf_f, crf_n);
}

// The Bayer cell of a raw_pattern: a permutation of the colour codes with its two greens (the odd codes) on a diagonal.
struct BayerCell {
    int pos[4];                        // colour code (R 0, G1 1, B 2, G2 3) = packed plane at cell position (0,0), (0,1), (1,0), (1,1)
    int r_row;                         // row parity of the R site
    bool g00;                          // position (0,0) is a G site
};
inline bool bayer_cell(const int* raw_pattern, BayerCell* c) {
    if (!raw_pattern || !bayer_permutation(raw_pattern)) return false;
    if ((raw_pattern[0] & 1) != (raw_pattern[3] & 1) || (raw_pattern[1] & 1) != (raw_pattern[2] & 1)) return false;
    for (int k = 0; k < 4; ++k) {
        c->pos[k] = raw_pattern[k];
        if (raw_pattern[k] == 0) c->r_row = k >> 1;
    }
    c->g00 = (raw_pattern[0] & 1) != 0;
    return true;
}

struct BayerArgs {                     // one record: the compiler schedules the Bayer kernels differently around two
    RenderArgs r;
    BayerCell cell;
};

__device__ __forceinline__ float gain_clamp(float p, float gain) { return fminf(fmaxf(p * gain, 0.f), 1.f); }

// K adjacent sites of one plane, v... as site_out left them, to element e of the output as the single widest vector: float2, float4 or two
// float4 (ELD_RENDER_LINEAR_F32); a 16-bit pair, a 32-bit word or a uint2 of codes (ELD_RENDER_SRGB8).  The caller owns the alignment: out is
// 16-byte aligned and every plane and row of the planar output an even number of elements, so e even gives K = 2 its 8 / 2 bytes; K = 4 and
// K = 8 need e % K == 0, which holds where the mosaic's width is a multiple of K and the run starts at a multiple of K.
// The sites travel by value: a reference to the caller's register array goes through a generic pointer, and the vectorised Bayer kernel then
// comes out with other registers and another schedule than with the stores written in place.
template <int TAIL, int K, class... F>
__device__ __forceinline__ void store_sites(void* out, size_t e, F... sites) {
    static_assert((K == 2 || K == 4 || K == 8) && sizeof...(F) == K, "a pair, a quad or two quads");
    const float v[K] = {sites...};
    if constexpr (TAIL == TAIL_LINEAR) {
        float* d = (float*)out + e;
        if constexpr (K == 2) *reinterpret_cast<float2*>(d) = make_float2(v[0], v[1]);
        else reinterpret_cast<float4*>(d)[0] = make_float4(v[0], v[1], v[2], v[3]);
        if constexpr (K == 8) reinterpret_cast<float4*>(d)[1] = make_float4(v[4], v[5], v[6], v[7]);
    } else {
        unsigned char* d = (unsigned char*)out + e;
        unsigned b2[K / 2];
#pragma unroll
        for (int q = 0; q < K / 2; ++q) b2[q] = (unsigned)v[2 * q] | ((unsigned)v[2 * q + 1] << 8);
        if constexpr (K == 2) *reinterpret_cast<unsigned short*>(d) = (unsigned short)b2[0];
        else if constexpr (K == 4) *reinterpret_cast<unsigned*>(d) = b2[0] | (b2[1] << 16);
        else *reinterpret_cast<uint2*>(d) = make_uint2(b2[0] | (b2[1] << 16), b2[2] | (b2[3] << 16));
    }
}
