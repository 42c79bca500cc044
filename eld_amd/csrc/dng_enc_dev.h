// dng_enc_dev.h -- the per-lane arithmetic of the lossless-JPEG encoder (dng_enc.hip), as functions a plain host compiler
// accepts too: tools/dng_enc_hostcheck.cpp runs them run by run under AddressSanitizer and UBSan, which is how the shifts of the bit assembly
// (a 31-bit word at every bit phase) are shown to be defined without a GPU.  Nothing here is HIP-only; under hipcc the functions are
// __host__ __device__.  Where a dword or a byte goes is the caller's: it passes a functor (an LDS atomic OR in the kernel, a plain OR into an
// exact-size heap buffer in the host check).
//
// The stream: ITU-T T.81 process 14, two components of tw / 2 samples per line over the tile's raster, predictor 1, no point transform.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/eld_amd.h"

#if defined(__HIPCC__)
#define DNG_ENC_HD __host__ __device__ __forceinline__
#else
#define DNG_ENC_HD inline
#endif

// one stored tile of the mosaic: th x tw samples from (y0, x0), padded by edge replication beyond the H x W image
struct DngEncSrc {
    const uint16_t* mos;
    int H, W, y0, x0, tw;
    uint32_t half;                                                   // 2^(P - 1): the prediction of the tile's first two samples
};

// 0 <= y0 < H, 0 <= x0 < W, r, c >= 0: the site read lies inside the mosaic whatever r and c are
DNG_ENC_HD uint32_t dng_enc_at(const DngEncSrc& s, int r, int c) {
    int y = s.y0 + r, x = s.x0 + c;
    y = y < s.H - 1 ? y : s.H - 1;
    x = x < s.W - 1 ? x : s.W - 1;
    return s.mos[(size_t)y * (size_t)s.W + (size_t)x];
}

// Where a lane stands in its run: the next sample (r, c), how many samples of the run lie behind it (j) and the last two of them.
struct DngEncCursor {
    int r, c;
    uint32_t j, p1, p2;
};

DNG_ENC_HD DngEncCursor dng_enc_cursor(const DngEncSrc& s, uint32_t first) {
    DngEncCursor k;
    k.r = (int)(first / (uint32_t)s.tw);
    k.c = (int)(first - (uint32_t)k.r * (uint32_t)s.tw);
    k.j = 0; k.p1 = 0; k.p2 = 0;
    return k;
}

// The next sample's difference modulo 65536; *code: the sample itself.  Predictor 1 over two interleaved components: (r, c - 2); the first two of
// a row: (r - 1, c); the first two of the tile: 2^(P - 1).  The sample two back is in a register once the run is two samples old (tw >= 2:
// after a row's end, c = 2 is again two samples behind c = 0).
DNG_ENC_HD uint32_t dng_enc_next(const DngEncSrc& s, DngEncCursor& k, uint32_t* code) {
    const uint32_t v = dng_enc_at(s, k.r, k.c);
    uint32_t px;
    if (k.c >= 2) px = k.j >= 2u ? k.p2 : dng_enc_at(s, k.r, k.c - 2);
    else px = k.r == 0 ? s.half : dng_enc_at(s, k.r - 1, k.c);
    k.p2 = k.p1; k.p1 = v; k.j++;
    if (++k.c == s.tw) { k.c = 0; ++k.r; }
    *code = v;
    return (v - px) & 0xFFFFu;
}

// the category of a difference d (modulo 65536, read as -32768 .. 32767): 0 for 0, else the bits of |d|; 16 for -32768 alone
DNG_ENC_HD uint32_t dng_enc_ssss(uint32_t d) {
    const uint32_t a = (d & 0x8000u) ? 0x10000u - d : d;             // 1 .. 32768
    return a ? 32u - (uint32_t)__builtin_clz(a) : 0u;
}

// One sample's bits, right-justified: the category's code, then SSSS extra bits (d for d > 0, d - 1 for d < 0, the low SSSS bits; none for
// SSSS = 16).  entry = (length << 16) | code with length 1..16; *nb = length + extra bits <= 31.  length 0 (a category the table lacks):
// *nb = 0, nothing to write.
DNG_ENC_HD uint32_t dng_enc_word(uint32_t d, const uint32_t* table, uint32_t* nb) {
    const uint32_t s = dng_enc_ssss(d), e = table[s];                // s <= 16: inside the 17 entries
    const uint32_t len = e >> 16, nx = s == 16u ? 0u : s;
    if (len < 1u || len > 16u) { *nb = 0u; return 0u; }
    const uint32_t x = ((d & 0x8000u) ? d - 1u : d) & ((1u << nx) - 1u);
    *nb = len + nx;
    return ((e & 0xFFFFu) << nx) | x;
}

// the bits of the run [first, first + count) of the tile's sample sequence
DNG_ENC_HD uint32_t dng_enc_run_bits(const DngEncSrc& s, const uint32_t* table, uint32_t first, uint32_t count) {
    DngEncCursor k = dng_enc_cursor(s, first);
    uint32_t bits = 0, code, nb;
    for (uint32_t j = 0; j < count; ++j) {
        (void)dng_enc_word(dng_enc_next(s, k, &code), table, &nb);
        bits += nb;
    }
    return bits;
}

// The bit assembly: up to 63 bits left-justified in acc, n < 32 of them waiting; a full dword leaves through put(dword index, value).
struct DngEncBits {
    uint64_t acc;
    uint32_t n, idx;
};

// word < 2^nb, nb <= 32; b.n < 32 on entry and on return.  The shift is 64 - n - nb, 1..63 for nb >= 1.
template <class Put>
DNG_ENC_HD void dng_enc_push(DngEncBits& b, uint32_t word, uint32_t nb, Put& put) {
    if (nb == 0u) return;
    b.acc |= (uint64_t)word << (64u - b.n - nb);
    b.n += nb;
    if (b.n >= 32u) {
        put(b.idx++, (uint32_t)(b.acc >> 32));
        b.acc <<= 32;
        b.n -= 32u;
    }
}

// The run's bits into the dword image whose bit 0 is the top bit of dword 0; the run starts at bit bit0 of it.  The bits before bit0 in the
// run's first dword and behind its end in its last are left zero: put() must OR.  pad: that many 1-bits behind the run (the stream's last
// run; 0..7).
template <class Put>
DNG_ENC_HD void dng_enc_run(const DngEncSrc& s, const uint32_t* table, uint32_t first, uint32_t count, uint32_t bit0, uint32_t pad, Put& put) {
    DngEncBits b;
    b.acc = 0; b.n = bit0 & 31u; b.idx = bit0 >> 5;
    DngEncCursor k = dng_enc_cursor(s, first);
    uint32_t code, nb;
    for (uint32_t j = 0; j < count; ++j) {
        const uint32_t w = dng_enc_word(dng_enc_next(s, k, &code), table, &nb);
        dng_enc_push(b, w, nb, put);
    }
    if (pad) dng_enc_push(b, (1u << pad) - 1u, pad, put);
    if (b.n) put(b.idx, (uint32_t)(b.acc >> 32));
}

// ---- byte stuffing: a lane's 16 bytes -------------------------------------------------------------------------------------------------
constexpr uint32_t DNG_ENC_LANE_BYTES = 16;

// the FF bytes among the first m <= 16 of b[16]
DNG_ENC_HD uint32_t dng_enc_count_ff(const uint8_t* b, uint32_t m) {
    uint32_t n = 0;
    for (uint32_t i = 0; i < DNG_ENC_LANE_BYTES; ++i) n += (i < m && b[i] == 0xFFu) ? 1u : 0u;
    return n;
}

// b[0 .. m) to dst from pos on, a 00 behind every FF; nothing at or beyond cap.  -> the position behind the last byte written
DNG_ENC_HD uint32_t dng_enc_stuff(const uint8_t* b, uint32_t m, uint8_t* dst, uint32_t pos, uint32_t cap) {
    for (uint32_t i = 0; i < DNG_ENC_LANE_BYTES; ++i) {
        if (i >= m) break;
        if (pos < cap) dst[pos] = b[i];
        ++pos;
        if (b[i] == 0xFFu) {
            if (pos < cap) dst[pos] = 0u;
            ++pos;
        }
    }
    return pos;
}
