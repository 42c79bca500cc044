// jpeg_dev.h -- the per-block arithmetic of the baseline-JPEG encoder (jpeg.hip), as functions a plain host compiler accepts
// too: tools/jpeg_hostcheck.cpp runs them block by block under AddressSanitizer and UBSan.  Nothing here is HIP-only; under hipcc the functions
// are __host__ __device__.  Two halves: one block of the picture -> its 64 quantised coefficients (colour conversion, edge replication, h2v2
// downsampling, libjpeg's slow-integer forward DCT, its quantiser, its dummy blocks), and one block's coefficients -> its symbols (the walk
// feeds a sink: a histogram, a bit count, or the word assembly of dng_enc_dev.h, which is shared and not copied).
#pragma once
#include "dng_enc_dev.h"

#define JPEG_HD DNG_ENC_HD

// the layout of the four alphabets in a histogram (ELD_JPEG_HIST bins) and in the code tables (ELD_JPEG_TABLE entries: a DC table has the 17
// entries dng_enc_word indexes)
constexpr uint32_t JPEG_HIST_DC = 12, JPEG_HIST_AC0 = 24, JPEG_HIST_AC1 = 280;
constexpr uint32_t JPEG_TAB_DC = 17, JPEG_TAB_AC0 = 34, JPEG_TAB_AC1 = 290;

struct JpegGeom {
    int H, W, sub;
    uint32_t mcux, mcuy, bpm, nblocks;                               // MCUs per row and column, blocks per MCU, blocks in all
    uint32_t bw, bh;                                                 // ceil(W / 8), ceil(H / 8): the Y blocks that hold a pixel
};

// false for what every entry point refuses
JPEG_HD bool jpeg_geom(JpegGeom* g, int H, int W, int sub) {
    if (H < 1 || W < 1 || H > 65535 || W > 65535 || (uint64_t)H * (uint64_t)W >= (1ull << 31)) return false;
    if (sub != ELD_JPEG_444 && sub != ELD_JPEG_420) return false;
    const uint32_t m = sub == ELD_JPEG_420 ? 16u : 8u;
    g->H = H; g->W = W; g->sub = sub;
    g->mcux = ((uint32_t)W + m - 1) / m; g->mcuy = ((uint32_t)H + m - 1) / m;
    g->bpm = sub == ELD_JPEG_420 ? 6u : 3u;
    g->nblocks = g->mcux * g->mcuy * g->bpm;                         // < 2^31 / 64 * 3
    g->bw = ((uint32_t)W + 7) / 8; g->bh = ((uint32_t)H + 7) / 8;
    return true;
}

// the component (0 Y, 1 Cb, 2 Cr) of the k-th block of an MCU
JPEG_HD uint32_t jpeg_comp(const JpegGeom& g, uint32_t k) { return k < g.bpm - 2 ? 0u : k - (g.bpm - 3); }

// the block in front of b among those of its component (the DC predictor); false for the component's first block
JPEG_HD bool jpeg_prev_block(const JpegGeom& g, uint32_t b, uint32_t* prev) {
    const uint32_t k = b % g.bpm;
    const uint32_t back = (k == 0 || k >= g.bpm - 2) ? (k == 0 ? 3u : g.bpm) : 1u;       // Y: the last Y of the MCU before; chroma: one MCU back
    if (back > b) return false;
    *prev = b - back;
    return true;
}

struct JpegSrc {
    const uint8_t* rgb;                                              // (3, H, W)
    int H, W;
};

// libjpeg's colour conversion, 16 fraction bits
JPEG_HD int jpeg_ycc(int r, int g, int b, uint32_t comp) {
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// component comp at pixel (y, x), y and x >= 0: the last row and column are replicated
JPEG_HD int jpeg_at(const JpegSrc& s, uint32_t comp, int y, int x) {
    y = y < s.H - 1 ? y : s.H - 1;
    x = x < s.W - 1 ? x : s.W - 1;
    const size_t plane = (size_t)s.H * (size_t)s.W, i = (size_t)y * (size_t)s.W + (size_t)x;
    return jpeg_ycc(s.rgb[i], s.rgb[plane + i], s.rgb[2 * plane + i], comp);
}

// chroma sample (cy, cx) of a 4:2:0 picture: the downsampled rows are replicated below ceil(H / 2), the full-size columns beyond W, and the
// bias alternates with the output column (libjpeg's h2v2_downsample on its expanded input)
JPEG_HD int jpeg_at_h2v2(const JpegSrc& s, uint32_t comp, int cy, int cx) {
    const int ch = (s.H + 1) / 2;
    cy = cy < ch - 1 ? cy : ch - 1;
    const int y = 2 * cy, x = 2 * cx;
    return (jpeg_at(s, comp, y, x) + jpeg_at(s, comp, y, x + 1) + jpeg_at(s, comp, y + 1, x) + jpeg_at(s, comp, y + 1, x + 1) + 1 + (cx & 1)) >> 2;
}

// one pass of jfdctint over p[0], p[st], .. p[7 * st]; the first pass leaves its results scaled up by 4, the second removes that
JPEG_HD void jpeg_fdct_1d(int* p, int st, bool first) {
    const int d0 = p[0], d1 = p[st], d2 = p[2 * st], d3 = p[3 * st], d4 = p[4 * st], d5 = p[5 * st], d6 = p[6 * st], d7 = p[7 * st];
    int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    const int n = first ? 11 : 15, r = 1 << (n - 1);
    p[0] = first ? (t10 + t11) * 4 : (t10 + t11 + 2) >> 2;           // << PASS1_BITS as a product: the operand may be negative
    p[4 * st] = first ? (t10 - t11) * 4 : (t10 - t11 + 2) >> 2;
    int z1 = (t12 + t13) * 4433;
    p[2 * st] = (z1 + t13 * 6270 + r) >> n;
    p[6 * st] = (z1 - t12 * 15137 + r) >> n;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    t4 *= 2446; t5 *= 16819; t6 *= 25172; t7 *= 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
    p[7 * st] = (t4 + z1 + z3 + r) >> n;
    p[5 * st] = (t5 + z2 + z4 + r) >> n;
    p[3 * st] = (t6 + z2 + z3 + r) >> n;
    p[st] = (t7 + z1 + z4 + r) >> n;
}

JPEG_HD int jpeg_zigzag(int k) {
    constexpr uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return zz[k];
}

// q in 1..255: sign(c) * ((|c| + 4q) / 8q), the DCT's results being scaled by 8
JPEG_HD int jpeg_quant(int c, int q) {
    const int qv = 8 * q, a = c < 0 ? -c : c, v = (a + (qv >> 1)) / qv;
    return c < 0 ? -v : v;
}

// the samples of block (by, bx) of component comp, less 128, transformed: d[8 * row + column], scaled by 8
JPEG_HD void jpeg_block_dct(const JpegSrc& s, int sub, uint32_t comp, uint32_t by, uint32_t bx, int* d) {
    const int y0 = (int)by * 8, x0 = (int)bx * 8;
    const bool half = sub == ELD_JPEG_420 && comp != 0;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) d[8 * i + j] = (half ? jpeg_at_h2v2(s, comp, y0 + i, x0 + j) : jpeg_at(s, comp, y0 + i, x0 + j)) - 128;
#pragma unroll
    for (int i = 0; i < 8; ++i) jpeg_fdct_1d(d + 8 * i, 1, true);
#pragma unroll
    for (int j = 0; j < 8; ++j) jpeg_fdct_1d(d + j, 8, false);
}

// Block b of the scan -> out[64], zigzag order.  q: 2 x 64 divisors in natural order, luma then chroma.  b < g.nblocks.
JPEG_HD void jpeg_block_coef(const JpegSrc& s, const JpegGeom& g, const uint16_t* q, uint32_t b, int16_t* out) {
    const uint32_t m = b / g.bpm, k = b - m * g.bpm, my = m / g.mcux, mx = m - my * g.mcux, comp = jpeg_comp(g, k);
    const uint16_t* qt = q + (comp ? 64 : 0);
    int d[64];
    if (g.sub == ELD_JPEG_420 && comp == 0) {
        const bool right = 2 * mx + 1 >= g.bw, below = 2 * my + 1 >= g.bh;
        uint32_t from = k;                                           // a dummy block takes its DC from block `from` of the MCU
        if (k >= 2 && below) from = right ? 0u : 1u;
        else if ((k & 1u) && right) from = k - 1;
        jpeg_block_dct(s, g.sub, 0, 2 * my + (from >> 1), 2 * mx + (from & 1u), d);
        if (from != k) {
            out[0] = (int16_t)jpeg_quant(d[0], qt[0]);
            for (int i = 1; i < 64; ++i) out[i] = 0;
            return;
        }
    } else {
        jpeg_block_dct(s, g.sub, comp, my, mx, d);
    }
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        const int z = jpeg_zigzag(i);
        out[i] = (int16_t)jpeg_quant(d[z], qt[z]);
    }
}

// ---- the symbols of one block -----------------------------------------------------------------------------------------------------------
// the bits of a magnitude: 0 for 0
JPEG_HD uint32_t jpeg_size(int v) {
    const uint32_t a = (uint32_t)(v < 0 ? -v : v);
    return a ? 32u - (uint32_t)__builtin_clz(a) : 0u;
}

// The walk: sink.dc(difference modulo 65536), then sink.ac(run/size byte, value) per non-zero coefficient, F0 per 16 zeros in front of one and
// 00 behind the last unless coefficient 63 is non-zero.  pred: the DC of the component's previous block.
// blk[k]: coefficient k, from memory (const int16_t*) or from registers (JpegBlockRegs: k is then static, the loop being unrolled).
template <class Blk, class Sink>
JPEG_HD void jpeg_walk(const Blk& blk, int pred, Sink& sink) {
    sink.dc((uint32_t)((int)blk[0] - pred) & 0xFFFFu);
    uint32_t run = 0;
#pragma unroll
    for (int k = 1; k < 64; ++k) {
        const int v = blk[k];
        if (v == 0) { ++run; continue; }
        for (; run >= 16u; run -= 16u) sink.ac(0xF0u, 0);
        const uint32_t sz = jpeg_size(v);
        sink.ac((run << 4) | (sz < 10u ? sz : 10u), v);
        run = 0;
    }
    if (run) sink.ac(0x00u, 0);
}

// an AC symbol's bits, right-justified: the code, then the low size bits of v (v - 1 for v < 0).  *nb = 0 for a symbol without a code.
JPEG_HD uint32_t jpeg_ac_word(uint32_t sym, int v, const uint32_t* ac, uint32_t* nb) {
    const uint32_t e = ac[sym & 255u], len = e >> 16, sz = sym & 15u;
    if (len < 1u || len > 16u) { *nb = 0u; return 0u; }
    const uint32_t x = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << sz) - 1u);
    *nb = len + sz;                                                  // at most 16 + 10
    return ((e & 0xFFFFu) << sz) | x;
}

// counts into the bins of one histogram through add(bin): comp selects the luma or chroma alphabets
template <class Add>
struct JpegHistSink {
    Add& add;
    uint32_t chroma;
    JPEG_HD void dc(uint32_t d) {
        const uint32_t s = dng_enc_ssss(d);
        add((chroma ? JPEG_HIST_DC : 0u) + (s < 11u ? s : 11u));
    }
    JPEG_HD void ac(uint32_t sym, int) { add((chroma ? JPEG_HIST_AC1 : JPEG_HIST_AC0) + sym); }
};

struct JpegBitsSink {
    const uint32_t* dct;
    const uint32_t* act;
    uint32_t bits;
    JPEG_HD void dc(uint32_t d) {
        uint32_t nb;
        (void)dng_enc_word(d, dct, &nb);
        bits += nb;
    }
    JPEG_HD void ac(uint32_t sym, int v) {
        uint32_t nb;
        (void)jpeg_ac_word(sym, v, act, &nb);
        bits += nb;
    }
};

template <class Put>
struct JpegPackSink {
    const uint32_t* dct;
    const uint32_t* act;
    DngEncBits& b;
    Put& put;
    JPEG_HD void dc(uint32_t d) {
        uint32_t nb;
        const uint32_t w = dng_enc_word(d, dct, &nb);
        dng_enc_push(b, w, nb, put);
    }
    JPEG_HD void ac(uint32_t sym, int v) {
        uint32_t nb;
        const uint32_t w = jpeg_ac_word(sym, v, act, &nb);
        dng_enc_push(b, w, nb, put);
    }
};

// A block's 64 coefficients in 32 dwords, read like an array: what a lane holds after eight 16-byte loads.
struct JpegBlockRegs {
    uint32_t w[32];
    JPEG_HD int operator[](int k) const { return (int)(int16_t)(uint16_t)(w[k >> 1] >> (16 * (k & 1))); }
};

// The coefficient buffer as the walks see it: coef.block(b) is indexable by k, coef.dc(b) is coefficient 0 of block b.  This one reads memory
// element by element (the host check); jpeg.hip's loads a block into registers.
struct JpegCoefMem {
    const int16_t* p;
    JPEG_HD const int16_t* block(uint32_t b) const { return p + (size_t)b * 64; }
    JPEG_HD int dc(uint32_t b) const { return p[(size_t)b * 64]; }
};

// the DC predictor of block b, read from the coefficients
template <class Coef>
JPEG_HD int jpeg_pred(const Coef& coef, const JpegGeom& g, uint32_t b) {
    uint32_t p;
    return jpeg_prev_block(g, b, &p) ? coef.dc(p) : 0;
}

template <class Coef, class Add>
JPEG_HD void jpeg_block_hist(const Coef& coef, const JpegGeom& g, uint32_t b, Add& add) {
    JpegHistSink<Add> sink = {add, jpeg_comp(g, b % g.bpm) ? 1u : 0u};
    jpeg_walk(coef.block(b), jpeg_pred(coef, g, b), sink);
}

// the bits of the blocks [first, first + count) of the scan; tables: ELD_JPEG_TABLE entries
template <class Coef>
JPEG_HD uint32_t jpeg_run_bits(const Coef& coef, const JpegGeom& g, const uint32_t* tables, uint32_t first, uint32_t count) {
    uint32_t bits = 0;
    for (uint32_t b = first; b < first + count; ++b) {
        const bool c = jpeg_comp(g, b % g.bpm) != 0;
        JpegBitsSink sink = {tables + (c ? JPEG_TAB_DC : 0u), tables + (c ? JPEG_TAB_AC1 : JPEG_TAB_AC0), 0u};
        jpeg_walk(coef.block(b), jpeg_pred(coef, g, b), sink);
        bits += sink.bits;                                           // a block: at most 27 + 63 * 26 bits
    }
    return bits;
}

// The run's bits into the dword image whose bit 0 is the top bit of dword 0, from bit bit0 on (dng_enc_run's contract: put() must OR; pad
// 1-bits behind the scan's last block).
template <class Coef, class Put>
JPEG_HD void jpeg_run_pack(const Coef& coef, const JpegGeom& g, const uint32_t* tables, uint32_t first, uint32_t count, uint32_t bit0, uint32_t pad,
                           Put& put) {
    DngEncBits bb;
    bb.acc = 0; bb.n = bit0 & 31u; bb.idx = bit0 >> 5;
    for (uint32_t b = first; b < first + count; ++b) {
        const bool c = jpeg_comp(g, b % g.bpm) != 0;
        JpegPackSink<Put> sink = {tables + (c ? JPEG_TAB_DC : 0u), tables + (c ? JPEG_TAB_AC1 : JPEG_TAB_AC0), bb, put};
        jpeg_walk(coef.block(b), jpeg_pred(coef, g, b), sink);
    }
    if (pad) dng_enc_push(bb, (1u << pad) - 1u, pad, put);
    if (bb.n) put(bb.idx, (uint32_t)(bb.acc >> 32));
}
