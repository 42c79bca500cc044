// dng_dev.h -- the per-stream decoders of the DNG reader (dng.hip), as functions a plain host compiler accepts too:
// tools/dng_hostcheck.cpp runs them under AddressSanitizer on truncated and corrupted streams, which is how "a corrupt file never turns
// into a wild access" is shown without a GPU.  Nothing here is HIP-only; under hipcc the functions are __host__ __device__.
//
// The rule of the file: no address is formed from the stream's bytes or from a record's fields before it has been compared with the buffer
// it indexes.  A stream stops at its first violation and returns the ELD_DNG_* status that names it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/eld_amd.h"

#if defined(__HIPCC__)
#define DNG_HD __host__ __device__ __forceinline__
#else
#define DNG_HD inline
#endif

// where the decoded samples go: the visible mosaic, the active area applied on the write
struct DngOut {
    uint16_t* out;
    int H, W, top, left, Hm, Wm;
    const uint16_t* lin;
    int lin_len;
};

// sample v of the full image's site (y, x): dropped beyond the image (an edge tile's padding) and outside the active area
DNG_HD void dng_put(const DngOut& o, int y, int x, uint32_t v) {
    if (y < 0 || x < 0 || y >= o.H || x >= o.W) return;
    const int yy = y - o.top, xx = x - o.left;
    if (yy < 0 || xx < 0 || yy >= o.Hm || xx >= o.Wm) return;
    if (o.lin) v = o.lin[v < (uint32_t)(o.lin_len - 1) ? v : (uint32_t)(o.lin_len - 1)];
    o.out[(size_t)yy * (size_t)o.Wm + (size_t)xx] = (uint16_t)v;
}

// The bit reader: up to 64 bits, left-justified (the next bit is bit 63).  Bytes come from [pos, end) of the blob with the FF 00 stuffing
// removed; any other FF xx is a marker and ends the data.
struct DngBits {
    const uint8_t* p;
    uint64_t acc;
    uint32_t pos, end;
    int n;
};

// at least 33 bits afterwards, or every byte of the stream taken
DNG_HD void dng_refill(DngBits& b) {
    while (b.n <= 32 && b.pos < b.end) {
        if (b.end - b.pos >= 4u) {
            const uint32_t b0 = b.p[b.pos], b1 = b.p[b.pos + 1], b2 = b.p[b.pos + 2], b3 = b.p[b.pos + 3];
            if (b0 != 0xFFu && b1 != 0xFFu && b2 != 0xFFu && b3 != 0xFFu) {
                const uint32_t w = (b0 << 24) | (b1 << 16) | (b2 << 8) | b3;
                b.acc |= (uint64_t)w << (32 - b.n);
                b.n += 32;
                b.pos += 4;
                continue;
            }
        }
        const uint32_t v = b.p[b.pos];
        if (v == 0xFFu) {
            if (b.end - b.pos < 2u || b.p[b.pos + 1] != 0u) {      // a marker (EOI), or an FF that the stream's end cuts: no more data
                b.pos = b.end;
                break;
            }
            b.pos += 2;
        } else {
            b.pos += 1;
        }
        b.acc |= (uint64_t)v << (56 - b.n);
        b.n += 8;
    }
}

// One difference: Huffman symbol SSSS, then SSSS extra bits.  -> ELD_DNG_OK with the difference (modulo 65536) in *diff.
DNG_HD int dng_diff(DngBits& b, const EldDngHuff& t, uint32_t* diff) {
    dng_refill(b);
    const uint32_t top16 = (uint32_t)(b.acc >> 48);
    uint32_t e = t.fast[top16 >> (16 - ELD_DNG_FAST_BITS)];       // the index has ELD_DNG_FAST_BITS bits: inside fast[]
    int len = (int)(e >> 8);
    uint32_t sym = e & 0xFFu;
    if (e == 0u) {
        len = 0;
        for (int l = ELD_DNG_FAST_BITS + 1; l <= 16; ++l) {
            const int32_t c = (int32_t)(top16 >> (16 - l));
            if (c <= t.maxcode[l]) {
                const int32_t i = c + t.valoff[l];
                if (i < 0 || i >= t.nvals || i >= 32) return ELD_DNG_BADCODE;
                sym = t.vals[i];
                len = l;
                break;
            }
        }
        if (len == 0) return b.n < 16 ? ELD_DNG_TRUNCATED : ELD_DNG_BADCODE;
    }
    if (len < 1 || len > 16 || sym > 16u) return ELD_DNG_BADCODE;
    if (len > b.n) return ELD_DNG_TRUNCATED;
    b.acc <<= len;
    b.n -= len;
    if (sym == 0u) {
        *diff = 0u;
    } else if (sym == 16u) {
        *diff = 32768u;
    } else {
        if ((int)sym > b.n) return ELD_DNG_TRUNCATED;
        uint32_t v = (uint32_t)(b.acc >> (64 - sym));
        b.acc <<= sym;
        b.n -= (int)sym;
        if (v < (1u << (sym - 1u))) v -= (1u << sym) - 1u;          // negative differences: wraps, and the sum below is modulo 65536
        *diff = v & 0xFFFFu;
    }
    return ELD_DNG_OK;
}

// A record's fields, before anything is read through them.
DNG_HD bool dng_record_ok(const EldDngStream& s, size_t blob_bytes, int ntables, size_t ws_elems) {
    if ((uint64_t)s.data_off + (uint64_t)s.data_len > (uint64_t)blob_bytes || (uint64_t)s.data_off + (uint64_t)s.data_len > 0xFFFFFFFFull) return false;
    if (s.x0 < 0 || s.y0 < 0 || s.tw < 1 || s.th < 1 || s.tw > 65536 || s.th > 65536) return false;
    if (s.P < 2 || s.P > 16 || s.Nf < 1 || s.Nf > 4 || s.pred < 1 || s.pred > 7 || s.X < 1 || s.Y < 1 || s.X > 65535 || s.Y > 65535) return false;
    for (int k = 0; k < s.Nf; ++k)
        if ((int)s.table[k] >= ntables) return false;
    if (s.pred >= 2 && (uint64_t)s.ws_off + (uint64_t)s.X * (uint64_t)s.Nf > (uint64_t)ws_elems) return false;
    return true;
}

// One lossless-JPEG stream (ITU-T T.81 process 14, one scan, no restart interval, no point transform): X * Y * Nf samples, written into the
// tile linearly.  Predictors: 1 Ra, 2 Rb, 3 Rc, 4 Ra + Rb - Rc, 5 Ra + ((Rb - Rc) >> 1), 6 Rb + ((Ra - Rc) >> 1), 7 (Ra + Rb) >> 1 with
// Ra the left, Rb the upper and Rc the upper-left sample of the same component; the first sample 2^(P-1), the rest of the first line Ra, the
// first column Rb.  Ra, Rc and the first column live in registers; Rb comes from the stream's row in ws (predictors 2..7 only).
DNG_HD int dng_ljpeg_stream(const uint8_t* blob, size_t blob_bytes, const EldDngStream& s, const EldDngHuff* tables, int ntables, uint16_t* ws,
                            size_t ws_elems, const DngOut& o) {
    if (!dng_record_ok(s, blob_bytes, ntables, ws_elems)) return ELD_DNG_BADRECORD;
    DngBits b;
    b.p = blob; b.acc = 0; b.pos = s.data_off; b.end = s.data_off + s.data_len; b.n = 0;
    const bool rows = s.pred >= 2;
    uint16_t* row = rows ? ws + s.ws_off : nullptr;
    uint32_t left[4] = {0, 0, 0, 0}, up0[4] = {0, 0, 0, 0}, upl[4] = {0, 0, 0, 0};
    int r = 0, c = 0;                                                // where the next sample lands in the tile
    for (int y = 0; y < s.Y; ++y) {
        for (int x = 0; x < s.X; ++x) {
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int k = 0; k < 4; ++k) {
                if (k >= s.Nf) break;
                if (r >= s.th) return ELD_DNG_TOOMANY;              // before a bit of the sample is read: the tile is full
                uint32_t d;
                const int st = dng_diff(b, tables[s.table[k]], &d);
                if (st != ELD_DNG_OK) return st;
                const int idx = x * s.Nf + k;                       // < X * Nf, which dng_record_ok compared with the row's room in ws
                uint32_t rb = 0;
                if (rows && y > 0) rb = row[idx];
                int32_t px;
                if (y == 0) px = x == 0 ? (int32_t)(1u << (s.P - 1)) : (int32_t)left[k];
                else if (x == 0) px = (int32_t)up0[k];
                else {
                    const int32_t ra = (int32_t)left[k], rc = (int32_t)upl[k], ub = (int32_t)rb;
                    switch (s.pred) {
                        case 1: px = ra; break;
                        case 2: px = ub; break;
                        case 3: px = rc; break;
                        case 4: px = ra + ub - rc; break;
                        case 5: px = ra + ((ub - rc) >> 1); break;
                        case 6: px = ub + ((ra - rc) >> 1); break;
                        default: px = (ra + ub) >> 1; break;
                    }
                }
                const uint32_t v = ((uint32_t)px + d) & 0xFFFFu;
                left[k] = v;
                upl[k] = rb;
                if (x == 0) up0[k] = v;
                if (rows) row[idx] = (uint16_t)v;
                dng_put(o, s.y0 + r, s.x0 + c, v);
                if (++c == s.tw) { c = 0; ++r; }
            }
        }
    }
    return ELD_DNG_OK;
}

// Four packed samples of an uncompressed stream: the quad g of row r.  bits in {8, 10, 12, 14, 16}; a quad starts on a byte boundary
// (4 * bits is a multiple of 8) and takes bits / 2 bytes, fewer at the row's end.  The caller has checked th * rowbytes against the stream.
DNG_HD void dng_unpack_quad(const uint8_t* rowp, uint32_t rowbytes, int g, int bits, bool big_endian, const EldDngStream& s, int r, const DngOut& o) {
    const uint32_t q = (uint32_t)bits >> 1, off = (uint32_t)g * q;
    uint64_t acc = 0;
    for (uint32_t i = 0; i < 8u; ++i) {
        if (i < q && off + i < rowbytes) acc |= (uint64_t)rowp[off + i] << (56 - 8 * i);
    }
    const uint32_t mask = (1u << bits) - 1u;
    for (int j = 0; j < 4; ++j) {
        const int c = 4 * g + j;
        if (c >= s.tw) break;
        uint32_t v = (uint32_t)(acc >> (64 - bits * (j + 1))) & mask;
        if (bits == 16 && !big_endian) v = ((v & 0xFFu) << 8) | (v >> 8);
        dng_put(o, s.y0 + r, s.x0 + c, v);
    }
}

// rows of `tw` samples of `bits` bits, each padded to a byte
DNG_HD uint32_t dng_row_bytes(int tw, int bits) { return (uint32_t)(((uint64_t)tw * (uint64_t)bits + 7u) >> 3); }

// an uncompressed stream's record: its rows lie inside its byte range, and that inside the blob
DNG_HD bool dng_unpack_record_ok(const EldDngStream& s, size_t blob_bytes, int bits) {
    if ((uint64_t)s.data_off + (uint64_t)s.data_len > (uint64_t)blob_bytes) return false;
    if (s.x0 < 0 || s.y0 < 0 || s.tw < 1 || s.th < 1 || s.tw > 65536 || s.th > 65536) return false;
    return (uint64_t)s.th * (uint64_t)dng_row_bytes(s.tw, bits) <= (uint64_t)s.data_len;
}
