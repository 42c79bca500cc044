// dng_opcodes_dev.h -- the per-site evaluator of the mosaic-domain DNG opcodes (dng_opcodes.hip, eld_amd/dng_opcodes.py),
// as functions a plain host compiler accepts too: tools/dng_opcodes_hostcheck.cpp runs them under AddressSanitizer on corrupted operation
// records.  Nothing here is HIP-only; under hipcc the functions are __host__ __device__.
//
// The rule of the file is dng_dev.h's: no address is formed from a record's field or from the blob before it has been compared with the
// buffer it indexes.  opc_record_ok compares every field of a record with the blob and the image; an operation whose record fails addresses
// no site, so the site keeps its value.  The blob's own contents (gains, tables, vectors) are values, never indices, with one exception: a
// GainMap's cell index comes from the record's float64 origin and spacing, and is clamped to the map (NaN included) before it is used.
//
// Arithmetic (the contract tests/dng_opcodes_ref.py restates bit for bit): every float32 product and sum is rounded on its own -- OPC_MUL /
// OPC_ADD / OPC_SUB are __fmul_rn and friends on the device, and the plain operators elsewhere, where the build passes -ffp-contract=off.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/eld_amd.h"

#if defined(__HIPCC__)
#define OPC_HD __host__ __device__ __forceinline__
#else
#define OPC_HD inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define OPC_MUL(a, b) __fmul_rn((a), (b))
#define OPC_ADD(a, b) __fadd_rn((a), (b))
#define OPC_SUB(a, b) __fsub_rn((a), (b))
#define OPC_DIV(a, b) __fdiv_rn((a), (b))
#else
#define OPC_MUL(a, b) ((float)(a) * (float)(b))
#define OPC_ADD(a, b) ((float)(a) + (float)(b))
#define OPC_SUB(a, b) ((float)(a) - (float)(b))
#define OPC_DIV(a, b) ((float)(a) / (float)(b))
#endif

// What an operation knows of one row (axis 0) or one column (axis 1): whether its area addresses it, and the part of its arithmetic that
// depends on that coordinate alone.  GainMap: the lower cell index and the weight towards the next one.  Per-row / per-column vectors: the
// vector's entry on their own axis.  The kernels keep these per row and per column of a block's tile; a site combines one of each.
struct OpcAxis {
    uint32_t idx;                        // bit 31: addressed; bits 0..30: GainMap i0
    float w;                             // GainMap weight; Delta / Scale: the entry
};
#define OPC_ADDRESSED 0x80000000u

OPC_HD bool opc_is_gain_kind(int kind) {
    return kind == ELD_DNG_OP_GAINMAP || kind == ELD_DNG_OP_SCALEPERROW || kind == ELD_DNG_OP_SCALEPERCOL || kind == ELD_DNG_OP_VIGNETTE;
}

// bytes of the operation's parameters in the blob
OPC_HD uint64_t opc_data_bytes(const EldDngOp& op) {
    switch (op.kind) {
        case ELD_DNG_OP_MAPTABLE: return 2ull * (uint64_t)(uint32_t)op.n0;
        case ELD_DNG_OP_MAPPOLY: return 4ull * ((uint64_t)(uint32_t)op.n0 + 1ull);
        case ELD_DNG_OP_GAINMAP: return 4ull * (uint64_t)(uint32_t)op.n0 * (uint64_t)(uint32_t)op.n1;
        case ELD_DNG_OP_DELTAPERROW: case ELD_DNG_OP_DELTAPERCOL: case ELD_DNG_OP_SCALEPERROW: case ELD_DNG_OP_SCALEPERCOL:
            return 4ull * (uint64_t)(uint32_t)op.n0;
        default: return 0;
    }
}

// A record's fields against the image and the blob, before anything is read through them.
OPC_HD bool opc_record_ok(const EldDngOp& op, size_t blob_bytes, int Hm, int Wm) {
    if (Hm < 1 || Wm < 1) return false;
    if (op.top < 0 || op.left < 0 || op.bottom <= op.top || op.right <= op.left || op.bottom > Hm || op.right > Wm) return false;
    if (op.row_pitch < 1 || op.col_pitch < 1) return false;
    switch (op.kind) {
        case ELD_DNG_OP_VIGNETTE: return true;
        case ELD_DNG_OP_MAPTABLE: if (op.n0 < 1 || op.n0 > 65536) return false; break;
        case ELD_DNG_OP_MAPPOLY: if (op.n0 < 0 || op.n0 > 8) return false; break;
        case ELD_DNG_OP_GAINMAP: if (op.n0 < 1 || op.n1 < 1 || (uint64_t)op.n0 * (uint64_t)op.n1 > (1ull << 24)) return false; break;
        case ELD_DNG_OP_DELTAPERROW: case ELD_DNG_OP_SCALEPERROW:
            if (op.n0 < 1 || ((int64_t)op.bottom - 1 - op.top) / op.row_pitch >= (int64_t)op.n0) return false;
            break;
        case ELD_DNG_OP_DELTAPERCOL: case ELD_DNG_OP_SCALEPERCOL:
            if (op.n0 < 1 || ((int64_t)op.right - 1 - op.left) / op.col_pitch >= (int64_t)op.n0) return false;
            break;
        default: return false;
    }
    if (op.data_off & 3u) return false;
    return (uint64_t)op.data_off + opc_data_bytes(op) <= (uint64_t)blob_bytes;
}

// the GainMap coordinate of pixel `c` of `extent`: float64, in this order; NaN and everything below 0 become 0
OPC_HD void opc_map_coord(int c, int extent, int points, double origin, double spacing, uint32_t* i0, float* w) {
    double v = 0.0;
    if (points > 1 && spacing != 0.0) v = (((double)c + 0.5) / (double)extent - origin) / spacing;
    if (!(v >= 0.0)) v = 0.0;
    const double hi = (double)(points - 1);
    if (v > hi) v = hi;
    const double f = floor(v);
    *i0 = (uint32_t)f;                                               // 0 <= f <= points - 1 < 2^24
    *w = (float)(v - f);
}

// One operation on one axis.  `ok` is opc_record_ok of the record; without it nothing is addressed and the blob is not read.
OPC_HD OpcAxis opc_axis(const EldDngOp& op, bool ok, const uint8_t* blob, int axis, int c, int Hm, int Wm) {
    OpcAxis e;
    e.idx = 0u;
    e.w = 0.f;
    if (!ok) return e;
    const int lo = axis == 0 ? op.top : op.left, hi = axis == 0 ? op.bottom : op.right, pitch = axis == 0 ? op.row_pitch : op.col_pitch;
    if (c < lo || c >= hi || (c - lo) % pitch != 0) return e;
    e.idx = OPC_ADDRESSED;
    if (op.kind == ELD_DNG_OP_GAINMAP) {
        uint32_t i0;
        if (axis == 0) opc_map_coord(c, Hm, op.n0, op.p[2], op.p[0], &i0, &e.w);
        else opc_map_coord(c, Wm, op.n1, op.p[3], op.p[1], &i0, &e.w);
        e.idx |= i0;
    } else if ((axis == 0 && (op.kind == ELD_DNG_OP_DELTAPERROW || op.kind == ELD_DNG_OP_SCALEPERROW)) ||
               (axis == 1 && (op.kind == ELD_DNG_OP_DELTAPERCOL || op.kind == ELD_DNG_OP_SCALEPERCOL))) {
        const int k = (c - lo) / pitch;                              // < n0: opc_record_ok compared the area's last line with it
        e.w = ((const float*)(blob + op.data_off))[k];
    }
    return e;
}

OPC_HD float opc_clip(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }          // NaN stays NaN

// A GainMap's gain from its axis entries.  g: the map's V x H float32 (in the blob, or the kernel's copy of it in LDS).
OPC_HD float opc_map_gain(const float* g, int n0, int n1, OpcAxis r, OpcAxis c) {
    const uint32_t i0 = r.idx & ~OPC_ADDRESSED, j0 = c.idx & ~OPC_ADDRESSED;
    const uint32_t i1 = i0 + 1u < (uint32_t)n0 ? i0 + 1u : (uint32_t)n0 - 1u, j1 = j0 + 1u < (uint32_t)n1 ? j0 + 1u : (uint32_t)n1 - 1u;
    const float wx = c.w, wy = r.w, ux = OPC_SUB(1.f, wx), uy = OPC_SUB(1.f, wy);
    const float* r0 = g + (size_t)i0 * (size_t)n1;
    const float* r1 = g + (size_t)i1 * (size_t)n1;
    const float a = OPC_ADD(OPC_MUL(r0[j0], ux), OPC_MUL(r0[j1], wx));
    const float b = OPC_ADD(OPC_MUL(r1[j0], ux), OPC_MUL(r1[j1], wx));
    return OPC_ADD(OPC_MUL(a, uy), OPC_MUL(b, wy));
}

// FixVignetteRadial at pixel centres, float64 throughout, rounded once.  p: k0..k4, cx, cy (relative).
OPC_HD float opc_vignette(const EldDngOp& op, int y, int x, int Hm, int Wm) {
    const double mx = op.p[5] * (double)Wm, my = op.p[6] * (double)Hm;
    const double ex = fmax(fabs(mx), fabs((double)Wm - mx)), ey = fmax(fabs(my), fabs((double)Hm - my));
    const double R2 = ex * ex + ey * ey;                             // the farthest image corner
    const double dx = ((double)x + 0.5) - mx, dy = ((double)y + 0.5) - my;
    const double r2 = (dx * dx + dy * dy) / R2;
    return (float)(1.0 + r2 * (op.p[0] + r2 * (op.p[1] + r2 * (op.p[2] + r2 * (op.p[3] + r2 * op.p[4])))));
}

// One list-2 operation on an addressed site's value (a NaN never comes here).  maps: where the GainMap's gains are read.
OPC_HD float opc_apply(const EldDngOp& op, const uint8_t* blob, const float* maps, OpcAxis r, OpcAxis c, float v) {
    switch (op.kind) {
        case ELD_DNG_OP_GAINMAP: return opc_clip(OPC_MUL(v, opc_map_gain(maps, op.n0, op.n1, r, c)));
        case ELD_DNG_OP_SCALEPERROW: return opc_clip(OPC_MUL(v, r.w));
        case ELD_DNG_OP_SCALEPERCOL: return opc_clip(OPC_MUL(v, c.w));
        case ELD_DNG_OP_DELTAPERROW: return opc_clip(OPC_ADD(v, r.w));
        case ELD_DNG_OP_DELTAPERCOL: return opc_clip(OPC_ADD(v, c.w));
        case ELD_DNG_OP_MAPPOLY: {
            const float* co = (const float*)(blob + op.data_off);
            float acc = co[op.n0];
            for (int k = op.n0 - 1; k >= 0; --k) acc = OPC_ADD(OPC_MUL(acc, v), co[k]);
            return opc_clip(acc);
        }
        case ELD_DNG_OP_MAPTABLE: {
            float t = rintf(OPC_MUL(v, 65535.f));                    // ties to even
            if (!(t >= 0.f)) t = 0.f;
            if (t > 65535.f) t = 65535.f;
            int i = (int)t;
            if (i > op.n0 - 1) i = op.n0 - 1;
            return OPC_DIV((float)((const uint16_t*)(blob + op.data_off))[i], 65535.f);
        }
        default: return v;
    }
}

// One operation's factor of the gain plane at an addressed site.
OPC_HD float opc_factor(const EldDngOp& op, const float* maps, OpcAxis r, OpcAxis c, int y, int x, int Hm, int Wm) {
    switch (op.kind) {
        case ELD_DNG_OP_GAINMAP: return opc_map_gain(maps, op.n0, op.n1, r, c);
        case ELD_DNG_OP_SCALEPERROW: return r.w;
        case ELD_DNG_OP_SCALEPERCOL: return c.w;
        case ELD_DNG_OP_VIGNETTE: return opc_vignette(op, y, x, Hm, Wm);
        default: return 1.f;
    }
}

// The whole program at one site, nothing cached: what the kernels compute, restated for the host check.  gain_mode: the product of the
// multiplicative operations, unclipped, from 1; else the list-2 chain on `v`.
OPC_HD float opc_eval_site(const EldDngOp* ops, int nops, const uint8_t* blob, size_t blob_bytes, int Hm, int Wm, int y, int x, float v,
                           bool gain_mode) {
    if (gain_mode) v = 1.f;
    else if (!(v == v)) return v;
    if (y < 0 || x < 0 || y >= Hm || x >= Wm) return v;
    for (int i = 0; i < nops; ++i) {
        const EldDngOp& op = ops[i];
        const bool ok = opc_record_ok(op, blob_bytes, Hm, Wm) && (gain_mode ? opc_is_gain_kind(op.kind) : op.kind != ELD_DNG_OP_VIGNETTE);
        const OpcAxis r = opc_axis(op, ok, blob, 0, y, Hm, Wm), c = opc_axis(op, ok, blob, 1, x, Hm, Wm);
        if (!(r.idx & c.idx & OPC_ADDRESSED)) continue;
        const float* maps = (const float*)(blob + op.data_off);
        v = gain_mode ? OPC_MUL(v, opc_factor(op, maps, r, c, y, x, Hm, Wm)) : opc_apply(op, blob, maps, r, c, v);
    }
    return v;
}
