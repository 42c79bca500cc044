"""NumPy restatement of DNG WarpRectilinear as DESIGN.md sec. 30 defines it (csrc/warp_dev.h, csrc/warp.hip).  It shares no code with the package:
the parameter bytes, the float64 map with every operation rounded on its own, the NaN-safe clamp, the replicated edge and the float32
Catmull-Rom sum are written out here in the stated order, vectorised over the image.  The tail (CCM, tone curve, quantiser) is the one
tests/demosaic_ref.py already restates."""
import struct

import numpy as np

import demosaic_ref as DM

F32, F64 = np.float32, np.float64
IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 0.0)


# ---- the opcode's bytes -------------------------------------------------------------------------------------------------------------------
def pack_params(sets, cx, cy):
    """big-endian: uint32 N, N x (kr0, kr1, kr2, kr3, kt0, kt1) float64, cx, cy float64"""
    sets = np.asarray(sets, F64).reshape(-1, 6)
    return struct.pack('>I', len(sets)) + b''.join(struct.pack('>6d', *row) for row in sets.tolist()) + struct.pack('>2d', cx, cy)


def spec(sets, cx, cy, flags=0):
    """the dict tests/dng_opcodes_ref.py pack_list takes for an opcode it does not type"""
    return {'id': 1, 'flags': flags, 'data': pack_params(sets, cx, cy)}


# ---- the map ------------------------------------------------------------------------------------------------------------------------------
def record(sets, cx, cy, Hm, Wm):
    """what the host forms: k with kr0 - 1 in place of kr0, the centre in pixels, m2 and m"""
    k = np.array(sets, F64).reshape(-1, 6)
    k[:, 0] = k[:, 0] - F64(1)
    cxp, cyp = F64(cx) * F64(Wm), F64(cy) * F64(Hm)
    mx, my = max(abs(cxp), abs(F64(Wm) - cxp)), max(abs(cyp), abs(F64(Hm) - cyp))
    m2 = mx * mx + my * my
    return {'k': k, 'cxp': cxp, 'cyp': cyp, 'm2': m2, 'm': np.sqrt(m2)}


def coords(k, rec, Hm, Wm):
    """(u, v), float64 (Hm,Wm), of one coefficient set k = (kr0 - 1, kr1, kr2, kr3, kt0, kt1), before the clamp"""
    with np.errstate(all='ignore'):
        px = (np.arange(Wm, dtype=F64) + F64(0.5))[None, :] + np.zeros((Hm, 1), F64)
        py = (np.arange(Hm, dtype=F64) + F64(0.5))[:, None] + np.zeros((1, Wm), F64)
        m, m2 = rec['m'], rec['m2']
        dx, dy = px - rec['cxp'], py - rec['cyp']
        r2 = (dx * dx + dy * dy) / m2
        g = k[0] + r2 * (k[1] + r2 * (k[2] + r2 * k[3]))
        nx, ny = dx / m, dy / m
        nxy2 = (F64(2) * nx) * ny
        tx = k[4] * nxy2 + k[5] * (r2 + (F64(2) * nx) * nx)
        ty = k[5] * nxy2 + k[4] * (r2 + (F64(2) * ny) * ny)
        u = (px + (g * dx + m * tx)) - F64(0.5)
        v = (py + (g * dy + m * ty)) - F64(0.5)
    return u, v


def cell(c, L):
    """clamp to [-1, L] with NaN -> -1, then (floor as int64, float32 fraction)"""
    c = np.where(c >= -1.0, c, F64(-1))                               # NaN compares false
    c = np.where(c > F64(L), F64(L), c)
    f = np.floor(c)
    return f.astype(np.int64), (c - f).astype(F32)


def weights(t):
    """Catmull-Rom, float32, every product and sum rounded on its own"""
    t = np.asarray(t, F32)
    tt = t * t
    w0 = t * ((t * ((F32(-0.5) * t) + F32(1))) - F32(0.5))
    w1 = (tt * ((F32(1.5) * t) - F32(2.5))) + F32(1)
    w2 = t * ((t * ((F32(-1.5) * t) + F32(2))) + F32(0.5))
    w3 = tt * ((F32(0.5) * t) - F32(0.5))
    return [w0, w1, w2, w3]


def sample(plane, u, v):
    """one (Hm,Wm) float32 plane at the float64 coordinates (u, v): taps clamped to the image, rows first, then their column"""
    Hm, Wm = plane.shape
    i0, ty = cell(v, Hm)
    j0, tx = cell(u, Wm)
    wx, wy = weights(tx), weights(ty)
    cols = [np.clip(j0 - 1 + q, 0, Wm - 1) for q in range(4)]
    with np.errstate(all='ignore'):
        h = []
        for i in range(4):
            row = np.clip(i0 - 1 + i, 0, Hm - 1)
            p = [plane[row, cols[j]] for j in range(4)]
            h.append(((wx[0] * p[0] + wx[1] * p[1]) + wx[2] * p[2]) + wx[3] * p[3])
        val = ((wy[0] * h[0] + wy[1] * h[1]) + wy[2] * h[2]) + wy[3] * h[3]
    assert val.dtype == F32
    return val


def footprint(u, v, Hm, Wm):
    """the clamped tap rows (4,Hm,Wm) and columns (4,Hm,Wm) of every destination pixel"""
    i0, _ = cell(v, Hm)
    j0, _ = cell(u, Wm)
    return (np.stack([np.clip(i0 - 1 + q, 0, Hm - 1) for q in range(4)]), np.stack([np.clip(j0 - 1 + q, 0, Wm - 1) for q in range(4)]))


def warp(rgb, sets, cx, cy):
    """(N,3,Hm,Wm) float32 camera RGB -> the resampled (N,3,Hm,Wm) float32, unclamped.  sets: one row for the three planes, or three (R, G, B)"""
    rgb = np.asarray(rgb, F32)
    N, _, Hm, Wm = rgb.shape
    rec = record(sets, cx, cy, Hm, Wm)
    uv = [coords(k, rec, Hm, Wm) for k in rec['k']]
    out = np.empty_like(rgb)
    for c in range(3):
        u, v = uv[c if len(uv) == 3 else 0]
        for n in range(N):
            out[n, c] = sample(rgb[n, c], u, v)
    return out


def warp_linear(rgb, sets, cx, cy, ccms=None):
    """ELD_RENDER_LINEAR_F32: the resampled values, after the CCM when there is one"""
    w = warp(rgb, sets, cx, cy)
    return w if ccms is None else DM.apply_ccm(w, ccms)


def warp_srgb8(rgb, sets, cx, cy, ccms=None, gamma=2.2, CRF=None):
    """ELD_RENDER_SRGB8: without a matrix the tail multiplies by the identity, as the kernels do"""
    w = warp(rgb, sets, cx, cy)
    eye = np.tile(np.eye(3, dtype=F32).reshape(1, 9), (w.shape[0], 1))
    return DM.srgb8(DM.apply_ccm(w, eye if ccms is None else ccms), gamma, CRF)
