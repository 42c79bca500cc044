"""NumPy restatement of the frame as DESIGN.md sec. 34 defines it (csrc/frame_dev.h, csrc/frame.hip, eld_amd/isp.py Frame).  It shares no code
with the package: the upright size, the per-axis tap tables (one output at a time, in the stated order of operations), the two float32 tap
sums and the orientation table are written out here.  The tail (CCM, tone curve, quantiser) is the one tests/demosaic_ref.py already
restates."""
import math

import numpy as np

import demosaic_ref as DM

F32, F64 = np.float32, np.float64
MAX_TAPS = 4096


# ---- geometry -----------------------------------------------------------------------------------------------------------------------------
def unoriented(o, Y, X, Hc, Wc):
    """upright pixel (Y, X) -> the unoriented pixel (i, j) of the Hc x Wc grid it takes; the table of the contract, row by row"""
    return {1: (Y, X), 2: (Y, Wc - 1 - X), 3: (Hc - 1 - Y, Wc - 1 - X), 4: (Hc - 1 - Y, X),
            5: (X, Y), 6: (Hc - 1 - X, Y), 7: (Hc - 1 - X, Wc - 1 - Y), 8: (X, Wc - 1 - Y)}[o]


def orient(planes, o):
    """(..., Hc, Wc) unoriented -> (..., Ho, Wo) upright, by the table above (index arithmetic only)"""
    Hc, Wc = planes.shape[-2:]
    Ho, Wo = (Hc, Wc) if o <= 4 else (Wc, Hc)
    Y, X = np.mgrid[0:Ho, 0:Wo]
    i, j = unoriented(o, Y, X, Hc, Wc)
    return np.ascontiguousarray(planes[..., i, j])


def nearest_side(v):
    return max(1, int(math.floor(float(v) + 0.5)))


def out_size(crop, o, size):
    """the upright (Ho, Wo): size None -> the crop's own sides rounded; an int -> the long edge, the other side in proportion; a pair -> itself"""
    ch, cw = float(crop[2]), float(crop[3])
    uh, uw = (ch, cw) if o <= 4 else (cw, ch)
    if size is None:
        return nearest_side(uh), nearest_side(uw)
    if isinstance(size, int):
        return (size, nearest_side(size * uw / uh)) if uh >= uw else (nearest_side(size * uh / uw), size)
    return int(size[0]), int(size[1])


# ---- tap tables ---------------------------------------------------------------------------------------------------------------------------
def lanczos3(x):
    if not abs(x) < 3.0:
        return F64(0)
    if x == 0:
        return F64(1)
    a, b = F64(np.pi) * x, (F64(np.pi) * x) / F64(3)
    return (np.sin(a) / a) * (np.sin(b) / b)


def axis_taps(S, q, c, n, flt, shift=0.0):
    """one axis: source length S, crop origin q, crop length c, n outputs -> (start (n,), count (n,), weights float32 (n,T)), padding zero.
    shift: added to every lanczos centre (a negative control of the tests; the contract has 0)."""
    q, c = F64(q), F64(c)
    scale = c / F64(n)
    rows = []
    for i in range(n):
        if flt == 'area':
            a = min(max(q + F64(i) * scale, F64(0)), F64(S))
            b = min(max(q + F64(i + 1) * scale, F64(0)), F64(S))
            lo, hi = int(math.floor(a)), int(math.ceil(b))
            w = [min(b, F64(k + 1)) - max(a, F64(k)) for k in range(lo, hi)]
        elif flt == 'lanczos':
            fs = max(scale, F64(1))
            centre = q + (F64(i) + F64(0.5)) * scale + F64(shift)
            lo = max(0, int(math.floor(centre - F64(3) * fs + F64(0.5))))
            hi = min(S, int(math.floor(centre + F64(3) * fs + F64(0.5))))
            w = [lanczos3(((F64(k) + F64(0.5)) - centre) / fs) for k in range(lo, hi)]
        else:
            raise ValueError(flt)
        assert hi > lo, (i, lo, hi)
        W = w[0]
        for v in w[1:]:
            W = W + v
        rows.append((lo, [F32(v / W) for v in w]))
    T = max(len(w) for _, w in rows)
    if T > MAX_TAPS:
        raise ValueError('%d taps' % T)
    start = np.array([lo for lo, _ in rows], np.int32)
    count = np.array([len(w) for _, w in rows], np.int32)
    wt = np.zeros((n, T), F32)
    for i, (_, w) in enumerate(rows):
        wt[i, :len(w)] = w
    return start, count, wt


def taps(Hs, Ws, crop, o, size, flt):
    """-> ((ystart, ycount, yw, xstart, xcount, xw), (Ho, Wo)); crop None: the full rectangle"""
    crop = (0.0, 0.0, float(Hs), float(Ws)) if crop is None else tuple(float(v) for v in crop)
    assert crop[0] >= 0 and crop[1] >= 0 and crop[2] > 0 and crop[3] > 0 and crop[0] + crop[2] <= Hs and crop[1] + crop[3] <= Ws
    Ho, Wo = out_size(crop, o, size)
    Hc, Wc = (Ho, Wo) if o <= 4 else (Wo, Ho)
    return axis_taps(Hs, crop[0], crop[2], Hc, flt) + axis_taps(Ws, crop[1], crop[3], Wc, flt), (Ho, Wo)


# ---- the sums -----------------------------------------------------------------------------------------------------------------------------
def tap_sum(lines, start, count, w):
    """lines (..., L, M) float32: out[..., i, :] = ((w[i,0]*lines[s] + w[i,1]*lines[s+1]) + ...) over the second-to-last axis, float32, ascending,
    every product and sum rounded on its own, no initial zero"""
    lines = np.asarray(lines, F32)
    out = np.empty(lines.shape[:-2] + (len(start), lines.shape[-1]), F32)
    with np.errstate(all='ignore'):
        for i in range(len(start)):
            s, n = int(start[i]), int(count[i])
            assert n >= 1 and s >= 0 and s + n <= lines.shape[-2], (i, s, n)
            v = F32(w[i, 0]) * lines[..., s, :]
            for k in range(1, n):
                v = v + F32(w[i, k]) * lines[..., s + k, :]
            assert v.dtype == F32
            out[..., i, :] = v
    return out


def resample(rgb, tables):
    """(N,3,Hs,Ws) float32 -> the unoriented (N,3,Hc,Wc) float32: horizontal sums first, then vertical ones"""
    ystart, ycount, yw, xstart, xcount, xw = tables
    rgb = np.asarray(rgb, F32)
    h = np.swapaxes(tap_sum(np.swapaxes(rgb, -1, -2), xstart, xcount, xw), -1, -2)      # (N,3,Hs,Wc)
    return tap_sum(h, ystart, ycount, yw)


def footprint(tables, o, Y, X, Hc, Wc):
    """the source rows and columns upright pixel (Y, X) reads"""
    ystart, ycount, _, xstart, xcount, _ = tables
    i, j = unoriented(o, Y, X, Hc, Wc)
    return range(int(ystart[i]), int(ystart[i] + ycount[i])), range(int(xstart[j]), int(xstart[j] + xcount[j]))


def frame_linear(rgb, tables, o, ccms=None):
    """ELD_RENDER_LINEAR_F32: the resampled values, after the CCM when there is one, upright"""
    v = resample(rgb, tables)
    return orient(v if ccms is None else DM.apply_ccm(v, ccms), o)


def frame_srgb8(rgb, tables, o, ccms=None, gamma=2.2, CRF=None):
    """ELD_RENDER_SRGB8: without a matrix the tail multiplies by the identity, as the kernels do"""
    v = resample(rgb, tables)
    eye = np.tile(np.eye(3, dtype=F32).reshape(1, 9), (v.shape[0], 1))
    return orient(DM.srgb8(DM.apply_ccm(v, eye if ccms is None else ccms), gamma, CRF), o)
