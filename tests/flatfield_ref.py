"""NumPy restatement of the flat-field contracts (include/eld_amd.h "flat-field maps"), operation for operation: the
yardstick of eld_amd/csrc/flatfield.hip and of the host formulas of eld_amd/flatfield.py.  Integer passes in int64, the maps in float64 with
one rounding to float32, the two float paths in float32 with one rounding per operation.  Nothing here imports eld_amd."""
import numpy as np

from shading_ref import XT_RC, XT_RC3, cell_map, step, xtrans_sites  # noqa: F401 (the index maps of the X-Trans pack are shared)

CODE_COLOUR = np.array([0, 1, 2, 1])               # rawpy colour code (R, G, B, G2) -> R 0, G 1, B 2
COLOURS = ('R', 'G', 'B')


def pack_bitmap(mask):
    """bool (Hm,Wm) -> uint32 (Hm, ceil(Wm/32)): bit x & 31 of word [y][x >> 5], pad bits zero."""
    Hm, Wm = mask.shape
    pitch = (Wm + 31) // 32
    words = np.zeros((Hm, pitch), np.uint32)
    for x in range(Wm):
        words[:, x >> 5] |= mask[:, x].astype(np.uint32) << np.uint32(x & 31)
    return words


# ---- pass 1 -----------------------------------------------------------------------------------------------------------------------------------
def sums(frames, white, mask=None):
    """frames (F,Hm,Wm) uint16, F even, pairs (2k, 2k+1) -> S int64, D int64, bad bool."""
    u = frames.astype(np.int64)
    S = u.sum(axis=0)
    d = u[0::2] - u[1::2]
    D = (d * d).sum(axis=0)
    bad = (u >= int(white)).any(axis=0)
    if mask is not None:
        bad = bad | mask
    return S, D, bad


# ---- pass 2 -----------------------------------------------------------------------------------------------------------------------------------
def box(S, bad, p, R):
    """Per site the sum of S and the number of the good sites of its window: the sites (y + p dy, x + p dx), |dy|, |dx| <= R, inside the frame."""
    Hm, Wm = S.shape
    g = np.where(bad, 0, S.astype(np.int64))
    n = (~bad).astype(np.int64)
    Bsum, Bcnt = np.zeros((Hm, Wm), np.int64), np.zeros((Hm, Wm), np.int64)
    for r in range(p):
        for c in range(p):
            for src, dst in ((g, Bsum), (n, Bcnt)):
                pl = src[r::p, c::p]
                if pl.size == 0:
                    continue
                h, w = pl.shape
                P = np.zeros((h + 1, w + 1), np.int64)
                P[1:, 1:] = pl.cumsum(axis=0).cumsum(axis=1)
                y0, y1 = np.clip(np.arange(h) - R, 0, h), np.clip(np.arange(h) + R + 1, 0, h)
                x0, x1 = np.clip(np.arange(w) - R, 0, w), np.clip(np.arange(w) + R + 1, 0, w)
                dst[r::p, c::p] = P[y1][:, x1] - P[y0][:, x1] - P[y1][:, x0] + P[y0][:, x0]
    return Bsum, Bcnt


def box_brute(S, bad, p, R):
    """The same by the definition, tap by tap: for tiny shapes, to check box() itself."""
    Hm, Wm = S.shape
    Bsum, Bcnt = np.zeros((Hm, Wm), np.int64), np.zeros((Hm, Wm), np.int64)
    for y in range(Hm):
        for x in range(Wm):
            for dy in range(-R, R + 1):
                for dx in range(-R, R + 1):
                    yy, xx = y + p * dy, x + p * dx
                    if 0 <= yy < Hm and 0 <= xx < Wm and not bad[yy, xx]:
                        Bsum[y, x] += int(S[yy, xx])
                        Bcnt[y, x] += 1
    return Bsum, Bcnt


# ---- the maps ---------------------------------------------------------------------------------------------------------------------------------
def maps(S, D, bad, Bsum, Bcnt, F, centre, colours):
    """-> dict: lens, prnu (float32), invalid, report, and the float64 planes V, r, ok.  centre, colours: (p,p) integer tables."""
    Hm, Wm = S.shape
    cen = cell_map(centre, Hm, Wm).astype(np.int64)
    cmap = cell_map(colours, Hm, Wm)
    n = Bcnt.astype(np.int64)
    num = (Bsum.astype(np.int64) - n * F * cen).astype(np.float64)               # the integers are below 2^53: the conversion is exact
    den = (n * F).astype(np.float64)
    V = np.where(n > 0, num / np.where(n > 0, den, 1.0), 0.0)
    r = (S.astype(np.int64) - F * cen).astype(np.float64) / np.float64(F)
    ok = (~bad) & (n > 0) & (V > 0) & (r > 0)
    Vs, rs = np.where(ok, V, 1.0), np.where(ok, r, 1.0)
    vref = np.ones((Hm, Wm), np.float64)
    for k in range(3):
        sel = ok & (cmap == k)
        if sel.any():
            vref = np.where(cmap == k, V[sel].max(), vref)
    lens = np.where(ok, (vref / Vs).astype(np.float32), np.float32(1))
    prnu = np.where(ok, (Vs / rs).astype(np.float32), np.float32(1))
    rho = rs / Vs
    nvar = D.astype(np.float64) / ((np.float64(F) * Vs) * (np.float64(F) * Vs))
    report = {}
    for k, name in enumerate(COLOURS):
        sel = ok & (cmap == k)
        m = int(sel.sum())
        if m == 0:
            report[name] = {'rho_var': float('nan'), 'noise_var': float('nan'), 'prnu_sigma': float('nan'), 'snr': float('nan'),
                            'falloff': float('nan'), 'sites': 0}
            continue
        rv, nv, v = float(np.var(rho[sel])), float(np.mean(nvar[sel])), V[sel]
        sig = float(np.sqrt(max(0.0, rv - nv)))
        report[name] = {'rho_var': rv, 'noise_var': nv, 'prnu_sigma': sig, 'snr': sig / float(np.sqrt(nv)) if nv > 0 else float('inf'),
                        'falloff': float(v.min() / v.max()), 'sites': m}
    return {'lens': lens.astype(np.float32), 'prnu': prnu.astype(np.float32), 'invalid': int((~ok).sum()), 'report': report, 'V': V, 'r': r,
            'ok': ok, 'vref': vref}


def fit(frames, centre, colours, white=16383, radius=16, mask=None):
    """frames (F,Hm,Wm) uint16 (pairs 2k, 2k+1); centre, colours (p,p) -> maps()."""
    p = np.asarray(centre).shape[0]
    S, D, bad = sums(frames, white, mask)
    Bsum, Bcnt = box(S, bad, p, radius)
    return maps(S, D, bad, Bsum, Bcnt, frames.shape[0], centre, colours)


# ---- the integer path -------------------------------------------------------------------------------------------------------------------------
def apply(u, gain, black, white, mask=None):
    """u (..., Hm, Wm) uint16; gain (Hm,Wm) float32; black (p,p) float32 per cell -> clamp(rint((u - black) * gain + black), 0, 65535);
    flagged sites and codes >= white unchanged."""
    f = np.float32
    Hm, Wm = u.shape[-2:]
    b = cell_map(np.asarray(black, f), Hm, Wm).astype(f)
    v = (u.astype(f) - b).astype(f)
    w = (v * gain.astype(f)).astype(f)
    o = np.clip(np.rint((w + b).astype(f)), f(0), f(65535)).astype(np.int64).astype(np.uint16)      # np.rint: ties to even
    keep = u >= int(white)
    if mask is not None:
        keep = keep | mask
    return np.where(keep, u, o)


# ---- the input stage --------------------------------------------------------------------------------------------------------------------------
def _clip01(v):
    f = np.float32
    return np.minimum(np.maximum(v, f(0)), f(1))


def _ratio(o, ratio):
    f = np.float32
    return np.maximum(np.minimum((o * f(ratio)).astype(f), f(1)), f(0))


def pack_bayer_flat(u, raw_pattern, black, white, ratios, gain, a=None, b=None, t=0.0):
    """u (N,2h,2w) uint16 -> (N,4,h,w) float32.  ratios None: no ratio step; a, b None: no subtraction."""
    f = np.float32
    pat = np.asarray(raw_pattern).reshape(-1)
    ds = None if a is None else step(a, b, t)
    N, Hm, Wm = u.shape
    out = np.empty((N, 4, Hm // 2, Wm // 2), f)
    for n in range(N):
        for k in range(4):
            i = int(np.flatnonzero(pat == k)[0])
            oy, ox = i >> 1, i & 1
            x = (u[n, oy::2, ox::2].astype(f) - f(black[k])).astype(f)
            if ds is not None:
                x = (x - ds[oy::2, ox::2]).astype(f)
            x = (x * gain[oy::2, ox::2].astype(f)).astype(f)
            v = _clip01((x / (f(white) - f(black[k])).astype(f)).astype(f))
            out[n, k] = v if ratios is None else _ratio(v, ratios[n])
    return out


def pack_xtrans_flat(u, black, white, ratios, gain, a=None, b=None, t=0.0):
    f = np.float32
    ds = None if a is None else step(a, b, t)
    N, Hm, Wm = u.shape
    rows, cols = xtrans_sites(Hm, Wm)
    out = np.empty((N,) + rows.shape, f)
    for n in range(N):
        x = (u[n][rows, cols].astype(f) - f(black)).astype(f)
        if ds is not None:
            x = (x - ds[rows, cols]).astype(f)
        x = (x * gain[rows, cols].astype(f)).astype(f)
        v = _clip01((x / (f(white) - f(black)).astype(f)).astype(f))
        out[n] = v if ratios is None else _ratio(v, ratios[n])
    return out


def pack_plane_bayer(plane, raw_pattern):
    """(2h,2w) -> (4,h,w): plane k from the cell position of colour code k."""
    pat = np.asarray(raw_pattern).reshape(-1)
    out = []
    for k in range(4):
        i = int(np.flatnonzero(pat == k)[0])
        out.append(plane[(i >> 1)::2, (i & 1)::2])
    return np.stack(out)


def pack_plane_xtrans(plane):
    rows, cols = xtrans_sites(*plane.shape)
    return plane[rows, cols]
