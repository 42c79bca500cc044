"""NumPy float32 restatement, operation by operation, of the full-resolution renders (csrc/demosaic.hip eld_render_bayer /
eld_render_xtrans; include/eld_amd.h states the same evaluation order): gains and clamp, demosaic (Bayer: Malvar-He-Cutler 2004 with
mirrored borders; X-Trans: two-stage normalised convolution on colour differences with windows clipped to the image), then the CCM and
the tail of oracle/isp_ref.py.  `dtype` lets the tests evaluate the same formulas in float64.  The reference has no demosaic to mint
fixtures from (it renders through rawpy), so this file is the only checker of that stage."""
import numpy as np

from oracle import isp_ref as I
from oracle import noise_ref as O
from xtrans_ref import PLANE_COLOUR

F32 = np.float32
CODE_COLOUR = (0, 1, 2, 1)                                 # rawpy colour code (R, G1, B, G2) -> colour class


# ---- mosaics --------------------------------------------------------------------------------------------------------------------
def bayer_colour_map(raw_pattern, Hm, Wm):
    pat = np.asarray(raw_pattern).reshape(2, 2)
    col = np.asarray(CODE_COLOUR)[pat]
    return col[np.arange(Hm)[:, None] % 2, np.arange(Wm)[None, :] % 2]


def xtrans_cell_colours():
    """(6,6) colour of each cell position, from the pack's own index map."""
    rows, cols = O.xtrans_source_index(2, 2)
    cell = np.full((6, 6), -1, np.int64)
    for k in range(9):
        cell[rows[k], cols[k]] = PLANE_COLOUR[k]
    assert (cell >= 0).all()
    return cell


def xtrans_colour_map(Hm, Wm):
    cell = xtrans_cell_colours()
    return cell[np.arange(Hm)[:, None] % 6, np.arange(Wm)[None, :] % 6]


def mosaic_bayer(packed, raw_pattern, wbs, dtype=F32):
    """(N,4,h,w), gains (N,4) by plane -> (N,2h,2w): v = min(max(p * gain, 0), 1) at the plane's place in the 2x2 cell."""
    p = np.asarray(packed, dtype)
    N, _, h, w = p.shape
    v = np.minimum(np.maximum(p * np.asarray(wbs, dtype).reshape(N, 4, 1, 1), dtype(0)), dtype(1))
    pat = np.asarray(raw_pattern).reshape(2, 2)
    out = np.zeros((N, 2 * h, 2 * w), dtype)
    for k in range(4):
        (oy,), (ox,) = np.where(pat == k)
        out[:, oy::2, ox::2] = v[:, k]
    return out


def mosaic_xtrans(packed, wbs, dtype=F32):
    """(N,9,h,w), gains (N,3) by plane colour -> (N,3h,3w)."""
    p = np.asarray(packed, dtype)
    N, _, h, w = p.shape
    v = np.minimum(np.maximum(p * np.asarray(wbs, dtype)[:, PLANE_COLOUR].reshape(N, 9, 1, 1), dtype(0)), dtype(1))
    rows, cols = O.xtrans_source_index(h, w)
    out = np.zeros((N, 3 * h, 3 * w), dtype)
    out[:, rows, cols] = v
    return out


# ---- Bayer: Malvar-He-Cutler, coefficients in eighths -------------------------------------------------------------------------------
def malvar(m, raw_pattern):
    """m (N,H,W) mosaic -> (N,3,H,W) camera RGB in m's dtype.  Borders mirrored without repeating the edge (np.pad 'reflect').
        S1 = (N+S)+(W+E)    S2 = (NN+SS)+(WW+EE)    D = (NW+NE)+(SW+SE)
        G at R/B site            : ((4c + 2*S1) - S2) * 0.125
        R at G site, R left/right: (((5c + 4*(W+E)) + 0.5*(NN+SS)) - (D + (WW+EE))) * 0.125     (B likewise; up/down case transposed)
        R at B site, B at R site : ((6c + 2*D) - 1.5*S2) * 0.125"""
    t = m.dtype.type
    Nf, H, W = m.shape
    P = np.pad(m, ((0, 0), (2, 2), (2, 2)), mode='reflect')

    def s(dy, dx):
        return P[:, 2 + dy:2 + dy + H, 2 + dx:2 + dx + W]
    c = s(0, 0)
    n_s, w_e = s(-1, 0) + s(1, 0), s(0, -1) + s(0, 1)
    nn_ss, ww_ee = s(-2, 0) + s(2, 0), s(0, -2) + s(0, 2)
    S1 = n_s + w_e
    S2 = nn_ss + ww_ee
    D = (s(-1, -1) + s(-1, 1)) + (s(1, -1) + s(1, 1))
    g_at_c = ((t(4) * c + t(2) * S1) - S2) * t(0.125)
    hor = (((t(5) * c + t(4) * w_e) + t(0.5) * nn_ss) - (D + ww_ee)) * t(0.125)
    ver = (((t(5) * c + t(4) * n_s) + t(0.5) * ww_ee) - (D + nn_ss)) * t(0.125)
    diag = ((t(6) * c + t(2) * D) - t(1.5) * S2) * t(0.125)
    col = bayer_colour_map(raw_pattern, H, W)
    col_h = np.roll(col, 1, axis=1)                        # colour of the horizontal neighbours (period 2: either side)
    out = np.zeros((Nf, 3, H, W), m.dtype)
    for k in (0, 2):                                       # R, B
        o = 2 - k
        own = col == k
        out[:, k] = np.where(own, c, np.where(col == o, diag, np.where(col_h == k, hor, ver)))
    out[:, 1] = np.where(col == 1, c, g_at_c)
    return out


# ---- X-Trans: normalised convolution on colour differences --------------------------------------------------------------------------
W3 = np.outer([1, 2, 1], [1, 2, 1])
W5 = np.outer([1, 2, 3, 2, 1], [1, 2, 3, 2, 1])


def _normconv(val, sel, wts):
    """sum(w * val over the selected sites of the window clipped to the image) / sum(w), taps in raster order (dy outer, dx inner)."""
    t = val.dtype.type
    Nf, H, W = val.shape
    r = wts.shape[0] // 2
    acc = np.zeros_like(val)
    ws = np.zeros((H, W), np.int64)
    Pv = np.pad(val, ((0, 0), (r, r), (r, r)))
    Ps = np.pad(sel, ((r, r), (r, r)))                     # padded with False: outside the image nothing is selected
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ok = Ps[r + dy:r + dy + H, r + dx:r + dx + W]
            v = Pv[:, r + dy:r + dy + H, r + dx:r + dx + W]
            wt = int(wts[dy + r, dx + r])
            acc = np.where(ok, acc + t(wt) * v, acc)
            ws = ws + wt * ok
    return acc, ws


def normconv_xtrans(m):
    """m (N,H,W) X-Trans mosaic (whole 6x6 cells) -> (N,3,H,W)."""
    t = m.dtype.type
    Nf, H, W = m.shape
    col = xtrans_colour_map(H, W)
    acc, ws = _normconv(m, col == 1, W3)
    assert (ws[col != 1] > 0).all()                        # every clipped 3x3 window of a non-G site holds a G site
    g = np.where(col == 1, m, acc / np.maximum(ws, 1).astype(m.dtype))
    out = np.zeros((Nf, 3, H, W), m.dtype)
    out[:, 1] = g
    for k in (0, 2):
        acc, ws = _normconv(m - g, col == k, W5)
        assert (ws[col != k] > 0).all()                    # every clipped 5x5 window holds an R and a B site
        out[:, k] = np.where(col == k, m, g + acc / np.maximum(ws, 1).astype(m.dtype))
    return out


# ---- the renders --------------------------------------------------------------------------------------------------------------------
def apply_ccm(rgb, ccms):
    """out[c] = ((r*m[c][0]) + g*m[c][1]) + b*m[c][2], no clamp."""
    m = np.asarray(ccms, rgb.dtype).reshape(-1, 3, 3)
    return np.stack([(rgb[:, 0] * m[:, c, 0, None, None] + rgb[:, 1] * m[:, c, 1, None, None]) + rgb[:, 2] * m[:, c, 2, None, None]
                     for c in range(3)], axis=1)


def linear_bayer(packed, raw_pattern, wbs, ccms=None, dtype=F32):
    rgb = malvar(mosaic_bayer(packed, raw_pattern, wbs, dtype), raw_pattern)
    return rgb if ccms is None else apply_ccm(rgb, ccms)


def linear_xtrans(packed, wbs, ccms=None, dtype=F32):
    rgb = normconv_xtrans(mosaic_xtrans(packed, wbs, dtype))
    return rgb if ccms is None else apply_ccm(rgb, ccms)


def srgb8(linear, gamma=2.2, CRF=None):
    """float32 linear RGB after the CCM -> uint8 codes of the existing quantiser (oracle/isp_ref.py)."""
    img = np.clip(np.asarray(linear, F32), 0.0, 1.0).astype(F32)
    q = I.gamma_compression(img, gamma) if CRF is None else I.camera_response_function(img, CRF[0], CRF[1])
    return np.rint(np.asarray(q, np.float64) * 255.0).astype(np.uint8)


# ---- the per-phase tables of the interior (what the kernel holds as compile-time tables), by brute force ---------------------------------
def xtrans_phase_tables():
    """36 rows (phase = 6 * row + col): colour, plane, then for G / R / B the bit mask of the window taps (bit = raster index, 3x3 for G,
    5x5 for R and B) that hold the colour and the sum of their weights -- scanned in the interior of a 3x3-cell frame."""
    col = xtrans_colour_map(18, 18)
    rows, cols = O.xtrans_source_index(6, 6)
    plane = np.zeros((18, 18), np.int64)
    for k in range(9):
        plane[rows[k], cols[k]] = k
    out = np.zeros((36, 8), np.int64)
    for r in range(6):
        for c in range(6):
            y, x = 6 + r, 6 + c
            row = [col[y, x], plane[y, x]]
            for k, wts in ((1, W3), (0, W5), (2, W5)):
                rad = wts.shape[0] // 2
                mask = wsum = 0
                for dy in range(-rad, rad + 1):
                    for dx in range(-rad, rad + 1):
                        if col[y + dy, x + dx] == k:
                            mask |= 1 << ((dy + rad) * wts.shape[0] + dx + rad)
                            wsum += int(wts[dy + rad, dx + rad])
                row += [mask, wsum]
            out[6 * r + c] = row
    return out


# ---- packed-resolution baseline of the quality test: binning followed by pixel replication ----------------------------------------------
def binning_replicated_bayer(packed, wbs, dtype=np.float64):
    p = np.asarray(packed, dtype)
    v = np.clip(p * np.asarray(wbs, dtype).reshape(p.shape[0], 4, 1, 1), 0, 1)
    rgb = np.stack([v[:, 0], (v[:, 1] + v[:, 3]) / 2, v[:, 2]], axis=1)
    return rgb.repeat(2, axis=2).repeat(2, axis=3)


def binning_replicated_xtrans(packed, wbs, dtype=np.float64):
    p = np.asarray(packed, dtype)
    v = np.clip(p * np.asarray(wbs, dtype)[:, PLANE_COLOUR].reshape(p.shape[0], 9, 1, 1), 0, 1)
    rgb = np.stack([v[:, PLANE_COLOUR == k].mean(axis=1) for k in range(3)], axis=1)
    return rgb.repeat(3, axis=2).repeat(3, axis=3)
