"""Noise-parameter calibration: bias frames and flat-field pairs -> a camera table in the release schema.

The reference ships the calibrated tables of five cameras (camera_params/release/*_params.npy, restated in camera_params.json) but
not the calibration method (README.md: "we are unable to provide the noise model as well as the calibration method").  This module
estimates the same table for any Bayer or X-Trans sensor, in DN (raw digital numbers, the sampler's ADU), so that NoiseModel(cameras=[name])
can synthesise its noise.  The estimators are the contract of DESIGN.md, "Calibration"; the pixel passes run in HIP
(eld_amd/csrc/calib.hip: exact integer sums, the float64 residual, the Tukey-lambda PPCC), the rest is float64 NumPy on the host.

    sessions = [{'iso': 100, 'bias': (F,Hm,Wm) uint16, 'flats': (P,2,Hm,Wm) uint16}, ...]
    sessions = [{'iso': 100, 'bias': (F,Hm,Wm) uint16, 'bursts': [(N,Hm,Wm) uint16, ...]}, ...]      # no flat field: bursts of a static scene
    params, diag = calibrate_camera(sessions, raw_pattern, black_level, white_level)
    save_camera_params(params, 'MyCam', 'camera_params/release')

X-Trans (cfa='xtrans'): raw_pattern is rawpy's 6x6 raw_pattern, the pixel passes return per-cell sums (eld_calib_cell_*) that the host
folds into the colours R, G, B; the table gains 'cfa': 'xtrans' and a (m, 3) color_bias in (R, G, B) order.

Command line: python -m eld_amd.calibrate manifest.json --camera NAME --out DIR (the manifest format is in INTEGRATION.md).
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

from . import _lib as L

DEFAULT_LAMBDAS = np.linspace(-1.0, 1.0, 141)     # scipy.stats.ppcc_plot(x, -1, 1, N=141): every shipped G_shape lies on it
PROFILE = 'Profile-1'
SIGMA_KEYS = ('G_scale', 'R_scale', 'g_scale')


# ---- argument checks (host only: they run before any device work) ---------------------------------------------------------------
def _pattern(raw_pattern):
    p = np.asarray(raw_pattern).reshape(-1)
    if p.size != 4 or sorted(int(v) for v in p) != [0, 1, 2, 3] or not np.all(p == np.round(p)):
        raise ValueError('raw_pattern must be a 2x2 permutation of 0..3, got %r' % (np.asarray(raw_pattern).tolist(),))
    return p.astype(np.int64).reshape(2, 2)


def _black(black_level):
    b = np.asarray(black_level, dtype=np.float64).reshape(-1)
    if b.size != 4:
        raise ValueError('black_level must hold 4 values (black_level_per_channel), got %d' % b.size)
    return b


XT_PERIOD = 6
CODE_COLOUR = np.array([0, 1, 2, 1])               # rawpy colour code (R, G, B, G2) -> colour class R 0, G 1, B 2


def _xpattern(raw_pattern):
    """rawpy's 6x6 X-Trans raw_pattern (0 = R, 2 = B, 1 and 3 = G) with 8 R, 20 G and 8 B -> int64 (6,6)."""
    p = np.asarray(raw_pattern)
    if p.shape != (XT_PERIOD, XT_PERIOD) or not np.all(np.isin(p, [0, 1, 2, 3])):
        raise ValueError('raw_pattern must be a 6x6 array of colour codes 0..3 for X-Trans, got %r' % (p.tolist(),))
    p = p.astype(np.int64)
    n = np.bincount(CODE_COLOUR[p].reshape(-1), minlength=3)
    if tuple(int(v) for v in n) != (8, 20, 8):
        raise ValueError('an X-Trans raw_pattern holds 8 R, 20 G and 8 B, got %d, %d, %d' % tuple(int(v) for v in n))
    return p


def _cfa(cfa):
    if cfa not in ('bayer', 'xtrans'):
        raise ValueError("cfa must be 'bayer' or 'xtrans', got %r" % (cfa,))
    return cfa


def cell_counts(Hm, Wm, p=XT_PERIOD):
    """(p,p) int64: pixels of an Hm x Wm mosaic in cell (r, c) = {(y, x): y % p == r, x % p == c}."""
    nr = np.array([(Hm - r + p - 1) // p for r in range(p)], np.int64)
    nc = np.array([(Wm - c + p - 1) // p for c in range(p)], np.int64)
    return np.outer(nr, nc)


def _shape(x):
    return tuple(int(s) for s in x.shape)


def _check_mosaics(x, ndim, what, cfa='bayer'):
    s = _shape(x)
    if len(s) != ndim:
        raise ValueError('%s: expected %d dimensions, got shape %s' % (what, ndim, s))
    if ndim == 4 and s[1] != 2:
        raise ValueError('%s: flat pairs must have shape (P, 2, Hm, Wm), got %s' % (what, s))
    Hm, Wm = s[-2:]
    if cfa == 'xtrans':
        if Wm % 2 or Hm < XT_PERIOD or Wm < XT_PERIOD:
            raise ValueError('%s: X-Trans mosaics need an even width and both sides >= 6, got %dx%d' % (what, Hm, Wm))
    elif Hm % 2 or Wm % 2 or Hm == 0 or Wm == 0:
        raise ValueError('%s: mosaic sides must be even and non-zero, got %dx%d' % (what, Hm, Wm))
    if isinstance(x, np.ndarray):
        if x.dtype != np.uint16:
            raise ValueError('%s: uint16 mosaics expected, got %s' % (what, x.dtype))
    else:
        import torch
        if not (x.is_cuda and x.dtype in (torch.int16, torch.uint16)):
            raise ValueError('%s: a tensor must be CUDA int16/uint16 codes, got %s on %s' % (what, x.dtype, x.device))
    return s


def _device_u16(x):
    """ndarray uint16 or CUDA int16/uint16 tensor -> contiguous CUDA tensor of the same bits, 4-byte aligned (the kernels read a row
    as 32-bit words: a view starting at an odd element is copied)."""
    import torch
    if isinstance(x, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.int16)).cuda()
    x = x.contiguous()
    return x.clone() if x.data_ptr() % 4 else x


def _ws(nbytes, device):
    import torch
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)


def _c_pattern(p):
    return (ctypes.c_int * 4)(*[int(v) for v in p.reshape(-1)])


# ---- host derivations from the exact sums ------------------------------------------------------------------------------------
def bias_stats_from_sums(chan_sums, row_sums, raw_pattern, black_level, Hm, Wm):
    """Host half of bias_frame_stats: per frame colour bias cb_c (F,4), row offsets rho_y (F,Hm), the g_scale and R_scale samples (F,)
    (DESIGN.md "Calibration"), float64, from chan_sums int64 (F,4,2) = (sum u, sum u^2) and row_sums int64 (F,Hm,2) = sum u over the
    even / odd columns."""
    pat, black = _pattern(raw_pattern), _black(black_level)
    chan_sums, row_sums = np.asarray(chan_sums), np.asarray(row_sums)
    F = chan_sums.shape[0]
    n, nc = Hm * Wm, Hm * Wm // 4
    mean_u = chan_sums[:, :, 0].astype(np.float64) / nc                  # black_c + cb_c
    cb = mean_u - black[None, :]
    se2 = np.zeros(F)                                                     # sum of e^2 = sum_c (Q_c - S_c^2 / n_c), exact numerator
    for f in range(F):
        se2[f] = sum(float(nc * int(chan_sums[f, c, 1]) - int(chan_sums[f, c, 0]) ** 2) / nc for c in range(4))
    par = np.arange(Hm) & 1                                               # channels of row y: pat[y&1][0], pat[y&1][1]
    mrow = 0.5 * (mean_u[:, pat[par, 0]] + mean_u[:, pat[par, 1]])        # (F,Hm)
    rho = (row_sums[:, :, 0] + row_sums[:, :, 1]).astype(np.float64) / Wm - mrow
    st2 = se2 - Wm * np.sum(rho * rho, axis=1)                            # sum t^2, t = e - rho_y
    g_scale = np.sqrt(se2 / n)
    R_scale = np.sqrt(np.maximum(0.0, np.mean(rho * rho, axis=1) - (st2 / n) / Wm))
    return {'color_bias': cb, 'row_offset': rho, 'g_scale': g_scale, 'R_scale': R_scale}


def xtrans_bias_stats_from_cell_sums(cell_sums, row_sums, raw_pattern, black_level, Hm, Wm):
    """X-Trans host half of bias_frame_stats, from the exact cell sums: cell_sums int64 (F,6,6,2) = (sum u, sum u^2) per cell, row_sums
    int64 (F,Hm,6) = sum u per row and column class.  Returns color_bias (F,3) (R, G, B: the mean of u - black_code over the colour's
    pixels), row_offset (F,Hm) (the row means of e = u - black_code - color_bias), g_scale and R_scale (F,), as the Bayer estimators."""
    pat, black = _xpattern(raw_pattern), _black(black_level)
    cs, rs = np.asarray(cell_sums).reshape(-1, XT_PERIOD, XT_PERIOD, 2), np.asarray(row_sums)
    F = cs.shape[0]
    ncell = cell_counts(Hm, Wm)
    bcell, col = black[pat], CODE_COLOUR[pat]                             # (6,6) black level and colour of each cell
    n = Hm * Wm
    S = cs[..., 0].astype(np.float64)                                     # < 2^53: exact
    cb = np.stack([np.sum((S - ncell * bcell)[:, col == k], axis=1) / ncell[col == k].sum() for k in range(3)], axis=1)
    se2 = np.zeros(F)                     # sum e^2 = sum over cells of (Q - S^2/n) [exact numerator] + n (S/n - black - cb)^2
    for f in range(F):
        for r in range(XT_PERIOD):
            for c in range(XT_PERIOD):
                m, s1, q = int(ncell[r, c]), int(cs[f, r, c, 0]), int(cs[f, r, c, 1])
                se2[f] += float(m * q - s1 * s1) / m + m * (s1 / m - bcell[r, c] - cb[f, col[r, c]]) ** 2
    ncol = cell_counts(1, Wm)[0]                                          # pixels per column class in one row
    off = (bcell[None, :, :] + cb[:, col]) * ncol[None, None, :]          # (F,6,6): sum over a row of class r of black + cb, per column class
    rho = (rs.sum(axis=2).astype(np.float64) - off.sum(axis=2)[:, np.arange(Hm) % XT_PERIOD]) / Wm
    st2 = se2 - Wm * np.sum(rho * rho, axis=1)
    g_scale = np.sqrt(se2 / n)
    R_scale = np.sqrt(np.maximum(0.0, np.mean(rho * rho, axis=1) - (st2 / n) / Wm))
    return {'color_bias': cb, 'row_offset': rho, 'g_scale': g_scale, 'R_scale': R_scale}


def xtrans_flat_stats_from_cell_sums(sums, raw_pattern, black_level, white_level, color_bias, Hm, Wm):
    """X-Trans host half of flat_pair_stats: sums int64 (P,6,6,4) per cell -> mu, var (P,3) float64 and usable (P,3) bool, one
    photon-transfer point per colour and pair (black = the mean black level of the colour's pixels)."""
    pat, black = _xpattern(raw_pattern), _black(black_level)
    sums = np.asarray(sums).reshape(-1, XT_PERIOD, XT_PERIOD, 4)
    P = sums.shape[0]
    cbm = np.asarray(color_bias, np.float64).reshape(3)
    ncell = cell_counts(Hm, Wm)
    bcell, col = black[pat], CODE_COLOUR[pat]
    mu, var, usable = np.zeros((P, 3)), np.zeros((P, 3)), np.zeros((P, 3), bool)
    for k in range(3):
        m = col == k
        nk = int(ncell[m].sum())
        bbar = float(np.sum(ncell[m] * bcell[m])) / nk
        for p in range(P):
            sab, d1, d2 = (sum(int(v) for v in sums[p][m][:, j]) for j in range(3))
            mu[p, k] = sab / (2 * nk) - bbar - cbm[k]
            var[p, k] = float(nk * d2 - d1 * d1) / (nk * nk) / 2.0
            usable[p, k] = int(sums[p][m][:, 3].sum()) == 0 and mu[p, k] > 0 and mu[p, k] <= 0.8 * (float(white_level) - bbar)
    return {'mu': mu, 'var': var, 'usable': usable}


def flat_stats_from_sums(sums, black_level, white_level, color_bias, Hm, Wm):
    """Host half of flat_pair_stats: sums int64 (P,4,4) -> mu, var (P,4) float64 and usable (P,4) bool."""
    black = _black(black_level)
    sums = np.asarray(sums)
    P = sums.shape[0]
    cbm = np.asarray(color_bias, np.float64).reshape(4)
    nc = Hm * Wm // 4
    mu = sums[:, :, 0].astype(np.float64) / (2 * nc) - black[None, :] - cbm[None, :]
    var = np.array([[float(nc * int(sums[p, c, 2]) - int(sums[p, c, 1]) ** 2) / (nc * nc) / 2.0 for c in range(4)] for p in range(P)])
    usable = (sums[:, :, 3] == 0) & (mu > 0) & (mu <= 0.8 * (float(white_level) - black[None, :]))
    return {'mu': mu, 'var': var.reshape(P, 4), 'usable': usable}


# ---- the same derivations over the unflagged sites of a defect map (count-aware) -------------------------------------------------------
def _masked_tail(se2, n_row, dev_row, n):
    """rho, g_scale, R_scale from sum e^2 (F,), per-row counts (Hm,), per-row sums of e (F,Hm) and the site count: the row offset is the
    mean of e over the row's unflagged sites, and the read noise averaged into it is (sum t^2 / n) / n_y, row by row."""
    if np.any(n_row == 0):
        raise ValueError('row %d has no unflagged site: the defect map flags a whole row' % int(np.flatnonzero(n_row == 0)[0]))
    rho = dev_row / n_row[None, :]
    st2 = se2 - np.sum(n_row[None, :] * rho * rho, axis=1)
    g_scale = np.sqrt(se2 / n)
    R_scale = np.sqrt(np.maximum(0.0, np.mean(rho * rho, axis=1) - (st2 / n) * np.mean(1.0 / n_row)))
    return rho, g_scale, R_scale


def bias_stats_from_sums_masked(chan_sums, row_sums, raw_pattern, black_level, Hm, Wm, chan_counts=None, row_counts=None):
    """bias_stats_from_sums over the unflagged sites only: chan_sums / row_sums are the sums over those sites, chan_counts (4,) and
    row_counts (Hm,2) (even / odd columns) their numbers.  Without counts (or with every site counted) it IS bias_stats_from_sums: the
    same call, hence the same bits."""
    pat, black = _pattern(raw_pattern), _black(black_level)
    if chan_counts is None or (np.all(np.asarray(chan_counts) == Hm * Wm // 4) and np.all(np.asarray(row_counts) == Wm // 2)):
        return bias_stats_from_sums(chan_sums, row_sums, pat, black, Hm, Wm)
    chan_sums, row_sums = np.asarray(chan_sums), np.asarray(row_sums)
    nc, nr = np.asarray(chan_counts, np.int64).reshape(4), np.asarray(row_counts, np.int64).reshape(Hm, 2)
    if np.any(nc == 0):
        raise ValueError('channel %d has no unflagged site' % int(np.flatnonzero(nc == 0)[0]))
    F = chan_sums.shape[0]
    mean_u = chan_sums[:, :, 0].astype(np.float64) / nc[None, :]
    cb = mean_u - black[None, :]
    se2 = np.zeros(F)
    for f in range(F):
        se2[f] = sum(float(int(nc[c]) * int(chan_sums[f, c, 1]) - int(chan_sums[f, c, 0]) ** 2) / int(nc[c]) for c in range(4))
    par = np.arange(Hm) & 1
    dev_row = (row_sums[:, :, 0] - nr[None, :, 0] * mean_u[:, pat[par, 0]]) + (row_sums[:, :, 1] - nr[None, :, 1] * mean_u[:, pat[par, 1]])
    rho, g_scale, R_scale = _masked_tail(se2, nr.sum(axis=1), dev_row, int(nc.sum()))
    return {'color_bias': cb, 'row_offset': rho, 'g_scale': g_scale, 'R_scale': R_scale}


def xtrans_bias_stats_from_cell_sums_masked(cell_sums, row_sums, raw_pattern, black_level, Hm, Wm, cell_n=None, row_n=None):
    """xtrans_bias_stats_from_cell_sums over the unflagged sites only: cell_n (6,6) and row_n (Hm,6) count them per cell and per row and
    column class.  Without counts (or with every site counted) it IS xtrans_bias_stats_from_cell_sums."""
    pat, black = _xpattern(raw_pattern), _black(black_level)
    if cell_n is None or (np.array_equal(cell_n, cell_counts(Hm, Wm)) and np.array_equal(row_n, np.broadcast_to(cell_counts(1, Wm)[0], (Hm, XT_PERIOD)))):
        return xtrans_bias_stats_from_cell_sums(cell_sums, row_sums, pat, black, Hm, Wm)
    cs, rs = np.asarray(cell_sums).reshape(-1, XT_PERIOD, XT_PERIOD, 2), np.asarray(row_sums)
    ncell, nrow = np.asarray(cell_n, np.int64).reshape(XT_PERIOD, XT_PERIOD), np.asarray(row_n, np.int64).reshape(Hm, XT_PERIOD)
    F = cs.shape[0]
    bcell, col = black[pat], CODE_COLOUR[pat]
    for k in range(3):
        if ncell[col == k].sum() == 0:
            raise ValueError('colour %d has no unflagged site' % k)
    S = cs[..., 0].astype(np.float64)
    cb = np.stack([np.sum((S - ncell * bcell)[:, col == k], axis=1) / ncell[col == k].sum() for k in range(3)], axis=1)
    se2 = np.zeros(F)
    for f in range(F):
        for r in range(XT_PERIOD):
            for c in range(XT_PERIOD):
                m, s1, q = int(ncell[r, c]), int(cs[f, r, c, 0]), int(cs[f, r, c, 1])
                if m:
                    se2[f] += float(m * q - s1 * s1) / m + m * (s1 / m - bcell[r, c] - cb[f, col[r, c]]) ** 2
    ry = np.arange(Hm) % XT_PERIOD
    level = bcell[None, :, :] + cb[:, col]                                # (F,6,6): black + cb of each cell
    dev_row = (rs.astype(np.float64) - nrow[None, :, :] * level[:, ry, :]).sum(axis=2)
    rho, g_scale, R_scale = _masked_tail(se2, nrow.sum(axis=1), dev_row, int(ncell.sum()))
    return {'color_bias': cb, 'row_offset': rho, 'g_scale': g_scale, 'R_scale': R_scale}


def flat_stats_from_sums_masked(sums, black_level, white_level, color_bias, Hm, Wm, chan_counts=None):
    """flat_stats_from_sums over the unflagged sites only (chan_counts (4,) of them per channel); without counts it IS flat_stats_from_sums."""
    if chan_counts is None or np.all(np.asarray(chan_counts) == Hm * Wm // 4):
        return flat_stats_from_sums(sums, black_level, white_level, color_bias, Hm, Wm)
    black, sums = _black(black_level), np.asarray(sums)
    nc = np.asarray(chan_counts, np.int64).reshape(4)
    if np.any(nc == 0):
        raise ValueError('channel %d has no unflagged site' % int(np.flatnonzero(nc == 0)[0]))
    P = sums.shape[0]
    cbm = np.asarray(color_bias, np.float64).reshape(4)
    mu = sums[:, :, 0].astype(np.float64) / (2 * nc[None, :]) - black[None, :] - cbm[None, :]
    var = np.array([[float(int(nc[c]) * int(sums[p, c, 2]) - int(sums[p, c, 1]) ** 2) / (int(nc[c]) ** 2) / 2.0 for c in range(4)] for p in range(P)])
    usable = (sums[:, :, 3] == 0) & (mu > 0) & (mu <= 0.8 * (float(white_level) - black[None, :]))
    return {'mu': mu, 'var': var.reshape(P, 4), 'usable': usable}


def xtrans_flat_stats_from_cell_sums_masked(sums, raw_pattern, black_level, white_level, color_bias, Hm, Wm, cell_n=None):
    """xtrans_flat_stats_from_cell_sums over the unflagged sites only (cell_n (6,6) of them per cell); without counts it IS that function."""
    if cell_n is None or np.array_equal(cell_n, cell_counts(Hm, Wm)):
        return xtrans_flat_stats_from_cell_sums(sums, raw_pattern, black_level, white_level, color_bias, Hm, Wm)
    pat, black = _xpattern(raw_pattern), _black(black_level)
    sums = np.asarray(sums).reshape(-1, XT_PERIOD, XT_PERIOD, 4)
    P = sums.shape[0]
    cbm = np.asarray(color_bias, np.float64).reshape(3)
    ncell = np.asarray(cell_n, np.int64).reshape(XT_PERIOD, XT_PERIOD)
    bcell, col = black[pat], CODE_COLOUR[pat]
    mu, var, usable = np.zeros((P, 3)), np.zeros((P, 3)), np.zeros((P, 3), bool)
    for k in range(3):
        m = col == k
        nk = int(ncell[m].sum())
        if nk == 0:
            raise ValueError('colour %d has no unflagged site' % k)
        bbar = float(np.sum(ncell[m] * bcell[m])) / nk
        for p in range(P):
            sab, d1, d2 = (sum(int(v) for v in sums[p][m][:, j]) for j in range(3))
            mu[p, k] = sab / (2 * nk) - bbar - cbm[k]
            var[p, k] = float(nk * d2 - d1 * d1) / (nk * nk) / 2.0
            usable[p, k] = int(sums[p][m][:, 3].sum()) == 0 and mu[p, k] > 0 and mu[p, k] <= 0.8 * (float(white_level) - bbar)
    return {'mu': mu, 'var': var, 'usable': usable}


def _site_counts(dmap, Hm, Wm, p):
    """Unflagged sites per cell (p,p) and per row and column class (Hm,p)."""
    keep = ~dmap.mask
    cell_n = np.array([[int(keep[r::p, c::p].sum()) for c in range(p)] for r in range(p)], np.int64)
    row_n = np.stack([keep[:, c::p].sum(axis=1) for c in range(p)], axis=1).astype(np.int64)
    return cell_n, row_n


def _gather_sites(u, dmap):
    """CUDA codes (..., Hm, Wm) -> host int64 (..., K): the codes at the map's sites."""
    import torch
    ys = torch.from_numpy(dmap.sites[:, 0].astype(np.int64)).to(u.device)
    xs = torch.from_numpy(dmap.sites[:, 1].astype(np.int64)).to(u.device)
    v = u.view(torch.int16) if u.dtype == torch.uint16 else u            # the same bits: indexing is defined for int16
    return (v[..., ys, xs].to(torch.int32) & 0xffff).cpu().numpy().astype(np.int64)


def _flat_terms(a, b, white):
    """host int64 codes (P,k) of the two flats at k sites -> (P,4): sum(a+b), sum(a-b), sum((a-b)^2), #sites with a or b >= white."""
    return np.stack([(a + b).sum(axis=1), (a - b).sum(axis=1), ((a - b) ** 2).sum(axis=1), ((a >= white) | (b >= white)).sum(axis=1)], axis=1)


def _drop_flagged(t, defects):
    """Residuals (F, Hm*Wm) -> (F, Hm*Wm - K): the flagged sites' entries removed (row-major order kept)."""
    if defects is None or not defects.count:
        return t
    import torch
    keep = torch.from_numpy(~defects.mask.reshape(-1)).to(t.device)
    return t[:, keep].contiguous()


def _check_defects(defects, cfa, shape=None, raw_pattern=None):
    """The map must be for this CFA, these sides and -- X-Trans -- this pattern: its neighbourhoods are those of the colours of the 6x6
    cell it was built for.  A Bayer map's neighbourhoods are the sites at offsets of +-2 whatever the 2x2 permutation, so a Bayer map
    made under another raw_pattern flags and repairs the same sites: its raw_pattern is not compared."""
    if defects is None or (isinstance(defects, str) and defects == 'auto'):
        return defects
    from .defects import DefectMap
    if not isinstance(defects, DefectMap):
        raise ValueError("defects must be a DefectMap, 'auto' or None, got %r" % (type(defects).__name__,))
    if cfa == 'xtrans' and defects.cfa == 'xtrans' and raw_pattern is not None and not np.array_equal(CODE_COLOUR[_xpattern(raw_pattern)], defects.classes):
        raise ValueError('calibration: the defect map was built for another X-Trans raw_pattern (the colours of its 6x6 cell differ)')
    if shape is not None:
        defects.check_frames(shape, cfa, 'calibration')
    elif defects.cfa != cfa:
        raise ValueError('calibration: the defect map is for cfa=%r, the frames are %r' % (defects.cfa, cfa))
    return defects


def ptc_gain(mu, var, usable, what='session'):
    """K = the OLS slope of var on mu over the usable photon-transfer points."""
    mu, var = np.asarray(mu)[np.asarray(usable)], np.asarray(var)[np.asarray(usable)]
    if mu.size < 2 or np.ptp(mu) <= 0:
        raise ValueError('%s: fewer than two usable flat points (%d): flats saturated, too dark or all alike' % (what, mu.size))
    K = _ols(mu, var)[0]
    if not K > 0:
        raise ValueError('%s: the photon-transfer slope is %r, not a positive gain' % (what, K))
    return K


def params_from_samples(frames, Ks):
    """Per-frame samples (dicts with K, lambda, G_scale, R_scale, g_scale, color_bias) and the session gains -> the release-schema
    table."""
    if len(frames) < 3:
        raise ValueError('at least 3 bias frames are needed for the log-linear fits, got %d' % len(frames))
    for j, fr in enumerate(frames):
        if not fr['R_scale'] > 0:
            raise ValueError('bias frame %d (iso %s): the row-noise sample is 0 (no log): the row offsets do not exceed the read noise '
                             'averaged into them' % (j, fr.get('iso')))
    if len(set(float(k) for k in Ks)) < 2:
        raise ValueError('the sessions give fewer than 2 distinct K: the log-linear fits need a range of gains')
    Kf = np.array([fr['K'] for fr in frames], np.float64)
    return {'Kmin': np.float64(min(Ks)), 'Kmax': np.float64(max(Ks)),
            'G_shape': np.array([fr['lambda'] for fr in frames], dtype=np.float64),
            'color_bias': np.array([fr['color_bias'] for fr in frames], dtype=np.float32).reshape(len(frames), -1),
            PROFILE: {k: fit_log_linear(Kf, [fr[k] for fr in frames]) for k in SIGMA_KEYS}}


def _ols(x, y):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    dx = x - x.mean()
    sxx = float(np.sum(dx * dx))
    if sxx <= 0:
        raise ValueError('least squares needs at least two distinct abscissae')
    slope = float(np.sum(dx * (y - y.mean())) / sxx)
    return slope, float(y.mean() - slope * x.mean())


# ---- public steps -----------------------------------------------------------------------------------------------------------
def bias_frame_stats(bias, raw_pattern, black_level, residual=False, defects=None):
    """Bias frames (F,Hm,Wm) uint16 [ndarray or CUDA int16/uint16 tensor] -> dict of host arrays:
    chan_sums int64 (F,4,2) (sum u, sum u^2 per channel), row_sums int64 (F,Hm,2) (sum u over even / odd columns), color_bias (F,4),
    row_offset (F,Hm), g_scale (F,), R_scale (F,) float64; with residual=True also 't', the CUDA float32 (F,Hm*Wm) residuals
    float32(((u - black_c) - cb_c) - rho_y).
    defects (a DefectMap): every statistic is over its unflagged sites only -- the sums have the flagged sites' contributions taken out
    (exactly, on the host), 'chan_counts' (4,) and 'row_counts' (Hm,2) count what is left, and 't' is (F, Hm*Wm - K): the flagged
    entries are dropped."""
    import torch
    pat, black = _pattern(raw_pattern), _black(black_level)
    F, Hm, Wm = _check_mosaics(bias, 3, 'bias')
    defects = _check_defects(defects, 'bayer', (Hm, Wm))
    u = _device_u16(bias)
    dev = u.device
    cs = torch.empty((F, 4, 2), dtype=torch.int64, device=dev)
    rs = torch.empty((F, Hm, 2), dtype=torch.int64, device=dev)
    cp = _c_pattern(pat)
    ws = _ws(L.lib().eld_calib_bias_stats_workspace_bytes(F, Hm), dev)
    L.check(L.lib().eld_calib_bias_stats(L.dptr(u), F, Hm, Wm, cp, L.dptr(cs), L.dptr(rs), L.dptr(ws), ws.numel(), L.cur_stream()),
            'eld_calib_bias_stats')
    out = {'chan_sums': cs.cpu().numpy(), 'row_sums': rs.cpu().numpy()}
    if defects is not None and defects.count:
        g, ys, xs = _gather_sites(u, defects), defects.sites[:, 0], defects.sites[:, 1]
        ch = pat[ys & 1, xs & 1]
        for c in range(4):
            out['chan_sums'][:, c, 0] -= g[:, ch == c].sum(axis=1)
            out['chan_sums'][:, c, 1] -= (g[:, ch == c] ** 2).sum(axis=1)
        for f in range(F):
            np.subtract.at(out['row_sums'][f], (ys, xs & 1), g[f])
        cell_n, out['row_counts'] = _site_counts(defects, Hm, Wm, 2)
        out['chan_counts'] = np.array([cell_n[pat == c][0] for c in range(4)], np.int64)
    out.update(bias_stats_from_sums_masked(out['chan_sums'], out['row_sums'], pat, black, Hm, Wm, out.get('chan_counts'), out.get('row_counts')))
    if residual:
        t = torch.empty((F, Hm * Wm), dtype=torch.float32, device=dev)
        cbd = torch.from_numpy(np.ascontiguousarray(out['color_bias'])).to(dev)
        rhod = torch.from_numpy(np.ascontiguousarray(out['row_offset'])).to(dev)
        L.check(L.lib().eld_calib_bias_residual(L.dptr(u), F, Hm, Wm, cp, (ctypes.c_double * 4)(*black.tolist()), L.dptr(cbd), L.dptr(rhod),
                                                L.dptr(t), L.cur_stream()), 'eld_calib_bias_residual')
        out['t'] = _drop_flagged(t, defects)
    return out


def tukey_lambda_ppcc(t, lambdas=None, presorted=False):
    """Tukey-lambda probability-plot correlation of the samples t ((n,) or (F,n); ndarray or CUDA tensor; n >= 3) over the shape
    grid (default DEFAULT_LAMBDAS), as scipy.stats.ppcc_plot / probplot(fit=True) define it with Filliben's medians.
    Returns {'lambdas' (L,), 'r' (F,L), 'slope' (F,L), 'lam_hat' (F,), 'scale' (F,), 'index' (F,)} (float64 host arrays; the F axis
    is dropped for 1-D input).  lam_hat = the arg-max of r (lowest index on a tie), scale = the probplot slope there."""
    import torch
    lam = np.asarray(DEFAULT_LAMBDAS if lambdas is None else lambdas, dtype=np.float64).reshape(-1)
    if lam.size == 0:
        raise ValueError('empty lambda grid')
    one = len(_shape(t)) == 1
    if len(_shape(t)) not in (1, 2):
        raise ValueError('t must have shape (n,) or (F,n), got %s' % (_shape(t),))
    n = _shape(t)[-1]
    if n < 3:
        raise ValueError('PPCC needs n >= 3 samples, got %d' % n)
    if not isinstance(t, np.ndarray) and not t.is_cuda:
        raise ValueError('t: a tensor must live on the GPU (CUDA), got one on %s; pass an ndarray to have it uploaded' % (t.device,))
    x = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)).cuda() if isinstance(t, np.ndarray) else t.float()
    x = x.reshape(-1, n)
    if not presorted:
        x = torch.sort(x, dim=1).values
    x = x.contiguous()
    F, dev = x.shape[0], x.device
    lamd = torch.from_numpy(lam.astype(np.float32)).to(dev)
    sums = torch.empty((F, lam.size, 2), dtype=torch.float64, device=dev)
    tsums = torch.empty((F, 2), dtype=torch.float64, device=dev)
    ws = _ws(L.lib().eld_calib_ppcc_workspace_bytes(F, n, lam.size), dev)
    L.check(L.lib().eld_calib_ppcc(L.dptr(x), F, n, L.dptr(lamd), lam.size, L.dptr(sums), L.dptr(tsums), L.dptr(ws), ws.numel(),
                                   L.cur_stream()), 'eld_calib_ppcc')
    s, ts = sums.cpu().numpy(), tsums.cpu().numpy()
    stm, smm = s[:, :, 0], s[:, :, 1]
    stt = ts[:, 1] - ts[:, 0] * ts[:, 0] / n                                # centred sum of squares of t
    with np.errstate(invalid='ignore', divide='ignore'):
        r = stm / np.sqrt(smm * stt[:, None])
    slope = stm / smm
    idx = np.argmax(np.where(np.isnan(r), -np.inf, r), axis=1)
    out = {'lambdas': lam, 'r': r, 'slope': slope, 'index': idx, 'lam_hat': lam[idx], 'scale': slope[np.arange(F), idx]}
    if one:
        out = {k: (v if k == 'lambdas' else v[0]) for k, v in out.items()}
    return out


def flat_pair_stats(flats, raw_pattern, black_level, white_level, color_bias, defects=None):
    """Flat pairs (P,2,Hm,Wm) uint16 -> dict: sums int64 (P,4,4) = per channel (sum(a+b), sum(a-b), sum((a-b)^2), saturated pixels),
    mu (P,4) = mean((a+b)/2) - black_c - color_bias_c, var (P,4) = var(a-b)/2, usable (P,4) bool (no saturated pixel and
    0 < mu <= 0.8 (white - black_c)).  color_bias: the session's mean colour bias (4,)."""
    import torch
    pat, black = _pattern(raw_pattern), _black(black_level)
    P, _, Hm, Wm = _check_mosaics(flats, 4, 'flats')
    defects = _check_defects(defects, 'bayer', (Hm, Wm))
    cbm = np.asarray(color_bias, np.float64).reshape(4)
    ab = _device_u16(flats)
    out = torch.empty((P, 4, 4), dtype=torch.int64, device=ab.device)
    ws = _ws(L.lib().eld_calib_flat_stats_workspace_bytes(P, Hm), ab.device)
    L.check(L.lib().eld_calib_flat_stats(L.dptr(ab), P, Hm, Wm, _c_pattern(pat), int(white_level), L.dptr(out), L.dptr(ws), ws.numel(),
                                         L.cur_stream()), 'eld_calib_flat_stats')
    res = {'sums': out.cpu().numpy()}
    if defects is not None and defects.count:                 # the sums (and the saturation count) over the unflagged sites only
        g, ch = _gather_sites(ab, defects), pat[defects.sites[:, 0] & 1, defects.sites[:, 1] & 1]
        for c in range(4):
            res['sums'][:, c] -= _flat_terms(g[:, 0][:, ch == c], g[:, 1][:, ch == c], int(white_level))
        cell_n = _site_counts(defects, Hm, Wm, 2)[0]
        res['chan_counts'] = np.array([cell_n[pat == c][0] for c in range(4)], np.int64)
    res.update(flat_stats_from_sums_masked(res['sums'], black, white_level, cbm, Hm, Wm, res.get('chan_counts')))
    return res


def xtrans_bias_frame_stats(bias, raw_pattern, black_level, residual=False, defects=None):
    """X-Trans bias frames (F,Hm,Wm) uint16 -> dict: cell_sums int64 (F,6,6,2), row_sums int64 (F,Hm,6), color_bias (F,3), row_offset
    (F,Hm), g_scale, R_scale (F,); with residual=True also 't' (CUDA float32 (F,Hm*Wm)) = float32(((u - black_code) - cb) - rho_y)."""
    import torch
    pat, black = _xpattern(raw_pattern), _black(black_level)
    F, Hm, Wm = _check_mosaics(bias, 3, 'bias', 'xtrans')
    defects = _check_defects(defects, 'xtrans', (Hm, Wm), raw_pattern)
    u = _device_u16(bias)
    dev = u.device
    p = XT_PERIOD
    cs = torch.empty((F, p, p, 2), dtype=torch.int64, device=dev)
    rs = torch.empty((F, Hm, p), dtype=torch.int64, device=dev)
    ws = _ws(L.lib().eld_calib_cell_stats_workspace_bytes(F, Hm, p), dev)
    L.check(L.lib().eld_calib_cell_stats(L.dptr(u), F, Hm, Wm, p, L.dptr(cs), L.dptr(rs), L.dptr(ws), ws.numel(), L.cur_stream()),
            'eld_calib_cell_stats')
    out = {'cell_sums': cs.cpu().numpy(), 'row_sums': rs.cpu().numpy()}
    if defects is not None and defects.count:                 # as bias_frame_stats: the flagged sites leave the sums, exactly
        g, ys, xs = _gather_sites(u, defects), defects.sites[:, 0], defects.sites[:, 1]
        for f in range(F):
            np.subtract.at(out['cell_sums'][f, :, :, 0], (ys % p, xs % p), g[f])
            np.subtract.at(out['cell_sums'][f, :, :, 1], (ys % p, xs % p), g[f] ** 2)
            np.subtract.at(out['row_sums'][f], (ys, xs % p), g[f])
        out['cell_counts'], out['row_counts'] = _site_counts(defects, Hm, Wm, p)
    out.update(xtrans_bias_stats_from_cell_sums_masked(out['cell_sums'], out['row_sums'], pat, black, Hm, Wm, out.get('cell_counts'),
                                                       out.get('row_counts')))
    if residual:
        t = torch.empty((F, Hm * Wm), dtype=torch.float32, device=dev)
        cbc = np.ascontiguousarray(out['color_bias'][:, CODE_COLOUR[pat].reshape(-1)])          # (F,36) bias of each cell's colour
        cbd = torch.from_numpy(cbc).to(dev)
        rhod = torch.from_numpy(np.ascontiguousarray(out['row_offset'])).to(dev)
        L.check(L.lib().eld_calib_cell_residual(L.dptr(u), F, Hm, Wm, p, (ctypes.c_double * (p * p))(*black[pat].reshape(-1).tolist()),
                                                L.dptr(cbd), L.dptr(rhod), L.dptr(t), L.cur_stream()), 'eld_calib_cell_residual')
        out['t'] = _drop_flagged(t, defects)
    return out


def xtrans_flat_pair_stats(flats, raw_pattern, black_level, white_level, color_bias, defects=None):
    """X-Trans flat pairs (P,2,Hm,Wm) uint16 -> dict: sums int64 (P,6,6,4) per cell, mu, var (P,3), usable (P,3) per colour.
    color_bias: the session's mean (R, G, B) bias."""
    import torch
    pat, black = _xpattern(raw_pattern), _black(black_level)
    P, _, Hm, Wm = _check_mosaics(flats, 4, 'flats', 'xtrans')
    defects = _check_defects(defects, 'xtrans', (Hm, Wm), raw_pattern)
    ab = _device_u16(flats)
    p = XT_PERIOD
    out = torch.empty((P, p, p, 4), dtype=torch.int64, device=ab.device)
    ws = _ws(L.lib().eld_calib_cell_flat_stats_workspace_bytes(P, Hm, p), ab.device)
    L.check(L.lib().eld_calib_cell_flat_stats(L.dptr(ab), P, Hm, Wm, p, int(white_level), L.dptr(out), L.dptr(ws), ws.numel(),
                                              L.cur_stream()), 'eld_calib_cell_flat_stats')
    res = {'sums': out.cpu().numpy()}
    if defects is not None and defects.count:
        g, ys, xs = _gather_sites(ab, defects), defects.sites[:, 0], defects.sites[:, 1]
        for r in range(p):
            for c in range(p):
                m = (ys % p == r) & (xs % p == c)
                res['sums'][:, r, c] -= _flat_terms(g[:, 0][:, m], g[:, 1][:, m], int(white_level))
        res['cell_counts'] = _site_counts(defects, Hm, Wm, p)[0]
    res.update(xtrans_flat_stats_from_cell_sums_masked(res['sums'], pat, black, white_level, color_bias, Hm, Wm, res.get('cell_counts')))
    return res


def fit_log_linear(K, sigma):
    """log sigma_j = slope * log K_j + bias by ordinary least squares; sigma = sqrt(SSR / (m - 2)).  The release tables' regression
    records ({'slope', 'bias', 'sigma'}, float64) that NoiseModel._sample_params draws from."""
    x, y = np.log(np.asarray(K, np.float64)), np.log(np.asarray(sigma, np.float64))
    if x.size != y.size or x.size < 3:
        raise ValueError('fit_log_linear needs m >= 3 matching samples, got %d and %d' % (x.size, y.size))
    if not np.all(np.isfinite(x)) or not np.all(np.isfinite(y)):
        raise ValueError('fit_log_linear: K and sigma must be positive and finite')
    slope, bias = _ols(x, y)
    res = y - (slope * x + bias)
    return {'slope': np.float64(slope), 'bias': np.float64(bias), 'sigma': np.float64(np.sqrt(np.sum(res * res) / (x.size - 2)))}


def _check_sessions(sessions, cfa='bayer'):
    if not isinstance(sessions, (list, tuple)) or len(sessions) == 0:
        raise ValueError('sessions must be a non-empty list of {"iso", "bias", "flats" or "bursts"}')
    shape, nbias = None, 0
    for i, s in enumerate(sessions):
        if 'bias' not in s:
            raise ValueError('session %d has no %r' % (i, 'bias'))
        if 'flats' not in s and 'bursts' not in s:
            raise ValueError("session %d has neither 'flats' (flat-field pairs) nor 'bursts' (stacks of a static scene): the gain needs one of them" % i)
        F, Hm, Wm = _check_mosaics(s['bias'], 3, 'session %d bias' % i, cfa)
        if shape is None:
            shape = (Hm, Wm)
        if 'flats' in s:
            P = _check_mosaics(s['flats'], 4, 'session %d flats' % i, cfa)[0]
            if (Hm, Wm) != shape or _shape(s['flats'])[-2:] != shape:
                raise ValueError('session %d: mosaic shapes differ (%s vs %s / %s)' % (i, shape, (Hm, Wm), _shape(s['flats'])[-2:]))
            if F == 0 or P == 0:
                raise ValueError('session %d: needs at least one bias frame and one flat pair' % i)
        elif (Hm, Wm) != shape or F == 0:
            raise ValueError('session %d: needs at least one bias frame of %s, got %s' % (i, shape, (F, Hm, Wm)))
        if 'bursts' in s:
            if not isinstance(s['bursts'], (list, tuple)) or len(s['bursts']) == 0:
                raise ValueError("session %d: 'bursts' is a non-empty list of stacks (N, Hm, Wm)" % i)
            for j, b in enumerate(s['bursts']):
                bs = _check_mosaics(b, 3, 'session %d burst %d' % (i, j), cfa)
                if bs[-2:] != shape:
                    raise ValueError('session %d burst %d: mosaic shapes differ (%s vs %s)' % (i, j, shape, bs[-2:]))
                if bs[0] < 2 or bs[0] > 256:
                    raise ValueError('session %d burst %d: a burst holds 2 to 256 frames, got %d' % (i, j, bs[0]))
        nbias += F
    if nbias < 3:
        raise ValueError('at least 3 bias frames are needed for the log-linear fits, got %d' % nbias)
    if len(sessions) < 2:
        raise ValueError('at least 2 sessions (2 distinct K) are needed, got %d' % len(sessions))


def calibrate_camera(sessions, raw_pattern, black_level, white_level, lambdas=None, cfa='bayer', defects=None):
    """Sessions of bias frames and flat pairs (or, in a session without 'flats', 'bursts': stacks (N,Hm,Wm) of a static scene whose gain is
    eld_amd.burst.burst_gain over the session's bursts; bursts next to flats are reported as diag['ptc'][i]['burst']) -> (params, diagnostics).  params has exactly the release schema
    (Kmin, Kmax, G_shape (m,), color_bias (m,4) float32, 'Profile-1': {G_scale, R_scale, g_scale: {slope, bias, sigma}}), one G_shape /
    color_bias row per bias frame; diagnostics holds the per-frame samples, r(lambda) and the photon-transfer points.
    cfa='xtrans': raw_pattern is the 6x6 X-Trans pattern and black_level rawpy's 4 values by colour code; the table's color_bias is
    (m,3) in (R, G, B) order and it carries 'cfa': 'xtrans'.
    defects: a DefectMap (eld_amd.defects) of the sensor -- every statistic is then taken over its unflagged sites only (colour bias, row
    offsets, g_scale, R_scale, the residuals of the PPCC, the flat-pair sums and their saturation count); 'auto' finds the map first from
    the bias frames of the lowest-ISO session (find_defects with its defaults) and returns it as diag['defects'].  X-Trans maps exist for
    the pattern phase the library packs only (row 0 = R B G B R G): another 6x6 raw_pattern with defects set is a ValueError.  None (default): every
    site counts, as before."""
    xt = _cfa(cfa) == 'xtrans'
    _xpattern(raw_pattern) if xt else _pattern(raw_pattern)
    _black(black_level)
    _check_defects(defects, cfa, raw_pattern=raw_pattern)
    _check_sessions(sessions, cfa)
    if defects is not None and not isinstance(defects, str):
        defects.check_frames(_shape(sessions[0]['bias']), cfa, 'calibration')
    elif defects == 'auto':
        from .defects import find_defects
        isos = [s.get('iso') for s in sessions]
        low = int(np.argmin([float(v) for v in isos])) if all(isinstance(v, (int, float)) for v in isos) else 0
        defects = find_defects(sessions[low]['bias'], cfa, raw_pattern)[0]
    bias_stats = xtrans_bias_frame_stats if xt else bias_frame_stats
    flat_stats = xtrans_flat_pair_stats if xt else flat_pair_stats
    frames, r_all, ptc, Ks = [], [], [], []
    lam = None
    for i, s in enumerate(sessions):
        st = bias_stats(s['bias'], raw_pattern, black_level, residual=True, defects=defects)
        pp = tukey_lambda_ppcc(st.pop('t'), lambdas)
        lam = pp['lambdas']
        what = 'session %d (iso %s)' % (i, s.get('iso'))
        burst = None
        if 'bursts' in s:
            from .burst import burst_gain, stack_burst
            burst = burst_gain([stack_burst(b, cfa, raw_pattern, np.rint(_black(black_level)), white_level, defects=defects) for b in s['bursts']],
                               what=what)
        if 'flats' in s:                                           # a session with flat pairs behaves as it always did; its bursts are reported beside
            fl = flat_stats(s['flats'], raw_pattern, black_level, white_level, st['color_bias'].mean(axis=0), defects=defects)
            K = ptc_gain(fl['mu'], fl['var'], fl['usable'], what)
            point = {'iso': s.get('iso'), 'mu': fl['mu'], 'var': fl['var'], 'usable': fl['usable'], 'K': K}
            if burst is not None:
                point['burst'] = burst
        else:
            K = burst['K']
            point = {'iso': s.get('iso'), 'mu': burst['mu'], 'var': burst['var'], 'usable': np.ones(burst['mu'].shape, bool), 'K': K,
                     'n': burst['n'], 'sigma0_sq': burst['sigma0_sq'], 'source': 'bursts'}
        Ks.append(K)
        ptc.append(point)
        for f in range(st['color_bias'].shape[0]):
            frames.append({'session': i, 'iso': s.get('iso'), 'K': K, 'lambda': float(pp['lam_hat'][f]), 'G_scale': float(pp['scale'][f]),
                           'R_scale': float(st['R_scale'][f]), 'g_scale': float(st['g_scale'][f]), 'color_bias': st['color_bias'][f]})
            r_all.append(pp['r'][f])
    params = params_from_samples(frames, Ks)
    if xt:
        params['cfa'] = 'xtrans'
    diag = {'frames': frames, 'lambdas': lam, 'r': np.array(r_all), 'K': np.array(Ks), 'ptc': ptc}
    if defects is not None:
        diag['defects'] = defects
    return params, diag


def save_camera_params(params, camera, out_dir):
    """Write <out_dir>/<camera>_params.npy (a pickled dict, as the release tables): load_camera_params(camera, out_dir) and the
    reference's np.load(...).item() read it; NoiseModel(cameras=[camera]) finds it under camera_params/release/ of the CWD."""
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, camera + '_params.npy')
    np.save(path, np.array(params, dtype=object), allow_pickle=True)
    return path


# ---- command line -------------------------------------------------------------------------------------------------------------
def manifest_defects(path):
    """The manifest's "defects" entry: None, 'auto', or the path of a saved map (relative to the manifest's directory)."""
    with open(path) as f:
        d = json.load(f).get('defects')
    if d is None or d == 'auto':
        return d
    return os.path.join(os.path.dirname(os.path.abspath(path)), d)


def load_manifest(path, with_cfa=False):
    """Manifest JSON -> (sessions, raw_pattern, black_level, white_level), and the manifest's "cfa" ('bayer' when absent) as a fifth
    item with with_cfa=True.  Paths are relative to the manifest's directory.  The optional "defects" entry is read by manifest_defects."""
    with open(path) as f:
        m = json.load(f)
    base = os.path.dirname(os.path.abspath(path))

    def load(p):
        return np.load(os.path.join(base, p))
    sessions = []
    for s in m['sessions']:
        bias = np.stack([load(p) for p in s['bias']])
        if 'flats' not in s and 'bursts' not in s:
            raise ValueError("%s: a session needs 'flats' ([[a.npy, b.npy], ...]) or 'bursts' ([[a0.npy, a1.npy, ...], ...])" % path)
        session = {'iso': s.get('iso'), 'bias': bias}
        if 'flats' in s:
            session['flats'] = np.stack([np.stack([load(a), load(b)]) for a, b in s['flats']])
        if 'bursts' in s:
            session['bursts'] = [np.stack([load(p) for p in b]) for b in s['bursts']]
        sessions.append(session)
    out = (sessions, m['raw_pattern'], m['black_level'], m['white_level'])
    return out + (_cfa(m.get('cfa', 'bayer')),) if with_cfa else out


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m eld_amd.calibrate', description=__doc__.split('\n')[0])
    ap.add_argument('manifest', help='JSON: raw_pattern, black_level, white_level, [cfa,] sessions [{iso, bias: [.npy], flats: [[a.npy, b.npy]] or bursts: [[a0.npy, a1.npy, ...]]}]')
    ap.add_argument('--camera', required=True, help='camera name: writes <out>/<camera>_params.npy')
    ap.add_argument('--out', default=os.path.join('camera_params', 'release'))
    ap.add_argument('--defects', help="a defect map written by eld_amd.defects (.npz), or 'auto' to find one from the bias frames of the lowest-ISO "
                                      "session and write <out>/<camera>_defects.npz; overrides the manifest's \"defects\"")
    a = ap.parse_args(argv)
    sessions, pattern, black, white, cfa = load_manifest(a.manifest, with_cfa=True)
    defects = a.defects if a.defects is not None else manifest_defects(a.manifest)
    if defects is not None and defects != 'auto':
        from .defects import as_defect_map
        defects = as_defect_map(defects, '--defects')
    params, diag = calibrate_camera(sessions, pattern, black, white, cfa=cfa, defects=defects)
    path = save_camera_params(params, a.camera, a.out)
    if defects is not None:
        print('%d defective sites kept out of every statistic' % diag['defects'].count)
        if defects == 'auto':
            print('wrote', diag['defects'].save(os.path.join(a.out, a.camera + '_defects.npz')))
    for fr in diag['frames']:
        print('iso %-6s K %.5g  lambda %+.4f  G_scale %.4g  R_scale %.4g  g_scale %.4g' % (fr['iso'], fr['K'], fr['lambda'], fr['G_scale'],
                                                                                          fr['R_scale'], fr['g_scale']))
    print('Kmin %.5g Kmax %.5g' % (params['Kmin'], params['Kmax']))
    for k in SIGMA_KEYS:
        r = params[PROFILE][k]
        print('%-8s slope %.5f bias %.5f sigma %.5f' % (k, r['slope'], r['bias'], r['sigma']))
    print('wrote', path)
    return 0


if __name__ == '__main__':
    sys.exit(main())
