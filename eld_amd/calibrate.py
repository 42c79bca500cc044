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

column=True (--column) adds the law of the per-sensor-column term, model letter C: per bias frame C_scale = sqrt(col_var_sensor) of
eld_amd.structure, regressed over log K like the other scales into 'Profile-1'['C_scale'].

Command line: python -m eld_amd.calibrate manifest.json --camera NAME --out DIR [--column] (the manifest format is in INTEGRATION.md).
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

from . import _lib as L
from .defects import as_defect_map, check_defects, find_defects
from .mosaic import XT_PERIOD, CfaLayout, black_levels, cell_counts, check_cfa, check_mosaics, check_sessions as _check_sessions, device_u16, shape_of, workspace

DEFAULT_LAMBDAS = np.linspace(-1.0, 1.0, 141)     # scipy.stats.ppcc_plot(x, -1, 1, N=141): every shipped G_shape lies on it
PROFILE = 'Profile-1'
SIGMA_KEYS = ('G_scale', 'R_scale', 'g_scale')
COLUMN_KEY = 'C_scale'                            # the optional fourth regression (calibrate_camera(column=True)): no release table has it


# ---- host derivations from the exact sums ------------------------------------------------------------------------------------
# Each takes the counts of the unflagged sites of a defect map (the *_masked names) or counts every site (the plain names: the same call
# without counts).  The flat derivations are one expression either way.  The bias derivations share the colour bias and sum e^2 but end in
# two tails, because the row offset of a full row, (sum over the row) / Wm - mean level, and of a masked one, sum of deviations / n_y, are
# different float64 expressions: with every site counted the plain tail runs, whatever the caller passed.
def _plain_tail(se2, rho, n, Wm):
    """g_scale, R_scale from sum e^2 (F,) and the row offsets (F,Hm) of full rows: the read noise averaged into a row is (sum t^2 / n) / Wm."""
    st2 = se2 - Wm * np.sum(rho * rho, axis=1)                            # sum t^2, t = e - rho_y
    return np.sqrt(se2 / n), np.sqrt(np.maximum(0.0, np.mean(rho * rho, axis=1) - (st2 / n) / Wm))


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


def bias_stats_from_sums(chan_sums, row_sums, raw_pattern, black_level, Hm, Wm):
    """Host half of bias_frame_stats: per frame colour bias cb_c (F,4), row offsets rho_y (F,Hm), the g_scale and R_scale samples (F,)
    (DESIGN.md "Calibration"), float64, from chan_sums int64 (F,4,2) = (sum u, sum u^2) and row_sums int64 (F,Hm,2) = sum u over the
    even / odd columns."""
    return bias_stats_from_sums_masked(chan_sums, row_sums, raw_pattern, black_level, Hm, Wm)


def bias_stats_from_sums_masked(chan_sums, row_sums, raw_pattern, black_level, Hm, Wm, chan_counts=None, row_counts=None):
    """bias_stats_from_sums over the unflagged sites only: chan_sums / row_sums are the sums over those sites, chan_counts (4,) and
    row_counts (Hm,2) (even / odd columns) their numbers.  Without counts (or with every site counted) it IS bias_stats_from_sums: the
    same expressions, hence the same bits."""
    lay = CfaLayout('bayer', raw_pattern, black_level)
    pat, black = lay.codes, lay.black
    full = chan_counts is None or (np.all(np.asarray(chan_counts) == Hm * Wm // 4) and np.all(np.asarray(row_counts) == Wm // 2))
    chan_sums, row_sums = np.asarray(chan_sums), np.asarray(row_sums)
    nc = np.full(4, Hm * Wm // 4, np.int64) if full else np.asarray(chan_counts, np.int64).reshape(4)
    if np.any(nc == 0):
        raise ValueError('channel %d has no unflagged site' % int(np.flatnonzero(nc == 0)[0]))
    F = chan_sums.shape[0]
    mean_u = chan_sums[:, :, 0].astype(np.float64) / nc[None, :]          # black_c + cb_c
    cb = mean_u - black[None, :]
    se2 = np.zeros(F)                                                     # sum of e^2 = sum_c (Q_c - S_c^2 / n_c), exact numerator
    for f in range(F):
        se2[f] = sum(float(int(nc[c]) * int(chan_sums[f, c, 1]) - int(chan_sums[f, c, 0]) ** 2) / int(nc[c]) for c in range(4))
    par = np.arange(Hm) & 1                                               # channels of row y: pat[y&1][0], pat[y&1][1]
    if full:
        mrow = 0.5 * (mean_u[:, pat[par, 0]] + mean_u[:, pat[par, 1]])    # (F,Hm)
        rho = (row_sums[:, :, 0] + row_sums[:, :, 1]).astype(np.float64) / Wm - mrow
        g_scale, R_scale = _plain_tail(se2, rho, Hm * Wm, Wm)
    else:
        nr = np.asarray(row_counts, np.int64).reshape(Hm, 2)
        dev_row = (row_sums[:, :, 0] - nr[None, :, 0] * mean_u[:, pat[par, 0]]) + (row_sums[:, :, 1] - nr[None, :, 1] * mean_u[:, pat[par, 1]])
        rho, g_scale, R_scale = _masked_tail(se2, nr.sum(axis=1), dev_row, int(nc.sum()))
    return {'color_bias': cb, 'row_offset': rho, 'g_scale': g_scale, 'R_scale': R_scale}


def xtrans_bias_stats_from_cell_sums(cell_sums, row_sums, raw_pattern, black_level, Hm, Wm):
    """X-Trans host half of bias_frame_stats, from the exact cell sums: cell_sums int64 (F,6,6,2) = (sum u, sum u^2) per cell, row_sums
    int64 (F,Hm,6) = sum u per row and column class.  Returns color_bias (F,3) (R, G, B: the mean of u - black_code over the colour's
    pixels), row_offset (F,Hm) (the row means of e = u - black_code - color_bias), g_scale and R_scale (F,), as the Bayer estimators."""
    return xtrans_bias_stats_from_cell_sums_masked(cell_sums, row_sums, raw_pattern, black_level, Hm, Wm)


def xtrans_bias_stats_from_cell_sums_masked(cell_sums, row_sums, raw_pattern, black_level, Hm, Wm, cell_n=None, row_n=None):
    """xtrans_bias_stats_from_cell_sums over the unflagged sites only: cell_n (6,6) and row_n (Hm,6) count them per cell and per row and
    column class.  Without counts (or with every site counted) it IS xtrans_bias_stats_from_cell_sums."""
    lay = CfaLayout('xtrans', raw_pattern, black_level)
    ncol = cell_counts(1, Wm)[0]                                          # pixels per column class in one row
    full = cell_n is None or (np.array_equal(cell_n, cell_counts(Hm, Wm)) and np.array_equal(row_n, np.broadcast_to(ncol, (Hm, XT_PERIOD))))
    cs, rs = np.asarray(cell_sums).reshape(-1, XT_PERIOD, XT_PERIOD, 2), np.asarray(row_sums)
    ncell = cell_counts(Hm, Wm) if full else np.asarray(cell_n, np.int64).reshape(XT_PERIOD, XT_PERIOD)
    F = cs.shape[0]
    bcell, col = lay.black_cells, lay.colour                              # (6,6) black level and colour of each cell
    for k in range(3):
        if ncell[col == k].sum() == 0:
            raise ValueError('colour %d has no unflagged site' % k)
    S = cs[..., 0].astype(np.float64)                                     # < 2^53: exact
    cb = np.stack([np.sum((S - ncell * bcell)[:, col == k], axis=1) / ncell[col == k].sum() for k in range(3)], axis=1)
    se2 = np.zeros(F)                     # sum e^2 = sum over cells of (Q - S^2/n) [exact numerator] + n (S/n - black - cb)^2
    for f in range(F):
        for r in range(XT_PERIOD):
            for c in range(XT_PERIOD):
                m, s1, q = int(ncell[r, c]), int(cs[f, r, c, 0]), int(cs[f, r, c, 1])
                if m:
                    se2[f] += float(m * q - s1 * s1) / m + m * (s1 / m - bcell[r, c] - cb[f, col[r, c]]) ** 2
    ry = np.arange(Hm) % XT_PERIOD
    level = bcell[None, :, :] + cb[:, col]                                # (F,6,6): black + cb of each cell
    if full:
        off = level * ncol[None, None, :]                                 # sum over a row of class r of black + cb, per column class
        rho = (rs.sum(axis=2).astype(np.float64) - off.sum(axis=2)[:, ry]) / Wm
        g_scale, R_scale = _plain_tail(se2, rho, Hm * Wm, Wm)
    else:
        nrow = np.asarray(row_n, np.int64).reshape(Hm, XT_PERIOD)
        dev_row = (rs.astype(np.float64) - nrow[None, :, :] * level[:, ry, :]).sum(axis=2)
        rho, g_scale, R_scale = _masked_tail(se2, nrow.sum(axis=1), dev_row, int(ncell.sum()))
    return {'color_bias': cb, 'row_offset': rho, 'g_scale': g_scale, 'R_scale': R_scale}


def flat_stats_from_sums(sums, black_level, white_level, color_bias, Hm, Wm):
    """Host half of flat_pair_stats: sums int64 (P,4,4) -> mu, var (P,4) float64 and usable (P,4) bool."""
    return flat_stats_from_sums_masked(sums, black_level, white_level, color_bias, Hm, Wm)


def flat_stats_from_sums_masked(sums, black_level, white_level, color_bias, Hm, Wm, chan_counts=None):
    """flat_stats_from_sums over the unflagged sites only (chan_counts (4,) of them per channel; default: every site)."""
    black, sums = black_levels(black_level), np.asarray(sums)
    nc = np.full(4, Hm * Wm // 4, np.int64) if chan_counts is None else np.asarray(chan_counts, np.int64).reshape(4)
    if np.any(nc == 0):
        raise ValueError('channel %d has no unflagged site' % int(np.flatnonzero(nc == 0)[0]))
    P = sums.shape[0]
    cbm = np.asarray(color_bias, np.float64).reshape(4)
    mu = sums[:, :, 0].astype(np.float64) / (2 * nc[None, :]) - black[None, :] - cbm[None, :]
    var = np.array([[float(int(nc[c]) * int(sums[p, c, 2]) - int(sums[p, c, 1]) ** 2) / (int(nc[c]) ** 2) / 2.0 for c in range(4)] for p in range(P)])
    usable = (sums[:, :, 3] == 0) & (mu > 0) & (mu <= 0.8 * (float(white_level) - black[None, :]))
    return {'mu': mu, 'var': var.reshape(P, 4), 'usable': usable}


def xtrans_flat_stats_from_cell_sums(sums, raw_pattern, black_level, white_level, color_bias, Hm, Wm):
    """X-Trans host half of flat_pair_stats: sums int64 (P,6,6,4) per cell -> mu, var (P,3) float64 and usable (P,3) bool, one
    photon-transfer point per colour and pair (black = the mean black level of the colour's pixels)."""
    return xtrans_flat_stats_from_cell_sums_masked(sums, raw_pattern, black_level, white_level, color_bias, Hm, Wm)


def xtrans_flat_stats_from_cell_sums_masked(sums, raw_pattern, black_level, white_level, color_bias, Hm, Wm, cell_n=None):
    """xtrans_flat_stats_from_cell_sums over the unflagged sites only (cell_n (6,6) of them per cell; default: every site)."""
    lay = CfaLayout('xtrans', raw_pattern, black_level)
    sums = np.asarray(sums).reshape(-1, XT_PERIOD, XT_PERIOD, 4)
    P = sums.shape[0]
    cbm = np.asarray(color_bias, np.float64).reshape(3)
    ncell = cell_counts(Hm, Wm) if cell_n is None else np.asarray(cell_n, np.int64).reshape(XT_PERIOD, XT_PERIOD)
    bcell, col = lay.black_cells, lay.colour
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


# ---- the device passes, for a pattern of period p (2: Bayer, 6: X-Trans) -------------------------------------------------------------
def _cell_sums(u, p, defects):
    """CUDA codes (F,Hm,Wm) -> host int64 cell_sums (F,p,p,2) = (sum u, sum u^2) per cell and row_sums (F,Hm,p) = sum u per row and column
    class; with a defect map the flagged sites' contributions are taken out (exactly, on the host) and (cell_n, row_n), the numbers of
    unflagged sites, follow -- (None, None) otherwise."""
    import torch
    F, Hm, Wm = shape_of(u)
    cs = torch.empty((F, p, p, 2), dtype=torch.int64, device=u.device)
    rs = torch.empty((F, Hm, p), dtype=torch.int64, device=u.device)
    ws = workspace(L.lib().eld_calib_cell_stats_workspace_bytes(F, Hm, p), u.device)
    L.check(L.lib().eld_calib_cell_stats(L.dptr(u), F, Hm, Wm, p, L.dptr(cs), L.dptr(rs), L.dptr(ws), ws.numel(), L.cur_stream()),
            'eld_calib_cell_stats')
    cs, rs = cs.cpu().numpy(), rs.cpu().numpy()
    if defects is None or not defects.count:
        return cs, rs, None, None
    g, ys, xs = _gather_sites(u, defects), defects.sites[:, 0], defects.sites[:, 1]
    for f in range(F):
        np.subtract.at(cs[f, :, :, 0], (ys % p, xs % p), g[f])
        np.subtract.at(cs[f, :, :, 1], (ys % p, xs % p), g[f] ** 2)
        np.subtract.at(rs[f], (ys, xs % p), g[f])
    return (cs, rs) + _site_counts(defects, Hm, Wm, p)


def _cell_flat_sums(ab, p, white_level, defects):
    """CUDA flat pairs (P,2,Hm,Wm) -> host int64 sums (P,p,p,4) per cell (sum(a+b), sum(a-b), sum((a-b)^2), saturated pixels) and cell_n
    (p,p), the unflagged sites of the defect map that were counted (None without one)."""
    import torch
    P, _, Hm, Wm = shape_of(ab)
    out = torch.empty((P, p, p, 4), dtype=torch.int64, device=ab.device)
    ws = workspace(L.lib().eld_calib_cell_flat_stats_workspace_bytes(P, Hm, p), ab.device)
    L.check(L.lib().eld_calib_cell_flat_stats(L.dptr(ab), P, Hm, Wm, p, int(white_level), L.dptr(out), L.dptr(ws), ws.numel(),
                                              L.cur_stream()), 'eld_calib_cell_flat_stats')
    sums = out.cpu().numpy()
    if defects is None or not defects.count:
        return sums, None
    g, ys, xs = _gather_sites(ab, defects), defects.sites[:, 0], defects.sites[:, 1]
    for r in range(p):
        for c in range(p):
            m = (ys % p == r) & (xs % p == c)
            sums[:, r, c] -= _flat_terms(g[:, 0][:, m], g[:, 1][:, m], int(white_level))
    return sums, _site_counts(defects, Hm, Wm, p)[0]


def _cell_residual(u, p, black_cell, bias_cell, row_offset, defects):
    """CUDA float32 (F, Hm*Wm - K) = float32(((u - black_cell[k]) - bias_cell[f][k]) - row_offset[f][y]) at every unflagged site, k the
    site's cell: black_cell (p,p) and bias_cell (F,p*p) are host float64 arrays."""
    import torch
    F, Hm, Wm = shape_of(u)
    t = torch.empty((F, Hm * Wm), dtype=torch.float32, device=u.device)
    cbd = torch.from_numpy(np.ascontiguousarray(bias_cell)).to(u.device)
    rhod = torch.from_numpy(np.ascontiguousarray(row_offset)).to(u.device)
    L.check(L.lib().eld_calib_cell_residual(L.dptr(u), F, Hm, Wm, p, (ctypes.c_double * (p * p))(*black_cell.reshape(-1).tolist()),
                                            L.dptr(cbd), L.dptr(rhod), L.dptr(t), L.cur_stream()), 'eld_calib_cell_residual')
    return _drop_flagged(t, defects)


def _to_channels(cells, pat, axis=1):
    """Per-cell values of a period-2 mosaic, (..., 2, 2, ...) from `axis`, in Bayer channel order (..., 4, ...): channel pat[r][c] is cell (r, c)."""
    s = cells.shape
    return np.take(cells.reshape(s[:axis] + (4,) + s[axis + 2:]), np.argsort(pat.reshape(-1)), axis=axis)


def _drop_flagged(t, defects):
    """Residuals (F, Hm*Wm) -> (F, Hm*Wm - K): the flagged sites' entries removed (row-major order kept)."""
    if defects is None or not defects.count:
        return t
    import torch
    keep = torch.from_numpy(~defects.mask.reshape(-1)).to(t.device)
    return t[:, keep].contiguous()


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
    table.  Where every sample also has 'C_scale' (calibrate_camera(column=True)) 'Profile-1' gains the 'C_scale' regression."""
    if len(frames) < 3:
        raise ValueError('at least 3 bias frames are needed for the log-linear fits, got %d' % len(frames))
    for j, fr in enumerate(frames):
        if not fr['R_scale'] > 0:
            raise ValueError('bias frame %d (iso %s): the row-noise sample is 0 (no log): the row offsets do not exceed the read noise '
                             'averaged into them' % (j, fr.get('iso')))
    keys = SIGMA_KEYS + ((COLUMN_KEY,) if frames and all(COLUMN_KEY in fr for fr in frames) else ())
    if COLUMN_KEY in keys:
        for j, fr in enumerate(frames):
            if not fr[COLUMN_KEY] > 0:
                raise ValueError('bias frame %d (iso %s): the column-noise sample is not positive (no log): the two row phases of the sensor '
                                 'columns share no offset beyond chance; drop --column (column=True) for this camera' % (j, fr.get('iso')))
    if len(set(float(k) for k in Ks)) < 2:
        raise ValueError('the sessions give fewer than 2 distinct K: the log-linear fits need a range of gains')
    Kf = np.array([fr['K'] for fr in frames], np.float64)
    return {'Kmin': np.float64(min(Ks)), 'Kmax': np.float64(max(Ks)),
            'G_shape': np.array([fr['lambda'] for fr in frames], dtype=np.float64),
            'color_bias': np.array([fr['color_bias'] for fr in frames], dtype=np.float32).reshape(len(frames), -1),
            PROFILE: {k: fit_log_linear(Kf, [fr[k] for fr in frames]) for k in keys}}


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
    lay = CfaLayout('bayer', raw_pattern, black_level)
    pat, black = lay.codes, lay.black
    F, Hm, Wm = check_mosaics(bias, 3, 'bias')
    defects = check_defects(defects, 'bayer', (Hm, Wm))
    u = device_u16(bias)
    cs, rs, cell_n, row_n = _cell_sums(u, 2, defects)
    out = {'chan_sums': _to_channels(cs, pat), 'row_sums': rs}
    if cell_n is not None:
        out['row_counts'], out['chan_counts'] = row_n, _to_channels(cell_n, pat, axis=0)
    out.update(bias_stats_from_sums_masked(out['chan_sums'], rs, pat, black, Hm, Wm, out.get('chan_counts'), row_n))
    if residual:
        out['t'] = _cell_residual(u, 2, lay.black_cells, out['color_bias'][:, pat.reshape(-1)], out['row_offset'], defects)
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
    one = len(shape_of(t)) == 1
    if len(shape_of(t)) not in (1, 2):
        raise ValueError('t must have shape (n,) or (F,n), got %s' % (shape_of(t),))
    n = shape_of(t)[-1]
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
    ws = workspace(L.lib().eld_calib_ppcc_workspace_bytes(F, n, lam.size), dev)
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
    lay = CfaLayout('bayer', raw_pattern, black_level)
    pat, black = lay.codes, lay.black
    P, _, Hm, Wm = check_mosaics(flats, 4, 'flats')
    defects = check_defects(defects, 'bayer', (Hm, Wm))
    cbm = np.asarray(color_bias, np.float64).reshape(4)
    sums, cell_n = _cell_flat_sums(device_u16(flats), 2, white_level, defects)   # the sums (and the saturation count) over the unflagged sites only
    res = {'sums': _to_channels(sums, pat)}
    if cell_n is not None:
        res['chan_counts'] = _to_channels(cell_n, pat, axis=0)
    res.update(flat_stats_from_sums_masked(res['sums'], black, white_level, cbm, Hm, Wm, res.get('chan_counts')))
    return res


def xtrans_bias_frame_stats(bias, raw_pattern, black_level, residual=False, defects=None):
    """X-Trans bias frames (F,Hm,Wm) uint16 -> dict: cell_sums int64 (F,6,6,2), row_sums int64 (F,Hm,6), color_bias (F,3), row_offset
    (F,Hm), g_scale, R_scale (F,); with residual=True also 't' (CUDA float32 (F,Hm*Wm)) = float32(((u - black_code) - cb) - rho_y).
    defects: as bias_frame_stats, with 'cell_counts' (6,6) and 'row_counts' (Hm,6)."""
    lay = CfaLayout('xtrans', raw_pattern, black_level)
    F, Hm, Wm = check_mosaics(bias, 3, 'bias', 'xtrans')
    defects = check_defects(defects, 'xtrans', (Hm, Wm), raw_pattern)
    u = device_u16(bias)
    cs, rs, cell_n, row_n = _cell_sums(u, XT_PERIOD, defects)
    out = {'cell_sums': cs, 'row_sums': rs}
    if cell_n is not None:
        out['cell_counts'], out['row_counts'] = cell_n, row_n
    out.update(xtrans_bias_stats_from_cell_sums_masked(cs, rs, lay.codes, lay.black, Hm, Wm, cell_n, row_n))
    if residual:                                              # the colour bias of each cell's colour, (F,36)
        out['t'] = _cell_residual(u, XT_PERIOD, lay.black_cells, out['color_bias'][:, lay.colour.reshape(-1)], out['row_offset'], defects)
    return out


def xtrans_flat_pair_stats(flats, raw_pattern, black_level, white_level, color_bias, defects=None):
    """X-Trans flat pairs (P,2,Hm,Wm) uint16 -> dict: sums int64 (P,6,6,4) per cell, mu, var (P,3), usable (P,3) per colour.
    color_bias: the session's mean (R, G, B) bias."""
    lay = CfaLayout('xtrans', raw_pattern, black_level)
    P, _, Hm, Wm = check_mosaics(flats, 4, 'flats', 'xtrans')
    defects = check_defects(defects, 'xtrans', (Hm, Wm), raw_pattern)
    sums, cell_n = _cell_flat_sums(device_u16(flats), XT_PERIOD, white_level, defects)
    res = {'sums': sums}
    if cell_n is not None:
        res['cell_counts'] = cell_n
    res.update(xtrans_flat_stats_from_cell_sums_masked(res['sums'], lay.codes, lay.black, white_level, color_bias, Hm, Wm, res.get('cell_counts')))
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


def column_samples(bias, cfa, raw_pattern, black_level, defects=None):
    """The column term of one session's bias frames (F,Hm,Wm), from the exact sums of eld_amd.structure (centre = the rounded black level of
    each cell; the flagged sites of `defects` contribute nothing) -> (samples, fixed): samples (F,) = col_var_sensor per frame, the
    covariance over the sensor columns of the column means of two row phases (white noise and the row term cancel: what is left is what the
    rows of a column share, the variance C_scale^2 models); fixed = None for a single frame, else {'col_var', 'col_fixed_var',
    'fixed_share'}: the session's mean column variance, the part of it that two frames share (mean over all frame pairs) and their ratio --
    near 1 a dark-shading map would remove the term, near 0 it is temporal and only the model letter C describes it."""
    from . import structure as ST
    F = shape_of(bias)[0]
    pairs = [(a, b) for a in range(F) for b in range(a + 1, F)]
    sums = ST.structure_sums(bias, cfa, raw_pattern, ST.cell_centres(cfa, raw_pattern, black_level), defects=defects, pairs=pairs)
    return column_samples_from_sums(sums, cfa, raw_pattern)


def column_samples_from_sums(sums, cfa, raw_pattern):
    """Host half of column_samples: the sums of structure_sums (or their restatement) -> (samples, fixed)."""
    from . import structure as ST
    st = ST.structure_stats(sums, cfa, raw_pattern, lags=1)
    samples = np.array([fr['col_var_sensor'] for fr in st['frames']], np.float64)
    fixed = None
    if st['pairs']:
        sm = ST.summarise(st)
        cv, cf = sm['col_var'], sm['col_fixed_var']
        fixed = {'col_var': cv, 'col_fixed_var': cf, 'fixed_share': float(cf / cv) if cv is not None and cf is not None and cv > 0 else None}
    return samples, fixed


def calibrate_camera(sessions, raw_pattern, black_level, white_level, lambdas=None, cfa='bayer', defects=None, column=False):
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
    site counts, as before.
    column=True: every frame sample gains 'C_scale' = sqrt(col_var_sensor) (column_samples), the table 'Profile-1'['C_scale'] by the same
    regression, and diag 'column': per session {'iso', 'col_var', 'col_fixed_var', 'fixed_share'} (the last three None for a session of one
    bias frame).  A frame whose sample is not positive is a ValueError that says to drop the flag.  False (default): table and diag are what
    they were, keys and bits."""
    xt = CfaLayout(cfa, raw_pattern, black_level).cfa == 'xtrans'
    check_defects(defects, cfa, raw_pattern=raw_pattern)
    _check_sessions(sessions, cfa)
    if defects is not None and not isinstance(defects, str):
        defects.check_frames(shape_of(sessions[0]['bias']), cfa, 'calibration')
    elif defects == 'auto':
        isos = [s.get('iso') for s in sessions]
        low = int(np.argmin([float(v) for v in isos])) if all(isinstance(v, (int, float)) for v in isos) else 0
        defects = find_defects(sessions[low]['bias'], cfa, raw_pattern)[0]
    bias_stats = xtrans_bias_frame_stats if xt else bias_frame_stats
    flat_stats = xtrans_flat_pair_stats if xt else flat_pair_stats
    frames, r_all, ptc, Ks, colrep = [], [], [], [], []
    lam = None
    for i, s in enumerate(sessions):
        st = bias_stats(s['bias'], raw_pattern, black_level, residual=True, defects=defects)
        if column:
            cvar, cfix = column_samples(s['bias'], cfa, raw_pattern, black_level, defects=defects)
            colrep.append(dict({'iso': s.get('iso')}, **(cfix or {'col_var': None, 'col_fixed_var': None, 'fixed_share': None})))
        pp = tukey_lambda_ppcc(st.pop('t'), lambdas)
        lam = pp['lambdas']
        what = 'session %d (iso %s)' % (i, s.get('iso'))
        burst = None
        if 'bursts' in s:
            from .burst import burst_gain, stack_burst
            burst = burst_gain([stack_burst(b, cfa, raw_pattern, np.rint(black_levels(black_level)), white_level, defects=defects) for b in s['bursts']],
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
            if column:
                if not cvar[f] > 0:
                    raise ValueError('session %d (iso %s), bias frame %d: the column-noise sample col_var_sensor is %r, not positive: the sensor '
                                     'shows no column term beyond chance; drop --column (column=True) for this camera' % (i, s.get('iso'), f, cvar[f]))
                frames[-1][COLUMN_KEY] = float(np.sqrt(cvar[f]))
            r_all.append(pp['r'][f])
    params = params_from_samples(frames, Ks)
    if xt:
        params['cfa'] = 'xtrans'
    diag = {'frames': frames, 'lambdas': lam, 'r': np.array(r_all), 'K': np.array(Ks), 'ptc': ptc}
    if defects is not None:
        diag['defects'] = defects
    if column:
        diag['column'] = colrep
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

    from .dng import common_meta, load_frame
    paths = []

    def load(p):
        paths.append(os.path.join(base, p))
        return load_frame(paths[-1])
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
    # what the manifest omits comes from the tags of its first DNG (every DNG of the manifest must agree with it); a manifest that names a value keeps it
    tags = common_meta(paths) if any(k not in m for k in ('raw_pattern', 'black_level', 'white_level', 'cfa')) else None
    if tags is not None:
        m = dict({'cfa': tags['cfa'], 'raw_pattern': tags['raw_pattern'], 'black_level': tags['black_level'], 'white_level': tags['white_point']}, **m)
    out = (sessions, m['raw_pattern'], m['black_level'], m['white_level'])
    return out + (check_cfa(m.get('cfa', 'bayer')),) if with_cfa else out


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m eld_amd.calibrate', description=__doc__.split('\n')[0])
    ap.add_argument('manifest', help='JSON: raw_pattern, black_level, white_level, [cfa,] sessions [{iso, bias: [.npy], flats: [[a.npy, b.npy]] or bursts: [[a0.npy, a1.npy, ...]]}]')
    ap.add_argument('--camera', required=True, help='camera name: writes <out>/<camera>_params.npy')
    ap.add_argument('--out', default=os.path.join('camera_params', 'release'))
    ap.add_argument('--defects', help="a defect map written by eld_amd.defects (.npz), or 'auto' to find one from the bias frames of the lowest-ISO "
                                      "session and write <out>/<camera>_defects.npz; overrides the manifest's \"defects\"")
    ap.add_argument('--column', action='store_true', help="also estimate the per-sensor-column term (model letter C): adds 'C_scale' to the table's "
                                                          "'Profile-1' and prints, per session of 2+ bias frames, the share of the column variance that is fixed")
    a = ap.parse_args(argv)
    sessions, pattern, black, white, cfa = load_manifest(a.manifest, with_cfa=True)
    defects = a.defects if a.defects is not None else manifest_defects(a.manifest)
    if defects is not None and defects != 'auto':
        defects = as_defect_map(defects, '--defects')
    params, diag = calibrate_camera(sessions, pattern, black, white, cfa=cfa, defects=defects, column=a.column)
    path = save_camera_params(params, a.camera, a.out)
    if defects is not None:
        print('%d defective sites kept out of every statistic' % diag['defects'].count)
        if defects == 'auto':
            print('wrote', diag['defects'].save(os.path.join(a.out, a.camera + '_defects.npz')))
    for fr in diag['frames']:
        print('iso %-6s K %.5g  lambda %+.4f  G_scale %.4g  R_scale %.4g  g_scale %.4g' % (fr['iso'], fr['K'], fr['lambda'], fr['G_scale'],
                                                                                          fr['R_scale'], fr['g_scale'])
              + ('  C_scale %.4g' % fr[COLUMN_KEY] if a.column else ''))
    for c in diag.get('column', []):
        if c['fixed_share'] is not None:
            print('iso %-6s column variance %.4g DN^2, fixed share %.3f (near 1: a dark-shading map removes it; near 0: temporal, model letter C)'
                  % (c['iso'], c['col_var'], c['fixed_share']))
    print('Kmin %.5g Kmax %.5g' % (params['Kmin'], params['Kmax']))
    for k in SIGMA_KEYS + ((COLUMN_KEY,) if a.column else ()):
        r = params[PROFILE][k]
        print('%-8s slope %.5f bias %.5f sigma %.5f' % (k, r['slope'], r['bias'], r['sigma']))
    print('wrote', path)
    return 0


if __name__ == '__main__':
    sys.exit(main())
