"""The spatial structure of noise: row, column and fixed-pattern components of a stack of dark frames.

    sums = structure_sums(frames, cfa, raw_pattern, centre, defects=None, pairs=[(0, 1)])    # exact integer sums, on the device
    rep = structure_stats(sums, cfa, raw_pattern, lags=8)                                   # float64 on the host

structure_sums wraps eld_struct_sums_u16 / eld_struct_cross_u16 (eld_amd/csrc/structure.hip): per frame the (n, sum d) of every row and
every column by pattern phase, the (n, sum d, sum d^2) of every cell of the pattern, and per frame pair the sum d_a d_b of every cell;
d = code - centre[cell].  structure_stats turns those Hm p + Wm p + p^2 numbers per frame into variance components per colour group.
The estimators, their bias terms and the integer contract are DESIGN.md sec. 17.
"""
import ctypes

import numpy as np

from . import _lib as L
from . import mosaic as M
from .defects import check_defects


def cell_centres(cfa, raw_pattern, black_level):
    """The integer centre of every cell of the pattern, (p,p) int64: rint(black) of the cell's packed channel (Bayer) or colour code
    (X-Trans), clipped to the code range (CfaLayout.centres; the black levels are checked first, as they always were)."""
    return M.CfaLayout(cfa, raw_pattern, M.black_levels(black_level)).centres


def _centre(centre, p):
    c = np.asarray(centre if centre is not None else [], dtype=np.float64).reshape(-1)
    if c.size != p * p or not np.all(c == np.rint(c)) or np.any(c < 0) or np.any(c > 65535):
        raise ValueError('centre must hold %d integers in [0, 65535] (one per cell of the %dx%d pattern), got %r' % (p * p, p, p, centre))
    return [int(v) for v in c]


def _pairs(pairs, F):
    if pairs is None:
        return np.zeros((0, 2), np.int32)
    q = np.asarray(pairs)
    if q.size == 0:
        return np.zeros((0, 2), np.int32)
    if q.ndim != 2 or q.shape[1] != 2 or not np.all(q == np.rint(q)) or np.any(q < 0) or np.any(q >= F):
        raise ValueError('pairs must be (Q, 2) frame indices in [0, %d), got %r' % (F, pairs))
    return np.ascontiguousarray(q, dtype=np.int32)


def structure_sums(frames, cfa, raw_pattern, centre, defects=None, pairs=None):
    """Exact integer sums of d = code - centre[cell].  frames (F,Hm,Wm) uint16 [ndarray or CUDA int16/uint16 tensor]; centre: p*p integers
    in [0, 65535], one per cell (y % p, x % p) (cell_centres); defects: a DefectMap whose flagged sites contribute nothing; pairs: (Q,2)
    frame indices.  -> dict of int64 ndarrays, exactly what the kernels wrote:
        'row' (F,Hm,p,2) (n, sum d) per row and column phase     'col' (F,Wm,p,2) (n, sum d) per column and row phase
        'cell' (F,p*p,3) (n, sum d, sum d^2)                     'cross' (Q,p*p) sum d_a d_b (None without pairs)
    and 'pairs' (Q,2), 'period' p."""
    p = M.CfaLayout(cfa, raw_pattern).period
    F, Hm, Wm = M.check_mosaics(frames, 3, 'frames', None)
    cen = (ctypes.c_int32 * (p * p))(*_centre(centre, p))
    q = _pairs(pairs, F)
    if defects is not None:
        defects = check_defects(defects, cfa, (Hm, Wm), raw_pattern if cfa == 'xtrans' else None)
        if isinstance(defects, str):
            raise ValueError("structure_sums takes a DefectMap, not 'auto'")
    import torch
    u = M.device_u16(frames)
    bm = None if defects is None else defects.bitmap_on(u.device)
    row = torch.empty((F, Hm, p, 2), dtype=torch.int64, device=u.device)
    col = torch.empty((F, Wm, p, 2), dtype=torch.int64, device=u.device)
    cell = torch.empty((F, p * p, 3), dtype=torch.int64, device=u.device)
    L.check(L.lib().eld_struct_sums_u16(L.dptr(u), F, Hm, Wm, p, cen, L.dptr(bm), L.dptr(row), L.dptr(col), L.dptr(cell), L.cur_stream()),
            'eld_struct_sums_u16')
    cross = None
    if len(q):
        cross = torch.empty((len(q), p * p), dtype=torch.int64, device=u.device)
        L.check(L.lib().eld_struct_cross_u16(L.dptr(u), F, Hm, Wm, p, cen, L.dptr(bm), q.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(q),
                                             L.dptr(cross), L.cur_stream()), 'eld_struct_cross_u16')
        cross = cross.cpu().numpy()
    return {'row': row.cpu().numpy(), 'col': col.cpu().numpy(), 'cell': cell.cpu().numpy(), 'cross': cross, 'pairs': q.astype(np.int64), 'period': p}


# ---- the estimators (host, float64) ----------------------------------------------------------------------------------------------------
def check_lags(lags):
    if isinstance(lags, bool) or not isinstance(lags, (int, np.integer)) or lags < 1 or lags > 4096:
        raise ValueError('lags must be an integer in [1, 4096], got %r' % (lags,))
    return int(lags)


def _var(x):
    """Sample variance (n - 1) of a 1-d array; nan below two values."""
    return float(np.var(x, ddof=1)) if x.size >= 2 else float('nan')


def _cov(x, y):
    return float(np.sum((x - x.mean()) * (y - y.mean())) / (x.size - 1)) if x.size >= 2 else float('nan')


def _line_means(lines):
    """lines (L,p,2) (n, sum d) of one frame -> (mean (L,p), n (L,p)); the mean of an entry with n == 0 is nan."""
    n = lines[..., 0].astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        m = np.where(n > 0, lines[..., 1] / n, np.nan)
    return m, n


def _acf(m, n, lags):
    """Autocorrelation of the line means M[i] = sum_c n m / sum_c n (entries with n == 0 dropped; lines without a site dropped from every
    moment): c_k / c_0, c_k the mean over the valid pairs (i, i + k) of (M[i] - mean)(M[i+k] - mean).  White pixel noise is inside c_0
    (its sampling share sigma^2 / n dilutes the value); nan where undefined."""
    nn = n.sum(axis=1)
    s = np.where(n > 0, n * np.nan_to_num(m), 0.0).sum(axis=1)
    ok = nn > 0
    out = [float('nan')] * lags
    if ok.sum() < 2:
        return out
    M = np.where(ok, s / np.where(ok, nn, 1.0), 0.0)
    M = np.where(ok, M - M[ok].mean(), 0.0)
    c0 = float(np.sum(M * M) / ok.sum())
    if not c0 > 0:
        return out
    for k in range(1, lags + 1):
        if k >= len(M):
            break
        pair = ok[:-k] & ok[k:]
        if pair.sum() == 0:
            continue
        out[k - 1] = float(np.sum(M[:-k] * M[k:] * pair) / pair.sum() / c0)
    return out


def _frame_parts(row, col, cell, groups, G):
    """One frame's centred line means: cell mean removed from every row / column mean."""
    p = groups.shape[0]
    cn = cell[:, 0].astype(np.float64).reshape(p, p)
    cs = cell[:, 1].astype(np.float64).reshape(p, p)
    cq = cell[:, 2].astype(np.float64).reshape(p, p)
    with np.errstate(divide='ignore', invalid='ignore'):
        cmean = np.where(cn > 0, cs / cn, 0.0)
    Hm, Wm = row.shape[0], col.shape[0]
    rm, rn = _line_means(row)                        # (Hm,p): row y, column phase c -> cell (y % p, c)
    km, kn = _line_means(col)                        # (Wm,p): column x, row phase r -> cell (r, x % p)
    rphase = np.arange(Hm) % p
    cphase = np.arange(Wm) % p
    rm = rm - cmean[rphase, :]
    km = km - cmean[:, cphase].T
    rgrp = groups[rphase, :]                                     # (Hm,p) group of every row entry
    kgrp = groups[:, cphase].T                                   # (Wm,p)
    return {'cn': cn, 'cs': cs, 'cq': cq, 'rm': rm, 'rn': rn, 'km': km, 'kn': kn, 'rgrp': rgrp, 'kgrp': kgrp}


def _pix_var(P, groups, G):
    out = []
    for g in range(G):
        sel = (groups == g) & (P['cn'] > 0)
        n = P['cn'][sel]
        ss = np.sum(P['cq'][sel] - P['cs'][sel] ** 2 / n)
        dof = np.sum(n - 1)
        out.append(float(ss / dof) if dof > 0 else float('nan'))
    return np.array(out)


def _phase_cov(m, n):
    """Mean over the phase pairs (c < c') of the covariance, over the lines where both phases have sites, of the two phases' means."""
    p = m.shape[1]
    vals = []
    for c in range(p):
        for c2 in range(c + 1, p):
            ok = (n[:, c] > 0) & (n[:, c2] > 0)
            if ok.sum() >= 2:
                vals.append(_cov(m[ok, c], m[ok, c2]))
    return float(np.mean(vals)) if vals else float('nan')


def _line_moments(m, n, grp, G, m2=None):
    """Per group: the variance of the centred line means (their covariance with m2's when given) and mean(1 / n) over the entries."""
    v, a = [], []
    for g in range(G):
        ok = (grp == g) & (n > 0)
        if ok.sum() >= 2:
            v.append(_var(m[ok]) if m2 is None else _cov(m[ok], m2[ok]))
            a.append(float(np.mean(1.0 / n[ok])))
        else:
            v.append(float('nan'))
            a.append(float('nan'))
    return np.array(v), np.array(a)


def _split(V, VR, VC, ar, ac):
    """Per-site variance V = w + r + c, variance of row means VR = r + w ar, of column means VC = c + w ac (ar, ac = mean(1 / n): the
    sampling share of what is independent from site to site) -> (r, c).  w = (V - VR - VC) / (1 - ar - ac)."""
    w = (V - VR - VC) / (1.0 - ar - ac)
    return VR - w * ar, VC - w * ac


def structure_stats(sums, cfa, raw_pattern, lags=8):
    """The report of one stack, float64.  -> {'period', 'groups': G, 'lags', 'frames': [...], 'pairs': [...]}.
    Per frame and colour group g (Bayer: the four packed channels; X-Trans: R, G, B), lists of G values:
        pix_var    sum over the group's cells of (sum d^2 - (sum d)^2 / n) / sum (n - 1): the per-site variance about each cell's own mean
        row_var    var over the row entries (y, c) of the group of (row mean - cell mean), minus w * mean(1 / n), the sampling share of
                   the white part w of pix_var (w = pix_var - row_var - col_var: the three are solved together, _split): not clipped at 0
        col_var    the same over the column entries (x, r)
    and per frame: row_var_sensor (col_var_sensor) = the covariance of the row (column) means of two column (row) phases of one sensor row
    (column), averaged over the phase pairs -- free of white noise, the quantity R_scale models; row_acf, col_acf = `lags` autocorrelations
    of the sensor-row (column) means.  Per pair (a, b): pix_fixed_var (the covariance of the two frames per site, from cross),
    row_fixed_var, col_fixed_var (the covariance of the two frames' line means, minus the share of the fixed pixel part, solved the same way) and the temporal
    remainders pix_temporal_var, row_temporal_var, col_temporal_var = mean of the two frames' totals - the fixed part.
    Entries with n == 0 (fully masked) are dropped from every moment; a moment without data is nan."""
    lags = check_lags(lags)
    lay = M.CfaLayout(cfa, raw_pattern)
    p, groups, G = lay.period, lay.group_table, lay.G
    if int(sums['period']) != p:
        raise ValueError('the sums were taken with period %d, the pattern has period %d' % (int(sums['period']), p))
    row, col, cell = (np.asarray(sums[k]) for k in ('row', 'col', 'cell'))
    F = row.shape[0]
    parts, frames = [], []
    for f in range(F):
        P = _frame_parts(row[f], col[f], cell[f], groups, G)
        pix = _pix_var(P, groups, G)
        P['pix'] = pix
        VR, P['ar'] = _line_moments(P['rm'], P['rn'], P['rgrp'], G)
        VC, P['ac'] = _line_moments(P['km'], P['kn'], P['kgrp'], G)
        P['row_var'], P['col_var'] = _split(pix, VR, VC, P['ar'], P['ac'])
        parts.append(P)
        frames.append({'pix_var': pix.tolist(), 'row_var': P['row_var'].tolist(), 'col_var': P['col_var'].tolist(),
                       'row_var_sensor': _phase_cov(P['rm'], P['rn']), 'col_var_sensor': _phase_cov(P['km'], P['kn']),
                       'row_acf': _acf(P['rm'], P['rn'], lags), 'col_acf': _acf(P['km'], P['kn'], lags)})
    pairs = []
    if sums.get('cross') is not None:
        for (a, b), cr in zip(np.asarray(sums['pairs']).tolist(), np.asarray(sums['cross'])):
            A, B = parts[a], parts[b]
            cr = cr.astype(np.float64).reshape(p, p)
            fixed = []
            for g in range(G):
                sel = (groups == g) & (A['cn'] > 0)
                n = A['cn'][sel]
                dof = np.sum(n - 1)
                fixed.append(float(np.sum(cr[sel] - A['cs'][sel] * B['cs'][sel] / n) / dof) if dof > 0 else float('nan'))
            fixed = np.array(fixed)
            rfix, cfix = _split(fixed, _line_moments(A['rm'], A['rn'], A['rgrp'], G, B['rm'])[0],
                                _line_moments(A['km'], A['kn'], A['kgrp'], G, B['km'])[0], A['ar'], A['ac'])
            pairs.append({'pair': [int(a), int(b)], 'pix_fixed_var': fixed.tolist(), 'row_fixed_var': rfix.tolist(), 'col_fixed_var': cfix.tolist(),
                          'pix_temporal_var': (0.5 * (A['pix'] + B['pix']) - fixed).tolist(),
                          'row_temporal_var': (0.5 * (A['row_var'] + B['row_var']) - rfix).tolist(),
                          'col_temporal_var': (0.5 * (A['col_var'] + B['col_var']) - cfix).tolist()})
    return {'period': p, 'groups': G, 'lags': lags, 'frames': frames, 'pairs': pairs}


# ---- summaries for the validation report -----------------------------------------------------------------------------------------------
COMPONENTS = ('pix_var', 'row_var', 'col_var', 'row_var_sensor', 'col_var_sensor', 'row_acf1', 'col_acf1', 'pix_fixed_var', 'row_fixed_var',
              'col_fixed_var', 'pix_temporal_var', 'row_temporal_var', 'col_temporal_var')


def summarise(stats, with_pairs=True):
    """One number per component: the mean over frames (pairs) and colour groups, nan-aware; None where nothing is defined.  The fixed /
    temporal split is None when with_pairs is False."""
    def mean(vals):
        v = np.asarray(vals, np.float64).reshape(-1)
        v = v[np.isfinite(v)]
        return float(v.mean()) if v.size else None
    fr = stats['frames']
    out = {k: mean([f[k] for f in fr]) for k in ('pix_var', 'row_var', 'col_var', 'row_var_sensor', 'col_var_sensor')}
    out['row_acf1'] = mean([f['row_acf'][0] for f in fr])
    out['col_acf1'] = mean([f['col_acf'][0] for f in fr])
    for k in ('pix_fixed_var', 'row_fixed_var', 'col_fixed_var', 'pix_temporal_var', 'row_temporal_var', 'col_temporal_var'):
        out[k] = mean([q[k] for q in stats['pairs']]) if with_pairs and stats['pairs'] else None
    return out


def log_ratio(real, syn):
    """Per component log(syn / real) where both are positive, else None."""
    out = {}
    for k in COMPONENTS:
        r, s = real.get(k), syn.get(k)
        out[k] = float(np.log(s / r)) if r is not None and s is not None and r > 0 and s > 0 else None
    return out
