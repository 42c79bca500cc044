"""NumPy restatement of eld_struct_sums_u16 / eld_struct_cross_u16 (int64, exact) and of eld_amd.structure.structure_stats (float64,
written from the definitions with plain loops over groups and lines)."""
import numpy as np


def deviations(u, p, centre, mask=None):
    """u (F,Hm,Wm) uint16, centre p*p ints, mask (Hm,Wm) bool of flagged sites -> (d int64 with flagged sites at 0, good (Hm,Wm) bool)."""
    u = np.asarray(u)
    F, Hm, Wm = u.shape
    cen = np.asarray(centre, np.int64).reshape(p, p)
    cmap = cen[np.arange(Hm)[:, None] % p, np.arange(Wm)[None, :] % p]
    good = np.ones((Hm, Wm), bool) if mask is None else ~np.asarray(mask, bool)
    d = (u.astype(np.int64) - cmap[None]) * good[None]
    return d, good


def sums_ref(u, p, centre, mask=None):
    """-> row (F,Hm,p,2), col (F,Wm,p,2), cell (F,p*p,3), int64."""
    d, good = deviations(u, p, centre, mask)
    F, Hm, Wm = d.shape
    row = np.zeros((F, Hm, p, 2), np.int64)
    col = np.zeros((F, Wm, p, 2), np.int64)
    cell = np.zeros((F, p * p, 3), np.int64)
    for c in range(p):
        row[:, :, c, 0] = good[:, c::p].sum(axis=1)[None]
        row[:, :, c, 1] = d[:, :, c::p].sum(axis=2)
    for r in range(p):
        col[:, :, r, 0] = good[r::p, :].sum(axis=0)[None]
        col[:, :, r, 1] = d[:, r::p, :].sum(axis=1)
    for r in range(p):
        for c in range(p):
            s = d[:, r::p, c::p]
            cell[:, r * p + c, 0] = good[r::p, c::p].sum()
            cell[:, r * p + c, 1] = s.sum(axis=(1, 2))
            cell[:, r * p + c, 2] = (s * s).sum(axis=(1, 2))
    return row, col, cell


def cross_ref(u, p, centre, pairs, mask=None):
    """-> cross (Q,p*p) int64."""
    d, _ = deviations(u, p, centre, mask)
    out = np.zeros((len(pairs), p * p), np.int64)
    for q, (a, b) in enumerate(pairs):
        for r in range(p):
            for c in range(p):
                out[q, r * p + c] = (d[a, r::p, c::p] * d[b, r::p, c::p]).sum()
    return out


def sums_dict(u, p, centre, pairs=None, mask=None):
    """What eld_amd.structure.structure_sums returns, from the restatement."""
    row, col, cell = sums_ref(u, p, centre, mask)
    pairs = np.zeros((0, 2), np.int64) if pairs is None else np.asarray(pairs, np.int64).reshape(-1, 2)
    cross = cross_ref(u, p, centre, pairs.tolist(), mask) if len(pairs) else None
    return {'row': row, 'col': col, 'cell': cell, 'cross': cross, 'pairs': pairs, 'period': p}


# ---- structure_stats, from the definitions -------------------------------------------------------------------------------------------------
def _entries(lines, cmean_of, group_of, g):
    """The (centred mean, n) of every line entry of group g with n > 0.  lines (L,p,2)."""
    m, n = [], []
    for i in range(lines.shape[0]):
        for k in range(lines.shape[1]):
            if group_of(i, k) == g and lines[i, k, 0] > 0:
                m.append(lines[i, k, 1] / lines[i, k, 0] - cmean_of(i, k))
                n.append(float(lines[i, k, 0]))
    return np.array(m), np.array(n)


def _cov(x, y):
    return float(((x - x.mean()) * (y - y.mean())).sum() / (len(x) - 1))


def stats_ref(sums, groups, G):
    """groups (p,p) cell -> colour group.  -> per frame {'pix_var', 'row_var', 'col_var': G values, 'row_var_sensor', 'col_var_sensor'} and per
    pair {'pix_fixed_var', 'row_fixed_var', 'col_fixed_var': G values}."""
    groups = np.asarray(groups)
    p = groups.shape[0]
    frames, pairs = [], []
    F = sums['row'].shape[0]

    def cellmean(f):
        c = sums['cell'][f].astype(np.float64).reshape(p, p, 3)
        return np.where(c[..., 0] > 0, c[..., 1] / np.maximum(c[..., 0], 1), 0.0)

    def pix(f, g, second=None):
        num = den = 0.0
        for r in range(p):
            for c in range(p):
                n, s, q = (float(v) for v in sums['cell'][f, r * p + c])
                if groups[r, c] != g or n == 0:
                    continue
                if second is None:
                    num += q - s * s / n
                else:
                    b, cr = second
                    num += float(cr[r * p + c]) - s * float(sums['cell'][b, r * p + c, 1]) / n
                den += n - 1
        return num / den

    for f in range(F):
        cm = cellmean(f)
        rec = {'pix_var': [], 'row_var': [], 'col_var': []}
        for g in range(G):
            pv = pix(f, g)
            rec['pix_var'].append(pv)
            m, n = _entries(sums['row'][f], lambda y, c: cm[y % p, c], lambda y, c: groups[y % p, c], g)
            VR, ar = float(m.var(ddof=1)), float((1.0 / n).mean())
            m, n = _entries(sums['col'][f], lambda x, r: cm[r, x % p], lambda x, r: groups[r, x % p], g)
            VC, ac = float(m.var(ddof=1)), float((1.0 / n).mean())
            w = (pv - VR - VC) / (1.0 - ar - ac)            # pix_var = w + row + col, VR = row + w ar, VC = col + w ac
            rec['row_var'].append(VR - w * ar)
            rec['col_var'].append(VC - w * ac)
        for key, lines, cmo in (('row_var_sensor', sums['row'][f], lambda i, k: cm[i % p, k]), ('col_var_sensor', sums['col'][f], lambda i, k: cm[k, i % p])):
            vals = []
            for c in range(p):
                for c2 in range(c + 1, p):
                    ok = [i for i in range(lines.shape[0]) if lines[i, c, 0] > 0 and lines[i, c2, 0] > 0]
                    a = np.array([lines[i, c, 1] / lines[i, c, 0] - cmo(i, c) for i in ok])
                    b = np.array([lines[i, c2, 1] / lines[i, c2, 0] - cmo(i, c2) for i in ok])
                    vals.append(_cov(a, b))
            rec[key] = float(np.mean(vals))
        frames.append(rec)
    if sums.get('cross') is not None:
        for (a, b), cr in zip(np.asarray(sums['pairs']).tolist(), sums['cross']):
            cma, cmb = cellmean(a), cellmean(b)
            rec = {'pix_fixed_var': [], 'row_fixed_var': [], 'col_fixed_var': []}
            for g in range(G):
                fx = pix(a, g, (b, cr))
                rec['pix_fixed_var'].append(fx)
                ma, n = _entries(sums['row'][a], lambda y, c: cma[y % p, c], lambda y, c: groups[y % p, c], g)
                mb, _ = _entries(sums['row'][b], lambda y, c: cmb[y % p, c], lambda y, c: groups[y % p, c], g)
                CR, ar = _cov(ma, mb), float((1.0 / n).mean())
                ma, n = _entries(sums['col'][a], lambda x, r: cma[r, x % p], lambda x, r: groups[r, x % p], g)
                mb, _ = _entries(sums['col'][b], lambda x, r: cmb[r, x % p], lambda x, r: groups[r, x % p], g)
                CC, ac = _cov(ma, mb), float((1.0 / n).mean())
                w = (fx - CR - CC) / (1.0 - ar - ac)
                rec['row_fixed_var'].append(CR - w * ar)
                rec['col_fixed_var'].append(CC - w * ac)
            pairs.append(rec)
    return {'frames': frames, 'pairs': pairs}
