"""NumPy restatements the X-Trans noise and calibration tests share: the sampler's X-Trans row map and colour-bias layout (on top of
oracle/noise_ref.py), exact cell sums of a mosaic, and the X-Trans estimators computed from the pixels in float64."""
import numpy as np

from oracle import noise_ref as O

PLANE_COLOUR = np.array([0, 1, 2, 0, 2, 1, 1, 1, 1])      # colour (R 0, G 1, B 2) of each packed plane (noise.py:22-64)
CODE_COLOUR = np.array([0, 1, 2, 1])                      # rawpy colour code -> colour class


def sensor_rows(h, w):
    """(9,h,w): the sensor row each packed X-Trans position reads."""
    return O.xtrans_source_index(h, w)[0]


def row_offsets(h, w):
    """(9,h,w): d = sensor row - 3i, the table of the issue / csrc/noise.hip XT_DROW."""
    return sensor_rows(h, w) - 3 * np.arange(h)[None, :, None]


def plane_bias(cb3):
    """(R, G, B) colour bias -> the 9 per-plane values noise_arith adds."""
    return tuple(float(np.float32(cb3[k])) for k in PLANE_COLOUR)


def xtrans_pattern(g2=()):
    """The 6x6 raw_pattern of the pack's phase (row 0 = R B G B R G), colour codes 0 R, 1 G, 2 B; the G cells listed in g2 get code 3."""
    pat = np.zeros((6, 6), np.int64)
    rows, cols = O.xtrans_source_index(2, 2)
    for c in range(9):
        pat[rows[c], cols[c]] = (0, 1, 2)[PLANE_COLOUR[c]]
    for r, c in g2:
        assert pat[r, c] == 1
        pat[r, c] = 3
    return pat


# ---- exact cell sums (what eld_calib_cell_* return) -------------------------------------------------------------------------
def cell_sums_ref(u, p):
    """u (F,Hm,Wm) uint16 -> cell_sums int64 (F,p,p,2) (sum u, sum u^2), row_sums int64 (F,Hm,p)."""
    u = np.asarray(u).astype(np.int64)
    F, Hm, Wm = u.shape
    cs = np.zeros((F, p, p, 2), np.int64)
    rs = np.zeros((F, Hm, p), np.int64)
    for c in range(p):
        rs[:, :, c] = u[:, :, c::p].sum(axis=2)
        for r in range(p):
            blk = u[:, r::p, c::p]
            cs[:, r, c, 0] = blk.sum(axis=(1, 2))
            cs[:, r, c, 1] = (blk * blk).sum(axis=(1, 2))
    return cs, rs


def cell_flat_sums_ref(ab, p, white):
    """ab (P,2,Hm,Wm) uint16 -> int64 (P,p,p,4): sum(a+b), sum(a-b), sum((a-b)^2), #(a or b >= white) per cell."""
    ab = np.asarray(ab).astype(np.int64)
    a, b = ab[:, 0], ab[:, 1]
    out = np.zeros((ab.shape[0], p, p, 4), np.int64)
    for r in range(p):
        for c in range(p):
            x, z = a[:, r::p, c::p], b[:, r::p, c::p]
            d = x - z
            out[:, r, c] = np.stack([(x + z).sum(axis=(1, 2)), d.sum(axis=(1, 2)), (d * d).sum(axis=(1, 2)),
                                     ((x >= white) | (z >= white)).sum(axis=(1, 2))], axis=1)
    return out


def fold_bayer(cell2, pattern):
    """p = 2 cell sums (F,2,2,S) folded by a 2x2 Bayer pattern -> (F,4,S) per packed channel, as eld_calib_bias/flat_stats."""
    pat = np.asarray(pattern).reshape(2, 2)
    out = np.zeros((cell2.shape[0], 4, cell2.shape[-1]), np.int64)
    for r in range(2):
        for c in range(2):
            out[:, pat[r, c]] = cell2[:, r, c]
    return out


# ---- the X-Trans estimators from the pixels (float64) -----------------------------------------------------------------------
def colour_map(pattern, Hm, Wm):
    pat = np.asarray(pattern)
    return pat[np.arange(Hm)[:, None] % 6, np.arange(Wm)[None, :] % 6]      # code of each pixel


def xtrans_bias_ref(u, pattern, black):
    """One bias frame (Hm,Wm) -> cb (3,), rho (Hm,), g_scale, R_scale, t (float32 residual), by the definitions of DESIGN.md sec. 10."""
    u = np.asarray(u, np.float64)
    Hm, Wm = u.shape
    code = colour_map(pattern, Hm, Wm)
    col = CODE_COLOUR[code]
    ub = u - np.asarray(black, np.float64)[code]
    cb = np.array([ub[col == k].mean() for k in range(3)])
    e = ub - cb[col]
    rho = e.mean(axis=1)
    t = e - rho[:, None]
    n = e.size
    g = np.sqrt(np.sum(e * e) / n)
    R = np.sqrt(max(0.0, np.mean(rho * rho) - np.mean(t * t) / Wm))
    t32 = (((u - np.asarray(black, np.float64)[code]) - cb[col]) - rho[:, None]).astype(np.float32)
    return cb, rho, g, R, t32


def xtrans_flat_ref(a, b, pattern, black, white, cbm):
    """One flat pair -> mu (3,), var (3,), usable (3,) per colour."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    Hm, Wm = a.shape
    code = colour_map(pattern, Hm, Wm)
    col = CODE_COLOUR[code]
    bl = np.asarray(black, np.float64)[code]
    mu, var, ok = np.zeros(3), np.zeros(3), np.zeros(3, bool)
    for k in range(3):
        m = col == k
        mu[k] = np.mean((a[m] + b[m]) / 2) - bl[m].mean() - cbm[k]
        var[k] = np.var(a[m] - b[m]) / 2
        ok[k] = not np.any((a[m] >= white) | (b[m] >= white)) and mu[k] > 0 and mu[k] <= 0.8 * (white - bl[m].mean())
    return mu, var, ok
