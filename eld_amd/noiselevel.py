"""Gain and read noise from a single raw frame, without darks, flats or a burst.

    est = estimate_noise(frame_u16, cfa='bayer', raw_pattern=..., black_level=512, white_level=16383)
    est.K, est.sigma                                # DN per electron, read noise in DN: what ClassicalDenoiser and --baseline-K want
    est.points, est.kept_share, est.groups          # the (mu, var, n) points of the line, the share of tiles kept, the line per colour

The Poisson-Gaussian line var = K mu + sigma0^2 (Foi et al. 2008) is fitted to the frame itself.  One HIP pass (csrc/noiselevel.hip:
eld_tile_noise_sums_u16, integer adds only, restated bit for bit by tests/noiselevel_ref.py) sums, per tile of 16 x 16 same-colour sites
and per colour group, the squared 3 x 3 second difference R = sum r^2 (E r^2 = 36 sigma^2), the squared first differences
D = sum dx^2 + dy^2 (E = 4 sigma^2) and the level S.  The host, in float64 and a fixed order, keeps the tiles whose first-difference variance
does not exceed ratio = 3/2 times their second-difference variance -- texture and edges raise D far more than R; the test is scale-free
and needs no noise level --, pools the kept tiles by signal bin (the 61 bins of DESIGN.md sec. 19) and fits the line by iterated weighted
least squares.  Definitions, bounds, limits and measured accuracy are DESIGN.md sec. 26.

Limits: a texture finer than about two strides aliases into what the test cannot tell from noise, and K comes out high (X-Trans therefore
uses its greens at stride 3, not all colours at stride 6); the homogeneity cut leaves a small positive selection bias (about +2 %); the
frame must span a range of signal levels; sigma0^2 includes the quantisation step's 1/12.

Command line: python -m eld_amd.noiselevel frame.npy [more.npy] --meta sensor.json [--defects F] [--stride S] [--camera TABLE] [--json]
"""
import argparse
import json
import math
import sys

import numpy as np

from . import _lib as L
from . import mosaic as M
from .defects import as_defect_map

NB = L.PAIRSTATS_BINS
TILE = 16                       # csrc/noiselevel.hip NL_TS: a tile is TILE * stride sites on a side
STATS = ('n', 'sum_s9', 'sum_r2', 'sum_d2')
MAX_RATIO = 1024                # ratio = (num, den), both in [1, MAX_RATIO]: 9 den D < 2^60 and num R < 2^62 stay inside int64 (D < 2^47, R < 2^52)
MIN_POINTS = 4
FIT_ITERATIONS = 3


def tiles_along(n, s):
    """Tiles that cover the sites s <= i < n - s."""
    return -(-(n - 2 * s) // (TILE * s)) if n > 2 * s else 0


class TileSums:
    """What tile_sums returns and estimate_noise takes.

    sums     host int64 (F, nty, ntx, G, 4): per frame, tile and colour group STATS = (eligible sites, sum S9, sum r^2, sum dx^2 + dy^2)
    period, stride, group, G     the layout the sums were taken with: cell (y % p) * p + x % p -> colour group (-1: not counted)
    shape    (Hc, Wc): the part of the frames that was looked at"""

    def __init__(self, sums, period, stride, group, G, shape=None):
        s = np.asarray(sums)
        period, stride, G = int(period), int(stride), int(G)
        if s.dtype.kind not in 'iu' or s.ndim != 5 or s.shape[3:] != (G, 4):
            raise ValueError('sums must be an integer array (F, nty, ntx, %d, 4), got %s %s' % (G, s.dtype, s.shape))
        group = [int(v) for v in np.asarray(group).reshape(-1)]
        if period not in (2, 6) or len(group) != period * period or not (1 <= stride <= period) or period % stride:
            raise ValueError('period %d, stride %d and %d groups do not describe a layout' % (period, stride, len(group)))
        if not (1 <= G <= 4) or any(not (-1 <= g < G) for g in group):
            raise ValueError('group entries must lie in [-1, %d), got %r' % (G, group))
        self.sums, self.period, self.stride, self.group, self.G = s.astype(np.int64), period, stride, group, G
        self.shape = None if shape is None else (int(shape[0]), int(shape[1]))

    def eligible_cells(self):
        """Per group, the cells whose nine sites at the stride all belong to it: int64 (G,)."""
        p, s = self.period, self.stride
        g = np.asarray(self.group).reshape(p, p)
        n = np.zeros(self.G, np.int64)
        for cy in range(p):
            for cx in range(p):
                if g[cy, cx] >= 0 and all(g[(cy + a * s) % p, (cx + b * s) % p] == g[cy, cx] for a in (-1, 0, 1) for b in (-1, 0, 1)):
                    n[g[cy, cx]] += 1
        return n

    def full_sites(self):
        """Per group, the eligible sites of a full interior tile: (TILE stride)^2 cells_g / p^2, float64 (G,)."""
        return (TILE * self.stride) ** 2 * self.eligible_cells().astype(np.float64) / float(self.period * self.period)


class NoiseEstimate:
    """What estimate_noise returns.

    K, sigma0_sq     slope and intercept of var = K mu + sigma0^2 in DN per electron and DN^2
    sigma            sqrt(max(sigma0_sq, 0)): the read noise in DN (it includes the quantisation step's 1/12)
    negative_intercept   True when sigma0_sq < 0 (sigma is then 0)
    points           {'bin', 'n', 'mu', 'var'}: the points the line went through
    kept_share       kept / usable tile-group entries
    full_kept_share  the same over the entries of full tiles (every eligible site present)
    groups           per colour group with enough points of its own: {g: {'K', 'sigma0_sq', 'sigma', 'points'}}
    stride, period   the layout"""

    def __init__(self, K, sigma0_sq, points, kept_share, full_kept_share, groups, stride, period):
        self.K, self.sigma0_sq = float(K), float(sigma0_sq)
        self.negative_intercept = self.sigma0_sq < 0
        self.sigma = math.sqrt(max(self.sigma0_sq, 0.0))
        self.points, self.kept_share, self.full_kept_share, self.groups = points, float(kept_share), float(full_kept_share), groups
        self.stride, self.period = stride, period

    def as_dict(self):
        pts = {k: np.asarray(v).tolist() for k, v in self.points.items()}
        return {'K': self.K, 'sigma0_sq': self.sigma0_sq, 'sigma': self.sigma, 'negative_intercept': self.negative_intercept,
                'kept_share': self.kept_share, 'full_kept_share': self.full_kept_share, 'stride': self.stride, 'points': pts,
                'groups': {str(g): {k: (v if k != 'points' else {a: np.asarray(b).tolist() for a, b in v.items()}) for k, v in d.items()}
                           for g, d in self.groups.items()}}


# ---- the kernel's wrapper ---------------------------------------------------------------------------------------------------------------
def _layout(cfa, raw_pattern, black_level, stride, green_only):
    """-> (CfaLayout.for_codes, the groups that count, stride): the layout, then the defaults of the single-frame statistic."""
    lay = M.CfaLayout.for_codes(cfa, raw_pattern, black_level)
    p, group, xt = lay.period, lay.group, cfa == 'xtrans'
    if stride is None:
        stride = 3 if xt else 2
    if isinstance(stride, bool) or not isinstance(stride, (int, np.integer)) or not (1 <= stride <= p) or p % stride:
        raise ValueError('stride must be an integer in [1, %d] that divides %d, got %r' % (p, p, stride))
    if green_only is None:
        green_only = xt
    if green_only:
        if not xt:
            raise ValueError('green_only is the X-Trans layout (its greens have period 3); a Bayer frame counts all four positions')
        group = [g if g == 1 else -1 for g in group]
    return lay, list(group), int(stride)


def tile_sums(frames, cfa='bayer', raw_pattern=None, black_level=None, white_level=16383, defects=None, stride=None, green_only=None):
    """The per-tile difference sums of uint16 frames (Hm,Wm) or (F,Hm,Wm), NumPy or CUDA uint16 / int16-view tensors -> TileSums.
    raw_pattern, black_level: as eld_amd.evaluate.pair_level_stats; white_level: codes >= it are saturated; defects: a DefectMap (or its
    path) whose sites make every neighbourhood they lie in ineligible.  stride: the distance to the same-colour neighbours (default 2 for
    Bayer, 3 for X-Trans); green_only (X-Trans, default True): count the greens only, whose period is 3.  X-Trans looks at the whole 6 x 6
    cells.  Bad arguments raise ValueError before any device work."""
    lay, group, stride = _layout(cfa, raw_pattern, black_level, stride, green_only)
    p, G = lay.period, lay.G
    white = M.check_white(white_level)
    F, Hm, Wm = M.check_stack(frames, 'frames', limit=True)
    if F > 65535:
        raise ValueError('at most 65535 frames per call, got %d' % F)
    if defects is not None:
        defects = as_defect_map(defects)
        defects.check_frames((Hm, Wm), cfa, 'tile_sums')
    Hc, Wc = lay.whole_cells(Hm, Wm)
    import torch
    u = M.device_u16(frames).reshape(F, Hm, Wm)
    nty, ntx = tiles_along(Hc, stride), tiles_along(Wc, stride)
    lib = L.lib()
    with torch.cuda.device(u.device):
        out = torch.zeros((F, nty, ntx, G, 4), dtype=torch.int64, device=u.device)
        need = lib.eld_tile_noise_workspace_bytes(F, Hm, Wm)
        ws = M.workspace(need, u.device)
        bm = None if defects is None else defects.bitmap_on(u.device)
        L.check(lib.eld_tile_noise_sums_u16(L.dptr(u), F, Hm, Wm, Hc, Wc, p, stride, lay.c_group(group), G, lay.c_black(), white, L.dptr(bm),
                                            L.dptr(out), L.dptr(ws), need, L.cur_stream()), 'eld_tile_noise_sums_u16')
    return TileSums(out.cpu().numpy(), p, stride, group, G, (Hc, Wc))


# ---- the estimator (host, float64, fixed order) -----------------------------------------------------------------------------------------
def level_bins(lev):
    """The signal bin of integer levels above black by the rule of csrc/levelbins.h (s <= 0 -> 0, s < 8 -> s, quarter octaves above),
    from the bin edges eld_amd.evaluate states: the number of lower edges of bins 1 .. NB - 2 that are <= s."""
    from .evaluate import bin_lower_edges
    return np.searchsorted(bin_lower_edges()[1:NB - 1], np.asarray(lev, np.int64), side='right').astype(np.int64)


def _check_ratio(ratio):
    try:
        num, den = ratio
    except (TypeError, ValueError):
        raise ValueError('ratio takes two integers (num, den), got %r' % (ratio,))
    for v in (num, den):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not (1 <= v <= MAX_RATIO):
            raise ValueError('ratio takes two integers in [1, %d], got %r' % (MAX_RATIO, ratio))
    return int(num), int(den)


def _pool(n, S, R, bins):
    """Integer sums per bin of the kept entries -> Python-int lists (NB,).  R is summed as two 32-bit halves so that no int64 overflows."""
    pn = np.bincount(bins, minlength=NB)                                             # counts only: exact
    out_n, out_S, out_R = [0] * NB, [0] * NB, [0] * NB
    for b in np.nonzero(pn)[0]:
        m = bins == b
        out_n[b] = int(n[m].sum())
        out_S[b] = int(S[m].sum())                                                   # |S| < 2^33 per entry, fewer than 2^29 entries
        out_R[b] = (int((R[m] >> 32).sum()) << 32) + int((R[m] & 0xFFFFFFFF).sum())
    return out_n, out_S, out_R


def _fit(pn, pS, pR, min_sites, what):
    """Points and line from pooled integer sums -> (K, sigma0_sq, points).  ValueError in burst_gain's wording."""
    from .burst import weighted_line
    use = [b for b in range(1, NB - 1) if pn[b] >= max(int(min_sites), 1) and pR[b] > 0]
    n = np.array([pn[b] for b in use], np.float64)
    mu = np.array([pS[b] / (9 * pn[b]) for b in use], np.float64)                    # Python integers: rounded once
    var = np.array([pR[b] / (36 * pn[b]) for b in use], np.float64)
    if len(use) < MIN_POINTS or np.ptp(mu) <= 0:
        raise ValueError('%s: fewer than four usable points (%d): the frame is saturated, too dark, too small, too textured or all one level'
                         % (what, len(use)))
    line = var
    for _ in range(FIT_ITERATIONS):
        K, s0 = weighted_line(n, mu, var, line, what)
        line = np.maximum(K * mu + s0, 1e-3 * var)
    return K, s0, {'bin': np.array(use, np.int64), 'n': n.astype(np.int64), 'mu': mu, 'var': var}


def estimate_noise(sums_or_frames, cfa='bayer', raw_pattern=None, black_level=None, white_level=16383, defects=None, stride=None,
                   green_only=None, ratio=(3, 2), min_fill=0.5, min_sites=2048, what='frame'):
    """K and the read noise of the frames' sensor at their (one) ISO -> NoiseEstimate.  sums_or_frames: a TileSums, or frames as tile_sums
    takes them together with its arguments (cfa .. green_only, ignored for a TileSums).  All frames are pooled.

    1. a tile-group entry is usable when it holds at least min_fill of the eligible sites of a full tile;
    2. it is kept iff 9 den D <= num R (ratio = (num, den)): the first-difference variance D / 4n is at most num / den times the
       second-difference variance R / 36n.  Evaluated in int64 (the bounds: MAX_RATIO);
    3. its level (2 S + 9 n) // (18 n) chooses its signal bin; n, S, R are pooled per bin as integers;
    4. bins 1 .. NB - 2 with at least min_sites sites give the points mu = S / 9n, var = R / 36n;
    5. the line is fitted with weights n / line^2 in three passes: line = var first, then max(K mu + sigma0^2, var / 1000) -- a single
       pass with n / var^2 weights low draws high and is biased low by about 2 %.
    ValueError on fewer than four points, on one signal level, or on a slope that is not a positive gain."""
    num, den = _check_ratio(ratio)
    min_fill = float(min_fill)
    if not (0.0 < min_fill <= 1.0):
        raise ValueError('min_fill must lie in (0, 1], got %r' % (min_fill,))
    if isinstance(min_sites, bool) or not isinstance(min_sites, (int, np.integer)) or min_sites < 1:
        raise ValueError('min_sites must be a positive integer, got %r' % (min_sites,))
    ts = sums_or_frames if isinstance(sums_or_frames, TileSums) else tile_sums(sums_or_frames, cfa, raw_pattern, black_level, white_level,
                                                                               defects, stride, green_only)
    s = ts.sums.reshape(-1, ts.G, 4)
    n, S, R, D = s[..., 0], s[..., 1], s[..., 2], s[..., 3]
    full = ts.full_sites()                                                           # (G,)
    usable = (n > 0) & (n.astype(np.float64) >= min_fill * full[None, :])
    kept = usable & (9 * den * D <= num * R)
    whole = usable & (n.astype(np.float64) == full[None, :])
    lev = (2 * S + 9 * n) // np.maximum(18 * n, 1)                                   # floors, also below black
    bins = level_bins(lev)
    pn, pS, pR = _pool(n[kept], S[kept], R[kept], bins[kept])
    K, s0, points = _fit(pn, pS, pR, min_sites, what)
    groups = {}
    for g in range(ts.G):
        k = kept[:, g]
        if not k.any():
            continue
        try:
            Kg, sg, pg = _fit(*_pool(n[k, g], S[k, g], R[k, g], bins[k, g]), min_sites=min_sites, what=what)
        except ValueError:
            continue
        groups[g] = {'K': Kg, 'sigma0_sq': sg, 'sigma': math.sqrt(max(sg, 0.0)), 'points': pg}
    nu, nw = int(usable.sum()), int(whole.sum())
    return NoiseEstimate(K, s0, points, kept.sum() / nu if nu else 0.0, (kept & whole).sum() / nw if nw else 0.0, groups, ts.stride, ts.period)


# ---- command line -----------------------------------------------------------------------------------------------------------------------
def build_parser():
    p = argparse.ArgumentParser(prog='python -m eld_amd.noiselevel', description='Gain and read noise from single uint16 raw mosaics (.npy).')
    p.add_argument('inputs', nargs='+', help='frames of one ISO: .npy files or quoted globs, each (Hm, Wm) or (n, Hm, Wm) uint16; they are pooled')
    p.add_argument('--meta', help='JSON sidecar (eld_amd.denoise): cfa, raw_pattern, black_level, white_point (or rawpy names), defects')
    p.add_argument('--defects', metavar='F', help='a defect map written by eld_amd.defects (.npz)')
    p.add_argument('--stride', type=int, help='distance to the same-colour neighbours (default 2 for Bayer, 3 for X-Trans)')
    p.add_argument('--all-colours', action='store_true', help='X-Trans: count every colour (use with --stride 6), not the greens alone')
    p.add_argument('--camera', metavar='TABLE', help="a calibrated table to compare with: its K range and its g_scale line's read noise at log K")
    p.add_argument('--json', action='store_true', help='print the result as one JSON object instead of the table')
    return p


def estimate_from_options(frames, o, stride=None, green_only=None):
    """estimate_noise on loaded frames under sidecar options (cfa, raw_pattern, black_level, white_point, defects)."""
    return estimate_noise(frames, o.get('cfa', 'bayer'), o.get('raw_pattern'), o.get('black_level'), o.get('white_point', 16383),
                          o.get('defects'), stride, green_only)


def table_check(camera, K):
    """The 'does this table fit this capture' numbers: the table's K range and the read noise of its g_scale line at log K."""
    from .classical import camera_table, sigma_from_table
    t = camera_table(camera)
    out = {'sigma_table': sigma_from_table(t, K), 'K_min': None, 'K_max': None, 'K_inside': None}
    try:
        out['K_min'], out['K_max'] = float(t['Kmin']), float(t['Kmax'])
        out['K_inside'] = bool(out['K_min'] <= K <= out['K_max'])
    except (KeyError, TypeError, ValueError):
        pass
    return out


def main(argv=None):
    from .burst import load_burst
    from .denoise import read_sidecar
    a = build_parser().parse_args(sys.argv[1:] if argv is None else argv)
    o = read_sidecar(a.meta) if a.meta else {}
    if a.defects is not None:
        o['defects'] = a.defects
    import glob
    from .dng import fill_from_tags
    fill_from_tags(o, [n for pat in a.inputs for n in sorted(glob.glob(pat))])        # below the sidecar, above the defaults
    est = estimate_from_options(load_burst(a.inputs), o, a.stride, False if a.all_colours else None)
    res = est.as_dict()
    if a.camera:
        res['camera'] = table_check(a.camera, est.K)
    if a.json:
        print(json.dumps(res))
        return 0
    print('K %.5g DN/e-  sigma %.4g DN%s' % (est.K, est.sigma, '  (negative intercept %.4g DN^2)' % est.sigma0_sq if est.negative_intercept else ''))
    print('tiles kept: %.1f %% of the usable ones (%.1f %% of the full ones), stride %d' % (100 * est.kept_share, 100 * est.full_kept_share, est.stride))
    for g, d in sorted(est.groups.items()):
        print('group %d: K %.5g  sigma %.4g  (%d points)' % (g, d['K'], d['sigma'], len(d['points']['bin'])))
    if a.camera:
        c = res['camera']
        if c['K_min'] is not None:
            print('table %s: K in [%.4g, %.4g] (%s), read noise at this K %.4g DN' % (a.camera, c['K_min'], c['K_max'],
                                                                                      'inside' if c['K_inside'] else 'OUTSIDE', c['sigma_table']))
        else:
            print('table %s: read noise at this K %.4g DN' % (a.camera, c['sigma_table']))
    print('%4s %10s %12s %12s' % ('bin', 'sites', 'mu', 'var'))
    for b, n, mu, var in zip(est.points['bin'], est.points['n'], est.points['mu'], est.points['var']):
        print('%4d %10d %12.3f %12.3f' % (b, n, mu, var))
    return 0


if __name__ == '__main__':
    sys.exit(main())
