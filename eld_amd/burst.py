"""Stack a burst of a static scene: a clean training target and the photon-transfer gain, without a laboratory.

    stack = stack_burst(frames, 'bayer', raw_pattern, black_level, white_level)     # frames (N,Hm,Wm) uint16, one scene, tripod
    stack.mean                                      # uint16 CUDA tensor (Hm,Wm): what FramePool / train_frames take as a clean frame
    stack.kept                                      # uint8: samples kept per site (0 stands for 256); kept < N marks motion, hits, flicker
    K = burst_gain([stack])['K']                    # DN per electron, from the (temporal mean, temporal variance) of every site

The mean of N short frames is the clean frame a tripod gives: where a long exposure at a ratio of 100-300 is out of reach, it replaces
it; a sample that lies further than k deviations of the OTHER N - 1 samples from their mean (a cosmic-ray hit, a passing object) is left
out.  The same pass sums, per colour group and signal bin, the temporal mean and variance of the sites nothing was rejected at: one
scene covers every signal level, so a burst stands in for the flat-field pairs of eld_amd.calibrate (a session may give 'bursts').
There is NO registration: a burst is a tripod burst.  What moves shows up as kept < N and is averaged over the frames it is absent from.
The kernel is csrc/burst.hip (eld_burst_stack_u16: integer arithmetic only, defined bit for bit); the rule, the eligibility conditions
and their selection bias are DESIGN.md sec. 20.

Command line: python -m eld_amd.burst 'burst/*.npy' --meta sensor.json -o clean.npy [--kept kept.npy] [--ptc ptc.json] [--defects map.npz]
[--k 5] [--min-dev 2]
"""
import argparse
import ctypes
import glob
import json
import sys

import numpy as np

from . import _lib as L

NB = L.PAIRSTATS_BINS
MAX_FRAMES = 256
TILE_UNITS = 2048               # csrc/burst.hip BS_UNITS: units (8, 2 or 1 adjacent sites of a row) per workgroup; the tests size a frame by it
TILE_SITES = TILE_UNITS * 8     # sites per workgroup on the 16-byte path
FLICKER_FACTOR = 3.0            # warn when the frame means spread more than this times what the sites' own temporal noise explains


class BurstStack:
    """What stack_burst returns.

    mean     uint16 CUDA tensor (Hm,Wm): the kept samples' mean, rounded half up
    kept     uint8 CUDA tensor (Hm,Wm): samples kept; 0 stands for 256 (only N = 256 can reach it when k >= 1.23)
    ptc      host int64 (G, NB, 4): per colour group and signal bin (sites, sum S1, sum V mod 2^32, sum V >> 32) over the eligible sites
    N        frames in the burst
    period, group, G, black    the layout the sums were taken with: cell (y % p) * p + x % p -> colour group and black level
    group_black   the black level of each group (the mean over its cells)
    cfa, white, k2q, min_dev   as given"""

    def __init__(self, mean, kept, ptc, N, cfa, period, group, G, black, white, k2q, min_dev):
        self.mean, self.kept, self.ptc, self.N = mean, kept, ptc, N
        self.cfa, self.period, self.group, self.G, self.black, self.white = cfa, period, list(group), G, list(black), white
        self.k2q, self.min_dev = k2q, min_dev
        g, b = np.asarray(self.group), np.asarray(self.black, np.float64)
        self.group_black = np.array([b[g == i].mean() if np.any(g == i) else np.nan for i in range(G)])

    def rejected_share(self):
        """The share of sites that lost at least one sample."""
        k = self.kept.to('cpu').numpy().astype(np.int64)
        k[k == 0] = 256
        return float(np.mean(k != self.N))


# ---- argument checks (host only: they run before any device work) ----------------------------------------------------------------------
def _k2q(k):
    if isinstance(k, bool) or not isinstance(k, (int, float, np.integer, np.floating)) or not np.isfinite(k) or k < 0:
        raise ValueError('k (deviations of the other frames) must be a number >= 0, got %r' % (k,))
    q = int(round(4.0 * float(k) * float(k)))
    if q > 256:
        raise ValueError('k must be at most 8 (4 k^2 <= 256), got %r' % (k,))
    return q


def _min_dev(min_dev):
    if isinstance(min_dev, bool) or not isinstance(min_dev, (int, np.integer)) or min_dev < 0 or min_dev > 65535:
        raise ValueError('min_dev must be an integer in [0, 65535] (DN), got %r' % (min_dev,))
    return int(min_dev)


def _check_burst(frames, cfa, what='frames'):
    from .denoise import _as_u16, _check_sides
    try:
        _, batched = _as_u16(frames)
    except ValueError as e:
        raise ValueError('%s: %s' % (what, e))
    if not batched:
        raise ValueError('%s: a burst is a stack (N, Hm, Wm), got shape %s' % (what, tuple(frames.shape)))
    N, Hm, Wm = (int(v) for v in frames.shape)
    if N < 2 or N > MAX_FRAMES:
        raise ValueError('%s: a burst holds 2 to %d frames, got %d' % (what, MAX_FRAMES, N))
    _check_sides(Hm, Wm, cfa)
    if Hm * Wm >= 1 << 31:
        raise ValueError('%s: a frame of %d x %d has 2^31 sites or more' % (what, Hm, Wm))
    return N, Hm, Wm


# ---- the kernel's wrapper ----------------------------------------------------------------------------------------------------------------
def stack_burst(frames, cfa='bayer', raw_pattern=None, black_level=None, white_level=16383, k=5.0, min_dev=2, defects=None):
    """Stack N frames of one static scene.  frames: uint16 (N,Hm,Wm), 2 <= N <= 256, a NumPy array or a CUDA uint16 / int16-view tensor.
    raw_pattern, black_level: as eld_amd.evaluate.pair_level_stats (Bayer: 4 colour groups by CFA position; X-Trans: 3 by colour);
    white_level: codes >= it are saturated.  k: a sample further than k sample deviations of the other N - 1 from their mean is rejected
    (N >= 4; k = 0 switches the rule off; k <= 8), but never one within min_dev DN of that mean.  defects: a DefectMap (or its path) whose
    sites are kept out of the photon-transfer sums; they still get a mean (repair them downstream, as every frame).  -> BurstStack.
    Bad arguments raise ValueError before any device work."""
    from . import calibrate as CAL
    from .evaluate import _cells, _white
    p, group, G, black = _cells(cfa, raw_pattern, black_level)
    white = _white(white_level)
    k2q, min_dev = _k2q(k), _min_dev(min_dev)
    N, Hm, Wm = _check_burst(frames, cfa)
    if defects is not None:
        from .defects import as_defect_map
        defects = as_defect_map(defects)
        defects.check_frames((Hm, Wm), cfa, 'stack_burst')
    import torch
    u = CAL._device_u16(frames)
    lib = L.lib()
    with torch.cuda.device(u.device):
        mean = torch.empty((Hm, Wm), dtype=torch.int16, device=u.device)
        kept = torch.empty((Hm, Wm), dtype=torch.uint8, device=u.device)
        ptc = torch.empty((G, NB, 4), dtype=torch.int64, device=u.device)
        need = lib.eld_burst_stack_workspace_bytes(N, Hm, Wm)
        ws = torch.empty(need, dtype=torch.uint8, device=u.device) if need else None
        bm = None if defects is None else defects.bitmap_on(u.device)
        L.check(lib.eld_burst_stack_u16(L.dptr(u), N, Hm, Wm, p, (ctypes.c_int * (p * p))(*group), G, (ctypes.c_int32 * (p * p))(*black), white,
                                        L.dptr(bm), k2q, min_dev, L.dptr(mean), L.dptr(kept), L.dptr(ptc), L.dptr(ws), need, L.cur_stream()),
                'eld_burst_stack_u16')
    return BurstStack(mean.view(torch.uint16), kept, ptc.cpu().numpy(), N, cfa, p, group, G, black, white, k2q, min_dev)


# ---- photon transfer (host, float64) -----------------------------------------------------------------------------------------------------
def _ptc_of(stack):
    """BurstStack or a dict {'ptc', 'N', 'group_black'} -> (ptc int64 (G,NB,4), N, black per group)"""
    if isinstance(stack, dict):
        ptc, N, blk = stack['ptc'], stack['N'], stack['group_black']
    else:
        ptc, N, blk = stack.ptc, stack.N, stack.group_black
    ptc = np.asarray(ptc)
    if ptc.dtype.kind not in 'iu' or ptc.ndim != 3 or ptc.shape[1:] != (NB, 4):
        raise ValueError('ptc must be an integer array (G, %d, 4), got %s %s' % (NB, ptc.dtype, ptc.shape))
    N = int(N)
    if N < 2:
        raise ValueError('a burst holds at least 2 frames, got N = %d' % N)
    blk = np.broadcast_to(np.asarray(blk, np.float64), (ptc.shape[0],))
    return ptc, N, blk


def ptc_points(stack):
    """The photon-transfer points of a stack, per (group, bin): -> dict of (G, NB) arrays
        'n'    int64, eligible sites
        'mu'   sum S1 / (N n) - black: the mean signal in DN above black
        'var'  sum V / (N (N - 1) n): the mean temporal sample variance in DN^2
    nan where the bin is empty.  The two halves of sum V are recombined in Python integers first: the sum may exceed 2^53."""
    ptc, N, blk = _ptc_of(stack)
    G = ptc.shape[0]
    n = ptc[..., 0].astype(np.int64)
    mu = np.full((G, NB), np.nan)
    var = np.full((G, NB), np.nan)
    for g, b in zip(*np.nonzero(n)):
        c = int(n[g, b])
        mu[g, b] = int(ptc[g, b, 1]) / (N * c) - blk[g]
        var[g, b] = ((int(ptc[g, b, 3]) << 32) + int(ptc[g, b, 2])) / (N * (N - 1) * c)
    return {'n': n, 'mu': mu, 'var': var}


def burst_gain(stacks, min_sites=64, what='burst'):
    """K and the intercept of the photon-transfer line var = K mu + sigma0^2 through all points of `stacks` (BurstStacks of one ISO) that
    hold at least min_sites sites; bins 0 (at or below black) and NB - 1 (saturated) never count.  Weighted least squares with weights
    n / var^2: the variance of a variance estimate goes as var^2 / n.  -> {'K', 'sigma0_sq', 'mu', 'var', 'n'} (the points used).
    ValueError on fewer than two usable points or a slope that is not positive."""
    if isinstance(stacks, (BurstStack, dict)):
        stacks = [stacks]
    n, mu, var = [], [], []
    for s in stacks:
        q = ptc_points(s)
        for k_, dst in (('n', n), ('mu', mu), ('var', var)):
            dst.append(q[k_][:, 1:NB - 1].reshape(-1))
    if not n:
        raise ValueError('%s: no stacks given' % what)
    n, mu, var = np.concatenate(n), np.concatenate(mu), np.concatenate(var)
    use = (n >= max(int(min_sites), 1)) & (var > 0)
    n, mu, var = n[use].astype(np.float64), mu[use], var[use]
    if mu.size < 2 or np.ptp(mu) <= 0:
        raise ValueError('%s: fewer than two usable photon-transfer points (%d): the burst is saturated, too dark, too small or all one level'
                         % (what, mu.size))
    w = n / (var * var)
    sw = float(np.sum(w))
    mw, vw = float(np.sum(w * mu) / sw), float(np.sum(w * var) / sw)
    sxx = float(np.sum(w * (mu - mw) ** 2))
    if sxx <= 0:
        raise ValueError('%s: the photon-transfer points share one signal level' % what)
    K = float(np.sum(w * (mu - mw) * (var - vw)) / sxx)
    if not K * float(np.ptp(mu)) > 1e-9 * abs(vw):                 # a rise below rounding error over the whole range is a flat line
        raise ValueError('%s: the photon-transfer slope is %r, not a positive gain' % (what, K))
    return {'K': K, 'sigma0_sq': vw - K * mw, 'mu': mu, 'var': var, 'n': n.astype(np.int64)}


# ---- flicker -------------------------------------------------------------------------------------------------------------------------------
def frame_levels(frames, cfa='bayer', raw_pattern=None, black_level=None, defects=None):
    """The mean level of every frame in DN above black, float64 (N,), and the sites behind it: eld_struct_sums_u16's exact cell sums."""
    from .evaluate import _cells
    from .structure import structure_sums
    p, _, _, black = _cells(cfa, raw_pattern, black_level)
    if cfa == 'xtrans' and raw_pattern is None:
        from .defects import xtrans_tables
        raw_pattern = xtrans_tables()['colour']
    elif raw_pattern is None:
        from .denoise import DEFAULT_PATTERN
        raw_pattern = DEFAULT_PATTERN
    cell = structure_sums(frames, cfa, raw_pattern, black, defects=defects)['cell']          # (N, p*p, 3) = (n, sum d, sum d^2)
    n = cell[..., 0].sum(axis=1)
    return cell[..., 1].sum(axis=1) / np.maximum(n, 1), int(n[0])


def flicker_check(levels, sites, stack, factor=FLICKER_FACTOR):
    """Was the light constant?  levels: the frames' mean levels (frame_levels), sites: the sites behind each.  The spread of the frame
    means that the sites' own temporal noise explains is sqrt(sum of the per-site variances) / sites, estimated from the stack's
    photon-transfer sums; a measured spread above `factor` times that is reported.  -> {'spread', 'expected', 'ratio', 'rel_spread',
    'warning'}; 'warning' is None or the text.  Flicker of relative size f adds f^2 s^2 to the temporal variance at signal s: it bends the
    photon-transfer line upward and biases K high by about f^2 s / K at the brightest point."""
    levels = np.asarray(levels, np.float64)
    ptc, N, _ = _ptc_of(stack)
    sum_v = sum((int(v[3]) << 32) + int(v[2]) for v in ptc.reshape(-1, 4))
    expected = float(np.sqrt(sum_v / (N * (N - 1))) / max(int(sites), 1))
    spread = float(np.std(levels, ddof=1)) if levels.size > 1 else 0.0
    level = float(np.mean(levels))
    out = {'spread': spread, 'expected': expected, 'ratio': spread / expected if expected > 0 else float('inf') if spread > 0 else 0.0,
           'rel_spread': spread / level if level > 0 else float('nan'), 'factor': float(factor), 'warning': None}
    if out['ratio'] > factor:
        out['warning'] = ('the frame means spread by %.3g DN (%.3g of the level), %.1f times what the noise of the sites explains (%.3g DN): the '
                          'light was not constant; flicker adds variance that grows with the square of the signal and biases K upward'
                          % (spread, out['rel_spread'], out['ratio'], expected))
    return out


# ---- command line --------------------------------------------------------------------------------------------------------------------------
def build_parser():
    p = argparse.ArgumentParser(prog='python -m eld_amd.burst', description='Stack a tripod burst of uint16 raw mosaics (.npy): clean frame and gain.')
    p.add_argument('inputs', nargs='+', help="the burst's frames: .npy files or quoted globs, each (Hm, Wm) or (n, Hm, Wm) uint16")
    p.add_argument('--meta', help='JSON sidecar (eld_amd.denoise): cfa, raw_pattern, black_level, white_point (or rawpy names), defects')
    p.add_argument('-o', '--out', required=True, help='the stacked frame (.npy, uint16): what train_frames reads as a clean frame')
    p.add_argument('--kept', metavar='OUT', help='write the samples kept per site (.npy, uint8; 0 stands for 256)')
    p.add_argument('--ptc', metavar='OUT', help='write the photon-transfer sums and the fitted line as JSON')
    p.add_argument('--defects', metavar='F', help='a defect map written by eld_amd.defects (.npz)')
    p.add_argument('--k', type=float, default=5.0, help='reject a sample beyond k deviations of the other frames (default 5; 0: off)')
    p.add_argument('--min-dev', type=int, default=2, help='never reject a sample within this many DN of the mean of the others (default 2)')
    return p


def load_burst(patterns):
    """File names or globs -> uint16 (N,Hm,Wm), in sorted order per pattern."""
    names = []
    for pat in patterns:
        hit = sorted(glob.glob(pat))
        if not hit:
            raise ValueError('no such file: %s' % pat)
        names.extend(hit)
    frames = []
    for nme in names:
        a = np.load(nme)
        if a.dtype != np.uint16 or a.ndim not in (2, 3):
            raise ValueError('%s: a uint16 mosaic (Hm, Wm) or stack (n, Hm, Wm) expected, got %s %s' % (nme, a.dtype, a.shape))
        frames.extend(list(a) if a.ndim == 3 else [a])
    if len({f.shape for f in frames}) != 1:
        raise ValueError('the frames of a burst share one shape, got %s' % sorted({f.shape for f in frames}))
    return np.stack(frames)


def run(frames, o, k=5.0, min_dev=2):
    """The command line's work on loaded frames and sidecar options -> (BurstStack, result dict)."""
    kw = dict(cfa=o.get('cfa', 'bayer'), raw_pattern=o.get('raw_pattern'), black_level=o.get('black_level'))
    defects = o.get('defects')
    if defects is not None:
        from .defects import as_defect_map
        defects = as_defect_map(defects)
    stack = stack_burst(frames, white_level=o.get('white_point', 16383), k=k, min_dev=min_dev, defects=defects, **kw)
    levels, sites = frame_levels(frames, defects=defects, **kw)
    res = {'N': stack.N, 'rejected_share': stack.rejected_share(), 'flicker': flicker_check(levels, sites, stack), 'K': None, 'sigma0': None,
           'frame_levels': levels.tolist()}
    res['warning'] = res['flicker']['warning']
    try:
        fit = burst_gain([stack])
        res['K'], res['sigma0_sq'] = fit['K'], fit['sigma0_sq']
        res['sigma0'] = float(np.sqrt(fit['sigma0_sq'])) if fit['sigma0_sq'] >= 0 else float('nan')
    except ValueError as e:
        res['gain_error'] = str(e)
    return stack, res


def main(argv=None):
    from .denoise import read_sidecar
    a = build_parser().parse_args(sys.argv[1:] if argv is None else argv)
    o = read_sidecar(a.meta) if a.meta else {}
    if a.defects is not None:
        o['defects'] = a.defects
    stack, res = run(load_burst(a.inputs), o, a.k, a.min_dev)
    np.save(a.out, stack.mean.cpu().numpy())
    print('stacked %d frames -> %s' % (res['N'], a.out))
    print('sites with a rejected sample: %.4f %%' % (100.0 * res['rejected_share']))
    if res['K'] is not None:
        print('K %.5g DN/e-  sigma0 %.4g DN' % (res['K'], res['sigma0']))
    else:
        print('no gain: %s' % res['gain_error'])
    if res['warning']:
        print('WARNING: %s' % res['warning'])
    if a.kept:
        np.save(a.kept, stack.kept.cpu().numpy())
    if a.ptc:
        with open(a.ptc, 'w') as fh:
            json.dump(dict(res, ptc=stack.ptc.tolist(), group_black=stack.group_black.tolist(), k2q=stack.k2q, min_dev=stack.min_dev), fh, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
