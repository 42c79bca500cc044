"""Stack a burst of a static scene: a clean training target and the photon-transfer gain, without a laboratory.

    stack = stack_burst(frames, 'bayer', raw_pattern, black_level, white_level)     # frames (N,Hm,Wm) uint16, one scene, tripod
    stack.mean                                      # uint16 CUDA tensor (Hm,Wm): what FramePool / train_frames take as a clean frame
    stack.kept                                      # uint8: samples kept per site (0 stands for 256); kept < N marks motion, hits, flicker
    K = burst_gain([stack])['K']                    # DN per electron, from the (temporal mean, temporal variance) of every site

The mean of N short frames is the clean frame a tripod gives: where a long exposure at a ratio of 100-300 is out of reach, it replaces
it; a sample that lies further than k deviations of the OTHER N - 1 samples from their mean (a cosmic-ray hit, a passing object) is left
out.  The same pass sums, per colour group and signal bin, the temporal mean and variance of the sites nothing was rejected at: one
scene covers every signal level, so a burst stands in for the flat-field pairs of eld_amd.calibrate (a session may give 'bursts').
Without align= there is no registration: a burst is a tripod burst.  What moves shows up as kept < N and is averaged over the frames it is
absent from.  The kernel is csrc/burst.hip (eld_burst_stack_u16: integer arithmetic only, defined bit for bit); the rule, the eligibility
conditions and their selection bias are DESIGN.md sec. 20.

A hand-held burst is registered first:

    stack = stack_burst(frames, 'bayer', raw_pattern, black_level, white_level, align=True)      # every frame aligned to frame 0
    al = align_burst(frames, 'bayer', ref=2); al.shift_px(); al.outlier_share()                  # or the field on its own
    stack = stack_burst(frames, ..., align=al); stack.present                                    # samples found inside the frame, per site

align_burst is a coarse-to-fine search over 16 x 16 tiles of a luma pyramid (one luma pixel per CFA cell); displacements are whole CFA
periods, so every sample stays a raw code of its site's colour and nothing is resampled.  The stack then gathers each site's samples
through the field and the rule above rejects what alignment could not fix (csrc/align.hip).  The gain still wants a
tripod: misalignment below one CFA period adds variance wherever the scene has gradients and biases K upward.

Command line: python -m eld_amd.burst 'burst/*.npy' --meta sensor.json -o clean.npy [--kept kept.npy] [--ptc ptc.json] [--defects map.npz]
[--k 5] [--min-dev 2] [--align [--ref N] [--disp field.npy]]
An -o that ends in .dng writes the stack from the device tensor as lossless-JPEG tiles (eld_amd.dng.write_dng, compression 7) with the tags of
the first .dng input, else of the sidecar.
"""
import argparse
import glob
import json
import sys

import numpy as np

from . import _lib as L
from . import mosaic as M
from .defects import as_defect_map

NB = L.PAIRSTATS_BINS
MAX_FRAMES = 256
TILE_UNITS = 2048               # csrc/burst.hip BS_UNITS: units (8, 2 or 1 adjacent sites of a row) per workgroup; the tests size a frame by it
TILE_SITES = TILE_UNITS * 8     # sites per workgroup on the 16-byte path
FLICKER_FACTOR = 3.0            # warn when the frame means spread more than this times what the sites' own temporal noise explains
ALIGN_TILE = 16                 # csrc/align.hip AL_T: tile side in luma pixels (CFA cells)
ALIGN_RADIUS = 4                # AL_R: search radius per pyramid level
ALIGN_MAX_LEVELS = 4
ALIGN_MAX_DISP = ALIGN_RADIUS * (1 + 2 + 4 + 8)     # 60 luma pixels: what four levels can reach


class BurstStack:
    """What stack_burst returns.

    mean     uint16 CUDA tensor (Hm,Wm): the kept samples' mean, rounded half up
    kept     uint8 CUDA tensor (Hm,Wm): samples kept; 0 stands for 256 (only N = 256 can reach it when k >= 1.23)
    ptc      host int64 (G, NB, 4): per colour group and signal bin (sites, sum S1, sum V mod 2^32, sum V >> 32) over the eligible sites
    N        frames in the burst
    period, group, G, black    the layout the sums were taken with: cell (y % p) * p + x % p -> colour group and black level
    group_black   the black level of each group (the mean over its cells)
    cfa, white, k2q, min_dev   as given
    present  None, or for an aligned stack a uint8 CUDA tensor (Hm,Wm): the frames whose sample lay inside the frame (0 stands for 256);
             kept counts out of present, and only sites with present == N enter ptc
    align    None, or the BurstAlignment the samples were gathered through"""

    def __init__(self, mean, kept, ptc, N, cfa, period, group, G, black, white, k2q, min_dev, present=None, align=None):
        self.mean, self.kept, self.ptc, self.N = mean, kept, ptc, N
        self.present, self.align = present, align
        self.cfa, self.period, self.group, self.G, self.black, self.white = cfa, period, list(group), G, list(black), white
        self.k2q, self.min_dev = k2q, min_dev
        g, b = np.asarray(self.group), np.asarray(self.black, np.float64)
        self.group_black = np.array([b[g == i].mean() if np.any(g == i) else np.nan for i in range(G)])

    def rejected_share(self):
        """The share of sites that lost at least one sample."""
        k = self.kept.to('cpu').numpy().astype(np.int64)
        if self.present is None:
            k[k == 0] = 256
            return float(np.mean(k != self.N))
        m = self.present.to('cpu').numpy().astype(np.int64)
        if self.N == 256:
            m[m == 0] = 256                                        # frame ref is always present: 0 can only stand for 256
            k[(k == 0) & (m == 256)] = 256                         # k2q >= 6 keeps at least one sample
        return float(np.mean(k != m))

    def absent_share(self):
        """The share of sites that some frame's sample fell outside the frame for (aligned stacks; 0.0 otherwise)."""
        if self.present is None:
            return 0.0
        m = self.present.to('cpu').numpy().astype(np.int64)
        return float(np.mean(m != self.N % 256))


class BurstAlignment:
    """What align_burst returns, and what stack_burst(align=...) takes.

    disp     host int16 (N, TY, TX, 2): (dy, dx) of every 16 x 16-cell tile of every frame, in luma pixels = CFA periods; zero for frame ref
    cost     host uint32 (N, TY, TX): the winning candidate's sum of absolute luma differences over the tile (None when built by hand)
    period   the CFA period the field counts in (2 Bayer, 6 X-Trans);  tile = 16;  levels: pyramid levels searched;  ref: the reference frame"""

    def __init__(self, disp, cost=None, period=2, tile=ALIGN_TILE, levels=1, ref=0):
        disp = np.asarray(disp)
        if disp.dtype.kind not in 'iu' or disp.ndim != 4 or disp.shape[3] != 2:
            raise ValueError('disp must be an integer array (N, TY, TX, 2), got %s %s' % (disp.dtype, disp.shape))
        if disp.size and np.abs(disp.astype(np.int64)).max() > ALIGN_MAX_DISP:
            raise ValueError('a displacement beyond +-%d luma pixels' % ALIGN_MAX_DISP)
        if cost is not None:
            cost = np.asarray(cost)
            if cost.shape != disp.shape[:3]:
                raise ValueError('cost must have shape %s, got %s' % (disp.shape[:3], cost.shape))
            cost = cost.astype(np.uint32)
        if period not in (2, 6) or tile != ALIGN_TILE:
            raise ValueError('period must be 2 or 6 and tile %d, got %r and %r' % (ALIGN_TILE, period, tile))
        self.disp, self.cost = np.ascontiguousarray(disp.astype(np.int16)), cost
        self.period, self.tile, self.levels, self.ref = int(period), int(tile), int(levels), int(ref)

    def _median(self):
        N = self.disp.shape[0]
        return np.median(self.disp.reshape(N, -1, 2).astype(np.float64), axis=1)

    def shift_px(self):
        """float64 (N, 2): every frame's median displacement (dy, dx) in mosaic pixels."""
        return self._median() * self.period

    def outlier_share(self):
        """float64 (N,): per frame, the share of tiles more than 1 luma pixel (in either axis) from the frame's median displacement."""
        N = self.disp.shape[0]
        d = np.abs(self.disp.reshape(N, -1, 2).astype(np.float64) - self._median()[:, None, :])
        return np.mean(d.max(axis=2) > 1.0, axis=1)


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
    N, Hm, Wm = M.check_stack(frames, what)
    if len(frames.shape) != 3:
        raise ValueError('%s: a burst is a stack (N, Hm, Wm), got shape %s' % (what, tuple(frames.shape)))
    if N < 2 or N > MAX_FRAMES:
        raise ValueError('%s: a burst holds 2 to %d frames, got %d' % (what, MAX_FRAMES, N))
    M.check_sides(Hm, Wm, cfa)
    M.check_site_count(Hm, Wm, what)
    return N, Hm, Wm


def align_levels(Hm, Wm, p, levels=None):
    """The pyramid levels of a frame: the largest count (1..4) whose every level keeps both sides >= ALIGN_TILE luma pixels when levels is
    None, else `levels` checked against that.  ValueError when the frame is below one tile or the count does not fit."""
    h, w = Hm // p, Wm // p
    if h < ALIGN_TILE or w < ALIGN_TILE:
        raise ValueError('a frame of %d x %d has a luma plane of %d x %d, below one %d x %d tile: too small to align'
                         % (Hm, Wm, h, w, ALIGN_TILE, ALIGN_TILE))
    most = 1
    while most < ALIGN_MAX_LEVELS and (h + 1) // 2 >= ALIGN_TILE and (w + 1) // 2 >= ALIGN_TILE:
        h, w, most = (h + 1) // 2, (w + 1) // 2, most + 1
    if levels is None:
        return most
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or levels < 1 or levels > ALIGN_MAX_LEVELS:
        raise ValueError('levels must be an integer in [1, %d], got %r' % (ALIGN_MAX_LEVELS, levels))
    if levels > most:
        raise ValueError('levels = %d: level %d of a %d x %d frame has a side below %d (at most %d levels)'
                         % (levels, levels - 1, Hm, Wm, ALIGN_TILE, most))
    return int(levels)


def _tile_grid(Hm, Wm, p):
    return -(-(Hm // p) // ALIGN_TILE), -(-(Wm // p) // ALIGN_TILE)


def _check_ref(ref, N):
    if isinstance(ref, bool) or not isinstance(ref, (int, np.integer)) or ref < 0 or ref >= N:
        raise ValueError('ref must be a frame of the burst (0..%d), got %r' % (N - 1, ref))
    return int(ref)


# ---- the kernels' wrappers ---------------------------------------------------------------------------------------------------------------
def align_burst(frames, cfa='bayer', ref=0, levels=None):
    """Register every frame of a burst to frame `ref`: a coarse-to-fine search of 16 x 16-cell tiles over a luma pyramid of `levels` levels
    (default: as many as the frame allows, at most 4; each level doubles the reach: 4, 12, 28, 60 CFA periods).  -> BurstAlignment.
    Translation per tile in whole CFA periods; no rotation model, no exposure compensation.  Bad arguments raise ValueError before any
    device work."""
    p = M.period_of(cfa)
    N, Hm, Wm = _check_burst(frames, cfa)
    ref = _check_ref(ref, N)
    levels = align_levels(Hm, Wm, p, levels)
    TY, TX = _tile_grid(Hm, Wm, p)
    import torch
    lib = L.lib()
    u = M.device_u16(frames)
    with torch.cuda.device(u.device):
        disp = torch.empty((N, TY, TX, 2), dtype=torch.int16, device=u.device)
        cost = torch.empty((N, TY, TX), dtype=torch.int32, device=u.device)
        need = lib.eld_burst_align_workspace_bytes(N, Hm, Wm, p, levels)
        ws = torch.empty(max(need, 4), dtype=torch.uint8, device=u.device)
        L.check(lib.eld_burst_align_u16(L.dptr(u), N, Hm, Wm, p, ref, levels, L.dptr(disp), L.dptr(cost), L.dptr(ws), need, L.cur_stream()),
                'eld_burst_align_u16')
    return BurstAlignment(disp.cpu().numpy(), cost.cpu().numpy().view(np.uint32), p, ALIGN_TILE, levels, ref)


def _check_alignment(align, N, Hm, Wm, p):
    if not isinstance(align, BurstAlignment):
        raise ValueError('align must be None, True or a BurstAlignment, got %r' % (type(align).__name__,))
    if align.period != p:
        raise ValueError('the alignment counts in CFA periods of %d, the burst has %d' % (align.period, p))
    want = (N,) + _tile_grid(Hm, Wm, p) + (2,)
    if align.disp.shape != want:
        raise ValueError('the alignment field has shape %s, a burst of %d frames of %d x %d takes %s' % (align.disp.shape, N, Hm, Wm, want))
    return align


def stack_burst(frames, cfa='bayer', raw_pattern=None, black_level=None, white_level=16383, k=5.0, min_dev=2, defects=None, align=None):
    """Stack N frames of one static scene.  frames: uint16 (N,Hm,Wm), 2 <= N <= 256, a NumPy array or a CUDA uint16 / int16-view tensor.
    raw_pattern, black_level: as eld_amd.evaluate.pair_level_stats (Bayer: 4 colour groups by CFA position; X-Trans: 3 by colour);
    white_level: codes >= it are saturated.  k: a sample further than k sample deviations of the other N - 1 from their mean is rejected
    (N >= 4; k = 0 switches the rule off; k <= 8), but never one within min_dev DN of that mean.  defects: a DefectMap (or its path) whose
    sites are kept out of the photon-transfer sums; they still get a mean (repair them downstream, as every frame).  -> BurstStack.
    align: None stacks the frames as they lie (a tripod burst); True registers them to frame 0 first (align_burst), a BurstAlignment is used
    as given.  An aligned stack takes each site's samples through the field, reports in `present` how many lay inside the frame, applies
    the rule over those, and counts only sites with all N present in the photon-transfer sums.
    Bad arguments raise ValueError before any device work."""
    lay = M.CfaLayout.for_codes(cfa, raw_pattern, black_level)
    p, group, G, black = lay.period, lay.group, lay.G, lay.black_ints
    white = M.check_white(white_level)
    k2q, min_dev = _k2q(k), _min_dev(min_dev)
    N, Hm, Wm = _check_burst(frames, cfa)
    if defects is not None:
        defects = as_defect_map(defects)
        defects.check_frames((Hm, Wm), cfa, 'stack_burst')
    if align is not None and align is not False and align is not True:
        _check_alignment(align, N, Hm, Wm, p)
    if align is True:
        align_levels(Hm, Wm, p)
    import torch
    lib = L.lib()
    u = M.device_u16(frames)
    if align is not None and align is not False:
        if align is True:
            align = align_burst(u, cfa, 0)
        TY, TX = align.disp.shape[1:3]
        with torch.cuda.device(u.device):
            mean = torch.empty((Hm, Wm), dtype=torch.int16, device=u.device)
            kept = torch.empty((Hm, Wm), dtype=torch.uint8, device=u.device)
            present = torch.empty((Hm, Wm), dtype=torch.uint8, device=u.device)
            ptc = torch.empty((G, NB, 4), dtype=torch.int64, device=u.device)
            disp = torch.from_numpy(align.disp).to(u.device)
            need = lib.eld_burst_stack_aligned_workspace_bytes(N, Hm, Wm)
            ws = torch.empty(max(need, 4), dtype=torch.uint8, device=u.device)
            bm = None if defects is None else defects.bitmap_on(u.device)
            L.check(lib.eld_burst_stack_aligned_u16(L.dptr(u), N, Hm, Wm, p, lay.c_group(), G, lay.c_black(), white, L.dptr(bm), k2q, min_dev, L.dptr(disp), TY, TX, L.dptr(mean), L.dptr(kept),
                                                    L.dptr(present), L.dptr(ptc), L.dptr(ws), need, L.cur_stream()),
                    'eld_burst_stack_aligned_u16')
        return BurstStack(mean.view(torch.uint16), kept, ptc.cpu().numpy(), N, cfa, p, group, G, black, white, k2q, min_dev, present, align)
    with torch.cuda.device(u.device):
        mean = torch.empty((Hm, Wm), dtype=torch.int16, device=u.device)
        kept = torch.empty((Hm, Wm), dtype=torch.uint8, device=u.device)
        ptc = torch.empty((G, NB, 4), dtype=torch.int64, device=u.device)
        need = lib.eld_burst_stack_workspace_bytes(N, Hm, Wm)
        ws = M.workspace(need, u.device)
        bm = None if defects is None else defects.bitmap_on(u.device)
        L.check(lib.eld_burst_stack_u16(L.dptr(u), N, Hm, Wm, p, lay.c_group(), G, lay.c_black(), white, L.dptr(bm), k2q, min_dev, L.dptr(mean), L.dptr(kept), L.dptr(ptc), L.dptr(ws), need, L.cur_stream()),
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
    K, sigma0_sq = weighted_line(n, mu, var, var, what)
    return {'K': K, 'sigma0_sq': sigma0_sq, 'mu': mu, 'var': var, 'n': n.astype(np.int64)}


def weighted_line(n, mu, var, line, what='burst'):
    """The weighted least-squares line var = K mu + sigma0^2 through float64 points with weights n / line^2 (line: the variance each point
    is believed to have; the variance of a variance estimate goes as line^2 / n), in a fixed order of operations.  -> (K, sigma0_sq).
    ValueError when the points share one signal level or the slope is not a positive gain.  Shared by burst_gain (line = var, one pass)
    and eld_amd.noiselevel.estimate_noise (which iterates on the fitted line)."""
    w = n / (line * line)
    sw = float(np.sum(w))
    mw, vw = float(np.sum(w * mu) / sw), float(np.sum(w * var) / sw)
    sxx = float(np.sum(w * (mu - mw) ** 2))
    if sxx <= 0:
        raise ValueError('%s: the photon-transfer points share one signal level' % what)
    K = float(np.sum(w * (mu - mw) * (var - vw)) / sxx)
    if not K * float(np.ptp(mu)) > 1e-9 * abs(vw):                 # a rise below rounding error over the whole range is a flat line
        raise ValueError('%s: the photon-transfer slope is %r, not a positive gain' % (what, K))
    return K, vw - K * mw


# ---- flicker -------------------------------------------------------------------------------------------------------------------------------
def frame_levels(frames, cfa='bayer', raw_pattern=None, black_level=None, defects=None):
    """The mean level of every frame in DN above black, float64 (N,), and the sites behind it: eld_struct_sums_u16's exact cell sums."""
    from .structure import structure_sums
    lay = M.CfaLayout.for_codes(cfa, raw_pattern, black_level)
    cell = structure_sums(frames, cfa, M.default_pattern(cfa, raw_pattern), lay.black_ints, defects=defects)['cell']          # (N, p*p, 3) = (n, sum d, sum d^2)
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
    p.add_argument('-o', '--out', required=True, help='the stacked frame: .npy (uint16), or .dng (lossless-JPEG tiles written from the device, with the tags of the first '
                                                        '.dng input, else of the sidecar); train_frames reads either as a clean frame')
    p.add_argument('--kept', metavar='OUT', help='write the samples kept per site (.npy, uint8; 0 stands for 256)')
    p.add_argument('--ptc', metavar='OUT', help='write the photon-transfer sums and the fitted line as JSON')
    p.add_argument('--defects', metavar='F', help='a defect map written by eld_amd.defects (.npz)')
    p.add_argument('--k', type=float, default=5.0, help='reject a sample beyond k deviations of the other frames (default 5; 0: off)')
    p.add_argument('--min-dev', type=int, default=2, help='never reject a sample within this many DN of the mean of the others (default 2)')
    p.add_argument('--align', action='store_true', help='a hand-held burst: register every frame to the reference frame before stacking')
    p.add_argument('--ref', type=int, default=0, metavar='N', help='the reference frame of --align (default 0)')
    p.add_argument('--disp', metavar='OUT', help='with --align: write the displacement field (.npy, int16 (N, TY, TX, 2), CFA periods)')
    return p


def load_burst(patterns):
    """File names or globs -> uint16 (N,Hm,Wm), in sorted order per pattern."""
    names = []
    for pat in patterns:
        hit = sorted(glob.glob(pat))
        if not hit:
            raise ValueError('no such file: %s' % pat)
        names.extend(hit)
    from .dng import load_frame
    frames = []
    for nme in names:
        a = load_frame(nme)
        if a.dtype != np.uint16 or a.ndim not in (2, 3):
            raise ValueError('%s: a uint16 mosaic (Hm, Wm) or stack (n, Hm, Wm) expected, got %s %s' % (nme, a.dtype, a.shape))
        frames.extend(list(a) if a.ndim == 3 else [a])
    if len({f.shape for f in frames}) != 1:
        raise ValueError('the frames of a burst share one shape, got %s' % sorted({f.shape for f in frames}))
    return np.stack(frames)


def run(frames, o, k=5.0, min_dev=2, align=False, ref=0):
    """The command line's work on loaded frames and sidecar options -> (BurstStack, result dict).  align: register the frames to frame
    `ref` first; the result then carries 'shift_px', 'outlier_share' and 'absent_share'."""
    kw = dict(cfa=o.get('cfa', 'bayer'), raw_pattern=o.get('raw_pattern'), black_level=o.get('black_level'))
    defects = o.get('defects')
    if defects is not None:
        defects = as_defect_map(defects)
    field = align_burst(frames, kw['cfa'], ref) if align else None
    stack = stack_burst(frames, white_level=o.get('white_point', 16383), k=k, min_dev=min_dev, defects=defects, align=field, **kw)
    levels, sites = frame_levels(frames, defects=defects, **kw)
    res = {'N': stack.N, 'rejected_share': stack.rejected_share(), 'flicker': flicker_check(levels, sites, stack), 'K': None, 'sigma0': None,
           'frame_levels': levels.tolist()}
    res['warning'] = res['flicker']['warning']
    if field is not None:
        res.update(ref=field.ref, levels=field.levels, shift_px=field.shift_px().tolist(), outlier_share=field.outlier_share().tolist(),
                   absent_share=stack.absent_share())
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
    from .dng import fill_from_tags
    names = [n for pat in a.inputs for n in sorted(glob.glob(pat))]
    fill_from_tags(o, names)                                                          # below the sidecar, above the defaults
    if (a.disp or a.ref) and not a.align:
        raise SystemExit('--ref and --disp go with --align')
    stack, res = run(load_burst(a.inputs), o, a.k, a.min_dev, a.align, a.ref)
    from .dng import is_dng, write_dng
    if is_dng(a.out):                                                                 # straight from the device tensor
        like = next((n for n in names if is_dng(n)), None)
        meta = None if like is not None else {k: o.get(k) for k in ('cfa', 'raw_pattern', 'black_level', 'white_point', 'wb', 'ccm', 'iso')}
        write_dng(a.out, stack.mean, meta=meta, like=like, compression=7)
    else:
        np.save(a.out, stack.mean.cpu().numpy())
    print('stacked %d frames -> %s' % (res['N'], a.out))
    print('sites with a rejected sample: %.4f %%' % (100.0 * res['rejected_share']))
    if a.align:
        print('aligned to frame %d over %d pyramid levels' % (res['ref'], res['levels']))
        for i, (sh, out) in enumerate(zip(res['shift_px'], res['outlier_share'])):
            print('frame %d: shift %+.0f %+.0f px (dy dx), outlier tiles %.2f %%' % (i, sh[0], sh[1], 100.0 * out))
        print('sites with a sample outside the frame: %.4f %%' % (100.0 * res['absent_share']))
    if res['K'] is not None:
        print('K %.5g DN/e-  sigma0 %.4g DN' % (res['K'], res['sigma0']))
        if a.align:
            print('  (a hand-held burst: misalignment below one CFA period adds variance where the scene has gradients and biases K '
                  'upward; take the gain from a tripod burst)')
    else:
        print('no gain: %s' % res['gain_error'])
    if res['warning']:
        print('WARNING: %s' % res['warning'])
    if a.kept:
        np.save(a.kept, stack.kept.cpu().numpy())
    if a.disp:
        np.save(a.disp, stack.align.disp)
    if a.ptc:
        with open(a.ptc, 'w') as fh:
            json.dump(dict(res, ptc=stack.ptc.tolist(), group_black=stack.group_black.tolist(), k2q=stack.k2q, min_dev=stack.min_dev), fh, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
