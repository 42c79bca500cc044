"""Flat-field maps: measure what MULTIPLIES the signal from the flat frames of a calibration manifest and divide it out.

Calibration (eld_amd.calibrate, eld_amd.shading) measures what is added to the signal.  Two per-site gains are left:

    prnu   pixel response non-uniformity: the fixed pattern that grows with the signal.  Averaging does not remove it, so the clean targets of
           eld_amd.burst and eld_amd.train_frames carry it.
    lens   lens shading: the smooth per-colour falloff towards the corners.

Both come from the same flats, split by scale: V, the mean signal of the good sites of a site's window in its own position plane (y % p, x % p),
is the smooth field; the site's own mean r against V is the PRNU.

    ff = fit_flat_field(sessions, 'bayer', raw_pattern, black_level, white_level=16383, radius=16, defects=dmap)    # sessions: calibrate's
    ff.save('flat.npz');  ff = FlatField.load('flat.npz');  print(ff.report)
    clean = ff.apply(mosaics, part='prnu')                           # integer path: rint((u - black) * gain + black)  (eld_flat_apply_u16)
    denoise_raw(..., flatfield=ff, lens='srgb')                      # PRNU fused into the input stage, lens gain behind the network
    FramePool(frames, ..., flatfield=ff)                             # clean training frames, corrected once at upload

Everything up to the last division is integer arithmetic on the device (eld_flat_sums_u16, eld_flat_box_u32): the maps do not depend on the
order the device works in, and tests/flatfield_ref.py restates them bit for bit.

report[colour] (R, G, B): rho_var = var(r / V), noise_var = mean(D / (F V)^2) (the share of rho_var that is the shot and read noise of the flats
themselves, from the pair differences), prnu_sigma = sqrt(max(0, rho_var - noise_var)), snr = prnu_sigma / sqrt(noise_var), falloff =
min(V) / max(V).  With snr < 1 the PRNU plane is mostly the noise of the flats: applying it ADDS a fixed pattern.  Shoot more flats, or use
part='lens' only.

Command line: python -m eld_amd.flatfield manifest.json -o flat.npz [--radius R] [--defects defects.npz]
"""
import argparse
import ctypes
import os
import sys

import numpy as np

from . import _lib as L
from . import calibrate as CAL
from . import mosaic as M
from .defects import as_defect_map, find_defects

MAX_FRAMES = 65536                   # the sum of a site over all flats stays exact in uint32
MAX_RADIUS = 64
PARTS = ('prnu', 'lens', 'both')
LENS_MODES = ('off', 'srgb', 'all')                  # where the lens plane applies in denoise_raw (eld_amd.denoise)
COLOURS = ('R', 'G', 'B')
REPORT_KEYS = ('rho_var', 'noise_var', 'prnu_sigma', 'snr', 'falloff', 'sites')


# ---- argument checks (host only) ----------------------------------------------------------------------------------------------------------
def check_radius(radius):
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= int(radius) <= MAX_RADIUS:
        raise ValueError('radius is a whole number of cells in [0, %d], got %r' % (MAX_RADIUS, radius))
    return int(radius)


def check_white(white_level):
    return M.check_white(white_level, 65535, 'white_level')


def check_part(part):
    if not isinstance(part, str) or part not in PARTS:
        raise ValueError('part must be one of %r, got %r' % (PARTS, part))
    return part


def check_lens(lens):
    if not isinstance(lens, str) or lens not in LENS_MODES:
        raise ValueError('lens must be one of %r, got %r' % (LENS_MODES, lens))
    return lens


def flat_frames(sessions, cfa='bayer'):
    """-> list of (Hm,Wm) frames, a, b, a, b, ... over every session that has 'flats' ((P,2,Hm,Wm)); a session without is skipped."""
    if not isinstance(sessions, (list, tuple)) or len(sessions) == 0:
        raise ValueError('sessions must be a non-empty list of {"flats": (P,2,Hm,Wm), ...}')
    frames, shape = [], None
    for i, s in enumerate(sessions):
        if not isinstance(s, dict):
            raise ValueError('session %d is not a dict' % i)
        if 'flats' not in s:
            continue
        fl = s['flats']
        if not (isinstance(fl, np.ndarray) or hasattr(fl, 'is_cuda')):
            raise ValueError("session %d: 'flats' must be a uint16 array or CUDA tensor (P,2,Hm,Wm), got %r" % (i, type(fl).__name__))
        sh = M.check_mosaics(fl, 4, 'session %d flats' % i, cfa)
        if sh[-2] % 2:
            raise ValueError('session %d flats: mosaic sides must be even, got %dx%d' % (i, sh[-2], sh[-1]))
        if shape is None:
            shape = sh[-2:]
        if sh[-2:] != shape:
            raise ValueError('all flats must have one shape, got %s and %s' % (shape, sh[-2:]))
        for k in range(sh[0]):
            frames.extend([fl[k][0], fl[k][1]])
    if not frames:
        raise ValueError("no session has 'flats': a flat-field map needs flat pairs")
    if len(frames) > MAX_FRAMES:
        raise ValueError('a fit takes at most %d flat frames, got %d' % (MAX_FRAMES, len(frames)))
    return frames


def colour_table(cfa, pat):
    """(p,p) int64: the colour R 0, G 1, B 2 of every cell (both Bayer greens are G)."""
    return M.CODE_COLOUR[np.asarray(pat)].astype(np.int64)


cell_map = M.tile_cells                              # (p,p) table -> (Hm,Wm): the value of cell (y % p, x % p) at every site


def black_cells(cfa, pat, black):
    """(p,p) float32: the black level of every cell, per packed channel (Bayer) or colour code (X-Trans)."""
    return np.asarray(black, np.float64)[np.asarray(pat)].astype(np.float32)


def make_report(rho, nvar, V, ok, cmap):
    """The per-colour report from host float64 planes: rho = r / V, nvar = D / (F V)^2, V, the bool plane of the sites that count and the colour
    of every site.  NumPy reductions over the selected sites in row-major order (tests/flatfield_ref.py takes the same ones)."""
    out = {}
    for k, name in enumerate(COLOURS):
        sel = ok & (cmap == k)
        n = int(sel.sum())
        if n == 0:
            out[name] = dict(zip(REPORT_KEYS, [float('nan')] * 5 + [0]))
            continue
        rv, nv, v = float(np.var(rho[sel])), float(np.mean(nvar[sel])), V[sel]
        sig = float(np.sqrt(max(0.0, rv - nv)))
        out[name] = {'rho_var': rv, 'noise_var': nv, 'prnu_sigma': sig, 'snr': sig / float(np.sqrt(nv)) if nv > 0 else float('inf'),
                     'falloff': float(v.min() / v.max()), 'sites': n}
    return out


# ---- the map ------------------------------------------------------------------------------------------------------------------------------
class FlatField(M.FittedMap):
    """The flat-field map of one sensor and lens setting.

    lens, prnu   host float32 (Hm,Wm) gains (multiply the black-corrected signal); exactly 1.0 where nothing could be measured
    cfa, raw_pattern, shape, radius (cells), frames (flat frames of the fit), white_level, invalid (sites left at 1.0)
    report       {'R' | 'G' | 'B': {rho_var, noise_var, prnu_sigma, snr, falloff, sites}}"""
    NOUN = 'flat-field map'

    def __init__(self, lens, prnu, cfa='bayer', raw_pattern=None, radius=0, frames=0, white_level=16383, invalid=0, report=None):
        self.cfa = M.check_cfa(cfa)
        lens, prnu = np.ascontiguousarray(lens, dtype=np.float32), np.ascontiguousarray(prnu, dtype=np.float32)
        if lens.ndim != 2 or lens.shape != prnu.shape or lens.size == 0:
            raise ValueError('lens and prnu are two float32 planes of one shape (Hm, Wm), got %s and %s' % (lens.shape, prnu.shape))
        if lens.shape[1] % 2:
            raise ValueError('the mosaic width must be even, got %d' % lens.shape[1])
        for name, g in (('lens', lens), ('prnu', prnu)):
            if not np.all(np.isfinite(g)) or np.any(g <= 0):
                raise ValueError('the %s plane must be finite and > 0' % name)
        self.lens, self.prnu, self.shape = lens, prnu, tuple(int(v) for v in lens.shape)
        self.raw_pattern = M.CfaLayout.for_map(self.cfa, raw_pattern).codes
        self.radius, self.frames, self.white_level, self.invalid = check_radius(int(radius)), int(frames), check_white(white_level), int(invalid)
        self.report = {} if report is None else {c: {k: (int(v[k]) if k == 'sites' else float(v[k])) for k in REPORT_KEYS} for c, v in report.items()}
        self._both = None
        self._dev = {}
        self._packed = {}

    def plane(self, part):
        """The host gain plane of a part; 'both' is the float32 product of the two, formed once."""
        part = check_part(part)
        if part == 'both':
            if self._both is None:
                self._both = (self.lens * self.prnu).astype(np.float32)
            return self._both
        return self.lens if part == 'lens' else self.prnu

    def on(self, device, part='prnu'):
        """The gain plane of `part` as a float32 tensor on `device`, uploaded once."""
        import torch
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        key = (device, check_part(part))
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(self.plane(part)).to(device)
        return self._dev[key]

    def packed_lens(self, device):
        """The lens plane in the network's packed layout (1,C,h,w) on `device`: packed once with the existing packing routine, then cached."""
        return self.packed(device, 'lens')

    def packed(self, device, part='lens'):
        """The gain plane of `part` in the network's packed layout (1,C,h,w) on `device`, packed once per device and part."""
        import torch
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        key = (device, check_part(part))
        if key not in self._packed:
            Hm, Wm = self.shape
            src = self.on(device, part)
            with torch.cuda.device(device):
                if self.cfa == 'bayer':
                    # eld_pack_bayer's planes are the cell positions (0,0), (0,1), (1,1), (1,0); the network's plane k is the position of code k
                    out = torch.empty((1, 4, Hm // 2, Wm // 2), dtype=torch.float32, device=device)
                    L.check(L.lib().eld_pack_bayer(L.dptr(src), L.dptr(out), 1, Hm // 2, Wm // 2, L.cur_stream()), 'eld_pack_bayer')
                    plane_of_position = (0, 1, 3, 2)
                    order = [plane_of_position[int(np.flatnonzero(self.raw_pattern.reshape(-1) == k)[0])] for k in range(4)]
                    out = out[:, order].contiguous()
                else:
                    out = torch.empty((1, 9, 2 * (Hm // 6), 2 * (Wm // 6)), dtype=torch.float32, device=device)
                    L.check(L.lib().eld_pack_xtrans(L.dptr(src), L.dptr(out), 1, Hm, Wm, L.cur_stream()), 'eld_pack_xtrans')
            self._packed[key] = out
        return self._packed[key]

    def apply_device(self, t3, part, black, defects=None, out=None):
        """CUDA int16/uint16 codes (N,Hm,Wm), contiguous -> corrected codes in `out` (default: a new tensor; `t3` itself: in place).
        black: 4 black levels, per packed channel (Bayer) / colour code (X-Trans)."""
        import torch
        N, Hm, Wm = (int(v) for v in t3.shape)
        if out is None:
            out = torch.empty_like(t3)
        g = self.on(t3.device, part)
        p = self.period
        blk = (ctypes.c_float * (p * p))(*[float(v) for v in black_cells(self.cfa, self.raw_pattern, black).reshape(-1)])
        bm = None if defects is None else defects.bitmap_on(t3.device)
        with torch.cuda.device(t3.device):
            L.check(L.lib().eld_flat_apply_u16(L.dptr(t3), L.dptr(out), N, Hm, Wm, L.dptr(g), blk, p, self.white_level, L.dptr(bm), L.cur_stream()),
                    'eld_flat_apply_u16')
        return out

    def apply(self, mosaics, part='prnu', black_level=None, defects=None, out=None):
        """Multiply the black-corrected signal of uint16 mosaics, (Hm,Wm) or (N,Hm,Wm), by the gain plane of `part` ('prnu', 'lens' or 'both'):
        out = clamp(rint((u - black) * gain + black), 0, 65535) in float32, ties to even.  A site flagged in `defects` (a DefectMap) or with
        a code >= white_level passes through unchanged, so clipping stays detectable.  NumPy uint16 in -> NumPy out; CUDA uint16 / int16-view
        tensor in -> tensor out (out=: a contiguous CUDA tensor of the same shape and type, or `mosaics` itself for an in-place run with the
        same bits).  black_level: 1 or 4 values as fit_flat_field takes them.  Bad arguments raise ValueError before any device work."""
        part = check_part(part)
        kind, batched = M.as_u16(mosaics)
        shape = tuple(int(v) for v in mosaics.shape)
        self.check_frames(shape, self.cfa, 'apply')
        if batched and shape[0] < 1:
            raise ValueError('empty batch')
        black = M.CfaLayout.for_map(self.cfa, self.raw_pattern, black_level).black
        if defects is not None:
            defects = as_defect_map(defects)
            defects.check_frames(shape, self.cfa, 'apply')
        if kind == 'numpy':
            if out is not None:
                raise ValueError('out= takes a CUDA tensor; NumPy mosaics are returned as a new array')
            import torch
            t = torch.from_numpy(np.ascontiguousarray(mosaics).view(np.int16)).cuda().reshape((-1,) + self.shape)
            return self.apply_device(t, part, black, defects, t).cpu().numpy().view(np.uint16).reshape(shape)
        if out is not None:
            if not hasattr(out, 'is_cuda') or not out.is_cuda or out.dtype != mosaics.dtype or tuple(out.shape) != shape or not out.is_contiguous() \
                    or out.device != mosaics.device:
                raise ValueError('out must be a contiguous CUDA tensor of the shape, type and device of the mosaics')
        t = M.device_u16(mosaics)
        if out is not None and out.data_ptr() == mosaics.data_ptr() and t.data_ptr() != mosaics.data_ptr():
            raise ValueError('in-place correction needs contiguous, 4-byte aligned mosaics')
        o = self.apply_device(t.reshape((-1,) + self.shape), part, black, defects, None if out is None else out.reshape((-1,) + self.shape))
        return out if out is not None else o.reshape(shape)

    def save(self, path):
        """Write an .npz (no pickle).  Returns the path written ('.npz' is appended when it is missing, as np.savez does)."""
        path = os.fspath(path)
        if not path.endswith('.npz'):
            path += '.npz'
        rep = np.array([[self.report[c][k] for k in REPORT_KEYS] if c in self.report else [np.nan] * 5 + [0] for c in COLOURS], np.float64)
        np.savez(path, lens=self.lens, prnu=self.prnu, cfa=np.array(self.cfa), raw_pattern=np.asarray(self.raw_pattern, np.int64),
                 radius=np.int64(self.radius), frames=np.int64(self.frames), white_level=np.int64(self.white_level), invalid=np.int64(self.invalid),
                 report=rep)
        return path

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            for k in ('lens', 'prnu', 'cfa', 'raw_pattern', 'radius', 'frames', 'white_level', 'invalid', 'report'):
                if k not in z.files:
                    raise ValueError('%s is not a flat-field map: no %r' % (path, k))
            rep = {c: dict(zip(REPORT_KEYS, row)) for c, row in zip(COLOURS, z['report'])}
            return cls(z['lens'], z['prnu'], str(z['cfa']), z['raw_pattern'], int(z['radius']), int(z['frames']), int(z['white_level']),
                       int(z['invalid']), rep)


def as_flat_field(x, what='flatfield'):
    """A FlatField, or the path of a saved one -> FlatField; anything else is a ValueError."""
    if isinstance(x, FlatField):
        return x
    if isinstance(x, (str, os.PathLike)):
        if not os.path.exists(x):
            raise ValueError('%s: no such flat-field file: %s' % (what, x))
        return FlatField.load(x)
    raise ValueError('%s must be a FlatField or the path of a saved one, got %r' % (what, type(x).__name__))


# ---- the fit ------------------------------------------------------------------------------------------------------------------------------
def flat_sums(pool, white_level, defects=None):
    """eld_flat_sums_u16 on an uploaded FramePool whose frames all have one shape -> (S int32-view of uint32, D int64-view of uint64, bad
    int32-view of the uint32 bitmap) CUDA tensors."""
    import torch
    Hm, Wm = int(pool.frames['Hm'][0]), int(pool.frames['Wm'][0])
    S = torch.empty((Hm, Wm), dtype=torch.int32, device=pool.device)
    D = torch.empty((Hm, Wm), dtype=torch.int64, device=pool.device)
    bad = torch.empty((Hm, (Wm + 31) // 32), dtype=torch.int32, device=pool.device)
    bm = None if defects is None else defects.bitmap_on(pool.device)
    with torch.cuda.device(pool.device):
        L.check(L.lib().eld_flat_sums_u16(L.dptr(pool.buffer), pool.elems, L.dptr(pool._table_dev), len(pool), Hm, Wm, int(white_level), L.dptr(bm),
                                          L.dptr(S), L.dptr(D), L.dptr(bad), L.cur_stream()), 'eld_flat_sums_u16')
    return S, D, bad


def flat_box(S, bad, period, radius):
    """eld_flat_box_u32 -> (Bsum int64, Bcnt int32) CUDA tensors (Hm,Wm)."""
    import torch
    Hm, Wm = (int(v) for v in S.shape)
    Bsum = torch.empty((Hm, Wm), dtype=torch.int64, device=S.device)
    Bcnt = torch.empty((Hm, Wm), dtype=torch.int32, device=S.device)
    nbytes = L.lib().eld_flat_box_workspace_bytes(Hm, Wm)
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device=S.device)
    with torch.cuda.device(S.device):
        L.check(L.lib().eld_flat_box_u32(L.dptr(S), L.dptr(bad), Hm, Wm, int(period), int(radius), L.dptr(Bsum), L.dptr(Bcnt), L.dptr(ws), nbytes,
                                         L.cur_stream()), 'eld_flat_box_u32')
    return Bsum, Bcnt


def unpack_bad(bad, Wm):
    """The device bitmap (Hm, ceil(Wm/32)) int32 -> bool tensor (Hm,Wm)."""
    import torch
    bits = (bad.unsqueeze(-1) >> torch.arange(32, device=bad.device, dtype=torch.int32)) & 1
    return bits.reshape(bad.shape[0], -1)[:, :Wm].bool()


def flat_maps(S, D, bad, Bsum, Bcnt, F, centre, colours):
    """The float64 step on the device (elementwise torch).  S, D, Bsum, Bcnt as the kernels wrote them, bad: bool (Hm,Wm); centre, colours:
    (p,p) integer tables.  -> (lens, prnu float32 CUDA tensors, invalid, host float64 planes rho, nvar, V and the bool plane ok)."""
    import torch
    Hm, Wm = (int(v) for v in S.shape)
    dev = S.device
    cen = torch.from_numpy(cell_map(centre, Hm, Wm).astype(np.int64)).to(dev)
    cmap = torch.from_numpy(cell_map(colours, Hm, Wm).astype(np.int64)).to(dev)
    S64 = S.to(torch.int64) & 0xFFFFFFFF                                  # the uint32 sums
    n = Bcnt.to(torch.int64)
    one = torch.ones((), dtype=torch.float64, device=dev)
    den = (n * F).double()
    V = torch.where(n > 0, (Bsum - n * F * cen).double() / torch.where(n > 0, den, one), torch.zeros((), dtype=torch.float64, device=dev))
    # a device tensor as divisor: torch turns a division by a host scalar into a product with its reciprocal, which is not the correctly
    # rounded quotient unless F is a power of two
    r = (S64 - F * cen).double() / torch.full((), float(F), dtype=torch.float64, device=dev)
    ok = (~bad) & (n > 0) & (V > 0) & (r > 0)
    Vs, rs = torch.where(ok, V, one), torch.where(ok, r, one)
    vref = torch.ones((Hm, Wm), dtype=torch.float64, device=dev)
    for k in range(3):
        sel = ok & (cmap == k)
        if bool(sel.any()):
            vref = torch.where(cmap == k, V[sel].max(), vref)
    lens = torch.where(ok, (vref / Vs).float(), torch.ones((), dtype=torch.float32, device=dev))
    prnu = torch.where(ok, (Vs / rs).float(), torch.ones((), dtype=torch.float32, device=dev))
    rho = rs / Vs
    nvar = D.double() / ((float(F) * Vs) * (float(F) * Vs))
    invalid = int((~ok).sum())
    return lens, prnu, invalid, rho.cpu().numpy(), nvar.cpu().numpy(), V.cpu().numpy(), ok.cpu().numpy()


def fit_flat_field(sessions, cfa='bayer', raw_pattern=None, black_level=None, white_level=16383, radius=16, defects=None, device=None):
    """Flat pairs of all sessions -> FlatField.

    sessions     as eld_amd.calibrate takes them; every session with 'flats' ((P,2,Hm,Wm) uint16 ndarray or CUDA uint16 / int16-view tensor)
                 contributes all 2P frames, a session without is skipped; at most 65536 frames of one shape.  Sessions pool by plain summation:
                 summing codes weights each session by its signal, the weighting Poisson noise asks for.
    black_level  1 or 4 values, per packed channel (Bayer) or colour code (X-Trans) (default 512 / 1024); the signal is measured above
                 rint(black) of each site's cell (structure.cell_centres).
    white_level  a site with any code >= white_level is bad: it gets gain 1.0 and stays out of its neighbours' windows.
    radius       the window is (2 radius + 1)^2 cells of the site's position plane, clipped at the border; 0 <= radius <= 64.
    defects      a DefectMap or its path: flagged sites are bad likewise.
    Bad arguments raise ValueError before any device work; the fit itself needs a GPU."""
    cfa = M.check_cfa(cfa)
    lay = M.CfaLayout.for_map(cfa, raw_pattern, black_level)
    pat, centre, colours = lay.codes, lay.centres, lay.colour
    radius, white_level = check_radius(radius), check_white(white_level)
    frames = flat_frames(sessions, cfa)
    Hm, Wm = (int(v) for v in frames[0].shape)
    if defects is not None:
        defects = as_defect_map(defects)
        defects.check_frames((Hm, Wm), cfa, 'fit_flat_field')
    from .framepool import FramePool
    # the pool is the existing upload (one flat buffer, frames 16-byte aligned, an EldPoolFrame table); its levels are not used here
    pool = FramePool(frames, cfa=cfa, raw_pattern=pat if cfa == 'bayer' else None, white_point=65535, device=device)
    if pool.buffer is None:
        raise RuntimeError('fit_flat_field needs a GPU: there is no CPU fallback')
    p, F = centre.shape[0], len(frames)
    S, D, bad = flat_sums(pool, white_level, defects)
    Bsum, Bcnt = flat_box(S, bad, p, radius)
    lens, prnu, invalid, rho, nvar, V, ok = flat_maps(S, D, unpack_bad(bad, Wm), Bsum, Bcnt, F, centre, colours)
    report = make_report(rho, nvar, V, ok, cell_map(colours, Hm, Wm))
    out = FlatField(lens.cpu().numpy(), prnu.cpu().numpy(), cfa, pat, radius, F, white_level, invalid, report)
    out._dev[(lens.device, 'lens')], out._dev[(prnu.device, 'prnu')] = lens, prnu
    return out


# ---- command line -------------------------------------------------------------------------------------------------------------------------
def report_lines(ff):
    lines = []
    for c in COLOURS:
        r = ff.report.get(c)
        if r is None or r['sites'] == 0:
            lines.append('%s  no good sites' % c)
            continue
        lines.append('%s  prnu sigma %.4f %%  (var rho %.3e, noise %.3e, snr %.2f)  falloff %.3f  %d sites'
                     % (c, 100 * r['prnu_sigma'], r['rho_var'], r['noise_var'], r['snr'], r['falloff'], r['sites']))
        if r['snr'] < 1:
            lines.append("%s  snr < 1: the PRNU plane is mostly the shot noise of the flats; shoot more flats or apply part='lens' only" % c)
    return lines


def build_parser():
    ap = argparse.ArgumentParser(prog='python -m eld_amd.flatfield',
                                 description='Fit the flat-field map (PRNU and lens shading) of a sensor from the flat pairs of a calibration manifest.')
    ap.add_argument('manifest', help="calibrate's manifest JSON (the sessions with flats are used)")
    ap.add_argument('-o', '--out', required=True, help='the map to write (.npz)')
    ap.add_argument('--radius', type=int, default=16, help='window radius in cells of the CFA pattern, 0..64 (default 16)')
    ap.add_argument('--defects', metavar='PATH', help="a defect map (.npz); overrides the manifest's \"defects\"")
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    check_radius(a.radius)
    sessions, pattern, black, white, cfa = CAL.load_manifest(a.manifest, with_cfa=True)
    defects = a.defects if a.defects is not None else CAL.manifest_defects(a.manifest)
    if defects == 'auto':
        defects = find_defects(sessions[0]['bias'], cfa, pattern)[0]
    elif defects is not None:
        defects = as_defect_map(defects, '--defects')
    ff = fit_flat_field(sessions, cfa, pattern, black, white_level=white, radius=a.radius, defects=defects)
    out = ff.save(a.out)
    for line in report_lines(ff):
        print(line)
    print('%d flat frames, radius %d cells, %d x %d (%s), %d sites left at 1.0' % ((ff.frames, ff.radius) + ff.shape + (cfa, ff.invalid)))
    print('wrote', out)
    return 0


if __name__ == '__main__':
    sys.exit(main())
