"""Dark shading: fit per-site offset maps over ISO from the bias frames and subtract them.

The fixed pattern of a sensor -- per-pixel and per-column offsets that are the same in every frame -- is the one noise component that need
not be learned: it can be measured and subtracted.  Per site the mean of the dark frames is close to linear in ISO (Feng et al.,
"Learnability Enhancement for Low-light Raw Denoising"), so one weighted line per site, fitted across ALL sessions of a calibration
manifest, pools every bias frame the user shot:

    offset(y, x, iso) = a(y, x) + b(y, x) * (iso - x0)

    shading = fit_dark_shading(sessions, 'bayer', raw_pattern, black_level, defects=dmap)      # sessions: calibrate's, 'iso' required
    shading.save('shading.npz');  shading = DarkShading.load('shading.npz')
    clean = shading.apply(mosaics, iso=1600)                         # integer path: u - rint(a + b t), clamped (eld_shading_apply_u16)
    denoise_raw(..., shading=shading, iso=1600)                      # float path, fused into the input stage (eld_pack_raw_*_u16_shaded)
    DarkPool(sessions, ..., shading=shading)                         # the sampler's dark frames, corrected once at upload
    validate_camera(..., structure=True, shading=shading)            # the structure report with the correction applied

The integer path leaves the fixed remainder ds - rint(ds), |.| <= 0.5 DN: variance 1/12 for a spread-out ds, the scale of the quantisation
the U term already models.  The float path (the inference input stage) rounds nothing to codes.

centred=False (default) removes the whole mean dark level above the nominal black, the per-colour offset included: right when training
(a corrected DarkPool under PDU) and inference subtract the same map.  centred=True takes the mean of every cell of the CFA pattern out of
both planes, so the per-colour offset (the B term of PGRUB) stays in the frames for a parametric model to synthesise.

Command line: python -m eld_amd.shading manifest.json -o shading.npz [--defects defects.npz] [--centred]
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

MAX_SESSIONS = 16
MAX_FRAMES = 65536                   # per session: the sum of a site over a session stays exact in uint32


# ---- the regression weights (host, float64) ---------------------------------------------------------------------------------------------
def fit_coefficients(isos, weights):
    """-> (x0, alpha, beta): the weighted least-squares line through the session means y_s at abscissa iso_s - x0 is
    a = sum alpha_s y_s (the value at x0), b = sum beta_s y_s (the slope).  x0 = sum w iso / sum w.  Python floats (float64), sums taken in
    session order, the 2x2 normal matrix [[W, Sx], [Sx, Sxx]] inverted in closed form:
        det = W * Sxx - Sx * Sx;  alpha_s = (Sxx * w_s - Sx * (w_s * d_s)) / det;  beta_s = (W * (w_s * d_s) - Sx * w_s) / det
    With fewer than two distinct ISOs the slope is not defined: alpha_s = w_s / W, beta_s = 0."""
    iso = [float(v) for v in isos]
    w = [float(v) for v in weights]
    W = 0.0
    for v in w:
        W = W + v
    sx = 0.0
    for v, i in zip(w, iso):
        sx = sx + v * i
    x0 = sx / W
    if len(set(iso)) < 2:
        return x0, [v / W for v in w], [0.0 for _ in w]
    d = [i - x0 for i in iso]
    Sx = Sxx = 0.0
    for v, di in zip(w, d):
        Sx = Sx + v * di
        Sxx = Sxx + (v * di) * di
    det = W * Sxx - Sx * Sx
    alpha = [(Sxx * v - Sx * (v * di)) / det for v, di in zip(w, d)]
    beta = [(W * (v * di) - Sx * v) / det for v, di in zip(w, d)]
    return x0, alpha, beta


# ---- argument checks (host only) ----------------------------------------------------------------------------------------------------------
def _sessions(sessions):
    """-> (frames: list of (Hm,Wm) arrays / tensors, ranges [(first, count)], isos [float])."""
    if not isinstance(sessions, (list, tuple)) or len(sessions) == 0:
        raise ValueError('sessions must be a non-empty list of {"iso", "bias"}')
    if len(sessions) > MAX_SESSIONS:
        raise ValueError('a fit takes at most %d sessions, got %d' % (MAX_SESSIONS, len(sessions)))
    frames, ranges, isos = [], [], []
    for i, s in enumerate(sessions):
        if not isinstance(s, dict) or 'bias' not in s:
            raise ValueError("session %d has no 'bias'" % i)
        iso = s.get('iso')
        if isinstance(iso, bool) or not isinstance(iso, (int, float, np.integer, np.floating)) or not np.isfinite(iso) or iso <= 0:
            raise ValueError("session %d: the fit is over ISO and needs a finite 'iso' > 0, got %r" % (i, iso))
        b = s['bias']
        items = [b] if (isinstance(b, np.ndarray) or hasattr(b, 'is_cuda')) else list(b)
        mine = []
        for m in items:
            _, batched = M.as_u16(m)
            mine.extend(list(m) if batched else [m])
        if not 1 <= len(mine) <= MAX_FRAMES:
            raise ValueError('session %d: 1 to %d bias frames, got %d' % (i, MAX_FRAMES, len(mine)))
        ranges.append((len(frames), len(mine)))
        frames.extend(mine)
        isos.append(float(iso))
    shape = tuple(int(v) for v in frames[0].shape)
    for m in frames:
        if tuple(int(v) for v in m.shape) != shape:
            raise ValueError('all bias frames must have one shape, got %s and %s' % (shape, tuple(int(v) for v in m.shape)))
    return frames, ranges, isos


def _weights(weights, ranges):
    if weights is None:
        return [float(c) for _, c in ranges]
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    if w.size != len(ranges) or not np.all(np.isfinite(w)) or np.any(w <= 0):
        raise ValueError('weights holds one finite weight > 0 per session (%d), got %r' % (len(ranges), weights))
    return [float(v) for v in w]


def centre_planes(a, b, period, flagged=None):
    """Take the mean over the unflagged sites of every cell (y % p, x % p) out of both planes, in place.  a, b: float32 torch tensors
    (Hm,Wm) on any device; flagged: bool tensor or None.  The mean is a float64 reduction rounded to float32, the subtraction float32;
    flagged sites keep their value (+0.0 from the fit)."""
    import torch
    for plane in (a, b):
        for r in range(period):
            for c in range(period):
                v = plane[r::period, c::period]
                if v.numel() == 0:
                    continue
                if flagged is None:
                    m = v.double().mean().float()
                    v -= m
                else:
                    good = ~flagged[r::period, c::period]
                    n = int(good.sum())
                    if n == 0:
                        continue
                    m = (torch.where(good, v.double(), torch.zeros((), dtype=torch.float64, device=v.device)).sum() / n).float()
                    v.copy_(torch.where(good, v - m, v))
    return a, b


# ---- the map ------------------------------------------------------------------------------------------------------------------------------
class DarkShading(M.FittedMap):
    """The dark-shading map of one sensor.

    a, b         host float32 (Hm,Wm): offset(iso) = a + b * (iso - x0), in DN above the nominal black level
    x0           the weighted mean ISO of the fit
    iso_min, iso_max   the ISO range of the fit's sessions: t() refuses an ISO outside it unless extrapolate=True
    cfa, raw_pattern, shape, centred
    counts, isos       per session: bias frames and ISO"""
    NOUN = 'dark-shading map'

    def __init__(self, a, b, x0, iso_min, iso_max, cfa='bayer', raw_pattern=None, centred=False, counts=(), isos=()):
        self.cfa = M.check_cfa(cfa)
        a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
        if a.ndim != 2 or a.shape != b.shape or a.size == 0:
            raise ValueError('a and b are two float32 planes of one shape (Hm, Wm), got %s and %s' % (a.shape, b.shape))
        if a.shape[1] % 2:
            raise ValueError('the mosaic width must be even, got %d' % a.shape[1])
        if not (np.all(np.isfinite(a)) and np.all(np.isfinite(b))):
            raise ValueError('the planes must be finite')
        self.a, self.b, self.shape = a, b, tuple(int(v) for v in a.shape)
        self.x0, self.iso_min, self.iso_max = float(x0), float(iso_min), float(iso_max)
        if not (np.isfinite(self.x0) and self.iso_min <= self.iso_max):
            raise ValueError('x0 must be finite and iso_min <= iso_max, got %r, %r, %r' % (x0, iso_min, iso_max))
        self.raw_pattern = M.CfaLayout.for_map(self.cfa, raw_pattern).codes
        self.centred = bool(centred)
        self.counts = [int(v) for v in counts]
        self.isos = [float(v) for v in isos]
        self._dev = {}

    def t(self, iso, extrapolate=False):
        """float32(iso - x0): the abscissa the kernels take.  ValueError for an ISO outside [iso_min, iso_max] unless extrapolate=True
        (a map fitted at one ISO is valid at that ISO only)."""
        if isinstance(iso, bool) or not isinstance(iso, (int, float, np.integer, np.floating)) or not np.isfinite(iso):
            raise ValueError('iso must be a finite number, got %r' % (iso,))
        if not extrapolate and not (self.iso_min <= float(iso) <= self.iso_max):
            raise ValueError('iso %g lies outside the range [%g, %g] this dark-shading map was fitted over (extrapolate=True to allow it)'
                             % (iso, self.iso_min, self.iso_max))
        return np.float32(float(iso) - self.x0)

    def on(self, device):
        """(a, b) as float32 tensors on `device`, uploaded once."""
        import torch
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if device not in self._dev:
            self._dev[device] = (torch.from_numpy(self.a).to(device), torch.from_numpy(self.b).to(device))
        return self._dev[device]

    def apply_device(self, t3, tval, defects=None, out=None):
        """CUDA int16/uint16 codes (N,Hm,Wm), contiguous -> corrected codes in `out` (default: a new tensor; `t3` itself: in place)."""
        import torch
        N, Hm, Wm = (int(v) for v in t3.shape)
        if out is None:
            out = torch.empty_like(t3)
        a, b = self.on(t3.device)
        bm = None if defects is None else defects.bitmap_on(t3.device)
        with torch.cuda.device(t3.device):
            L.check(L.lib().eld_shading_apply_u16(L.dptr(t3), L.dptr(out), N, Hm, Wm, L.dptr(a), L.dptr(b), float(tval), L.dptr(bm), L.cur_stream()),
                    'eld_shading_apply_u16')
        return out

    def apply(self, mosaics, iso, defects=None, out=None, extrapolate=False):
        """Subtract the map at `iso` from uint16 mosaics, (Hm,Wm) or (N,Hm,Wm): out = clamp(u - rint(a + b t), 0, 65535).  NumPy uint16 in
        -> NumPy out; CUDA uint16 / int16-view tensor in -> tensor out (out=: a contiguous CUDA tensor of the same shape and type, or
        `mosaics` itself for an in-place run with the same bits).  defects: a DefectMap whose flagged sites pass through unchanged (they
        are repaired elsewhere).  Bad arguments raise ValueError before any device work."""
        kind, batched = M.as_u16(mosaics)
        shape = tuple(int(v) for v in mosaics.shape)
        self.check_frames(shape, self.cfa, 'apply')
        if batched and shape[0] < 1:
            raise ValueError('empty batch')
        tval = self.t(iso, extrapolate)
        if defects is not None:
            defects = as_defect_map(defects)
            defects.check_frames(shape, self.cfa, 'apply')
        if kind == 'numpy':
            if out is not None:
                raise ValueError('out= takes a CUDA tensor; NumPy mosaics are returned as a new array')
            import torch
            t = torch.from_numpy(np.ascontiguousarray(mosaics).view(np.int16)).cuda().reshape((-1,) + self.shape)
            return self.apply_device(t, tval, defects, t).cpu().numpy().view(np.uint16).reshape(shape)
        if out is not None:
            if not hasattr(out, 'is_cuda') or not out.is_cuda or out.dtype != mosaics.dtype or tuple(out.shape) != shape or not out.is_contiguous() \
                    or out.device != mosaics.device:
                raise ValueError('out must be a contiguous CUDA tensor of the shape, type and device of the mosaics')
        t = M.device_u16(mosaics)
        if out is not None and out.data_ptr() == mosaics.data_ptr() and t.data_ptr() != mosaics.data_ptr():
            raise ValueError('in-place correction needs contiguous, 4-byte aligned mosaics')
        o = self.apply_device(t.reshape((-1,) + self.shape), tval, defects, None if out is None else out.reshape((-1,) + self.shape))
        return out if out is not None else o.reshape(shape)

    def save(self, path):
        """Write an .npz (no pickle).  Returns the path written ('.npz' is appended when it is missing, as np.savez does)."""
        path = os.fspath(path)
        if not path.endswith('.npz'):
            path += '.npz'
        np.savez(path, a=self.a, b=self.b, x0=np.float64(self.x0), iso_range=np.array([self.iso_min, self.iso_max], np.float64),
                 cfa=np.array(self.cfa), raw_pattern=np.asarray(self.raw_pattern, np.int64), centred=np.array(self.centred),
                 counts=np.asarray(self.counts, np.int64), isos=np.asarray(self.isos, np.float64))
        return path

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            for k in ('a', 'b', 'x0', 'iso_range', 'cfa', 'raw_pattern', 'centred', 'counts', 'isos'):
                if k not in z.files:
                    raise ValueError('%s is not a dark-shading map: no %r' % (path, k))
            return cls(z['a'], z['b'], float(z['x0']), float(z['iso_range'][0]), float(z['iso_range'][1]), str(z['cfa']), z['raw_pattern'],
                       bool(z['centred']), z['counts'], z['isos'])


def as_dark_shading(x, what='shading'):
    """A DarkShading, or the path of a saved one -> DarkShading; anything else is a ValueError."""
    if isinstance(x, DarkShading):
        return x
    if isinstance(x, (str, os.PathLike)):
        if not os.path.exists(x):
            raise ValueError('%s: no such dark-shading file: %s' % (what, x))
        return DarkShading.load(x)
    raise ValueError('%s must be a DarkShading or the path of a saved one, got %r' % (what, type(x).__name__))


# ---- the fit ------------------------------------------------------------------------------------------------------------------------------
def fit_planes(pool, ranges, alpha, beta, centre, period, defects=None):
    """eld_shading_fit_u16 on an uploaded FramePool whose frames all have one shape -> (a, b) float32 CUDA tensors (Hm,Wm)."""
    import torch
    Hm, Wm = int(pool.frames['Hm'][0]), int(pool.frames['Wm'][0])
    S = len(ranges)
    ses = (ctypes.c_int32 * (2 * S))(*[int(v) for r in ranges for v in r])
    al, be = (ctypes.c_double * S)(*alpha), (ctypes.c_double * S)(*beta)
    cen = (ctypes.c_int32 * (period * period))(*[int(v) for v in np.asarray(centre).reshape(-1)])
    a = torch.empty((Hm, Wm), dtype=torch.float32, device=pool.device)
    b = torch.empty((Hm, Wm), dtype=torch.float32, device=pool.device)
    bm = None if defects is None else defects.bitmap_on(pool.device)
    with torch.cuda.device(pool.device):
        L.check(L.lib().eld_shading_fit_u16(L.dptr(pool.buffer), pool.elems, L.dptr(pool._table_dev), len(pool), Hm, Wm, ses, S, al, be, cen, period,
                                            L.dptr(bm), L.dptr(a), L.dptr(b), L.cur_stream()), 'eld_shading_fit_u16')
    return a, b


def fit_dark_shading(sessions, cfa='bayer', raw_pattern=None, black_level=None, defects=None, weights=None, centred=False, device=None):
    """Bias frames of all sessions -> DarkShading.

    sessions     as eld_amd.darkpool.DarkPool takes them ({'iso', 'bias'}: (F,Hm,Wm) uint16 ndarray or CUDA uint16 / int16-view tensor, or
                 a list of (Hm,Wm) frames); 'iso' is required, all frames have one shape; at most 16 sessions of at most 65536 frames.
    black_level  the nominal black level: 1 or 4 values, per packed channel (Bayer) or colour code (X-Trans) as eld_amd.calibrate takes
                 them (default 512 / 1024); the map is in DN above rint(black) of each site's cell (structure.cell_centres).
    defects      a DefectMap or its path: flagged sites get a zero map (they are NOT repaired before the fit; they are repaired downstream).
    weights      one positive weight per session (default: its frame count, which makes the fit the least-squares line over all frames).
    centred      take the mean over the unflagged sites of every cell of the CFA pattern out of both planes (see the module text).
    Bad arguments raise ValueError before any device work; the fit itself needs a GPU."""
    cfa = M.check_cfa(cfa)
    lay = M.CfaLayout.for_map(cfa, raw_pattern, black_level)
    pat, centre = lay.codes, lay.centres
    frames, ranges, isos = _sessions(sessions)
    w = _weights(weights, ranges)
    Hm, Wm = (int(v) for v in frames[0].shape)
    if defects is not None:
        defects = as_defect_map(defects)
        defects.check_frames((Hm, Wm), cfa, 'fit_dark_shading')
    from .framepool import FramePool
    x0, alpha, beta = fit_coefficients(isos, w)
    # the pool is the existing upload (one flat buffer, frames 16-byte aligned, an EldPoolFrame table); its levels are not used here
    pool = FramePool(frames, cfa=cfa, raw_pattern=pat if cfa == 'bayer' else None, white_point=65535, device=device)
    if pool.buffer is None:
        raise RuntimeError('fit_dark_shading needs a GPU: there is no CPU fallback')
    p = centre.shape[0]
    a, b = fit_planes(pool, ranges, alpha, beta, centre, p, defects)
    if centred:
        import torch
        flagged = None if defects is None or not defects.count else torch.from_numpy(defects.mask).to(a.device)
        centre_planes(a, b, p, flagged)
    out = DarkShading(a.cpu().numpy(), b.cpu().numpy(), x0, min(isos), max(isos), cfa, pat, centred, [c for _, c in ranges], isos)
    out._dev[a.device] = (a, b)
    return out


# ---- command line -------------------------------------------------------------------------------------------------------------------------
def group_rms(shading, iso, defects=None):
    """r.m.s. of the map at `iso` per colour group (CfaLayout.group), over the unflagged sites, float64."""
    lay = M.CfaLayout(shading.cfa, shading.raw_pattern)
    G = lay.G
    ds = shading.a + shading.b * shading.t(iso, extrapolate=True)
    Hm, Wm = shading.shape
    gm = lay.tile(lay.group, Hm, Wm)
    good = np.ones((Hm, Wm), bool) if defects is None else ~defects.mask
    return [float(np.sqrt(np.mean(ds[(gm == g) & good].astype(np.float64) ** 2))) if np.any((gm == g) & good) else float('nan') for g in range(G)]


def build_parser():
    ap = argparse.ArgumentParser(prog='python -m eld_amd.shading', description='Fit the dark-shading map of a sensor from the bias frames of a calibration manifest.')
    ap.add_argument('manifest', help="calibrate's manifest JSON (every session needs its iso)")
    ap.add_argument('-o', '--out', required=True, help='the map to write (.npz)')
    ap.add_argument('--defects', metavar='PATH', help="a defect map (.npz); overrides the manifest's \"defects\"")
    ap.add_argument('--centred', action='store_true', help='keep the per-colour offset in the frames (for parametric models with B)')
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    sessions, pattern, black, white, cfa = CAL.load_manifest(a.manifest, with_cfa=True)
    defects = a.defects if a.defects is not None else CAL.manifest_defects(a.manifest)
    if defects == 'auto':
        defects = find_defects(sessions[0]['bias'], cfa, pattern)[0]
    elif defects is not None:
        defects = as_defect_map(defects, '--defects')
    sh = fit_dark_shading(sessions, cfa, pattern, black, defects=defects, centred=a.centred)
    out = sh.save(a.out)
    for iso, n in zip(sh.isos, sh.counts):
        print('iso %-6g %3d frames  map r.m.s. per colour group (DN): %s' % (iso, n, ' '.join('%.3f' % v for v in group_rms(sh, iso, defects))))
    print('x0 %.6g, ISO range [%g, %g], %d x %d (%s)%s' % ((sh.x0, sh.iso_min, sh.iso_max) + sh.shape + (cfa, ', centred' if sh.centred else '')))
    print('wrote', out)
    return 0


if __name__ == '__main__':
    sys.exit(main())
