"""Defective-pixel maps: detect hot, dead and stuck pixels in a stack of dark frames, keep them out of the calibration statistics and
repair them before frames reach the network.

    dmap, diag = find_defects(bias_frames, 'bayer', raw_pattern)        # (F,Hm,Wm) uint16 -> DefectMap
    dmap.save('defects.npz');  dmap = DefectMap.load('defects.npz')
    clean = repair(mosaics, dmap)                                       # flagged sites <- lower median of their unflagged neighbours
    calibrate_camera(..., defects=dmap);  denoise_raw(..., defects=dmap);  FramePool(..., defects=dmap)

The contract is all integer (include/eld_amd.h "defective-pixel maps"; csrc/defect.hip): the colour class of a site, its
same-class neighbourhood N in a (2R + 1)^2 window (Bayer R = 2; X-Trans: the radius the library derives from its index map), the lower
median (rank (m - 1) // 2), the deviation D = S - median_N(S) of the stack sum S, the flags D > T_hi / -D > T_lo, and the repair.  The
reference has no such stage (it relies on rawpy / LibRaw upstream): this one is pinned to that contract and to its NumPy restatement
(tests/defects_ref.py), bit for bit.

The thresholds are an interface default, not a calibrated quantity: sigma = 1.4826 * median|D| (the robust scale of the deviation) and
T_hi = T_lo = max(ceil(k * sigma), F * floor_dn) with k = 8 and floor_dn = 16 DN per frame.  Nothing pins k and floor_dn: pass
thresholds=(T_hi, T_lo), on the scale of the stack sum, to set them yourself.

Command line: python -m eld_amd.defects manifest.json -o defects.npz [--session I] (the calibration manifest of INTEGRATION.md; the bias
frames of the lowest-ISO session, or of session I, are stacked).
"""
import argparse
import ctypes
import json
import math
import os
import sys

import numpy as np

from . import _lib as L
from .mosaic import (XT_PERIOD, CfaLayout, SensorMap, as_u16, check_cfa, check_mosaics, device_u16, shape_of, tile_cells, workspace,
                     xtrans_tables)              # xtrans_tables: the library lookup lives in mosaic and stays importable from here

MAX_FRAMES = 4096                    # the stack sum stays exact in uint32
INT32_MAX = 2 ** 31 - 1


# ---- geometry (host) --------------------------------------------------------------------------------------------------------------------
def _class_pattern(cfa, raw_pattern):
    """-> (raw_pattern as int64 (p,p), class table int64 (p,p): Bayer channel codes, X-Trans colours) by CfaLayout.for_map."""
    lay = CfaLayout.for_map(cfa, raw_pattern)
    return lay.codes, lay.group_table


def _radius(cfa):
    return 2 if cfa == 'bayer' else xtrans_tables()['R']


def _check_shape(shape, cfa):
    s = tuple(int(v) for v in shape)
    if len(s) != 2:
        raise ValueError('a defect map has a 2-D shape (Hm, Wm), got %r' % (shape,))
    Hm, Wm = s
    if Hm < 1 or Wm < 1 or Hm * Wm > INT32_MAX:
        raise ValueError('mosaic sides must be positive with fewer than 2^31 sites, got %d x %d' % (Hm, Wm))
    if cfa == 'xtrans' and (Hm < XT_PERIOD or Wm < XT_PERIOD):
        raise ValueError('an X-Trans mosaic needs sides of at least 6, got %d x %d' % (Hm, Wm))
    return s


def pack_bitmap(mask):
    """bool (Hm,Wm) -> uint32 (Hm, ceil(Wm/32)): bit x & 31 of word [y][x >> 5]."""
    Hm, Wm = mask.shape
    pitch = (Wm + 31) // 32
    bits = np.zeros((Hm, pitch * 32), np.uint8)
    bits[:, :Wm] = mask
    return np.packbits(bits, axis=1, bitorder='little').view('<u4').reshape(Hm, pitch)


def unpack_bitmap(words, Wm):
    """uint32 (Hm, pitch) -> bool (Hm,Wm); set pad bits are an error."""
    words = np.ascontiguousarray(words, dtype='<u4')
    bits = np.unpackbits(words.view(np.uint8).reshape(words.shape[0], -1), axis=1, bitorder='little')
    if bits[:, Wm:].any():
        raise ValueError('the bitmap has bits set beyond the row width %d' % Wm)
    return bits[:, :Wm].astype(bool)


def stranded_sites(mask, cls, R):
    """The flagged sites (K',2) that have no unflagged site in their neighbourhood (same class, |dy|, |dx| <= R, inside the image)."""
    Hm, Wm = mask.shape
    ys, xs = np.nonzero(mask)
    if ys.size == 0:
        return np.zeros((0, 2), np.int32)
    cm = tile_cells(cls, Hm, Wm)
    ok = np.zeros(ys.size, bool)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            if dy == 0 and dx == 0:
                continue
            yy, xx = ys + dy, xs + dx
            inside = (yy >= 0) & (yy < Hm) & (xx >= 0) & (xx < Wm)
            yc, xc = np.clip(yy, 0, Hm - 1), np.clip(xx, 0, Wm - 1)
            ok |= inside & (cm[yc, xc] == cm[ys, xs]) & ~mask[yc, xc]
    return np.stack([ys[~ok], xs[~ok]], axis=1).astype(np.int32)


# ---- the map -------------------------------------------------------------------------------------------------------------------------------
class DefectMap(SensorMap):
    """The defective sites of one sensor.

    shape        (Hm, Wm) of the mosaics it applies to
    cfa          'bayer' or 'xtrans'
    raw_pattern  (2,2) / (6,6) int64, as given (None: RGGB / the library's X-Trans cell)
    sites        host (K,2) int32 (y, x), row-major order
    count        K
    words        host uint32 (Hm, ceil(Wm/32)): the bitmap
    bitmap       the same on the device (uploaded on first use; None without a GPU)"""
    NOUN = 'defect map'

    def __init__(self, shape, cfa, raw_pattern, mask):
        self.cfa = check_cfa(cfa)
        self.shape = _check_shape(shape, cfa)
        self.raw_pattern, self._cls = _class_pattern(cfa, raw_pattern)
        mask = np.asarray(mask, bool)
        if mask.shape != self.shape:
            raise ValueError('the mask has shape %s, the map %s' % (mask.shape, self.shape))
        bad = stranded_sites(mask, self._cls, _radius(cfa))
        if len(bad):
            raise ValueError('%d flagged site(s) have no unflagged neighbour of their colour to be repaired from, the first at (%d, %d): '
                             'the map flags a whole neighbourhood' % (len(bad), bad[0, 0], bad[0, 1]))
        self.sites = np.argwhere(mask).astype(np.int32).reshape(-1, 2)
        self.count = int(len(self.sites))
        self.words = pack_bitmap(mask)
        self._dev = {}

    @classmethod
    def from_sites(cls, sites, shape, cfa='bayer', raw_pattern=None):
        """sites: (K,2) integer (y, x) pairs inside `shape`, in any order, without duplicates."""
        cfa = check_cfa(cfa)
        Hm, Wm = _check_shape(shape, cfa)
        s = np.asarray(sites)
        if s.size == 0:
            s = np.zeros((0, 2), np.int64)
        if s.ndim != 2 or s.shape[1] != 2 or s.dtype.kind not in 'iu':
            raise ValueError('sites are rows of integer (y, x), got an array of shape %s and type %s' % (s.shape, s.dtype))
        s = s.astype(np.int64)
        if np.any(s < 0) or np.any(s[:, 0] >= Hm) or np.any(s[:, 1] >= Wm):
            raise ValueError('a site lies outside the %d x %d mosaic' % (Hm, Wm))
        mask = np.zeros((Hm, Wm), bool)
        mask[s[:, 0], s[:, 1]] = True
        if int(mask.sum()) != len(s):
            raise ValueError('duplicate sites')
        return cls((Hm, Wm), cfa, raw_pattern, mask)

    @property
    def mask(self):
        return unpack_bitmap(self.words, self.shape[1])

    @property
    def classes(self):
        """(p,p) int64 class table: Bayer channel codes, X-Trans colours."""
        return self._cls

    def c_pattern(self):
        flat = [int(v) for v in self._cls.reshape(-1)]
        return (ctypes.c_int * len(flat))(*flat)

    @property
    def bitmap(self):
        import torch
        return self.bitmap_on(torch.device('cuda', torch.cuda.current_device())) if torch.cuda.is_available() else None

    def bitmap_on(self, device):
        import torch
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if device not in self._dev:
            self._dev[device] = torch.from_numpy(self.words.view(np.int32).copy()).to(device)
        return self._dev[device]

    def save(self, path):
        """Write an .npz (no pickle): shape, cfa, raw_pattern, sites.  Returns the path written: '.npz' is appended when it is missing
        (as np.savez does), so load(save(name)) works for any name."""
        path = os.fspath(path)
        if not path.endswith('.npz'):
            path += '.npz'
        np.savez(path, shape=np.array(self.shape, np.int64), cfa=np.array(self.cfa), raw_pattern=np.asarray(self.raw_pattern, np.int64),
                 sites=self.sites)
        return path

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            for k in ('shape', 'cfa', 'raw_pattern', 'sites'):
                if k not in z.files:
                    raise ValueError('%s is not a defect map: no %r' % (path, k))
            return cls.from_sites(z['sites'], tuple(int(v) for v in z['shape']), str(z['cfa']), z['raw_pattern'])


def check_defects(defects, cfa, shape=None, raw_pattern=None):
    """The map must be for this CFA, these sides and -- X-Trans -- this pattern: its neighbourhoods are those of the colours of the 6x6
    cell it was built for.  A Bayer map's neighbourhoods are the sites at offsets of +-2 whatever the 2x2 permutation, so a Bayer map
    made under another raw_pattern flags and repairs the same sites: its raw_pattern is not compared."""
    if defects is None or (isinstance(defects, str) and defects == 'auto'):
        return defects
    if not isinstance(defects, DefectMap):
        raise ValueError("defects must be a DefectMap, 'auto' or None, got %r" % (type(defects).__name__,))
    if cfa == 'xtrans' and defects.cfa == 'xtrans' and raw_pattern is not None and not np.array_equal(CfaLayout('xtrans', raw_pattern).colour, defects.classes):
        raise ValueError('calibration: the defect map was built for another X-Trans raw_pattern (the colours of its 6x6 cell differ)')
    if shape is not None:
        defects.check_frames(shape, cfa, 'calibration')
    elif defects.cfa != cfa:
        raise ValueError('calibration: the defect map is for cfa=%r, the frames are %r' % (defects.cfa, cfa))
    return defects


def as_defect_map(defects, what='defects'):
    """A DefectMap, or a path to a saved one -> DefectMap; anything else is a ValueError."""
    if isinstance(defects, DefectMap):
        return defects
    if isinstance(defects, (str, os.PathLike)):
        if not os.path.exists(defects):
            raise ValueError('%s: no such defect map file: %s' % (what, defects))
        return DefectMap.load(defects)
    raise ValueError('%s must be a DefectMap or the path of a saved one, got %r' % (what, type(defects).__name__))


# ---- device passes -------------------------------------------------------------------------------------------------------------------------
def _check_stack(frames, cfa):
    check_cfa(cfa)
    if len(shape_of(frames)) == 2:
        frames = frames[None]
    F, Hm, Wm = check_mosaics(frames, 3, 'frames', cfa)
    if F < 1 or F > MAX_FRAMES:
        raise ValueError('a stack holds 1 to %d frames, got %d' % (MAX_FRAMES, F))
    return frames, F, Hm, Wm


def deviation(frames, cfa='bayer', raw_pattern=None):
    """(F,Hm,Wm) uint16 [ndarray or CUDA int16/uint16 tensor] -> D, CUDA int32 (Hm,Wm): the stack sum minus the lower median of the stack
    sum over the site's same-class neighbours."""
    import torch
    frames, F, Hm, Wm = _check_stack(frames, cfa)
    _, cls = _class_pattern(cfa, raw_pattern)
    u = device_u16(frames)
    D = torch.empty((Hm, Wm), dtype=torch.int32, device=u.device)
    ws = workspace(L.lib().eld_defect_deviation_workspace_bytes(Hm, Wm), u.device)
    flat = [int(v) for v in cls.reshape(-1)]
    with torch.cuda.device(u.device):
        L.check(L.lib().eld_defect_deviation(L.dptr(u), F, Hm, Wm, cls.shape[0], (ctypes.c_int * len(flat))(*flat), L.dptr(D), L.dptr(ws),
                                             ws.numel(), L.cur_stream()), 'eld_defect_deviation')
    return D


def flag_bitmap(D, T_hi, T_lo):
    """D CUDA int32 (Hm,Wm) -> the bitmap, CUDA int32 (Hm, ceil(Wm/32)) holding the uint32 words."""
    import torch
    Hm, Wm = D.shape
    bm = torch.empty((Hm, (Wm + 31) // 32), dtype=torch.int32, device=D.device)
    with torch.cuda.device(D.device):
        L.check(L.lib().eld_defect_flags(L.dptr(D), Hm, Wm, int(T_hi), int(T_lo), L.dptr(bm), L.cur_stream()), 'eld_defect_flags')
    return bm


def _check_thresholds(thresholds, k, floor_dn):
    if thresholds is not None:
        try:
            t = [int(v) for v in thresholds]
            exact = all(float(v) == float(int(v)) for v in thresholds)
        except (TypeError, ValueError):
            t, exact = [], False
        if len(t) != 2 or not exact or min(t) < 0 or max(t) > INT32_MAX:
            raise ValueError('thresholds are two integers (T_hi, T_lo) in [0, 2^31), on the scale of the stack sum, got %r' % (thresholds,))
        return t
    if not (isinstance(k, (int, float)) and math.isfinite(k) and k > 0):
        raise ValueError('k must be a finite number > 0, got %r' % (k,))
    if not (isinstance(floor_dn, (int, float)) and math.isfinite(floor_dn) and floor_dn >= 0):
        raise ValueError('floor_dn must be a finite number >= 0, got %r' % (floor_dn,))
    return None


def find_defects(frames, cfa='bayer', raw_pattern=None, k=8.0, floor_dn=16, thresholds=None):
    """Dark (bias) frames (F,Hm,Wm) uint16 of one shape -> (DefectMap, diag).

    thresholds=(T_hi, T_lo): int32 on the scale of the stack sum, used as given.  Otherwise sigma = 1.4826 * median|D| (the lower median,
    taken on the device) and T_hi = T_lo = max(ceil(k * sigma), F * floor_dn); k and floor_dn are interface defaults that nothing pins.
    diag: sigma, T_hi, T_lo, hot, cold (counts), D_min, D_max, frames.  Bad arguments raise ValueError before any device work; so does a
    result in which a flagged site has no unflagged neighbour to be repaired from (thresholds far too low)."""
    import torch
    frames, F, Hm, Wm = _check_stack(frames, cfa)
    _class_pattern(cfa, raw_pattern)
    t = _check_thresholds(thresholds, k, floor_dn)
    D = deviation(frames, cfa, raw_pattern)
    sigma = None
    if t is None:
        sigma = 1.4826 * float(D.abs().reshape(-1).median())           # torch's median of an even count is the lower one
        T = max(int(math.ceil(k * sigma)), int(math.ceil(F * floor_dn)))
        if T > INT32_MAX:
            raise ValueError('the threshold %d does not fit int32' % T)
        t = [T, T]
    bm = flag_bitmap(D, t[0], t[1])
    mask = unpack_bitmap(bm.cpu().numpy().view(np.uint32), Wm)
    hot = int((D > t[0]).sum())
    dmap = DefectMap((Hm, Wm), cfa, raw_pattern, mask)
    diag = {'sigma': sigma, 'T_hi': t[0], 'T_lo': t[1], 'hot': hot, 'cold': dmap.count - hot, 'D_min': int(D.min()), 'D_max': int(D.max()),
            'frames': F}
    dmap._dev[D.device] = bm
    return dmap, diag


def repair_device(t, dmap, out=None):
    """CUDA int16/uint16 codes (N,Hm,Wm), contiguous -> repaired codes in `out` (default: a new tensor; `t` itself: in place)."""
    import torch
    N, Hm, Wm = t.shape
    if out is None:
        out = torch.empty_like(t)
    with torch.cuda.device(t.device):
        L.check(L.lib().eld_defect_repair_u16(L.dptr(t), L.dptr(out), N, Hm, Wm, dmap.period, dmap.c_pattern(), L.dptr(dmap.bitmap_on(t.device)),
                                              L.cur_stream()), 'eld_defect_repair_u16')
    return out


def repair(mosaics, dmap, out=None):
    """Repair uint16 mosaics, (Hm,Wm) or (N,Hm,Wm): NumPy uint16 in -> NumPy out; CUDA uint16 / int16-view tensor in -> tensor out.
    out: None (a new array / tensor), or for a tensor a contiguous CUDA tensor of the same shape and type -- `mosaics` itself repairs in
    place, with the same bits.  A shape or CFA mismatch with the map raises ValueError before any device work."""
    if not isinstance(dmap, DefectMap):
        raise ValueError('dmap must be a DefectMap, got %r' % (type(dmap).__name__,))
    kind, batched = as_u16(mosaics)
    shape = tuple(int(v) for v in mosaics.shape)
    dmap.check_frames(shape, dmap.cfa, 'repair')
    if batched and shape[0] < 1:
        raise ValueError('empty batch')
    if kind == 'numpy':
        if out is not None:
            raise ValueError('out= takes a CUDA tensor; NumPy mosaics are returned as a new array')
        import torch
        t = torch.from_numpy(np.ascontiguousarray(mosaics).view(np.int16)).cuda().reshape((-1,) + dmap.shape)
        return repair_device(t, dmap, t).cpu().numpy().view(np.uint16).reshape(shape)
    if out is not None:
        if not hasattr(out, 'is_cuda') or not out.is_cuda or out.dtype != mosaics.dtype or tuple(out.shape) != shape or not out.is_contiguous() \
                or out.device != mosaics.device:
            raise ValueError('out must be a contiguous CUDA tensor of the shape, type and device of the mosaics')
    t = mosaics.contiguous()
    if out is not None and out.data_ptr() == mosaics.data_ptr() and t.data_ptr() != mosaics.data_ptr():
        raise ValueError('in-place repair needs contiguous mosaics')
    o = repair_device(t.reshape((-1,) + dmap.shape), dmap, None if out is None else out.reshape((-1,) + dmap.shape))
    return out if out is not None else o.reshape(shape)


# ---- command line --------------------------------------------------------------------------------------------------------------------------
def manifest_bias(path, session=None):
    """Calibration manifest -> (bias frames (F,Hm,Wm) of the lowest-ISO session or of session `session`, cfa, raw_pattern, index)."""
    with open(path) as f:
        m = json.load(f)
    base = os.path.dirname(os.path.abspath(path))
    ss = m.get('sessions') or []
    if not ss:
        raise ValueError('%s: the manifest has no sessions' % path)
    if session is None:
        isos = [s.get('iso') for s in ss]
        session = int(np.argmin([float(i) for i in isos])) if all(isinstance(i, (int, float)) for i in isos) else 0
    if not 0 <= int(session) < len(ss):
        raise ValueError('--session %r: the manifest has sessions 0..%d' % (session, len(ss) - 1))
    from .dng import common_meta, load_frame
    paths = [os.path.join(base, p) for p in ss[int(session)]['bias']]
    bias = np.stack([load_frame(p) for p in paths])
    if 'raw_pattern' not in m or 'cfa' not in m:                   # as calibrate.load_manifest: the first DNG's tags fill what the manifest omits
        tags = common_meta(paths)
        if tags is not None:
            m = dict({'cfa': tags['cfa'], 'raw_pattern': tags['raw_pattern']}, **m)
    return bias, check_cfa(m.get('cfa', 'bayer')), m['raw_pattern'], int(session)


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m eld_amd.defects', description='Find the defective pixels of a sensor from its bias frames.')
    ap.add_argument('manifest', help='the calibration manifest (JSON) of eld_amd.calibrate')
    ap.add_argument('-o', '--out', required=True, help='the map to write (.npz)')
    ap.add_argument('--session', type=int, help='index of the session whose bias frames are stacked (default: the lowest ISO)')
    ap.add_argument('--k', type=float, default=8.0, help='threshold in robust sigmas of the deviation (default 8)')
    ap.add_argument('--floor-dn', type=float, default=16, help='lowest threshold, DN per frame (default 16)')
    a = ap.parse_args(argv)
    bias, cfa, pattern, idx = manifest_bias(a.manifest, a.session)
    dmap, diag = find_defects(bias, cfa, pattern, k=a.k, floor_dn=a.floor_dn)
    out = dmap.save(a.out)
    print('session %d: %d frames of %d x %d (%s); sigma %.4g, thresholds +%d / -%d on the stack sum' % ((idx, diag['frames']) + dmap.shape +
                                                                                                     (cfa, diag['sigma'], diag['T_hi'], diag['T_lo'])))
    print('%d defective sites: %d hot, %d cold (deviation range %d .. %d)' % (dmap.count, diag['hot'], diag['cold'], diag['D_min'], diag['D_max']))
    print('wrote', out)
    return 0


if __name__ == '__main__':
    sys.exit(main())
