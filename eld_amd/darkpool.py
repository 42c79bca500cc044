"""Sample signal-independent noise from the sensor's own dark frames (model letter 'D', flag DARK).

The bias frames a user shot for eld_amd.calibrate ARE samples of everything the sensor adds without light at that ISO: read noise of
whatever law, banding, fixed-pattern offsets, column structure, colour bias.  Instead of fitting a law to them, the sampler takes the shot
noise from the Poisson model and everything else from a random, CFA-aligned crop of a real dark frame, with a uniform dither that restores
the bits quantisation took (the SFRN recipe of Zhang et al., "Rethinking Noise Synthesis and Modeling in Raw Denoising", ICCV 2021).

    pool = DarkPool(sessions, raw_pattern=..., black_level=..., white_level=..., K=diag['K'])      # or DarkPool.from_manifest(path)
    nm = NoiseModel(model='PDU', dark=pool)            # _sample_params() draws a session; the kernel draws the frame and the crop
    engine.model.set_noise_model(nm)                   # python -m eld_amd.train_frames ... --noise PDU --dark manifest.json does this

The frames live in one flat uint16 device buffer with an EldPoolFrame table (a FramePool: same upload, same defect repair), each session's
frames contiguous; a parameter record names its session as a (first, count) range of that table (EldNoiseParams.reserved), and
eld_noise_forward_dark (csrc/noise.hip) picks frame and offsets from the record's Philox stream -- a function of (seed, sample id) alone.
"""
import ctypes

import numpy as np

from . import _lib as L
from . import calibrate as CAL
from .defects import find_defects
from .framepool import FramePool
from .mosaic import as_u16, check_cfa
from .shading import as_dark_shading


class DarkPool:
    """The dark (bias) frames of a camera, by session, on the device.

    sessions     the manifest's shape: a list of dicts with 'bias' -- (F, Hm, Wm) uint16 [ndarray or CUDA int16/uint16 tensor], or a list of
                 (Hm, Wm) frames whose sizes may differ -- and optionally 'iso'.  Other keys ('flats') are ignored.
    cfa, raw_pattern, black_level   as eld_amd.framepool.FramePool (X-Trans: one black level; raw_pattern is not used).
    white_level  the sensor's white level; saturation = white_level - max(black_level), eld_amd.validate's definition.
    K            one system gain per session (calibrate_camera's diag['K']), or None: NoiseModel then needs none only for direct
                 sampler calls with explicit parameters -- _sample_params() raises without gains.
    defects      a DefectMap or its path: the frames are repaired once, at upload, as FramePool does (a hot pixel would otherwise be stamped
                 into training patches at a moving position).
    shading      a DarkShading (eld_amd.shading) or its path: after the repair, each session's frames are corrected in place at that
                 session's ISO (eld_shading_apply_u16), so the sampler draws temporal noise only.  Every session then needs an 'iso' inside
                 the map's range and every frame the map's shape.  The sampler and its kernels are untouched.
    Bad arguments raise ValueError before any device work."""

    def __init__(self, sessions, cfa='bayer', raw_pattern=None, black_level=None, white_level=16383, K=None, defects=None, device=None, shading=None):
        check_cfa(cfa)
        if not isinstance(sessions, (list, tuple)) or len(sessions) == 0:
            raise ValueError('sessions must be a non-empty list of {"bias": frames[, "iso"]}')
        frames, ranges, isos = [], [], []
        for i, s in enumerate(sessions):
            if not isinstance(s, dict) or 'bias' not in s:
                raise ValueError("session %d has no 'bias'" % i)
            b = s['bias']
            items = [b] if (isinstance(b, np.ndarray) or hasattr(b, 'is_cuda')) else list(b)
            mine = []
            for m in items:
                _, batched = as_u16(m)
                mine.extend(list(m) if batched else [m])
            if not mine:
                raise ValueError('session %d has no bias frames' % i)
            ranges.append((len(frames), len(mine)))
            frames.extend(mine)
            isos.append(s.get('iso'))
        if K is not None:
            K = np.asarray(K, dtype=np.float64).reshape(-1)
            if K.size != len(sessions) or not np.all(np.isfinite(K)) or np.any(K <= 0):
                raise ValueError('K holds one finite gain > 0 per session (%d), got %r' % (len(sessions), K.tolist()))
        tvals = None
        if shading is not None:
            shading = as_dark_shading(shading)
            for i, m in enumerate(frames):
                shading.check_frames(m.shape, cfa, 'frame %d' % i)
            shading.check_pattern(raw_pattern if cfa == 'bayer' else None, 'DarkPool')
            for i, iso in enumerate(isos):
                if iso is None:
                    raise ValueError("session %d has no 'iso': the dark-shading map is subtracted at the session's ISO" % i)
            tvals = [shading.t(iso) for iso in isos]
        pool = FramePool(frames, cfa=cfa, raw_pattern=raw_pattern, black_level=black_level, white_point=white_level, device=device, defects=defects)
        self.pool, self.cfa, self.C = pool, cfa, pool.C
        self.raw_pattern, self.black_level, self.white_level = pool.raw_pattern, pool.black_level, pool.white_point
        self.saturation = float(pool.white_point) - float(max(pool.black_level))
        self.ranges, self.isos, self.K = ranges, isos, K
        self.min_extent = (int(pool.extent[:, 0].min()), int(pool.extent[:, 1].min()))
        self.shading = shading
        if shading is not None and pool.buffer is not None:
            Hm, Wm = shading.shape
            for (first, count), tv in zip(ranges, tvals):
                for f in pool.frames[first:first + count]:       # in place, frame by frame (the frames start 16-byte aligned, not back to back)
                    v = pool.buffer[int(f['offset']):int(f['offset']) + Hm * Wm].view(1, Hm, Wm)
                    shading.apply_device(v, tv, pool.defects, v)

    def __len__(self):
        return len(self.pool)

    @property
    def sessions(self):
        return len(self.ranges)

    @classmethod
    def from_manifest(cls, path, K=None, defects=None, device=None, shading=None):
        """calibrate's manifest -> a DarkPool.  K: None -- calibrate_camera runs here for the session gains (diag['K']); a sequence of
        gains, one per session; or the path of a table eld_amd.calibrate wrote.  A table keeps only the range [Kmin, Kmax] of the gains, not
        the gain of each session, so with a path the calibration runs as well and the gains it finds must lie in the table's range
        (ValueError otherwise: the table belongs to other frames)."""
        sessions, pattern, black, white, cfa = CAL.load_manifest(path, with_cfa=True)
        if defects is None:
            defects = CAL.manifest_defects(path)
        table = None
        if isinstance(K, str):
            table, K = np.load(K, allow_pickle=True).item(), None
        if K is None:
            _, diag = CAL.calibrate_camera(sessions, pattern, black, white, cfa=cfa, defects=defects)
            K = [float(v) for v in diag['K']]
            if defects == 'auto':
                defects = diag.get('defects')
            if table is not None and not (float(table['Kmin']) * (1 - 1e-6) <= min(K) and max(K) <= float(table['Kmax']) * (1 + 1e-6)):
                raise ValueError('the table covers K in [%g, %g]; the manifest calibrates to %r' % (float(table['Kmin']), float(table['Kmax']), K))
        if defects == 'auto':
            defects = find_defects(sessions[0]['bias'], cfa, pattern)[0]
        if cfa == 'xtrans':
            b = np.asarray(black, dtype=np.float64).reshape(-1)
            return cls(sessions, cfa=cfa, black_level=b, white_level=white, K=K, defects=defects, device=device, shading=shading)
        return cls(sessions, cfa=cfa, raw_pattern=pattern, black_level=black, white_level=white, K=K, defects=defects, device=device, shading=shading)

    def check_patch(self, H, W):
        """ValueError when a (H, W) packed patch does not fit the smallest dark frame (the entry's check, stated before upload)."""
        if H > self.min_extent[0] or W > self.min_extent[1]:
            raise ValueError('the %d x %d patch is larger than the smallest dark frame (packed %d x %d)' % ((H, W) + self.min_extent))

    def launch_args(self, table=None):
        """The pool arguments of eld_noise_forward_dark, in order.  table: a device copy of another frame table over the same buffer
        (eld_amd.validate's leave-one-out ranges) with its length, as (tensor, F); default: the pool's own."""
        if self.pool.buffer is None:
            raise RuntimeError('this DarkPool holds no frames on a device (built without a GPU)')
        tab, F = (self.pool._table_dev, len(self.pool)) if table is None else table
        if self.cfa == 'bayer':
            pat, blk = (ctypes.c_int * 4)(*self.raw_pattern), (ctypes.c_float * 4)(*self.black_level)
        else:
            pat, blk = None, (ctypes.c_float * 4)(float(self.black_level[0]), 0.0, 0.0, 0.0)
        return (L.dptr(self.pool.buffer), self.pool.elems, L.dptr(tab), int(F), self.min_extent[0], self.min_extent[1], pat, blk)
