"""Train from raw frames: a device-resident pool of clean sensor mosaics feeds the sampler.

The reference cuts its training patches on the host and stores them in LMDB patch databases (util/lmdb_data.py::create_lmdb_train, which
needs rawpy and lmdb).  Here the clean frames stay in HBM as the sensor's own uint16 mosaics -- the form eld_amd.calibrate and
eld_amd.denoise take -- and one HIP launch per batch (eld_crop_pack_raw_*_u16, csrc/framepool.hip) cuts B patches at arbitrary packed
positions and emits exactly the uint16 codes the reference would have stored: pack (lmdb_data.py:24-98), x ratio, clip, x 65535,
astype(uint16) (:201-210), bit for bit, in the reference's dtypes (Bayer float32 throughout; X-Trans float64 after the float32 pack).
Everything downstream (sampler, augmentation, U-Net, Adam) runs unchanged on those codes.

    pool = FramePool(mosaics, cfa='bayer', raw_pattern=..., black_level=..., white_point=16383)
    codes = pool.patches(pool.grid((4, 512, 512), (4, 512, 512)))      # the content of the reference's SID_Sony_Raw.db, record for record
    loader = FramePoolLoader(pool, noise_model, batch_size=8, patch=512)
    engine.train(loader)                                               # as with a DataLoader (python -m eld_amd.train_frames does this)

Every rank of a data-parallel run can hold the whole pool (161 Sony frames are 3.9 GB of 288); the pool is not sharded.
"""
import ctypes

import numpy as np

from . import _lib as L
from .defects import as_defect_map, repair_device
from .mosaic import PLANES, as_u16, check_cfa, check_sides, levels

MAX_LAUNCH = 65528          # patches per launch (a patch is a blockIdx.y slice, at most 65535; a multiple of 8 keeps every chunk's output 16-byte aligned)


def packed_extent(Hm, Wm, cfa):
    """Packed sides of an Hm x Wm mosaic: Bayer (Hm//2, Wm//2); X-Trans whole 6x6 cells only, (2*(Hm//6), 2*(Wm//6))."""
    return (Hm // 2, Wm // 2) if cfa == 'bayer' else (2 * (Hm // 6), 2 * (Wm // 6))


class Crops:
    """B crop records (structured, _lib.CROP_RECORD_DTYPE: frame, y0, x0 in packed coordinates, ratio) and their common patch size."""

    def __init__(self, records, ph, pw):
        self.records = np.ascontiguousarray(records, dtype=L.CROP_RECORD_DTYPE).reshape(-1)
        self.ph, self.pw = int(ph), int(pw)

    def __len__(self):
        return len(self.records)

    def __getitem__(self, idx):
        return Crops(self.records[idx], self.ph, self.pw)

    @classmethod
    def make(cls, frames, y0, x0, ph, pw, ratios=1.0):
        frames = np.asarray(frames).reshape(-1)
        rec = np.zeros(frames.size, L.CROP_RECORD_DTYPE)
        rec['frame'], rec['y0'], rec['x0'], rec['ratio'] = frames, np.asarray(y0).reshape(-1), np.asarray(x0).reshape(-1), ratios
        return cls(rec, ph, pw)


class FramePool:
    """F clean mosaics of possibly different sizes in one flat uint16 device buffer.

    mosaics      NumPy uint16 arrays or CUDA uint16 / int16-view tensors, each (Hm, Wm) (a (N, Hm, Wm) stack counts as N frames); uploaded once.
    cfa, raw_pattern, black_level, white_point   as eld_amd.denoise.denoise_raw (same checks, same defaults).
    defects      a DefectMap (eld_amd.defects) or the path of a saved one: every frame is repaired once, at upload (no per-step cost);
                 every frame must then have the map's shape.  Paired mode takes the same map for both pools.
    flatfield    a FlatField (eld_amd.flatfield) or the path of a saved one: after the repair every frame is multiplied by the map's PRNU
                 plane through the integer path (FlatField.apply(part='prnu'), in place, once, at upload): averaging the exposures of a
                 clean target does not remove a fixed pattern.  Every frame must have the map's shape.
    device       the CUDA device of the pool (default: the current one).  Without a GPU the pool keeps its geometry only: grid() and the
                 loader's draws work, patches() does not.
    Bad arguments raise ValueError before any device work; a missing libeld_amd raises LibraryMissing."""

    def __init__(self, mosaics, cfa='bayer', raw_pattern=None, black_level=None, white_point=16383, device=None, defects=None, flatfield=None):
        check_cfa(cfa)
        if isinstance(mosaics, np.ndarray) or hasattr(mosaics, 'is_cuda'):
            mosaics = [mosaics]
        frames = []
        for m in mosaics:
            _, batched = as_u16(m)
            frames.extend(list(m) if batched else [m])
        if not frames:
            raise ValueError('FramePool needs at least one mosaic')
        for m in frames:
            check_sides(int(m.shape[0]), int(m.shape[1]), cfa)
        if defects is not None:
            defects = as_defect_map(defects)
            for i, m in enumerate(frames):
                defects.check_frames(m.shape, cfa, 'frame %d' % i)
        self.defects = defects
        self.cfa, self.C = cfa, PLANES[cfa]
        self.raw_pattern, self.black_level, self.white_point = levels(cfa, raw_pattern, black_level, white_point)
        if flatfield is not None:
            from .flatfield import as_flat_field
            flatfield = as_flat_field(flatfield)
            for i, m in enumerate(frames):
                flatfield.check_frames(m.shape, cfa, 'frame %d' % i)
            flatfield.check_pattern(None if cfa == 'xtrans' else np.asarray(self.raw_pattern).reshape(2, 2), 'FramePool')
        self.flatfield = flatfield
        table = np.zeros(len(frames), L.POOL_FRAME_DTYPE)
        off = 0
        for i, m in enumerate(frames):
            table[i] = (off, m.shape[0], m.shape[1])
            off += -(-int(m.shape[0]) * int(m.shape[1]) // 8) * 8          # every frame starts on a 16-byte boundary
        self.frames, self.elems = table, off
        self.extent = np.array([packed_extent(int(f['Hm']), int(f['Wm']), cfa) for f in table], np.int64).reshape(-1, 2)
        L.lib()                                                              # LibraryMissing here: there is no fallback
        self.buffer = self._table_dev = self.device = None
        import torch
        if device is not None or torch.cuda.is_available():
            self._upload(frames, device)

    def __len__(self):
        return len(self.frames)

    def _upload(self, frames, device):
        import torch
        dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != 'cuda':
            raise ValueError('a FramePool lives on a CUDA device, got %s' % dev)
        buf = torch.zeros(self.elems, dtype=torch.int16, device=dev)
        for f, m in zip(self.frames, frames):
            n = int(f['Hm']) * int(f['Wm'])
            src = torch.from_numpy(np.ascontiguousarray(m).view(np.int16)) if isinstance(m, np.ndarray) else m.contiguous().view(torch.int16)
            buf[int(f['offset']):int(f['offset']) + n].copy_(src.reshape(-1))
        if self.defects is not None and self.defects.count:
            for f in self.frames:                             # in place, frame by frame (the frames start 16-byte aligned, not back to back)
                v = buf[int(f['offset']):int(f['offset']) + int(f['Hm']) * int(f['Wm'])].view(1, int(f['Hm']), int(f['Wm']))
                repair_device(v, self.defects, v)
        if self.flatfield is not None:
            for f in self.frames:
                v = buf[int(f['offset']):int(f['offset']) + int(f['Hm']) * int(f['Wm'])].view(1, int(f['Hm']), int(f['Wm']))
                self.flatfield.apply(v, part='prnu', black_level=self.black_level, defects=self.defects, out=v)
        self.buffer, self.device = buf, dev
        self._table_dev = torch.from_numpy(self.frames.view(np.uint8).copy()).to(dev)

    # ---- the reference's enumeration ------------------------------------------------------------------------------------------------
    def grid(self, ksize, stride):
        """The crop records of create_lmdb_train's enumeration (lmdb_data.py:142-153): per frame, centre crop of the packed image to a
        whole number of strides (crop_center, :17-21, 147-150), then Data2Volume's patch order (:108-127: rows of patches, left to right).
        ksize, stride: (C, kh, kw) and (C, sh, sw) as the reference takes them.  Ratio 1 in every record."""
        ksize, stride = tuple(int(v) for v in ksize), tuple(int(v) for v in stride)
        if len(ksize) != 3 or len(stride) != 3 or ksize[0] != self.C or stride[0] != self.C:
            raise ValueError('ksize and stride are (C, h, w) with C = %d planes, got %r and %r' % (self.C, ksize, stride))
        (_, kh, kw), (_, sh, sw) = ksize, stride
        if min(kh, kw, sh, sw) < 1:
            raise ValueError('patch sides and strides must be positive, got %r and %r' % (ksize, stride))
        fr, ys, xs = [], [], []
        for f, (hp, wp) in enumerate(self.extent):
            hp, wp = int(hp), int(wp)
            if kh > hp or kw > wp:
                raise ValueError('frame %d packs to %d x %d, smaller than the %d x %d patch' % (f, hp, wp, kh, kw))
            cropy, cropx = (hp - kh) // sh * sh + kh, (wp - kw) // sw * sw + kw
            sy, sx = hp // 2 - cropy // 2, wp // 2 - cropx // 2
            for y in range(sy, sy + cropy - kh + 1, sh):
                for x in range(sx, sx + cropx - kw + 1, sw):
                    fr.append(f), ys.append(y), xs.append(x)
        return Crops.make(fr, ys, xs, kh, kw)

    # ---- records -> codes --------------------------------------------------------------------------------------------------------------
    def check(self, records, ratios=None, patch=None):
        """-> Crops with the ratios filled in, every record checked against its frame (ValueError otherwise).  Host only."""
        if isinstance(records, Crops):
            crops = Crops(records.records.copy(), records.ph, records.pw)
        else:
            if patch is None:
                raise ValueError('records without a patch size: pass a Crops (grid() returns one) or patch=(ph, pw)')
            ph, pw = (patch, patch) if np.isscalar(patch) else patch
            a = np.asarray(records)
            if a.dtype == L.CROP_RECORD_DTYPE:
                crops = Crops(a.copy(), ph, pw)
            else:
                a = np.atleast_2d(a)
                if a.ndim != 2 or a.shape[1] != 3 or a.dtype.kind not in 'iu':
                    raise ValueError('records are rows of integer (frame, y0, x0), got an array of shape %s' % (np.shape(records),))
                crops = Crops.make(a[:, 0], a[:, 1], a[:, 2], ph, pw)
        rec, ph, pw = crops.records, crops.ph, crops.pw
        if len(rec) == 0:
            raise ValueError('no crop records')
        if ph < 1 or pw < 1:
            raise ValueError('patch sides must be positive, got %d x %d' % (ph, pw))
        if ratios is not None:
            r = np.asarray(ratios, dtype=np.float64).reshape(-1)
            if r.size not in (1, len(rec)):
                raise ValueError('ratios takes one value or one per record (%d), got %d' % (len(rec), r.size))
            rec['ratio'] = r
        if not np.all(np.isfinite(rec['ratio'])) or np.any(rec['ratio'] <= 0):
            raise ValueError('ratios must be finite and > 0')
        f = rec['frame'].astype(np.int64)
        if np.any(f < 0) or np.any(f >= len(self.frames)):
            raise ValueError('frame index outside [0, %d)' % len(self.frames))
        hp, wp = self.extent[f, 0], self.extent[f, 1]
        y0, x0 = rec['y0'].astype(np.int64), rec['x0'].astype(np.int64)
        bad = (y0 < 0) | (x0 < 0) | (y0 + ph > hp) | (x0 + pw > wp)
        if np.any(bad):
            i = int(np.flatnonzero(bad)[0])
            raise ValueError('record %d: the %d x %d patch at (%d, %d) does not lie inside frame %d (packed %d x %d)'
                             % (i, ph, pw, y0[i], x0[i], f[i], hp[i], wp[i]))
        return crops

    def wide_loads(self, crops):
        """Per record: True where the kernel reads that patch with 16-byte loads (pw % 8 == 0, the row pitch a multiple of 8 codes and the
        patch's first code on a 16-byte boundary), False where it takes the 4-byte path -- the predicate of csrc/framepool.hip."""
        rec = crops.records
        f = rec['frame'].astype(np.int64)
        cell = 2 if self.cfa == 'bayer' else 3
        start = self.frames['offset'][f].astype(np.int64) + cell * rec['x0'].astype(np.int64)
        return (crops.pw % 8 == 0) & (start % 8 == 0) & (self.frames['Wm'][f] % 8 == 0)

    def patches(self, records, ratios=None, patch=None):
        """(B, C, ph, pw) uint16 codes on the device, as the int16 view eld_amd.noise.is_u16_codes recognises.  records: a Crops (grid(),
        Crops.make) or rows of (frame, y0, x0) with patch=(ph, pw); ratios: None (the records' own, 1 from grid()), one value or one per
        record.  Every record is checked on the host before upload."""
        crops = self.check(records, ratios, patch)
        if self.buffer is None:
            raise RuntimeError('this FramePool holds no frames on a device (built without a GPU): patches() needs one')
        import torch
        from .noise import _upload
        B, ph, pw = len(crops), crops.ph, crops.pw
        with torch.cuda.device(self.device):
            out = torch.empty((B, self.C, ph, pw), dtype=torch.int16, device=self.device)
            max_h, max_w = int(self.extent[:, 0].max()), int(self.extent[:, 1].max())
            for a in range(0, B, MAX_LAUNCH):
                rec = crops.records[a:a + MAX_LAUNCH]
                dev_rec = _upload(rec.view(np.uint8), self.device)
                head = (L.dptr(self.buffer), self.elems, L.dptr(self._table_dev), len(self.frames), max_h, max_w, L.dptr(dev_rec), len(rec), ph, pw)
                if self.cfa == 'bayer':
                    pat, blk = (ctypes.c_int * 4)(*self.raw_pattern), (ctypes.c_float * 4)(*self.black_level)
                    L.check(L.lib().eld_crop_pack_raw_bayer_u16(*head, pat, blk, float(self.white_point), L.dptr(out[a:]), L.cur_stream()),
                            'eld_crop_pack_raw_bayer_u16')
                else:
                    L.check(L.lib().eld_crop_pack_raw_xtrans_u16(*head, float(self.black_level[0]), float(self.white_point), L.dptr(out[a:]),
                                                                 L.cur_stream()), 'eld_crop_pack_raw_xtrans_u16')
        return out


class FramePoolLoader:
    """What Engine.train takes in place of a DataLoader: an iterable with __len__ that yields the dicts ELDModel.set_input takes,
        {'target': codes on the device, 'params': (B, 64) records, 'aug': (B,), 'burst': (B,)}
    with the patches cut from `pool` at random positions.  The host draws come from np.random (np.random.seed reproduces a run), per
    sample in this order:
        1. frame index            np.random.randint(F)
        2. y0                     np.random.randint(number of valid offsets)      uniform over all valid packed offsets; X-Trans: over the
        3. x0                     np.random.randint(number of valid offsets)      even ones, so a patch starts on a 6x6 cell
        4. noise parameters       noise_maker._sample_params(), once per sample (= once per burst)
        5. augmentation bits      np.random.randint(2, size=1)[0] three times (flip H, flip W, transpose), as ELDTrainDataset; none when
                                  augment is False
    X-Trans needs even patch sides (the sampler's row map and plane colours assume patches that start on a cell); augmentation needs a
    square patch (the transpose).
    Paired mode (inputs=a second pool of short exposures with the same frame geometry, ratios=one exposure ratio per frame): the same
    record cuts both pools, no noise model is needed and no parameters are drawn; the batch is {'input': float32 clip(codes / 65535) of
    the ratio-scaled short frame (decode_augment_u16), 'target': codes, 'aug': (B,)} and the model augments both alike."""

    def __init__(self, pool, noise_maker, batch_size, patch=512, steps_per_epoch=None, augment=True, num_burst=1, inputs=None, ratios=None):
        ph, pw = (int(patch), int(patch)) if np.isscalar(patch) else (int(patch[0]), int(patch[1]))
        if not isinstance(pool, FramePool):
            raise ValueError('pool must be a FramePool, got %r' % (type(pool).__name__,))
        if int(batch_size) < 1 or int(batch_size) > MAX_LAUNCH:
            raise ValueError('batch_size must be in [1, %d], got %r' % (MAX_LAUNCH, batch_size))
        if ph < 1 or pw < 1:
            raise ValueError('patch sides must be positive, got %d x %d' % (ph, pw))
        if pool.cfa == 'xtrans' and (ph % 2 or pw % 2):
            raise ValueError('an X-Trans patch needs even sides (it starts and ends on a 6x6 cell), got %d x %d' % (ph, pw))
        if augment and ph != pw:
            raise ValueError('augmentation transposes patches: it needs a square patch, got %d x %d' % (ph, pw))
        if np.any(pool.extent[:, 0] < ph) or np.any(pool.extent[:, 1] < pw):
            raise ValueError('a frame of the pool packs to less than the %d x %d patch' % (ph, pw))
        if int(num_burst) < 1:
            raise ValueError('num_burst must be >= 1, got %r' % (num_burst,))
        if inputs is not None:
            if not isinstance(inputs, FramePool) or inputs.cfa != pool.cfa or not np.array_equal(inputs.extent, pool.extent):
                raise ValueError('paired mode: `inputs` must be a FramePool of the same CFA with the same geometry per frame')
            r = np.asarray(ratios if ratios is not None else [], dtype=np.float64).reshape(-1)
            if r.size != len(pool) or not np.all(np.isfinite(r)) or np.any(r <= 0):
                raise ValueError('paired mode: `ratios` holds one finite exposure ratio > 0 per frame (%d)' % len(pool))
            self.ratios = r.astype(np.float32)
        elif ratios is not None:
            raise ValueError('`ratios` belongs to paired mode (inputs=...)')
        elif noise_maker is None or not hasattr(noise_maker, '_sample_params'):
            raise ValueError('noise_maker must be a NoiseModel (its _sample_params is drawn per sample)')
        self.pool, self.inputs, self.noise_maker = pool, inputs, noise_maker
        self.batch_size, self.ph, self.pw, self.augment, self.num_burst = int(batch_size), ph, pw, bool(augment), int(num_burst)
        self.step = 2 if pool.cfa == 'xtrans' else 1
        if steps_per_epoch is None:                          # one epoch = as many patches as tile the frames without overlap
            n = int(np.sum((pool.extent[:, 0] // ph) * (pool.extent[:, 1] // pw)))
            steps_per_epoch = max(1, -(-n // self.batch_size))
        if int(steps_per_epoch) < 1:
            raise ValueError('steps_per_epoch must be >= 1, got %r' % (steps_per_epoch,))
        self.steps_per_epoch = int(steps_per_epoch)

    def __len__(self):
        return self.steps_per_epoch

    def draw(self):
        """The host draws of one batch, in the documented order -> (Crops, list of NoiseParams or None, list of bits).  No device work."""
        from .noise import NoiseParams
        fr, ys, xs, params, bits = [], [], [], [], []
        for _ in range(self.batch_size):
            f = int(np.random.randint(len(self.pool)))
            hp, wp = int(self.pool.extent[f, 0]), int(self.pool.extent[f, 1])
            y = self.step * int(np.random.randint((hp - self.ph) // self.step + 1))
            x = self.step * int(np.random.randint((wp - self.pw) // self.step + 1))
            if self.inputs is None:
                params.append(NoiseParams.coerce(self.noise_maker._sample_params()))
            b = 0
            if self.augment:                                 # sid_dataset.py:344-352: flip H, flip W, transpose
                for bit in (1, 2, 4):
                    if np.random.randint(2, size=1)[0] == 1:
                        b |= bit
            fr.append(f), ys.append(y), xs.append(x), bits.append(b)
        return Crops.make(fr, ys, xs, self.ph, self.pw), (params if self.inputs is None else None), bits

    def batch(self, crops, params, bits):
        """Draws -> the batch dict (device work: one crop launch per pool)."""
        target = self.pool.patches(crops)
        aug = np.asarray(bits, dtype=np.int64)
        if self.inputs is not None:
            from .noise import decode_augment_u16
            codes = self.inputs.patches(crops, ratios=self.ratios[crops.records['frame']])
            return {'input': decode_augment_u16(codes), 'target': target, 'aug': aug}
        recs = np.stack([p.record(0) for p in params]).view(np.uint8).reshape(len(params), 64)
        return {'target': target, 'params': recs, 'aug': aug, 'burst': np.full(len(params), self.num_burst, dtype=np.int64)}

    def __iter__(self):
        for _ in range(self.steps_per_epoch):
            yield self.batch(*self.draw())
