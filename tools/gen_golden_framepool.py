#!/usr/bin/env python3
"""Mint tests/golden/framepool.npz from the reference itself: its util/lmdb_data.py::create_lmdb_train runs on stand-in raw objects and a
stand-in lmdb whose transaction records what the reference would have stored, so every code in the fixture comes out of the reference's
own pack_raw_bayer / pack_raw_xtrans, ratio, clip, x 65535, astype(uint16), crop_center and Data2Volume.  The centre-crop offsets are the
reference's too: crop_center and Data2Volume applied to an image of flat indices.

    python tools/gen_golden_framepool.py --ref <reference checkout>

Needs the reference checkout, so no test runs it; the tests read the .npz (data only)."""
import argparse
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'framepool.npz')
KSIZE = 16
RATIOS = (1, 100, 300)              # ratio 1 is minted as the chain WITHOUT the ratio multiply (ratios=None)


class Raw:
    """What create_lmdb_train reads off rawpy's object."""
    def __init__(self, mosaic, raw_pattern=None, black=None):
        self.raw_image_visible = mosaic
        self.raw_pattern = None if raw_pattern is None else np.asarray(raw_pattern)
        self.black_level_per_channel = black
        self.camera_whitebalance = np.array([2.0, 1.0, 1.5, 1.0])
        self.rgb_camera_matrix = np.eye(3, 4)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


class Txn:
    def __init__(self, store):
        self.store = store

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def put(self, key, data):
        self.store.append(bytes(data))


def install_stand_ins(frames, store):
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class Env:
        def begin(self, write=False):
            return Txn(store)

    def lmdb_open(path, **kw):
        os.makedirs(path)
        return Env()
    mod('rawpy', imread=lambda fn: frames[fn])
    mod('lmdb', open=lmdb_open)
    for _ in range(32):                                      # util/process.py's absent imports
        try:
            import process  # noqa: F401
            break
        except ModuleNotFoundError as e:
            mod(e.name)
        except Exception:
            mod('process')
            break


def mosaic(rng, shape, black):
    """Codes below black, around it, mid-range, at the white point, and dark ones that only saturate under a ratio."""
    kind = rng.integers(0, 8, size=shape)
    u = np.where(kind < 4, black + rng.integers(-40, 200, size=shape),                 # dark: some below black; x 100 / x 300 partly saturates
                 np.where(kind < 7, rng.integers(0, 16384, size=shape), 16383))        # anywhere in range; exactly white
    return np.clip(u, 0, 16383).astype(np.uint16)


def telling_codes(black, white=16383):
    """Sensor codes whose patch code depends on the dtype of the chain (float32 against float64) for one of RATIOS: planted into the
    mosaics so that the fixture pins the dtypes.  Chooses INPUTS only; every stored code still comes out of the reference."""
    def chain(p, ratio, dtype):
        x = p.astype(dtype) if ratio is None else p.astype(dtype) * dtype(ratio)
        return (np.clip(x, dtype(0), dtype(1)) * dtype(65535)).astype(np.uint16)
    u = np.arange(int(black), white + 1)
    p = np.clip((u.astype(np.float32) - np.float32(black)) / (np.float32(white) - np.float32(black)), 0, 1).astype(np.float32)
    differ = np.zeros(u.shape, bool)
    for r in RATIOS:
        differ |= chain(p, None if r == 1 else r, np.float32) != chain(p, None if r == 1 else r, np.float64)
    return u[differ].astype(np.uint16)


def plant(rng, u, cells, blacks):
    """Overwrite about a tenth of the pixels of each channel (cells: its (row, col, step) slices) with that channel's telling codes."""
    for (oy, ox, step), b in zip(cells, blacks):
        sub = u[oy::step, ox::step]
        pick = rng.random(sub.shape) < 0.1
        sub[pick] = rng.choice(telling_codes(b), size=int(pick.sum()))
    return u


def mint(ref_lmdb, frames, store, name, cfa, ratio):
    del store[:]
    C = 4 if cfa == 'bayer' else 9
    with tempfile.TemporaryDirectory() as d:
        ref_lmdb.create_lmdb_train([name], os.path.join(d, 'db'), ksize=(C, KSIZE, KSIZE), stride=(C, KSIZE, KSIZE), cfa=cfa,
                                   ratios=None if ratio == 1 else [ratio])
    return np.stack([np.frombuffer(b, np.uint16).reshape(C, KSIZE, KSIZE) for b in store])


def offsets(ref_lmdb, hp, wp):
    """(y0, x0) of every patch, from the reference's crop_center and Data2Volume on an image of flat packed indices."""
    idx = np.arange(hp * wp, dtype=np.float64).reshape(1, hp, wp)
    cy, cx = int((hp - KSIZE) / KSIZE) * KSIZE + KSIZE, int((wp - KSIZE) / KSIZE) * KSIZE + KSIZE
    vol = ref_lmdb.Data2Volume(ref_lmdb.crop_center(idx, cx, cy), [1, KSIZE, KSIZE], [1, KSIZE, KSIZE])
    first = vol[:, 0, 0, 0].astype(np.int64)
    return np.stack([first // wp, first % wp], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True, help='the reference checkout')
    a = ap.parse_args()
    ref = os.path.abspath(a.ref)
    sys.path.insert(0, os.path.join(ref, 'util'))
    sys.path.insert(0, ref)
    rng = np.random.default_rng(20261016)
    cases = {'bayer_a': ('bayer', (70, 74), [[0, 1], [3, 2]], [512, 520, 500, 516]),
             'bayer_b': ('bayer', (38, 74), [[2, 3], [1, 0]], [256, 250, 260, 254]),
             'xtrans': ('xtrans', (56, 106), None, [1024])}
    frames, store, out = {}, [], {}
    for name, (cfa, shape, pat, blk) in cases.items():
        if cfa == 'bayer':
            where = [tuple(int(v[0]) for v in np.where(np.asarray(pat) == k)) + (2,) for k in range(4)]
            u = plant(rng, mosaic(rng, shape, blk[0]), where, blk)
        else:
            u = plant(rng, mosaic(rng, shape, blk[0]), [(0, 0, 1)], blk)
        frames[name] = Raw(u, pat, blk if cfa == 'bayer' else None)
    install_stand_ins(frames, store)
    import contextlib
    import io
    import lmdb_data as ref_lmdb                             # the reference module itself
    for name, (cfa, shape, pat, blk) in cases.items():
        hp, wp = (shape[0] // 2, shape[1] // 2) if cfa == 'bayer' else (2 * (shape[0] // 6), 2 * (shape[1] // 6))
        out[name + '_mosaic'] = frames[name].raw_image_visible
        out[name + '_black'] = np.array(blk, np.int64)
        if pat is not None:
            out[name + '_pattern'] = np.array(pat, np.int64)
        out[name + '_offsets'] = offsets(ref_lmdb, hp, wp)
        for r in RATIOS:
            with contextlib.redirect_stdout(io.StringIO()):
                out['%s_codes_r%d' % (name, r)] = mint(ref_lmdb, frames, store, name, cfa, r)
            assert len(out['%s_codes_r%d' % (name, r)]) == len(out[name + '_offsets'])
    out['ratios'] = np.array(RATIOS, np.int64)
    out['ksize'] = np.array(KSIZE, np.int64)
    out['white'] = np.array(16383, np.int64)
    np.savez_compressed(OUT, **out)
    print('wrote %s (%d bytes): %s' % (OUT, os.path.getsize(OUT), ', '.join('%s %s' % (k, v.shape) for k, v in out.items())))


if __name__ == '__main__':
    main()
