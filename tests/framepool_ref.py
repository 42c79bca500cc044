"""NumPy restatement of the frame pool's contract (eld_amd/framepool.py, csrc/framepool.hip), shared by its CPU and GPU tests: the patch
codes the reference's create_lmdb_train stores -- pack, x ratio, clip, x 65535, astype(uint16) (util/lmdb_data.py:24-98, 201-210) -- in
the reference's dtypes, and its enumeration of patches (centre crop, then Data2Volume's order).

The dtype is the point: the Bayer pack returns float32 and the chain stays float32; the X-Trans pack writes its float32 values into a
float64 array, so ratio, clip and x 65535 run in float64.  `chain` makes the dtype an argument so that a test can show the fixture tells
the two apart."""
import numpy as np

from denoise_ref import pack_bayer, pack_xtrans

F32, F64 = np.float32, np.float64
CHAIN_DTYPE = {'bayer': F32, 'xtrans': F64}


def chain(p, ratio, dtype):
    """Packed float32 values -> uint16 codes, evaluated in `dtype`.  ratio None: the chain without the ratio multiply."""
    x = np.asarray(p, F32).astype(dtype)
    if ratio is not None:
        x = x * dtype(F32(ratio))                         # the record carries the ratio as float32
    x = np.clip(x, dtype(0), dtype(1))
    return (x * dtype(65535)).astype(np.uint16)


def frame_codes(u, cfa, raw_pattern, black, white, ratio=None, dtype=None):
    """One mosaic (Hm, Wm) uint16 -> the codes of its whole packed image (C, h, w)."""
    u = np.asarray(u)[None]
    p = pack_bayer(u, raw_pattern, black, white)[0] if cfa == 'bayer' else pack_xtrans(u, np.reshape(black, -1)[0], white)[0]
    return chain(p, ratio, CHAIN_DTYPE[cfa] if dtype is None else dtype)


def patches(mosaics, cfa, records, ph, pw, raw_pattern=None, black=None, white=16383, dtype=None):
    """records: rows of (frame, y0, x0, ratio) in packed coordinates -> (B, C, ph, pw) uint16."""
    out, cache = [], {}
    for f, y0, x0, ratio in records:
        key = (int(f), None if ratio is None else float(F32(ratio)))
        if key not in cache:
            cache[key] = frame_codes(mosaics[int(f)], cfa, raw_pattern, black, white, ratio, dtype)
        out.append(cache[key][:, int(y0):int(y0) + ph, int(x0):int(x0) + pw])
        assert out[-1].shape[1:] == (ph, pw), 'record outside its frame'
    return np.stack(out)


def packed_extent(Hm, Wm, cfa):
    return (Hm // 2, Wm // 2) if cfa == 'bayer' else (2 * (Hm // 6), 2 * (Wm // 6))


def grid(extents, kh, kw, sh, sw):
    """Rows of (frame, y0, x0): centre crop to a whole number of strides, then rows of patches, left to right."""
    rows = []
    for f, (hp, wp) in enumerate(extents):
        cy, cx = int((hp - kh) / sh) * sh + kh, int((wp - kw) / sw) * sw + kw
        sy, sx = hp // 2 - cy // 2, wp // 2 - cx // 2
        rows += [(f, sy + a * sh, sx + b * sw) for a in range((cy - kh) // sh + 1) for b in range((cx - kw) // sw + 1)]
    return np.array(rows, np.int64).reshape(-1, 3)
