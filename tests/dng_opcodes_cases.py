"""Opcode programs for the CPU and GPU tests of eld_amd.dng_opcodes, as the plain dicts of tests/dng_opcodes_ref.py, and the one bridge from
those dicts to the package's Opcode objects (plain module: no fixture)."""
import numpy as np

import dng_opcodes_ref as R


def to_opcode(s):
    """a spec dict of dng_opcodes_ref -> eld_amd.dng_opcodes.Opcode"""
    from eld_amd import dng_opcodes as O
    i = s['id']
    if i == 3:
        f = {'k': tuple(float(v) for v in s['k']), 'cx': float(s['cx']), 'cy': float(s['cy'])}
    elif i == 4:
        f = {'constant': s['constant'], 'bayer_phase': s['bayer_phase']}
    elif i == 5:
        f = {'bayer_phase': s['bayer_phase'], 'points': np.asarray(s['points'], np.int64).reshape(-1, 2),
             'rects': np.asarray(s['rects'], np.int64).reshape(-1, 4)}
    elif i in range(7, 14):
        f = O.area(s['top'], s['left'], s['bottom'], s['right'], s['row_pitch'], s['col_pitch'], s['plane'], s['planes'])
        if i == 7:
            f['table'] = np.asarray(s['table'], np.uint16)
        elif i == 8:
            f['coefficients'] = np.asarray(s['coefficients'], np.float64)
        elif i == 9:
            f.update({k: s[k] for k in ('spacing_v', 'spacing_h', 'origin_v', 'origin_h')})
            f['gains'] = np.asarray(s['gains'], np.float32)
        else:
            f['values'] = np.asarray(s['values'], np.float32)
    else:
        return O.Opcode(i, None, s.get('data', b''), s.get('flags', 0))
    return O.Opcode(i, f, b'', s.get('flags', 0))


def to_opcodes(specs):
    return [to_opcode(s) for s in specs]


def phone_program(Hm, Wm, seed=0, points=(13, 17)):
    """the phone layout: four GainMaps, pitch 2, offsets (0,0) (0,1) (1,0) (1,1); corner gains several-fold, different per position"""
    rng = np.random.default_rng(seed)
    V, H = points
    yy, xx = np.mgrid[0:V, 0:H]
    r2 = ((yy - (V - 1) / 2.0) / max((V - 1) / 2.0, 1)) ** 2 + ((xx - (H - 1) / 2.0) / max((H - 1) / 2.0, 1)) ** 2
    out = []
    for k, (oy, ox) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        g = 1.0 + (0.9 + 0.3 * k) * r2 + rng.uniform(0, 0.02, (V, H))
        out.append(R.gm(oy, ox, Hm, Wm, g.astype(np.float32), 2, 2, spacing=(1.0 / max(V - 1, 1), 1.0 / max(H - 1, 1)), origin=(0.0, 0.0)))
    return out


def each_alone(Hm, Wm, seed=1):
    """{name: [spec]}: each of the opcodes 7..13 alone, on areas with offsets and pitches, values that reach both clips"""
    rng = np.random.default_rng(seed)
    t, l, b, r = 1, 2, Hm - 1, Wm - 1
    table = np.clip(np.sqrt(np.arange(4096) / 4095.0) * 65535.0, 0, 65535).astype(np.uint16)   # shorter than 65536: the last entry serves the rest
    nr, nc = R.count_of(t, b, 2), R.count_of(l, r, 3)
    return {
        'MapTable': [R.area_op(7, t, l, b, r, 1, 2, table=table)],
        'MapPolynomial': [R.area_op(8, 0, 0, Hm, Wm, 2, 1, coefficients=[-0.05, 0.7, 1.9, -1.3])],
        'GainMap': [R.gm(t, l, b, r, rng.uniform(0.5, 3.0, (5, 7)).astype(np.float32), 1, 1, spacing=(0.25, 1.0 / 6), origin=(0.05, -0.1))],
        'DeltaPerRow': [R.area_op(10, t, l, b, r, 2, 1, values=rng.uniform(-0.6, 0.6, nr).astype(np.float32))],
        'DeltaPerColumn': [R.area_op(11, t, l, b, r, 1, 3, values=rng.uniform(-0.6, 0.6, nc).astype(np.float32))],
        'ScalePerRow': [R.area_op(12, t, l, b, r, 2, 1, values=rng.uniform(0.2, 2.5, nr).astype(np.float32))],
        'ScalePerColumn': [R.area_op(13, t, l, b, r, 1, 3, values=rng.uniform(0.2, 2.5, nc).astype(np.float32))],
    }


def small_maps(Hm, Wm):
    """maps of 1 x 1, 1 x 5 and 2 x 2"""
    return [R.gm(0, 0, Hm, Wm, [[1.5]], spacing=(0.0, 0.0)),
            R.gm(0, 1, Hm, Wm, [[0.6, 0.8, 1.0, 1.3, 1.7]], 1, 2, spacing=(1.0, 0.25), origin=(0.0, 0.0)),
            R.gm(1, 0, Hm, Wm, [[1.0, 2.0], [3.0, 4.0]], 2, 1, spacing=(1.0, 1.0), origin=(0.0, 0.0))]


def odd_areas(Hm, Wm):
    """an area partly outside the image, an empty one, one on another plane and one wholly outside"""
    return [R.area_op(12, Hm // 2, 0, Hm + 40, Wm + 9, 1, 1, values=np.linspace(0.5, 1.5, 40 + Hm - Hm // 2).astype(np.float32)),
            R.area_op(10, 3, 3, 3, 9, 1, 1, values=np.zeros(0, np.float32)),
            R.area_op(13, 0, 0, Hm, Wm, 1, 1, plane=1, values=np.full(Wm, 9.0, np.float32)),
            R.area_op(11, Hm + 5, Wm + 5, Hm + 9, Wm + 8, 1, 1, values=np.full(3, 0.5, np.float32)),
            R.gm(0, Wm // 3, Hm + 7, Wm + 100, [[2.0, 0.5], [0.25, 1.0]], 3, 2, spacing=(1.0, 1.0))]


def chain32(Hm, Wm, seed=2):
    """32 operations of all seven types"""
    rng = np.random.default_rng(seed)
    one = each_alone(Hm, Wm, seed)
    names = list(one)
    out = []
    for k in range(32):
        s = dict(one[names[k % 7]][0])
        if s['id'] == 9:
            s['gains'] = rng.uniform(0.7, 1.4, (3 + k % 4, 2 + k % 5, 1)).astype(np.float32)
            s['spacing_v'], s['spacing_h'] = 1.0 / (2 + k % 4), 1.0 / max(1 + k % 5, 1)
        elif s['id'] in (10, 11):
            s['values'] = (s['values'] * np.float32(0.3)).astype(np.float32)
        elif s['id'] in (12, 13):
            s['values'] = rng.uniform(0.8, 1.25, len(s['values'])).astype(np.float32)
        out.append(s)
    return out


def big_maps(Hm, Wm, seed=3):
    """two maps of 96 x 128 points (48 KiB each): beyond the LDS the kernels give to maps, so the second (or both) is read from the blob"""
    rng = np.random.default_rng(seed)
    return [R.gm(0, 0, Hm, Wm, rng.uniform(0.5, 2.0, (96, 128)).astype(np.float32), spacing=(1.0 / 95, 1.0 / 127)),
            R.gm(0, 1, Hm, Wm, rng.uniform(0.5, 2.0, (96, 128)).astype(np.float32), 1, 2, spacing=(1.0 / 90, 1.0 / 120), origin=(0.02, 0.03))]


def frame(Hm, Wm, seed=5, N=None):
    """float32 in [0,1] with exact 0 and 1 among the values"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0, 1, ((Hm, Wm) if N is None else (N, Hm, Wm))).astype(np.float32)
    flat = v.reshape(-1)
    flat[::17] = 0.0
    flat[5::23] = 1.0
    return v
