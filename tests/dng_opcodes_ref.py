"""NumPy restatement of the DNG opcode arithmetic (include/eld_amd.h "DNG opcode lists"), in float32 / float64 with one
rounding per operation.  It shares no code with the package: opcodes are plain dicts here, and the list packer below is written from the
layout alone.

    spec = {'id': 9, 'flags': 0, 'top': .., 'left': .., 'bottom': .., 'right': .., 'plane': 0, 'planes': 1, 'row_pitch': 1, 'col_pitch': 1, ...}
        7   'table' uint16            8   'coefficients' float64          9   'spacing_v', 'spacing_h', 'origin_v', 'origin_h', 'gains' (V,H,planes)
        10..13 'values' float32       3   'k' (5), 'cx', 'cy'             4   'constant', 'bayer_phase'       5   'bayer_phase', 'points', 'rects'
        any other id: 'data' bytes
    pack_list(specs) -> bytes         apply_list2(img, specs) -> float32        gain_plane(specs2, specs3, Hm, Wm) -> float32"""
import struct

import numpy as np

F = np.float32
AREA = ('top', 'left', 'bottom', 'right', 'plane', 'planes', 'row_pitch', 'col_pitch')


def gm(top, left, bottom, right, gains, row_pitch=1, col_pitch=1, spacing=(1.0, 1.0), origin=(0.0, 0.0), plane=0, flags=0):
    g = np.asarray(gains, np.float32)
    if g.ndim == 2:
        g = g[:, :, None]
    return {'id': 9, 'flags': flags, 'top': top, 'left': left, 'bottom': bottom, 'right': right, 'plane': plane, 'planes': 1, 'row_pitch': row_pitch,
            'col_pitch': col_pitch, 'spacing_v': float(spacing[0]), 'spacing_h': float(spacing[1]), 'origin_v': float(origin[0]),
            'origin_h': float(origin[1]), 'gains': g}


def area_op(id_, top, left, bottom, right, row_pitch=1, col_pitch=1, plane=0, flags=0, **kw):
    d = {'id': id_, 'flags': flags, 'top': top, 'left': left, 'bottom': bottom, 'right': right, 'plane': plane, 'planes': 1, 'row_pitch': row_pitch,
         'col_pitch': col_pitch}
    d.update(kw)
    return d


def count_of(top, bottom, pitch):
    return -(-(bottom - top) // pitch)


def params(s):
    i = s['id']
    if i == 3:
        return struct.pack('>7d', *(list(s['k']) + [s['cx'], s['cy']]))
    if i == 4:
        return struct.pack('>II', s['constant'], s['bayer_phase'])
    if i == 5:
        pts, rects = np.asarray(s['points'], np.int64).reshape(-1, 2), np.asarray(s['rects'], np.int64).reshape(-1, 4)
        return (struct.pack('>III', s['bayer_phase'], len(pts), len(rects)) + b''.join(struct.pack('>II', *p) for p in pts.tolist()) +
                b''.join(struct.pack('>IIII', *r) for r in rects.tolist()))
    if i not in range(7, 14):
        return bytes(s.get('data', b''))
    head = struct.pack('>8I', *(s[k] for k in AREA))
    if i == 7:
        t = [int(v) for v in s['table']]
        return head + struct.pack('>I', len(t)) + struct.pack('>%dH' % len(t), *t)
    if i == 8:
        c = [float(v) for v in s['coefficients']]
        return head + struct.pack('>I', len(c) - 1) + struct.pack('>%dd' % len(c), *c)
    if i == 9:
        g = np.asarray(s['gains'], np.float32)
        return (head + struct.pack('>II', g.shape[0], g.shape[1]) + struct.pack('>4d', s['spacing_v'], s['spacing_h'], s['origin_v'], s['origin_h']) +
                struct.pack('>I', g.shape[2]) + struct.pack('>%df' % g.size, *g.reshape(-1).tolist()))
    v = [float(x) for x in s['values']]
    return head + struct.pack('>I', len(v)) + struct.pack('>%df' % len(v), *v)


def pack_list(specs, version=0x01030000):
    out = struct.pack('>I', len(specs))
    for s in specs:
        p = params(s)
        out += struct.pack('>4I', s['id'], s.get('version', version), s.get('flags', 0), len(p)) + p
    return out


def addressed(s, Hm, Wm):
    """-> (rows bool (Hm,), cols bool (Wm,))"""
    y, x = np.arange(Hm), np.arange(Wm)
    if s['plane'] >= 1:
        return np.zeros(Hm, bool), np.zeros(Wm, bool)
    ry = (y >= s['top']) & (y < s['bottom']) & ((y - s['top']) % s['row_pitch'] == 0)
    cx = (x >= s['left']) & (x < s['right']) & ((x - s['left']) % s['col_pitch'] == 0)
    return ry, cx


def map_axis(n, extent, points, origin, spacing):
    """-> (i0 int64, i1 int64, w float32) of the pixels 0..n-1 of an axis of `extent` pixels"""
    c = np.arange(n, dtype=np.float64)
    if points == 1 or spacing == 0:
        v = np.zeros(n, np.float64)
    else:
        with np.errstate(all='ignore'):
            v = ((c + 0.5) / np.float64(extent) - np.float64(origin)) / np.float64(spacing)
    v = np.where(v >= 0, v, 0.0)                                     # NaN too
    v = np.minimum(v, np.float64(points - 1))
    i0 = np.floor(v)
    w = (v - i0).astype(np.float32)
    i0 = i0.astype(np.int64)
    return i0, np.minimum(i0 + 1, points - 1), w


def map_gain(s, Hm, Wm, rows=None):
    """the GainMap's bilinear gain at every site, float32 with every operation rounded: (Hm,Wm); rows: a slice of the rows alone"""
    g = np.asarray(s['gains'], np.float32)[:, :, 0]
    i0, i1, wy = map_axis(Hm, Hm, g.shape[0], s['origin_v'], s['spacing_v'])
    if rows is not None:
        i0, i1, wy = i0[rows], i1[rows], wy[rows]
    j0, j1, wx = map_axis(Wm, Wm, g.shape[1], s['origin_h'], s['spacing_h'])
    wx, wy = wx[None, :], wy[:, None]
    ux, uy = F(1) - wx, F(1) - wy
    with np.errstate(all='ignore'):
        a = g[i0][:, j0] * ux + g[i0][:, j1] * wx
        b = g[i1][:, j0] * ux + g[i1][:, j1] * wx
        out = a * uy + b * wy
    assert out.dtype == np.float32
    return out


def clip01(v):
    return np.where(v < 0, F(0), np.where(v > 1, F(1), v)).astype(np.float32)       # NaN stays


def vignette(s, Hm, Wm):
    mx, my = np.float64(s['cx']) * np.float64(Wm), np.float64(s['cy']) * np.float64(Hm)
    R2 = max((mx - X) * (mx - X) + (my - Y) * (my - Y) for X in (0.0, float(Wm)) for Y in (0.0, float(Hm)))
    dx = (np.arange(Wm, dtype=np.float64) + 0.5) - mx
    dy = (np.arange(Hm, dtype=np.float64) + 0.5) - my
    r2 = (dx[None, :] * dx[None, :] + dy[:, None] * dy[:, None]) / R2
    k = [np.float64(v) for v in s['k']]
    return (1.0 + r2 * (k[0] + r2 * (k[1] + r2 * (k[2] + r2 * (k[3] + r2 * k[4]))))).astype(np.float32)


def vector_plane(s, Hm, Wm):
    """the per-row / per-column entry at every site (0 where the opcode does not address)"""
    vals = np.asarray(s['values'], np.float32)
    rows = s['id'] in (10, 12)
    n, lo, pitch = (Hm, s['top'], s['row_pitch']) if rows else (Wm, s['left'], s['col_pitch'])
    if len(vals) == 0:                                               # an empty area: nothing is addressed
        return np.zeros((Hm, Wm), np.float32)
    k = np.clip((np.arange(n) - lo) // pitch, 0, len(vals) - 1)
    line = vals[k]
    return np.broadcast_to(line[:, None] if rows else line[None, :], (Hm, Wm))


def apply_one(s, v):
    """one list-2 opcode on a float32 image"""
    Hm, Wm = v.shape
    ry, cx = addressed(s, Hm, Wm)
    sel = ry[:, None] & cx[None, :] & ~np.isnan(v)
    i = s['id']
    with np.errstate(all='ignore'):
        if i == 9:
            new = clip01(v * map_gain(s, Hm, Wm))
        elif i in (12, 13):
            new = clip01(v * vector_plane(s, Hm, Wm))
        elif i in (10, 11):
            new = clip01(v + vector_plane(s, Hm, Wm))
        elif i == 8:
            c = np.asarray(s['coefficients'], np.float64).astype(np.float32)
            acc = np.full(v.shape, c[-1], np.float32)
            for k in range(len(c) - 2, -1, -1):
                acc = (acc * v).astype(np.float32) + c[k]
            new = clip01(acc)
        elif i == 7:
            tab = np.asarray(s['table'], np.uint16)
            t = np.rint(v * F(65535))
            t = np.where(t >= 0, t, F(0))
            t = np.minimum(t, F(65535))
            idx = np.minimum(np.where(np.isnan(v), 0, t).astype(np.int64), len(tab) - 1)
            new = tab[idx].astype(np.float32) / F(65535)
        else:
            raise ValueError('apply_list2 takes the opcodes 7..13, got %d' % i)
    assert new.dtype == np.float32
    return np.where(sel, new, v)


def apply_list2(img, specs):
    v = np.asarray(img, np.float32)
    if v.ndim == 3:
        return np.stack([apply_list2(f, specs) for f in v])
    for s in specs:
        v = apply_one(s, v)
    return v


def gain_plane(specs2, specs3, Hm, Wm, rows=None):
    """rows: a slice; the plane of those rows alone (a 24 MP frame's band for the timing tool)"""
    rows = slice(None) if rows is None else rows
    g = np.ones((len(range(Hm)[rows]), Wm), np.float32)
    for s in list(specs2):
        if s['id'] not in (9, 12, 13):
            continue
        ry, cx = addressed(s, Hm, Wm)
        ry = ry[rows]
        f = map_gain(s, Hm, Wm, rows) if s['id'] == 9 else vector_plane(s, Hm, Wm)[rows]
        with np.errstate(all='ignore'):
            g = np.where(ry[:, None] & cx[None, :], g * f, g)
    for s in list(specs3):
        if s['id'] == 3:
            with np.errstate(all='ignore'):
                g = g * vignette(s, Hm, Wm)[rows]
    assert g.dtype == np.float32
    return g


def list1_sites(specs1, codes, active_area):
    """the sites of the visible mosaic that list 1 flags: (K,2) int64, row-major order"""
    top, left, bottom, right = active_area
    Hm, Wm = bottom - top, right - left
    mask = np.zeros((Hm, Wm), bool)
    for s in specs1:
        if s['id'] == 4:
            mask |= np.asarray(codes) == s['constant']
        elif s['id'] == 5:
            for r, c in np.asarray(s['points'], np.int64).reshape(-1, 2).tolist():
                if top <= r < bottom and left <= c < right:
                    mask[r - top, c - left] = True
            for t, l, b, r in np.asarray(s['rects'], np.int64).reshape(-1, 4).tolist():
                for y in range(max(t, top), min(b, bottom)):
                    for x in range(max(l, left), min(r, right)):
                        mask[y - top, x - left] = True
    return np.argwhere(mask)
