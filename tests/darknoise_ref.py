"""NumPy restatement of the sampler's dark-frame term (flag DARK, model letter 'D'): which crop the kernel chooses and what
it computes from it, in float32 with one rounding per operation.  Test infrastructure only."""
import ctypes

import numpy as np

from oracle import noise_ref as O
from oracle import philox_ref as PR

STREAM_DARK = 8
DARK = 1024
CFA_XTRANS = 512
F32 = np.float32


def packed_extent(Hm, Wm, cfa):
    return (Hm // 2, Wm // 2) if cfa == 'bayer' else (2 * (Hm // 6), 2 * (Wm // 6))


def umulhi(a, b):
    return (int(a) * int(b)) >> 32


def dark_choice(seed, sample_id, first, count, extents, H, W, cfa):
    """-> (frame, y0, x0): w = philox(index 0, sample id, STREAM_DARK); frame = first + umulhi(w.x, count); Bayer offsets uniform over all valid
    ones, X-Trans over the even ones.  extents: the packed (hp, wp) of every frame of the table."""
    w = [int(v) for v in PR.sampler_words(0, sample_id, STREAM_DARK, seed)]
    f = first + umulhi(w[0], count)
    hp, wp = extents[f]
    assert H <= hp and W <= wp
    if cfa == 'xtrans':
        return f, 2 * umulhi(w[1], (hp - H) // 2 + 1), 2 * umulhi(w[2], (wp - W) // 2 + 1)
    return f, umulhi(w[1], hp - H + 1), umulhi(w[2], wp - W + 1)


def dark_codes(mosaic, cfa, raw_pattern, y0, x0, H, W):
    """The uint16 codes of packed elements (c, y0 + h, x0 + w) of one mosaic -> int64 (C, H, W).  Bayer: plane k sits at the 2x2 cell position
    where raw_pattern holds k; X-Trans: the oracle's index map (whole 6x6 cells only)."""
    m = np.asarray(mosaic).astype(np.int64)
    if cfa == 'xtrans':
        Hm, Wm = m.shape
        planes = O.pack_raw_xtrans(m[:Hm // 6 * 6, :Wm // 6 * 6].astype(np.float64))
        return np.asarray(planes)[:, y0:y0 + H, x0:x0 + W].astype(np.int64)
    pat = [int(v) for v in np.asarray(raw_pattern).reshape(-1)]
    out = np.zeros((4, H, W), np.int64)
    for i, k in enumerate(pat):
        r, c = i >> 1, i & 1
        out[k] = m[2 * y0 + r:2 * (y0 + H):2, 2 * x0 + c:2 * (x0 + W):2]
    return out


def plane_black(cfa, black):
    b = np.asarray(black, F32).reshape(-1)
    return np.full(9, b[0], F32) if cfa == 'xtrans' else b[:4].copy()


def dark_arith(y, params, flags, choice, mosaics, raw_pattern, black, variates):
    """The op chain of a DARK model on one image, float32:
        zz = counts * K                     (or y2 / y2 + n_shot * sqrt(max(K * y2, 1e-10)) without SHOT_POISSON)
        zz = zz + (float(code) - black_c)
        zz = zz + (u_q - 0.5) * q_step      with QUANT
        zz = zz * ratio;  zz = zz / S;  clip with CLIP
    y (C,H,W) float32; params: an oracle Params; choice: dark_choice's (frame, y0, x0); mosaics: the pool's frames; variates: the dumped planes
    by name ('counts', 'u_q', 'n_shot'), each of y's shape."""
    cfa = 'xtrans' if flags & CFA_XTRANS else 'bayer'
    y = np.asarray(y, F32)
    C, H, W = y.shape
    f, y0, x0 = choice
    S, r, K = F32(params['saturation']), F32(params['ratio']), F32(params['K'])
    y2 = ((y * S).astype(F32) / r).astype(F32)
    if flags & O.SHOT_POISSON:
        z = (np.asarray(variates['counts']).astype(F32) * K).astype(F32)
    elif flags & O.SHOT_GAUSS:
        sd = np.sqrt(np.maximum((K * y2).astype(F32), F32(1e-10))).astype(F32)
        z = (y2 + (np.asarray(variates['n_shot'], F32) * sd).astype(F32)).astype(F32)
    else:
        z = y2
    code = dark_codes(mosaics[f], cfa, raw_pattern, y0, x0, H, W).astype(F32)
    d = (code - plane_black(cfa, black).reshape(C, 1, 1)).astype(F32)
    z = (z + d).astype(F32)
    if flags & O.QUANT:
        z = (z + ((np.asarray(variates['u_q'], F32) - F32(0.5)).astype(F32) * F32(params['q_step'])).astype(F32)).astype(F32)
    z = (z * r).astype(F32)
    z = (z / S).astype(F32)
    if flags & O.CLIP:
        z = np.maximum(np.minimum(z, F32(1.0)), F32(0.0)).astype(F32)
    return z


# ---- the shapes the CPU and the GPU tests share ------------------------------------------------------------------------------------------
SEED = 2018
BAYER_SHAPES = ((20, 28), (24, 40), (22, 30))
BAYER_OFFSETS = (0, 562, 1528)                   # the middle frame starts at an even offset that is not a multiple of 8
BAYER_PATCHES = ((4, 5, 7), (4, 8, 12), (4, 10, 14))
XTRANS_SHAPES = ((18, 24), (24, 36), (20, 26))   # the last has sides that are not multiples of 6
XTRANS_OFFSETS = (0, 434, 1304)
XTRANS_PATCHES = ((9, 4, 6), (9, 6, 8))
PATTERNS = ([0, 1, 3, 2], [2, 3, 1, 0])
BLACK = (512.0, 520.0, 500.0, 531.0)


def mosaics_of(shapes):
    """Codes f(frame, row, col), all distinct over the pool: a running index from 300."""
    out, base = [], 300
    for Hm, Wm in shapes:
        out.append((base + np.arange(Hm * Wm)).reshape(Hm, Wm).astype(np.uint16))
        base += Hm * Wm
    return out


def extents_of(shapes, cfa):
    return [packed_extent(Hm, Wm, cfa) for Hm, Wm in shapes]


def wide(offset, Wm, x0):
    """The 16-byte-load predicate of the Bayer vector path."""
    return (offset + 2 * x0) % 8 == 0 and Wm % 8 == 0


class HandPool:
    """A pool with a hand-made frame table (offsets the DarkPool's own upload would not produce), with the three members the sampler call
    takes from a DarkPool: cfa, check_patch, launch_args."""

    def __init__(self, mosaics, offsets, cfa, raw_pattern, black, device):
        import torch
        from eld_amd import _lib as L
        self.cfa = cfa
        self.mosaics = mosaics
        elems = -(-(offsets[-1] + mosaics[-1].size) // 8) * 8
        buf = np.zeros(elems, np.uint16)
        tab = np.zeros(len(mosaics), L.POOL_FRAME_DTYPE)
        for i, (m, off) in enumerate(zip(mosaics, offsets)):
            buf[off:off + m.size] = m.reshape(-1)
            tab[i] = (off, m.shape[0], m.shape[1])
        self.elems = elems
        self.buffer = torch.from_numpy(buf.view(np.int16)).to(device)
        self.table = torch.from_numpy(tab.view(np.uint8).copy()).to(device)
        self.F = len(mosaics)
        self.raw_pattern, self.black = raw_pattern, black
        ext = np.array(extents_of([m.shape for m in mosaics], cfa))
        self.min_extent = (int(ext[:, 0].min()), int(ext[:, 1].min()))

    def check_patch(self, H, W):
        assert H <= self.min_extent[0] and W <= self.min_extent[1]

    def launch_args(self, table=None):
        from eld_amd import _lib as L
        pat = None if self.cfa == 'xtrans' else (ctypes.c_int * 4)(*self.raw_pattern)
        blk = (ctypes.c_float * 4)(*[float(v) for v in self.black])
        return (L.dptr(self.buffer), self.elems, L.dptr(self.table), self.F, self.min_extent[0], self.min_extent[1], pat, blk)
