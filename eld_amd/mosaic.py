"""Mosaic arguments shared by every module that takes raw frames: the CFA and the layout of its cell (CfaLayout), black and white levels,
the shapes and dtypes of uint16 mosaics, their upload, the checks the saved sensor maps share, and the sessions of a calibration manifest.

The leaf of the package: at module level it imports nothing from it (the library's X-Trans cell is read through a lazy `_lib` import), so the
import order that holds is
    mosaic <- defects, structure <- calibrate <- shading, flatfield <- denoise, framepool <- darkpool, validate, evaluate, burst, noiselevel
Every module to the right takes its argument checks from here, none from another module's private helpers; denoise, the command-line front
end, imports the map modules at module level and nothing imports it for argument handling."""
import ctypes
import math

import numpy as np

PLANES = {'bayer': 4, 'xtrans': 9}
DEFAULT_BLACK = {'bayer': 512, 'xtrans': 1024}      # SID Sony (rawpy black_level_per_channel) / the reference's X-Trans constant
DEFAULT_PATTERN = ((0, 1), (3, 2))                   # RGGB as rawpy codes (R 0, G1 1, B 2, G2 3)
XT_PERIOD = 6
CODE_COLOUR = np.array([0, 1, 2, 1])               # rawpy colour code (R, G, B, G2) -> colour class R 0, G 1, B 2


# ---- argument checks (host only: they run before any device work) ---------------------------------------------------------------
def check_cfa(cfa):
    if cfa not in ('bayer', 'xtrans'):
        raise ValueError("cfa must be 'bayer' or 'xtrans', got %r" % (cfa,))
    return cfa


def period_of(cfa):
    return XT_PERIOD if check_cfa(cfa) == 'xtrans' else 2


def bayer_pattern(raw_pattern):
    p = np.asarray(raw_pattern).reshape(-1)
    if p.size != 4 or sorted(int(v) for v in p) != [0, 1, 2, 3] or not np.all(p == np.round(p)):
        raise ValueError('raw_pattern must be a 2x2 permutation of 0..3, got %r' % (np.asarray(raw_pattern).tolist(),))
    return p.astype(np.int64).reshape(2, 2)


def black_levels(black_level):
    b = np.asarray(black_level, dtype=np.float64).reshape(-1)
    if b.size != 4:
        raise ValueError('black_level must hold 4 values (black_level_per_channel), got %d' % b.size)
    return b


def xtrans_pattern(raw_pattern):
    """rawpy's 6x6 X-Trans raw_pattern (0 = R, 2 = B, 1 and 3 = G) with 8 R, 20 G and 8 B -> int64 (6,6)."""
    p = np.asarray(raw_pattern)
    if p.shape != (XT_PERIOD, XT_PERIOD) or not np.all(np.isin(p, [0, 1, 2, 3])):
        raise ValueError('raw_pattern must be a 6x6 array of colour codes 0..3 for X-Trans, got %r' % (p.tolist(),))
    p = p.astype(np.int64)
    n = np.bincount(CODE_COLOUR[p].reshape(-1), minlength=3)
    if tuple(int(v) for v in n) != (8, 20, 8):
        raise ValueError('an X-Trans raw_pattern holds 8 R, 20 G and 8 B, got %d, %d, %d' % tuple(int(v) for v in n))
    return p


def xtrans_tables():
    """The library's X-Trans tables (host call, no device work): {'R': window radius, 'colour' (6,6) R 0 / G 1 / B 2, 'count' (6,6)
    same-colour taps of the (2R + 1)^2 window, 'mask' (6,6) uint64 (bit = raster index of the tap in the window)}."""
    from . import _lib as L
    buf = (ctypes.c_int * 145)()
    L.check(L.lib().eld_debug_xtrans_defect_tables(buf, 145), 'eld_debug_xtrans_defect_tables')
    a = np.array(buf[1:], np.int64).reshape(6, 6, 4)
    mask = (a[..., 2] & 0xffffffff).astype(np.uint64) | ((a[..., 3] & 0xffffffff).astype(np.uint64) << np.uint64(32))
    return {'R': int(buf[0]), 'colour': a[..., 0].copy(), 'count': a[..., 1].copy(), 'mask': mask}


def default_pattern(cfa, raw_pattern=None):
    """raw_pattern, or for None RGGB / the cell the library packs (R 0, G 1, B 2 are valid colour codes)."""
    if raw_pattern is not None:
        return raw_pattern
    return xtrans_tables()['colour'] if cfa == 'xtrans' else DEFAULT_PATTERN


def _black4(cfa, black_level, integers):
    """1 or 4 black levels in [0, 65535] (None: DEFAULT_BLACK) -> float64 (4,), per packed channel (Bayer) / colour code (X-Trans)."""
    b = np.asarray(DEFAULT_BLACK[cfa] if black_level is None else black_level, dtype=np.float64).reshape(-1)
    if b.size not in (1, 4) or not np.all(np.isfinite(b)) or np.any(b < 0) or np.any(b > 65535) or (integers and np.any(b != np.rint(b))):
        raise ValueError('black_level takes 1 or 4 %s in [0, 65535], got %r' % ('integers' if integers else 'values', black_level))
    return np.repeat(b, 4) if b.size == 1 else b


NO_BLACK = object()                                  # CfaLayout(cfa, raw_pattern): a layout that is asked for no black level


def tile_cells(values, Hm, Wm):
    """(p,p) table -> (Hm,Wm): the value of cell (y % p, x % p) at every site."""
    v = np.asarray(values)
    p = v.shape[0]
    return v[np.arange(Hm)[:, None] % p, np.arange(Wm)[None, :] % p]


class CfaLayout:
    """The cell of a CFA and what every kernel wrapper asks of it.  Immutable; built from (cfa, raw_pattern, black_level).

    cfa, period   'bayer' / 'xtrans', 2 / 6
    codes         (p,p) int64 rawpy colour codes (R 0, G 1, B 2, G2 3), the raw_pattern as checked
    colour        (p,p) int64 colour classes R 0, G 1, B 2
    group, G      p*p ints, cell -> colour group: the packed channel = code (Bayer, G = 4) or the colour (X-Trans, G = 3); group_table (p,p)
    black         float64 (4,) per code, or None when built without; black_cells float64 (p,p), black_ints p*p ints, centres (p,p) int64
    tile(values, Hm, Wm), whole_cells(Hm, Wm), c_group(), c_black()

    Three rule sets build one; the accepted inputs of each are those of the callers it serves:
        CfaLayout(cfa, raw_pattern[, black_level])      the given pattern, strictly; exactly 4 black values (black_levels) or none
                                                        calibrate, validate.group_map_u16, structure (cell_centres rounds and clips)
        CfaLayout.for_codes(cfa, raw_pattern=None, black_level=None)
                                                        1 or 4 integers in [0, 65535] (default 512 / 1024), checked first; a missing pattern
                                                        is RGGB / the library's cell -- evaluate, burst, noiselevel
        CfaLayout.for_map(cfa, raw_pattern=None, black_level=None)
                                                        the same pattern default, and an X-Trans pattern must be the cell the library packs;
                                                        then 1 or 4 finite values in [0, 65535] -- defects, shading, flatfield
    validate.group_black (per group, no pattern; equal rounded greens for X-Trans) and levels() below (the network's input stage: one X-Trans
    black level, white > black) keep their own lines."""
    __slots__ = ('cfa', 'period', 'codes', 'colour', 'group', 'G', 'black')

    def __init__(self, cfa, raw_pattern, black_level=NO_BLACK):
        xt = check_cfa(cfa) == 'xtrans'
        codes = xtrans_pattern(raw_pattern) if xt else bayer_pattern(raw_pattern)
        colour = CODE_COLOUR[codes]
        black = None if black_level is NO_BLACK else black_levels(black_level).copy()
        for a in (codes, colour, black):
            if a is not None:
                a.setflags(write=False)
        for k, v in (('cfa', cfa), ('period', codes.shape[0]), ('codes', codes), ('colour', colour), ('black', black), ('G', 3 if xt else 4),
                     ('group', tuple(int(v) for v in (colour if xt else codes).reshape(-1)))):
            object.__setattr__(self, k, v)

    def __setattr__(self, name, value):
        raise AttributeError('a CfaLayout is immutable')

    @classmethod
    def for_codes(cls, cfa, raw_pattern=None, black_level=None):
        black = _black4(check_cfa(cfa), black_level, True)
        return cls(cfa, default_pattern(cfa, raw_pattern), black)

    @classmethod
    def for_map(cls, cfa, raw_pattern=None, black_level=None):
        lay = cls(cfa, default_pattern(check_cfa(cfa), raw_pattern))
        if cfa == 'xtrans' and not np.array_equal(lay.colour, xtrans_tables()['colour']):      # the library's tap lists are compiled for its cell
            raise ValueError('this X-Trans raw_pattern is not the 6x6 cell the library packs (row 0 = R B G B R G): crop the mosaic so that it '
                             'starts on that phase; got %r' % (lay.codes.tolist(),))
        return cls(cfa, lay.codes, _black4(cfa, black_level, False))

    @property
    def group_table(self):
        return np.asarray(self.group, np.int64).reshape(self.period, self.period)

    @property
    def black_cells(self):
        return self.black[self.codes]

    @property
    def black_ints(self):
        return [int(v) for v in self.black_cells.reshape(-1)]

    @property
    def centres(self):
        """rint(black) of every cell, clipped to the code range: the integer centre the structure, shading and flat-field kernels take."""
        return np.clip(np.rint(self.black).astype(np.int64)[self.codes], 0, 65535)

    def tile(self, values, Hm, Wm):
        """p*p values, one per cell -> (Hm,Wm): the value of cell (y % p, x % p) at every site."""
        return tile_cells(np.asarray(values).reshape(self.period, self.period), Hm, Wm)

    def whole_cells(self, Hm, Wm):
        """The sides the sums look at: X-Trans counts whole 6x6 cells only."""
        p = self.period
        return (Hm // p * p, Wm // p * p) if self.cfa == 'xtrans' else (Hm, Wm)

    def c_group(self, group=None):
        return (ctypes.c_int * (self.period * self.period))(*(self.group if group is None else group))

    def c_black(self):
        return (ctypes.c_int32 * (self.period * self.period))(*self.black_ints)


def cell_counts(Hm, Wm, p=XT_PERIOD):
    """(p,p) int64: pixels of an Hm x Wm mosaic in cell (r, c) = {(y, x): y % p == r, x % p == c}."""
    nr = np.array([(Hm - r + p - 1) // p for r in range(p)], np.int64)
    nc = np.array([(Wm - c + p - 1) // p for c in range(p)], np.int64)
    return np.outer(nr, nc)


def shape_of(x):
    return tuple(int(s) for s in x.shape)


def check_mosaics(x, ndim, what, cfa='bayer'):
    """uint16 ndarray or CUDA int16/uint16 tensor of `ndim` dimensions -> its shape.  cfa 'bayer': even, non-zero sides; 'xtrans': an even
    width and both sides >= 6; None (the histogram and structure passes, any period): an even width and fewer than 2^31 sites."""
    s = shape_of(x)
    if len(s) != ndim:
        raise ValueError('%s: expected %s, got shape %s' % (what, '(F, Hm, Wm)' if cfa is None else '%d dimensions' % ndim, s))
    if ndim == 4 and s[1] != 2:
        raise ValueError('%s: flat pairs must have shape (P, 2, Hm, Wm), got %s' % (what, s))
    Hm, Wm = s[-2:]
    if cfa is None:
        if Wm % 2:
            raise ValueError('%s: the mosaic width must be even (rows are read as 32-bit words), got %d' % (what, Wm))
        check_site_count(Hm, Wm, what, 'pixels')
    elif cfa == 'xtrans':
        if Wm % 2 or Hm < XT_PERIOD or Wm < XT_PERIOD:
            raise ValueError('%s: X-Trans mosaics need an even width and both sides >= 6, got %dx%d' % (what, Hm, Wm))
    elif Hm % 2 or Wm % 2 or Hm == 0 or Wm == 0:
        raise ValueError('%s: mosaic sides must be even and non-zero, got %dx%d' % (what, Hm, Wm))
    if isinstance(x, np.ndarray):
        if x.dtype != np.uint16:
            raise ValueError('%s: uint16 mosaics expected, got %s' % (what, x.dtype))
    else:
        import torch
        if not (x.is_cuda and x.dtype in (torch.int16, torch.uint16)):
            raise ValueError('%s: a tensor must be CUDA int16/uint16 codes, got %s on %s' % (what, x.dtype, x.device))
    return s


def as_u16(mosaic):
    """-> (kind, batched).  kind: 'numpy' or 'torch'.  Refuses anything that is not uint16 codes, (Hm, Wm) or (N, Hm, Wm)."""
    if isinstance(mosaic, np.ndarray):
        if mosaic.dtype != np.uint16:
            raise ValueError('mosaic must be a uint16 array, got %s' % mosaic.dtype)
        kind = 'numpy'
    else:
        try:
            import torch
        except ImportError:                                     # pragma: no cover
            torch = None
        if torch is None or not isinstance(mosaic, torch.Tensor):
            raise ValueError('mosaic must be a NumPy uint16 array or a CUDA uint16 / int16 tensor, got %r' % (type(mosaic).__name__,))
        if mosaic.dtype not in (torch.uint16, torch.int16):
            raise ValueError('mosaic must hold uint16 codes (torch.uint16, or its int16 view), got %s' % mosaic.dtype)
        if not mosaic.is_cuda:
            raise ValueError('a mosaic tensor must be on a CUDA device (NumPy arrays are uploaded)')
        kind = 'torch'
    if mosaic.ndim not in (2, 3):
        raise ValueError('mosaic must be (Hm, Wm) or (N, Hm, Wm), got shape %s' % (tuple(mosaic.shape),))
    return kind, mosaic.ndim == 3


def check_sides(Hm, Wm, cfa):
    if Hm % 2 or Wm % 2:
        raise ValueError('mosaic sides must be even, got %d x %d' % (Hm, Wm))
    if cfa == 'xtrans' and (Hm < 6 or Wm < 6):
        raise ValueError('an X-Trans mosaic needs sides of at least 6 (one 6x6 cell), got %d x %d' % (Hm, Wm))
    if Hm < 2 or Wm < 2:
        raise ValueError('empty mosaic: %d x %d' % (Hm, Wm))


def check_site_count(Hm, Wm, what=None, noun='sites'):
    if Hm * Wm >= 1 << 31:
        raise ValueError('%sa frame of %d x %d has 2^31 %s or more' % ('' if what is None else what + ': ', Hm, Wm, noun))


def check_stack(x, what, limit=False):
    """as_u16 under the prefix `what` -> (F, Hm, Wm), F = 1 for one (Hm, Wm) mosaic; limit: also fewer than 2^31 sites (evaluate,
    noiselevel).  burst puts its frame-count rule, check_sides and check_site_count behind it; check_mosaics is the calibration's check."""
    try:
        _, batched = as_u16(x)
    except ValueError as e:
        raise ValueError('%s: %s' % (what, e))
    s = shape_of(x)
    F, Hm, Wm = s if batched else (1,) + s
    if limit:
        check_site_count(Hm, Wm)
    return F, Hm, Wm


def check_white(white, top=65536, name='white_point'):
    """An integer white level in [1, top] -> int.  evaluate, burst and noiselevel allow 65536 (no code is saturated); a flat-field map 65535."""
    w = float(white)
    if not (1 <= w <= top) or w != math.floor(w):
        raise ValueError('%s must be an integer in [1, %d], got %r' % (name, top, white))
    return int(w)


def levels(cfa, raw_pattern, black_level, white_point):
    """The levels of the network's input stage and write-back -> (pattern as 4 ints or None, black levels: 4 floats for Bayer / one for
    X-Trans, white)"""
    white = float(white_point)
    if not (0 < white <= 65535) or white != math.floor(white):
        raise ValueError('white_point must be an integer in (0, 65535], got %r' % (white_point,))
    if black_level is None:
        black_level = DEFAULT_BLACK[cfa]
    blk = np.asarray(black_level, dtype=np.float64).reshape(-1)
    if cfa == 'bayer':
        pat = np.asarray(DEFAULT_PATTERN if raw_pattern is None else raw_pattern).reshape(-1)
        if pat.size != 4 or sorted(int(v) for v in pat) != [0, 1, 2, 3]:
            raise ValueError('raw_pattern must be a 2x2 permutation of the codes 0..3, got %r' % (raw_pattern,))
        pat = [int(v) for v in pat]
        if blk.size == 1:
            blk = np.repeat(blk, 4)
        if blk.size != 4:
            raise ValueError('Bayer black_level takes 1 or 4 values (black_level_per_channel), got %d' % blk.size)
    else:
        pat = None
        if blk.size > 1:
            if not np.all(blk == blk[0]):
                raise ValueError('X-Trans takes one black level for all planes (as the reference), got %r' % (blk.tolist(),))
            blk = blk[:1]
    if np.any(blk < 0) or np.any(blk != np.floor(blk)):
        raise ValueError('black levels must be non-negative integers, got %r' % (blk.tolist(),))
    if np.any(white <= blk):
        raise ValueError('white_point (%g) must exceed every black level %r' % (white, blk.tolist()))
    return pat, [float(v) for v in blk], white


def device_u16(x):
    """ndarray uint16 or CUDA int16/uint16 tensor -> contiguous CUDA tensor of the same bits, 4-byte aligned (the kernels read a row
    as 32-bit words: a view starting at an odd element is copied)."""
    import torch
    if isinstance(x, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.int16)).cuda()
    x = x.contiguous()
    return x.clone() if x.data_ptr() % 4 else x


def workspace(nbytes, device):
    import torch
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)


# ---- what the saved sensor maps share ---------------------------------------------------------------------------------------------
class SensorMap:
    """Base of DefectMap, DarkShading and FlatField: a map made for mosaics of one `shape` and `cfa`; NOUN names it in the messages."""
    NOUN = 'map'

    @property
    def period(self):
        return period_of(self.cfa)

    def check_frames(self, shape, cfa, what='frames'):
        """ValueError unless mosaics of `shape` ((..., Hm, Wm)) and `cfa` are what this map was made for."""
        if cfa != self.cfa:
            raise ValueError('%s: the %s is for cfa=%r, the frames are %r' % (what, self.NOUN, self.cfa, cfa))
        if tuple(int(v) for v in shape[-2:]) != self.shape:
            raise ValueError('%s: the %s is for %d x %d mosaics, got %d x %d' % ((what, self.NOUN) + self.shape + tuple(int(v) for v in shape[-2:])))


class FittedMap(SensorMap):
    """A map fitted under one Bayer raw_pattern (DarkShading, FlatField)."""

    def check_pattern(self, raw_pattern, what='frames'):
        """ValueError when a Bayer raw_pattern is given that is not the map's (None: not compared)."""
        if raw_pattern is not None and self.cfa == 'bayer' and not np.array_equal(bayer_pattern(raw_pattern), self.raw_pattern):
            raise ValueError('%s: the %s was fitted under raw_pattern %r, got %r'
                             % (what, self.NOUN, self.raw_pattern.tolist(), np.asarray(raw_pattern).tolist()))


def check_sessions(sessions, cfa='bayer'):
    if not isinstance(sessions, (list, tuple)) or len(sessions) == 0:
        raise ValueError('sessions must be a non-empty list of {"iso", "bias", "flats" or "bursts"}')
    shape, nbias = None, 0
    for i, s in enumerate(sessions):
        if 'bias' not in s:
            raise ValueError('session %d has no %r' % (i, 'bias'))
        if 'flats' not in s and 'bursts' not in s:
            raise ValueError("session %d has neither 'flats' (flat-field pairs) nor 'bursts' (stacks of a static scene): the gain needs one of them" % i)
        F, Hm, Wm = check_mosaics(s['bias'], 3, 'session %d bias' % i, cfa)
        if shape is None:
            shape = (Hm, Wm)
        if 'flats' in s:
            P = check_mosaics(s['flats'], 4, 'session %d flats' % i, cfa)[0]
            if (Hm, Wm) != shape or shape_of(s['flats'])[-2:] != shape:
                raise ValueError('session %d: mosaic shapes differ (%s vs %s / %s)' % (i, shape, (Hm, Wm), shape_of(s['flats'])[-2:]))
            if F == 0 or P == 0:
                raise ValueError('session %d: needs at least one bias frame and one flat pair' % i)
        elif (Hm, Wm) != shape or F == 0:
            raise ValueError('session %d: needs at least one bias frame of %s, got %s' % (i, shape, (F, Hm, Wm)))
        if 'bursts' in s:
            if not isinstance(s['bursts'], (list, tuple)) or len(s['bursts']) == 0:
                raise ValueError("session %d: 'bursts' is a non-empty list of stacks (N, Hm, Wm)" % i)
            for j, b in enumerate(s['bursts']):
                bs = check_mosaics(b, 3, 'session %d burst %d' % (i, j), cfa)
                if bs[-2:] != shape:
                    raise ValueError('session %d burst %d: mosaic shapes differ (%s vs %s)' % (i, j, shape, bs[-2:]))
                if bs[0] < 2 or bs[0] > 256:
                    raise ValueError('session %d burst %d: a burst holds 2 to 256 frames, got %d' % (i, j, bs[0]))
        nbias += F
    if nbias < 3:
        raise ValueError('at least 3 bias frames are needed for the log-linear fits, got %d' % nbias)
    if len(sessions) < 2:
        raise ValueError('at least 2 sessions (2 distinct K) are needed, got %d' % len(sessions))
