"""Mosaic arguments shared by every module that takes raw frames: the CFA and its raw_pattern, black levels, the shapes and dtypes of
uint16 mosaics, their upload, and the sessions of a calibration manifest.  A leaf module: it imports nothing from the package, so calibrate,
defects, shading, structure, validate, evaluate and burst can all import it."""
import numpy as np


# ---- argument checks (host only: they run before any device work) ---------------------------------------------------------------
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


XT_PERIOD = 6
CODE_COLOUR = np.array([0, 1, 2, 1])               # rawpy colour code (R, G, B, G2) -> colour class R 0, G 1, B 2


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


def check_cfa(cfa):
    if cfa not in ('bayer', 'xtrans'):
        raise ValueError("cfa must be 'bayer' or 'xtrans', got %r" % (cfa,))
    return cfa


def cell_counts(Hm, Wm, p=XT_PERIOD):
    """(p,p) int64: pixels of an Hm x Wm mosaic in cell (r, c) = {(y, x): y % p == r, x % p == c}."""
    nr = np.array([(Hm - r + p - 1) // p for r in range(p)], np.int64)
    nc = np.array([(Wm - c + p - 1) // p for c in range(p)], np.int64)
    return np.outer(nr, nc)


def shape_of(x):
    return tuple(int(s) for s in x.shape)


def check_mosaics(x, ndim, what, cfa='bayer'):
    s = shape_of(x)
    if len(s) != ndim:
        raise ValueError('%s: expected %d dimensions, got shape %s' % (what, ndim, s))
    if ndim == 4 and s[1] != 2:
        raise ValueError('%s: flat pairs must have shape (P, 2, Hm, Wm), got %s' % (what, s))
    Hm, Wm = s[-2:]
    if cfa == 'xtrans':
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
