"""NumPy restatement of the dark-shading contracts (include/eld_amd.h "dark shading"), operation for operation: the
yardstick of eld_amd/csrc/shading.hip and of the host formulas of eld_amd/shading.py.  Nothing here imports eld_amd."""
import numpy as np

XT_RC = np.array([[[[0, 0], [0, 4]], [[3, 1], [3, 3]]],
                  [[[0, 2], [0, 5]], [[3, 2], [3, 5]]],
                  [[[0, 1], [0, 3]], [[3, 0], [3, 4]]],
                  [[[1, 2], [2, 5]], [[5, 2], [4, 5]]],
                  [[[2, 2], [1, 5]], [[4, 2], [5, 5]]]])
XT_RC3 = np.array([[1, 0], [1, 1], [2, 0], [2, 1]])


def coefficients(isos, weights):
    """(x0, alpha, beta) of the weighted line through the session means: Python floats, sums in session order, the closed form of the 2x2
    inverse as eld_amd.shading.fit_coefficients states it."""
    iso, w = [float(v) for v in isos], [float(v) for v in weights]
    W = 0.0
    for v in w:
        W = W + v
    sx = 0.0
    for v, i in zip(w, iso):
        sx = sx + v * i
    x0 = sx / W
    if len(set(iso)) < 2:
        return x0, [v / W for v in w], [0.0] * len(w)
    d = [i - x0 for i in iso]
    Sx = Sxx = 0.0
    for v, di in zip(w, d):
        Sx = Sx + v * di
        Sxx = Sxx + (v * di) * di
    det = W * Sxx - Sx * Sx
    return x0, [(Sxx * v - Sx * (v * di)) / det for v, di in zip(w, d)], [(W * (v * di) - Sx * v) / det for v, di in zip(w, d)]


def cell_map(values, Hm, Wm):
    """(p,p) table -> (Hm,Wm): the value of cell (y % p, x % p) at every site."""
    v = np.asarray(values)
    p = v.shape[0]
    return v[np.arange(Hm)[:, None] % p, np.arange(Wm)[None, :] % p]


def fit(sessions, alpha, beta, centre, mask=None):
    """sessions: list of (F_s,Hm,Wm) uint16; centre (p,p) ints; mask: bool (Hm,Wm) of flagged sites -> (a, b) float32."""
    Hm, Wm = sessions[0].shape[1:]
    cen = cell_map(centre, Hm, Wm).astype(np.float64)
    A = np.zeros((Hm, Wm), np.float64)
    B = np.zeros((Hm, Wm), np.float64)
    for u, al, be in zip(sessions, alpha, beta):
        T = u.astype(np.int64).sum(axis=0)
        c = np.float64(u.shape[0])
        ys = (T.astype(np.float64) - c * cen) / c
        A = A + np.float64(al) * ys
        B = B + np.float64(be) * ys
    a, b = A.astype(np.float32), B.astype(np.float32)
    if mask is not None:
        a[mask] = 0.0
        b[mask] = 0.0
    return a, b


def step(a, b, t):
    """float32 ds = a + b * t (product rounded, sum rounded)."""
    return (a.astype(np.float32) + (b.astype(np.float32) * np.float32(t)).astype(np.float32)).astype(np.float32)


def apply(u, a, b, t, mask=None):
    """u (..., Hm, Wm) uint16 -> clamp(u - rint(a + b t), 0, 65535); flagged sites unchanged."""
    r = np.clip(np.rint(step(a, b, t)), -65536.0, 65536.0).astype(np.int64)        # np.rint: ties to even
    out = np.clip(u.astype(np.int64) - r, 0, 65535).astype(np.uint16)
    if mask is not None:
        out = np.where(mask, u, out)
    return out


def _tail(v, ratio):
    f = np.float32
    o = np.minimum(np.maximum(v, f(0)), f(1))
    return np.maximum(np.minimum((o * f(ratio)).astype(f), f(1)), f(0))


def pack_bayer_shaded(u, raw_pattern, black, white, ratios, a, b, t):
    """u (N,2h,2w) uint16 -> (N,4,h,w) float32: plane k from the cell position of colour code k."""
    f = np.float32
    pat = np.asarray(raw_pattern).reshape(-1)
    ds = step(a, b, t)
    N, Hm, Wm = u.shape
    out = np.empty((N, 4, Hm // 2, Wm // 2), f)
    for n in range(N):
        for k in range(4):
            i = int(np.flatnonzero(pat == k)[0])
            oy, ox = i >> 1, i & 1
            x = ((u[n, oy::2, ox::2].astype(f) - f(black[k])).astype(f) - ds[oy::2, ox::2]).astype(f)
            v = (x / (f(white) - f(black[k])).astype(f)).astype(f)
            out[n, k] = _tail(v, ratios[n])
    return out


def xtrans_sites(Hm, Wm):
    """(9,h,w) row and column of the mosaic site every packed element reads."""
    h, w = 2 * (Hm // 6), 2 * (Wm // 6)
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    rows, cols = np.empty((9, h, w), np.int64), np.empty((9, h, w), np.int64)
    for c in range(5):
        rows[c] = 6 * (i >> 1) + XT_RC[c][i & 1, j & 1, 0]
        cols[c] = 6 * (j >> 1) + XT_RC[c][i & 1, j & 1, 1]
    for c in range(5, 9):
        rows[c] = 3 * i + XT_RC3[c - 5][0]
        cols[c] = 3 * j + XT_RC3[c - 5][1]
    return rows, cols


def pack_xtrans_shaded(u, black, white, ratios, a, b, t):
    f = np.float32
    ds = step(a, b, t)
    N, Hm, Wm = u.shape
    rows, cols = xtrans_sites(Hm, Wm)
    out = np.empty((N,) + rows.shape, f)
    for n in range(N):
        x = ((u[n][rows, cols].astype(f) - f(black)).astype(f) - ds[rows, cols]).astype(f)
        v = (x / (f(white) - f(black)).astype(f)).astype(f)
        out[n] = _tail(v, ratios[n])
    return out


# ---- the closed loop of DESIGN.md sec. 18: a planted linear pattern, three sessions -------------------------------------------------------
LOOP = dict(seed=7, Hm=256, Wm=384, isos=(800, 1600, 3200), sigmas=(2.0, 3.5, 6.0), frames=8, black=512, a_sigma=1.5, b_sigma=3.0)


def closed_loop_inputs():
    """-> dict: sessions (list of (8,256,384) uint16), A, B (planted planes), held (2 further frames at ISO 1600), and the constants."""
    c = LOOP
    rng = np.random.default_rng(c['seed'])
    A = c['a_sigma'] * rng.standard_normal((c['Hm'], c['Wm']))
    B = c['b_sigma'] * rng.standard_normal((c['Hm'], c['Wm'])) / 3200.0
    sessions = []
    for iso, sg in zip(c['isos'], c['sigmas']):
        noise = sg * rng.standard_normal((c['frames'], c['Hm'], c['Wm']))
        sessions.append(np.rint(c['black'] + A + B * iso + noise).astype(np.uint16))
    held = np.rint(c['black'] + A + B * 1600 + 3.5 * rng.standard_normal((2, c['Hm'], c['Wm']))).astype(np.uint16)
    return {'sessions': sessions, 'A': A, 'B': B, 'held': held}
