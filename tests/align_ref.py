"""NumPy / Python-int restatement of the burst alignment (include/eld_amd.h, "aligning a hand-held burst"): the bit-exact
yardstick of eld_amd/csrc/align.hip.  Written from the definition; nothing here imports eld_amd, and the merge rule is burst_ref's.

    luma      L0[Y][X] = (sum of the p x p codes of cell (Y, X) + p p / 2) // (p p)
    pyramid   L[l+1][Y][X] = (a + b + c + d + 2) >> 2 over the 2 x 2 block at (2Y, 2X), coordinates clamped to the level
    tiles     T x T, origin min(t T, side - T): the last tile of a row or column is a whole tile shifted back
    search    coarsest level first; start = 2 x the parent tile's displacement; 81 candidates start + (v, u), |v|, |u| <= R, ranked by
              (|v| + |u|, v, u); cost = sum |ref - alt(clamped)| over the tile; the winner minimises (cost << 7) | rank
    stack     site (y, x) of tile (min(y / p / T, TY - 1), min(x / p / T, TX - 1)) takes frames[i][y + p dy][x + p dx] where that lies
              inside the frame; over its M present samples the rule of burst_ref with N = M"""
import numpy as np

import burst_ref
from pairstats_ref import NB, bin_index

T = 16
R = 4
MAX_LEVELS = 4
MAX_DISP = R * (1 + 2 + 4 + 8)

# candidate k = (v + R) * (2R + 1) + (u + R) -> rank
_CANDS = [(v, u) for v in range(-R, R + 1) for u in range(-R, R + 1)]
_ORDER = sorted(range(len(_CANDS)), key=lambda k: (abs(_CANDS[k][0]) + abs(_CANDS[k][1]), _CANDS[k][0], _CANDS[k][1]))
RANK = np.empty(len(_CANDS), np.int64)
RANK[_ORDER] = np.arange(len(_CANDS))


def luma(frames, p):
    """uint16 (N,Hm,Wm) -> uint16 (N, Hm // p, Wm // p)"""
    x = np.asarray(frames).astype(np.int64)
    N, Hm, Wm = x.shape
    Hl, Wl = Hm // p, Wm // p
    s = x[:, :p * Hl, :p * Wl].reshape(N, Hl, p, Wl, p).sum(axis=(2, 4))
    return ((s + p * p // 2) // (p * p)).astype(np.uint16)


def down(a):
    """One pyramid step on (N,h,w)."""
    a = np.asarray(a).astype(np.int64)
    h, w = a.shape[1:]
    y0 = np.minimum(2 * np.arange((h + 1) // 2), h - 1)
    y1 = np.minimum(2 * np.arange((h + 1) // 2) + 1, h - 1)
    x0 = np.minimum(2 * np.arange((w + 1) // 2), w - 1)
    x1 = np.minimum(2 * np.arange((w + 1) // 2) + 1, w - 1)
    s = a[:, y0][:, :, x0] + a[:, y0][:, :, x1] + a[:, y1][:, :, x0] + a[:, y1][:, :, x1]
    return ((s + 2) >> 2).astype(np.uint16)


def level_sides(Hm, Wm, p, levels):
    sides = [(Hm // p, Wm // p)]
    for _ in range(levels - 1):
        h, w = sides[-1]
        sides.append(((h + 1) // 2, (w + 1) // 2))
    return sides


def default_levels(Hm, Wm, p):
    """The largest count of levels (1..4) whose every level has both sides >= T; ValueError when level 0 has not."""
    h, w = Hm // p, Wm // p
    if h < T or w < T:
        raise ValueError('a frame of %d x %d has a luma plane of %d x %d: below one %d x %d tile' % (Hm, Wm, h, w, T, T))
    n = 1
    while n < MAX_LEVELS and (h + 1) // 2 >= T and (w + 1) // 2 >= T:
        h, w, n = (h + 1) // 2, (w + 1) // 2, n + 1
    return n


def check_levels(Hm, Wm, p, levels):
    most = default_levels(Hm, Wm, p)
    if levels is None:
        return most
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or levels < 1 or levels > MAX_LEVELS:
        raise ValueError('levels must be an integer in [1, %d], got %r' % (MAX_LEVELS, levels))
    if levels > most:
        raise ValueError('level %d of a %d x %d frame has a side below %d' % (levels - 1, Hm, Wm, T))
    return int(levels)


def pyramid(frames, p, levels):
    """-> list of uint16 (N,h,w), finest first"""
    out = [luma(frames, p)]
    for _ in range(levels - 1):
        out.append(down(out[-1]))
    return out


def tiles(side):
    """-> (count, origins) along one side"""
    n = -(-side // T)
    return n, [min(t * T, side - T) for t in range(n)]


def parent(origin, count_above):
    """The parent tile index, one level up, of the tile with this origin."""
    return min(((origin + T // 2) >> 1) // T, count_above - 1)


def tile_costs(ref, alt, y0, x0, sy, sx):
    """int64 (81,): the cost of every candidate of the tile at (y0, x0) around the start (sy, sx)."""
    h, w = ref.shape
    rt = ref[y0:y0 + T, x0:x0 + T].astype(np.int64)
    out = np.empty(len(_CANDS), np.int64)
    for k, (v, u) in enumerate(_CANDS):
        ys = np.clip(np.arange(y0, y0 + T) + sy + v, 0, h - 1)
        xs = np.clip(np.arange(x0, x0 + T) + sx + u, 0, w - 1)
        out[k] = np.abs(rt - alt[ys][:, xs].astype(np.int64)).sum()
    return out


def pick(costs):
    """-> (v, u, cost, key) of the winner"""
    keys = [(int(c) << 7) | int(r) for c, r in zip(costs, RANK)]
    k = int(np.argmin(keys))
    assert keys[k] < 1 << 31
    return _CANDS[k][0], _CANDS[k][1], int(costs[k]), keys[k]


def align(frames, p, ref=0, levels=None, all_levels=False):
    """-> (disp int16 (N,TY0,TX0,2), cost uint32 (N,TY0,TX0)); all_levels: -> the list of (disp, cost) per level, finest first."""
    frames = np.asarray(frames)
    N, Hm, Wm = frames.shape
    if not 0 <= ref < N:
        raise ValueError('ref must be a frame of the burst (0..%d), got %r' % (N - 1, ref))
    levels = check_levels(Hm, Wm, p, levels)
    pyr = pyramid(frames, p, levels)
    res = [None] * levels
    for l in range(levels - 1, -1, -1):
        h, w = pyr[l].shape[1:]
        (TY, oy), (TX, ox) = tiles(h), tiles(w)
        disp = np.zeros((N, TY, TX, 2), np.int16)
        cost = np.zeros((N, TY, TX), np.uint32)
        for i in range(N):
            if i == ref:
                continue
            for ty in range(TY):
                for tx in range(TX):
                    sy = sx = 0
                    if l + 1 < levels:
                        up = res[l + 1][0]
                        sy, sx = (2 * int(q) for q in up[i, parent(oy[ty], up.shape[1]), parent(ox[tx], up.shape[2])])
                    v, u, c, _ = pick(tile_costs(pyr[l][ref], pyr[l][i], oy[ty], ox[tx], sy, sx))
                    disp[i, ty, tx] = (sy + v, sx + u)
                    cost[i, ty, tx] = c
        res[l] = (disp, cost)
    assert np.abs(res[0][0]).max() <= MAX_DISP
    return res if all_levels else res[0]


def gather(frames, p, disp):
    """-> (samples int64 (N,Hm,Wm), present bool (N,Hm,Wm)): every site's sample from every frame through the field."""
    x = np.asarray(frames).astype(np.int64)
    N, Hm, Wm = x.shape
    disp = np.asarray(disp).astype(np.int64)
    TY, TX = disp.shape[1:3]
    ty = np.minimum(np.arange(Hm) // p // T, TY - 1)[:, None]
    tx = np.minimum(np.arange(Wm) // p // T, TX - 1)[None, :]
    yy = np.arange(Hm)[:, None] + p * disp[:, ty, tx, 0]
    xx = np.arange(Wm)[None, :] + p * disp[:, ty, tx, 1]
    present = (yy >= 0) & (yy < Hm) & (xx >= 0) & (xx < Wm)
    s = x[np.arange(N)[:, None, None], np.clip(yy, 0, Hm - 1), np.clip(xx, 0, Wm - 1)]
    return np.where(present, s, 0), present


def stack_aligned(frames, p, group, G, black, white, k2q, min_dev, disp, mask=None):
    """-> (mean uint16, kept uint8, present uint8 (256 written as 0), ptc int64 (G,NB,4)).  Per site the rule of burst_ref.reject_mask over
    its M present samples; a site with M = 0 gets mean 0 and kept 0.  Sites are grouped by M so that burst_ref's own code judges them."""
    if np.abs(np.asarray(disp).astype(np.int64)).max(initial=0) > MAX_DISP:
        raise ValueError('a displacement beyond +-%d' % MAX_DISP)
    s, present = gather(frames, p, disp)
    N, Hm, Wm = s.shape
    M = present.sum(axis=0)
    n = np.zeros((Hm, Wm), np.int64)
    S = np.zeros((Hm, Wm), np.int64)
    order = np.argsort(~present, axis=0, kind='stable')             # per site: the present frames first, in frame order
    packed = np.take_along_axis(s, order, axis=0)
    for m in np.unique(M):
        if m == 0:
            continue
        at = M == m
        x = packed[:m][:, at]
        rej = burst_ref.reject_mask(x, k2q, min_dev)
        n[at] = m - rej.sum(axis=0)
        S[at] = np.where(rej, 0, x).sum(axis=0)
    mean = np.where(n > 0, (2 * S + n) // np.maximum(2 * n, 1), 0)
    S1 = s.sum(axis=0)
    V = N * (s * s).sum(axis=0) - S1 * S1
    cell = (np.arange(Hm)[:, None] % p) * p + np.arange(Wm)[None, :] % p
    g = np.asarray(group, np.int64).reshape(-1)[cell]
    blk = np.asarray(black, np.int64).reshape(-1)[cell]
    ok = (g >= 0) & (M == N) & (n == N) & (s.max(axis=0) < white) & (s.min(axis=0) > 0)
    if mask is not None:
        ok = ok & ~np.asarray(mask, bool)
    b = bin_index(mean, blk, white)
    ptc = np.zeros((G, NB, 4), np.int64)
    idx = (g[ok], b[ok])
    np.add.at(ptc[..., 0], idx, 1)
    np.add.at(ptc[..., 1], idx, S1[ok])
    np.add.at(ptc[..., 2], idx, V[ok] % (1 << 32))
    np.add.at(ptc[..., 3], idx, V[ok] >> 32)
    return mean.astype(np.uint16), (n % 256).astype(np.uint8), (M % 256).astype(np.uint8), ptc


def scene(seed, Hm, Wm, p, margin=24):
    """The closed loop's signal in DN over a (Hm + margin p) x (Wm + margin p) grid, and the generator, for the noise, in its state after it."""
    rng = np.random.default_rng(seed)
    H, W = Hm + margin * p, Wm + margin * p
    a = rng.uniform(size=(H, W))
    for k in (1, 2, 4, 8):
        u = rng.uniform(size=(-(-H // k), -(-W // k)))
        a = a + k * np.kron(u, np.ones((k, k)))[:H, :W]
    a = (a - a.min()) / (a.max() - a.min())
    return 600.0 + 5000.0 * a * a, rng


def shifted_burst(seed, Hm, Wm, p, N=5, span=6, K=2.0, read=3.0, black=512, white=16383, margin=24):
    """-> (frames uint16 (N,Hm,Wm), shifts int (N,2) in CFA periods, noisy uint16 (N, H, W)): frame i is the window at
    p (margin / 2 + shift_i) of its own noisy realisation of the scene; frame 0 has no shift."""
    sig, rng = scene(seed, Hm, Wm, p, margin)
    shifts = np.zeros((N, 2), np.int64)
    shifts[1:] = rng.integers(-span, span + 1, size=(N - 1, 2))
    noisy = K * rng.poisson(sig / K, size=(N,) + sig.shape) + rng.normal(0.0, read, size=(N,) + sig.shape) + black
    noisy = np.clip(np.rint(noisy), 0, white).astype(np.uint16)
    o = p * (margin // 2)
    frames = np.stack([noisy[i, o + p * a:o + p * a + Hm, o + p * b:o + p * b + Wm] for i, (a, b) in enumerate(shifts)])
    return frames, shifts, noisy
