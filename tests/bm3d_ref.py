"""NumPy restatement of BM3D on stabilised codes (include/eld_amd.h: eld_bm3d_vst_f32; eld_amd/classical.py).

The kernel's contract twice -- bm3d_direct follows the definition with Python loops over reference blocks, candidates, sites and coefficients
in Python integers (tiny shapes), bm3d_fast builds the block distances as box sums over sliding windows and transforms whole batches of groups
with Hadamard matrices in int64 -- and the host side: the threshold tables, the aggregation window and the whole pipeline on packed planes.
Nothing here imports eld_amd; the code rule, the forward tables and the inverse are nlm_ref's."""
import numpy as np

import nlm_ref as NR

Q = NR.Q
FRAC = NR.FRAC
BIG = (1 << 62)

WIN = np.array([[3, 5, 6, 7, 7, 6, 5, 3],
                [5, 7, 10, 11, 11, 10, 7, 5],
                [6, 10, 12, 14, 14, 12, 10, 6],
                [7, 11, 14, 16, 16, 14, 11, 7],
                [7, 11, 14, 16, 16, 14, 11, 7],
                [6, 10, 12, 14, 14, 12, 10, 6],
                [5, 7, 10, 11, 11, 10, 7, 5],
                [3, 5, 6, 7, 7, 6, 5, 3]], np.uint8)               # rint(16 kaiser(8, 2) x kaiser(8, 2))


# ---- what both forms share: the codes and the grid ----------------------------------------------------------------------------------------
def guide_codes(v, guide, frac):
    """g = v without a guide, else clamp((guide + half) >> frac, 0, 32767)"""
    if guide is None:
        return v
    g = (np.asarray(guide).astype(np.int64) + ((1 << frac) >> 1)) >> frac
    return np.clip(g, 0, 32767)


def grid(n, step):
    """top-left corners along an axis of n sites: 0, step, ... <= n - 8, and n - 8"""
    p = list(range(0, n - 8 + 1, step))
    if p[-1] != n - 8:
        p.append(n - 8)
    return p


def rank(dy, dx, S):
    """the low 11 bits of a key: 0 for the reference block itself, so that it leads its group whatever exact duplicates there are, else
    1 + (dy + S)(2S + 1) + (dx + S)"""
    return 0 if dy == 0 and dx == 0 else 1 + (dy + S) * (2 * S + 1) + (dx + S)


def offset_of(r, S):
    """rank -> (dy, dx)"""
    r = np.asarray(r)
    k = np.where(r == 0, S * (2 * S + 1) + S, r - 1)
    return k // (2 * S + 1) - S, k % (2 * S + 1) - S


def _check(C, h, w, S, step, Gmax, mix, tau, par, win, frac, step2):
    assert 1 <= C <= 16 and h >= 8 and w >= 8 and 0 <= S <= 16 and 1 <= step <= 8 and Gmax in (1, 2, 4, 8, 16) and mix in (0, 1)
    assert not mix or C in (1, 2, 4, 8, 16)
    assert 0 <= frac <= 4 and 0 <= tau < (1 << 30) and len(par) == 5 and len(win) == 64
    assert all(0 <= int(p) < (1 << 32) for p in par) and all(1 <= int(t) <= 16 for t in win)
    assert not step2 or all(int(p) >= 1 for p in par)


def _wiener_ratio(E, p):
    """floor(E * 4096 / (E + p)) without the 72-bit product: 4096 - ceil(4096 p / (E + p))"""
    return 4096 + ((-(p << 12)) // (E + p))


# ---- the definition, block by block -----------------------------------------------------------------------------------------------------------
def _wht_axis(a, lo, n):
    """a: list of 2^k Python integers, flattened [M][G][8][8]; the unnormalised Walsh-Hadamard transform (Sylvester, natural order) along the
    axis whose index occupies the bits lo .. lo + log2(n) - 1: out[.., k, ..] = sum_j (-1)^popcount(j & k) a[.., j, ..]"""
    out = [0] * len(a)
    mask = (n - 1) << lo
    for i in range(len(a)):
        k = (i & mask) >> lo
        base = i & ~mask
        s = 0
        for j in range(n):
            t = a[base | (j << lo)]
            s += -t if bin(j & k).count('1') & 1 else t
        out[i] = s
    return out


def _wht4(a, M, G):
    lg = G.bit_length() - 1
    a = _wht_axis(a, 0, 8)
    a = _wht_axis(a, 3, 8)
    a = _wht_axis(a, 6, G)
    return _wht_axis(a, 6 + lg, M)


def bm3d_direct(x, qscale, fwd, guide, S, step, Gmax, mix, tau, par, win, frac, stats=None):
    """The definition in Python integers.  stats: a dict that receives the number of groups per lg."""
    v = NR.stabilised(x, qscale, fwd)
    N, C, h, w = v.shape
    par = [int(p) for p in np.asarray(par).reshape(-1)]
    win = [int(t) for t in np.asarray(win).reshape(-1)]
    _check(C, h, w, S, step, Gmax, mix, tau, par, win, frac, guide is not None)
    g = guide_codes(v, guide, frac)
    M = C if mix else 1
    lm = M.bit_length() - 1
    nsets = C // M
    out = np.empty((N, C, h, w), np.int64)
    for n in range(N):
        vn, gn = v[n].tolist(), g[n].tolist()
        num = [[[0] * w for _ in range(h)] for _ in range(C)]
        den = [[[0] * w for _ in range(h)] for _ in range(nsets)]
        for py in grid(h, step):
            for px in grid(w, step):
                keys = []
                for dy in range(-S, S + 1):
                    for dx in range(-S, S + 1):
                        if not (0 <= py + dy <= h - 8 and 0 <= px + dx <= w - 8):
                            continue
                        D = 0
                        for c in range(C):
                            for uy in range(8):
                                for ux in range(8):
                                    df = gn[c][py + uy][px + ux] - gn[c][py + dy + uy][px + dx + ux]
                                    df = min(max(df, -1023), 1023)
                                    D += df * df
                        if D <= tau:
                            keys.append((D << 11) | rank(dy, dx, S))
                keys.sort()
                lg = min(len(keys), Gmax).bit_length() - 1
                G = 1 << lg
                if stats is not None:
                    stats[lg] = stats.get(lg, 0) + 1
                pos = []
                assert keys[0] == 0                                                              # the reference block leads
                for k in keys[:G]:
                    dy, dx = offset_of(k & 2047, S)
                    pos.append((py + int(dy), px + int(dx)))
                sh = 6 + lg + lm - frac
                for s in range(nsets):
                    planes = range(s * M, (s + 1) * M)

                    def blocks(src):
                        return [src[c][qy + uy][qx + ux] for c in planes for (qy, qx) in pos for uy in range(8) for ux in range(8)]

                    T = _wht4(blocks(vn), M, G)
                    if guide is None:
                        T = [t if abs(t) > par[lg] else 0 for t in T]
                        W = (1 << 20) // max(sum(1 for t in T if t != 0), 1)
                    else:
                        Tb = _wht4(blocks(gn), M, G)
                        R = [((e * e) << 12) // (e * e + par[lg]) for e in Tb]
                        T = [(t * r + 2048) >> 12 for t, r in zip(T, R)]
                        W = (1 << 44) // max(sum(r * r for r in R), 1 << 24)
                    I = _wht4(T, M, G)
                    i = 0
                    for m, c in enumerate(planes):
                        for (qy, qx) in pos:
                            for uy in range(8):
                                for ux in range(8):
                                    est = min(max((I[i] + (1 << (sh - 1))) >> sh, 0), 32767 << frac)
                                    i += 1
                                    ww = W * win[uy * 8 + ux]
                                    num[c][qy + uy][qx + ux] += ww * est
                                    if m == 0:
                                        den[s][qy + uy][qx + ux] += ww
        for c in range(C):
            for y in range(h):
                for x_ in range(w):
                    d = den[c // M][y][x_]
                    out[n, c, y, x_] = (2 * num[c][y][x_] + d) // (2 * d)
    return out.astype(np.int32)


# ---- the same numbers from sliding windows and Hadamard matrices --------------------------------------------------------------------------
def hadamard(n):
    H = np.ones((1, 1), np.int64)
    while H.shape[0] < n:
        H = np.block([[H, H], [H, -H]])
    return H


def _wht4_batch(a):
    """a (B, M, G, 8, 8) int64 -> the transform along the last four axes"""
    B, M, G = a.shape[:3]
    H8 = hadamard(8)
    a = np.einsum('bmgyx,kx->bmgyk', a, H8)
    a = np.einsum('bmgyx,ky->bmgkx', a, H8)
    a = np.einsum('bmgyx,kg->bmkyx', a, hadamard(G))
    return np.einsum('bmgyx,km->bkgyx', a, hadamard(M))


def match(gn, S, step, Gmax, tau):
    """gn (C,h,w) guide codes of one frame -> (py, px, n, order): the reference corners (ny,), (nx,), the number of counted candidates
    (ny,nx) and the candidates' ranks (the low bits of their keys) in key order (ny,nx,min(Gmax, K)), -1 beyond n."""
    C, h, w = gn.shape
    ys, xs = np.asarray(grid(h, step)), np.asarray(grid(w, step))
    K = (2 * S + 1) ** 2
    keys = np.full((K, len(ys), len(xs)), BIG, np.int64)
    for dy in range(-S, S + 1):
        for dx in range(-S, S + 1):
            k = (dy + S) * (2 * S + 1) + (dx + S)
            r = rank(dy, dx, S)
            y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)           # positions r with r and r + d in the plane
            if y1 - y0 < 8 or x1 - x0 < 8:
                continue
            E = (np.clip(gn[:, y0:y1, x0:x1] - gn[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx], -1023, 1023) ** 2).sum(axis=0)
            I = np.zeros((E.shape[0] + 1, E.shape[1] + 1), np.int64)
            I[1:, 1:] = E.cumsum(axis=0).cumsum(axis=1)
            D = I[8:, 8:] - I[:-8, 8:] - I[8:, :-8] + I[:-8, :-8]                                # corner p = (y0 + i, x0 + j)
            yi, xi = ys - y0, xs - x0
            oky, okx = (yi >= 0) & (yi < D.shape[0]), (xi >= 0) & (xi < D.shape[1])
            sub = D[np.ix_(yi[oky], xi[okx])]
            blk = keys[k]
            tgt = blk[np.ix_(oky, okx)]
            tgt[sub <= tau] = (sub[sub <= tau] << 11) | r
            blk[np.ix_(oky, okx)] = tgt
    keys.sort(axis=0)
    n = (keys < BIG).sum(axis=0)
    top = keys[:min(Gmax, K)]
    order = np.where(top < BIG, top & 2047, -1)
    return ys, xs, n, np.moveaxis(order, 0, -1)


def bm3d_fast(x, qscale, fwd, guide, S, step, Gmax, mix, tau, par, win, frac, stats=None, wide=None):
    """stats: as bm3d_direct's; wide: a list that receives, per transformed set, whether sum |T'| reaches 2^31 (the inverse then leaves 32 bits)"""
    v = NR.stabilised(x, qscale, fwd)
    N, C, h, w = v.shape
    par = [int(p) for p in np.asarray(par).reshape(-1)]
    win = np.asarray(win).reshape(-1).astype(np.int64)
    _check(C, h, w, S, step, Gmax, mix, tau, par, win, frac, guide is not None)
    g = guide_codes(v, guide, frac)
    M = C if mix else 1
    lm = M.bit_length() - 1
    nsets = C // M
    out = np.empty((N, C, h, w), np.int64)
    uy, ux = np.mgrid[0:8, 0:8]
    for n in range(N):
        ys, xs, cnt, order = match(g[n], S, step, Gmax, tau)
        lgs = np.floor(np.log2(np.minimum(cnt, Gmax))).astype(np.int64)
        pv = np.lib.stride_tricks.sliding_window_view(v[n], (8, 8), axis=(1, 2))                 # (C, h-7, w-7, 8, 8)
        pg = np.lib.stride_tricks.sliding_window_view(g[n], (8, 8), axis=(1, 2))
        num = np.zeros((C, h, w), np.int64)
        den = np.zeros((nsets, h, w), np.int64)
        for lg in range(5):
            by, bx = np.nonzero(lgs == lg)
            if stats is not None and len(by):
                stats[lg] = stats.get(lg, 0) + len(by)
            if not len(by):
                continue
            G = 1 << lg
            dy, dx = offset_of(order[by, bx, :G], S)                                             # (B, G)
            qy, qx = ys[by][:, None] + dy, xs[bx][:, None] + dx
            B = len(by)

            def blocks(p):
                a = np.moveaxis(p[:, qy, qx], 0, 1).astype(np.int64)                             # (B, C, G, 8, 8)
                return a.reshape(B * nsets, M, G, 8, 8)

            T = _wht4_batch(blocks(pv))
            if guide is None:
                T = np.where(np.abs(T) > par[lg], T, 0)
                W = (1 << 20) // np.maximum((T != 0).sum(axis=(1, 2, 3, 4)), 1)
            else:
                Tb = _wht4_batch(blocks(pg))
                R = _wiener_ratio(Tb * Tb, par[lg])
                T = (T * R + 2048) >> 12
                W = (1 << 44) // np.maximum((R * R).sum(axis=(1, 2, 3, 4)), 1 << 24)
            if wide is not None:
                wide.extend((np.abs(T).sum(axis=(1, 2, 3, 4)) >= (1 << 31)).tolist())
            I = _wht4_batch(T)
            sh = 6 + lg + lm - frac
            est = np.clip((I + (1 << (sh - 1))) >> sh, 0, 32767 << frac)                         # (B * nsets, M, G, 8, 8)
            ww = W[:, None, None, None] * win.reshape(1, 1, 8, 8)                                # (B * nsets, 1, 8, 8)
            sy = (qy[:, :, None, None] + uy)[:, None].repeat(nsets, axis=1).reshape(B * nsets, G, 8, 8)
            sx = (qx[:, :, None, None] + ux)[:, None].repeat(nsets, axis=1).reshape(B * nsets, G, 8, 8)
            sets = np.tile(np.arange(nsets), B)
            np.add.at(den, (sets[:, None, None, None], sy, sx), np.broadcast_to(ww, sy.shape))
            for m in range(M):
                np.add.at(num, ((sets * M + m)[:, None, None, None], sy, sx), ww * est[:, m])
        d = np.repeat(den, M, axis=0)
        out[n] = (2 * num + d) // (2 * d)
    return out.astype(np.int32)


# ---- the host side ----------------------------------------------------------------------------------------------------------------------------
def bm3d_tables(C, mix, strength=1.0, lam=2.7):
    """-> (tau1, thr[5], tau2, s2[5], win[64]) with n = 64 C terms in a block distance and M planes per transformed set"""
    n = 64 * C
    M = C if mix else 1
    s = float(strength)
    tau1 = int(np.rint(4.0 * Q * Q * n * s * s))
    tau2 = int(np.rint(0.64 * Q * Q * n * s * s))
    thr = np.array([np.rint(lam * 8.0 * Q * s * np.sqrt(float(M << lg))) for lg in range(5)]).astype(np.uint32)
    s2 = np.array([np.rint((8.0 * Q * s) ** 2 * float(M << lg)) for lg in range(5)]).astype(np.uint32)
    return tau1, thr, tau2, s2, WIN.reshape(-1).copy()


def bm3d_two_steps(x, qscale, fwd, S, step, Gmax, mix, tables, frac, stats=None):
    """step 1 (hard threshold), then step 2 (Wiener) guided by step 1's output -> (step 1, step 2), int32 each"""
    tau1, thr, tau2, s2, win = tables
    s1 = None if stats is None else stats.setdefault(1, {})
    s2s = None if stats is None else stats.setdefault(2, {})
    a = bm3d_fast(x, qscale, fwd, None, S, step, Gmax, mix, tau1, thr, win, frac, s1)
    b = bm3d_fast(x, qscale, fwd, a, S, step, Gmax, mix, tau2, s2, win, frac, s2s)
    return a, b


def denoise_planes_bm3d(codes, K, sigma, black_per_plane, white, ratio, search=12, step=3, group=16, mix=None, strength=1.0, first_only=False):
    """codes (N,C,h,w): the sensor's codes of every packed plane -> (N,C,h,w) float32 in the network's output convention,
    z * ratio / (white - black_c).  mix None: grouped across the planes when their number is a power of two."""
    codes = np.asarray(codes)
    C = codes.shape[1]
    if mix is None:
        mix = C & (C - 1) == 0
    x = (codes.astype(np.float32) / np.float32(65535.0)).astype(np.float32)
    fwd = NR.vst_tables(K, sigma, black_per_plane)
    a, b = bm3d_two_steps(x, 65535.0, fwd, search, step, group, int(bool(mix)), bm3d_tables(C, mix, strength), FRAC)
    z = NR.unbiased_inverse(a if first_only else b, FRAC, K, sigma)
    res = np.empty(codes.shape, np.float32)
    for c, bl in enumerate(black_per_plane):
        res[:, c] = (z[:, c] * float(ratio) / (float(white) - float(bl))).astype(np.float32)
    return res


# ---- inputs in which every group size occurs ------------------------------------------------------------------------------------------------
def identity_tables(C):
    """fwd[c][i] = min(i, 32767): the codes are the stabilised codes"""
    return np.stack([np.minimum(np.arange(65536), 32767).astype(np.uint16)] * C)


def flat_noise_x(N, C, h, w, seed, level=800):
    """codes rint(level + Q N(0, 1)) over 65535: a flat signal under unit-variance noise, where the block distances straddle any threshold near
    their expectation 2 Q^2 n"""
    rng = np.random.default_rng(seed)
    codes = np.rint(level + Q * rng.standard_normal((N, C, h, w))).astype(np.int64)
    return (codes.astype(np.float32) / np.float32(65535.0)).astype(np.float32)


GROUP_SIZE_CASES = {                                  # name -> (C, h, w, S, step, mix, seed, the step-1 threshold over 2 Q^2 n)
    'two planes': (2, 24, 27, 4, 3, 1, 3, 0.95),
    'four planes': (4, 19, 33, 6, 2, 0, 5, 0.9),
}


def group_size_case(name):
    """-> (x, fwd, S, step, Gmax, mix, (tau1, thr, tau2, s2, win)): with these every group size 1, 2, 4, 8, 16 occurs in step 1 and, guided by
    step 1's output, in step 2 (tau2 = 0.02 Q^2 n); the tests assert it on the `stats` of the restatement."""
    C, h, w, S, step, mix, seed, f1 = GROUP_SIZE_CASES[name]
    n = 64 * C
    _, thr, _, s2, win = bm3d_tables(C, mix)
    return flat_noise_x(1, C, h, w, seed), identity_tables(C), S, step, 16, mix, (int(f1 * 2 * Q * Q * n), thr, int(0.02 * Q * Q * n), s2, win)
