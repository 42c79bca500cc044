"""NumPy restatement of the classical baseline (include/eld_amd.h: eld_nlm_vst_f32; eld_amd/classical.py).

The kernel's contract twice -- nlm_direct follows the definition with Python loops over q, d, u and c (tiny shapes), nlm_cumsum builds the
patch distance as a box sum of the per-position squared difference through an integral image -- and the host side in float64: the forward
tables, the weight table, the closed-form unbiased inverse and the whole pipeline on packed planes.  Nothing here imports eld_amd."""
import math

import numpy as np

Q = 16                                    # stabilised codes per noise standard deviation
FRAC = 4                                  # fractional bits of the kernel's output the pipeline asks for


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------------
def codes_of(x, qscale):
    """clamp(rintf(x * qscale), 0, 65535) in float32, NaN -> 0"""
    with np.errstate(invalid='ignore', over='ignore'):
        f = np.rint(np.asarray(x, np.float32) * np.float32(qscale))
    f = np.where(np.isnan(f), np.float32(0), f)
    return np.clip(f, 0, 65535).astype(np.int64)


def stabilised(x, qscale, fwd):
    """x (N,C,h,w) float32, fwd (C,65536) uint16 -> v (N,C,h,w) int64 = min(fwd[c][i], 32767)"""
    i = codes_of(x, qscale)
    fwd = np.asarray(fwd)
    v = np.empty(i.shape, np.int64)
    for c in range(i.shape[1]):
        v[:, c] = np.minimum(fwd[c].astype(np.int64)[i[:, c]], 32767)
    return v


def _quotient(num, den, frac):
    return (2 * (num << frac) + den) // (2 * den)


def nlm_direct(x, qscale, fwd, S, P, sh, wtab, frac, stats=None):
    """The definition, site by site."""
    v = stabilised(x, qscale, fwd)
    N, C, h, w = v.shape
    wtab = [int(t) for t in np.asarray(wtab).reshape(256)]
    out = np.empty((N, C, h, w), np.int64)

    def V(n, c, y, x_):
        return int(v[n, c, min(max(y, 0), h - 1), min(max(x_, 0), w - 1)])

    for n in range(N):
        for y in range(h):
            for x_ in range(w):
                num, den = [0] * C, 0
                for dy in range(-S, S + 1):
                    for dx in range(-S, S + 1):
                        if not (0 <= y + dy < h and 0 <= x_ + dx < w):
                            continue
                        D = 0
                        for c in range(C):
                            for uy in range(-P, P + 1):
                                for ux in range(-P, P + 1):
                                    df = V(n, c, y + uy, x_ + ux) - V(n, c, y + uy + dy, x_ + ux + dx)
                                    df = min(max(df, -1023), 1023)
                                    D += df * df
                        wt = wtab[min(D >> sh, 255)]
                        if stats is not None:
                            stats.add(wt)
                        den += wt
                        for c in range(C):
                            num[c] += wt * int(v[n, c, y + dy, x_ + dx])
                for c in range(C):
                    out[n, c, y, x_] = _quotient(num[c], den, frac)
    return out.astype(np.int32)


def nlm_cumsum(x, qscale, fwd, S, P, sh, wtab, frac, stats=None):
    """The same numbers with D_d as a box sum of E_d(r) = sum_c clamp(V_c(r) - V_c(r + d))^2 over the (2P + 1)^2 positions around q.
    stats: a set that receives every weight a counted candidate got."""
    v = stabilised(x, qscale, fwd)
    N, C, h, w = v.shape
    H = S + P
    wt_tab = np.asarray(wtab).reshape(256).astype(np.int64)
    Vp = np.pad(v, ((0, 0), (0, 0), (H, H), (H, H)), mode='edge')
    num = np.zeros((N, C, h, w), np.int64)
    den = np.zeros((N, 1, h, w), np.int64)
    yy, xx = np.arange(h)[:, None], np.arange(w)[None, :]
    eh, ew = h + 2 * P, w + 2 * P
    for dy in range(-S, S + 1):
        for dx in range(-S, S + 1):
            ok = (yy + dy >= 0) & (yy + dy < h) & (xx + dx >= 0) & (xx + dx < w)
            if not ok.any():
                continue
            A = Vp[:, :, S:S + eh, S:S + ew]                              # positions r = q + u, u >= -P
            B = Vp[:, :, S + dy:S + dy + eh, S + dx:S + dx + ew]          # r + d, replicated where it leaves the plane
            E = (np.clip(A - B, -1023, 1023) ** 2).sum(axis=1)           # (N, eh, ew)
            I = np.zeros((N, eh + 1, ew + 1), np.int64)
            I[:, 1:, 1:] = E.cumsum(axis=1).cumsum(axis=2)
            k = 2 * P + 1
            D = I[:, k:k + h, k:k + w] - I[:, :h, k:k + w] - I[:, k:k + h, :w] + I[:, :h, :w]
            wt = wt_tab[np.minimum(D >> sh, 255)] * ok
            if stats is not None:
                stats.update(np.unique(wt[:, ok]).tolist())
            den[:, 0] += wt
            num += wt[:, None] * Vp[:, :, H + dy:H + dy + h, H + dx:H + dx + w]
    return _quotient(num, den, frac).astype(np.int32)


# ---- the host side, float64 in a fixed order ---------------------------------------------------------------------------------------------
def vst_tables(K, sigma, black_per_plane):
    """fwd[c][i] = min(rint(Q * (2 / K) * sqrt(max(K * (i - black_c) + 3/8 K^2 + sigma^2, 0))), 32767), uint16 (C, 65536)"""
    K, sigma = float(K), float(sigma)
    i = np.arange(65536, dtype=np.float64)
    out = np.empty((len(black_per_plane), 65536), np.uint16)
    for c, b in enumerate(black_per_plane):
        arg = np.maximum(K * (i - float(b)) + 0.375 * K * K + sigma * sigma, 0.0)
        out[c] = np.minimum(np.rint(Q * (2.0 / K) * np.sqrt(arg)), 32767.0).astype(np.uint16)
    return out


def nlm_weight_table(C, P, strength):
    """-> (sh, wtab uint16 (256,)): bin k of D >> sh holds D in [k 2^sh, (k + 1) 2^sh); its weight is taken at the bin's middle.  The
    expected distance of two patches of the same signal, 2 Q^2 n, is subtracted first; the table ends where the weight is below 1/510."""
    n = C * (2 * P + 1) ** 2
    h2 = float(strength) ** 2 * Q * Q * n
    bias = 2.0 * Q * Q * n
    top = bias + h2 * math.log(510.0)
    sh = 0
    while (256 << sh) < top:
        sh += 1
    k = np.arange(256, dtype=np.float64)
    wt = np.rint(255.0 * np.exp(-np.maximum((k + 0.5) * float(1 << sh) - bias, 0.0) / h2)).astype(np.uint16)
    wt[0] = max(int(wt[0]), 1)
    return sh, wt


def unbiased_inverse(out, frac, K, sigma):
    """The closed-form approximation of the exact unbiased inverse of the generalised Anscombe transform (Makitalo and Foi): DN above black."""
    K, sigma = float(K), float(sigma)
    D = np.asarray(out, np.float64) / (Q * (1 << frac))
    s = sigma / K
    Dm = np.maximum(D, 2.0 * math.sqrt(0.375 + s * s))
    r = math.sqrt(1.5)
    return K * (Dm * Dm / 4.0 + r / (4.0 * Dm) - 11.0 / (8.0 * Dm * Dm) + 5.0 * r / (8.0 * Dm * Dm * Dm) - 0.125 - s * s)


def denoise_planes(codes, K, sigma, black_per_plane, white, ratio, search=7, patch=2, strength=0.5):
    """codes (N,C,h,w): the sensor's codes of every packed plane (integers) -> (N,C,h,w) float32 in the network's output convention,
    z * ratio / (white - black_c)."""
    codes = np.asarray(codes)
    C = codes.shape[1]
    x = (codes.astype(np.float32) / np.float32(65535.0)).astype(np.float32)        # what pack_input(black 0, white 65535, ratio 1) yields
    fwd = vst_tables(K, sigma, black_per_plane)
    sh, wtab = nlm_weight_table(C, patch, strength)
    out = nlm_cumsum(x, 65535.0, fwd, search, patch, sh, wtab, FRAC)
    z = unbiased_inverse(out, FRAC, K, sigma)
    res = np.empty(codes.shape, np.float32)
    for c, b in enumerate(black_per_plane):
        res[:, c] = (z[:, c] * float(ratio) / (float(white) - float(b))).astype(np.float32)
    return res


# ---- the synthetic scene of the tests -----------------------------------------------------------------------------------------------------
def scene_planes(C, h, w):
    """Clean signal in DN above black, (C,h,w) float64 in [0.05, 7]: a sinusoid plus a 16-pixel checkerboard plus a ramp; the planes differ by
    a gain (a colour)."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    s = 0.5 + 0.5 * np.sin(2 * np.pi * (xx / 23.0 + yy / 37.0))
    chk = ((yy // 16 + xx // 16) % 2)
    ramp = (xx + yy) / float(max(h + w - 2, 1))
    base = 0.4 * s + 0.3 * chk + 0.3 * ramp                                        # [0, 1]
    gains = 0.6 + 0.4 * np.cos(np.arange(C) * 1.3) ** 2                            # (0.6, 1]
    return 0.05 + (7.0 - 0.05) * base[None] * gains[:, None, None]


def noisy_codes(clean_dn, K, sigma, black, white, seed):
    """Poisson-Gaussian sensor codes of a clean signal in DN above black: K * Poisson(clean / K) + N(0, sigma^2) + black, rounded, clipped
    to [0, white]."""
    rng = np.random.default_rng(seed)
    z = K * rng.poisson(np.maximum(clean_dn, 0.0) / K) + sigma * rng.standard_normal(clean_dn.shape) + black
    return np.clip(np.rint(z), 0, white).astype(np.uint16)


def psnr(a, b):
    mse = float(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))
    return 10.0 * math.log10(1.0 / mse)
