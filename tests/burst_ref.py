"""NumPy / Python-int restatement of eld_burst_stack_u16 (include/eld_amd.h, "a burst of a static scene"): the bit-exact yardstick of
eld_amd/csrc/burst.hip.  Written from the definition: every sample of every site is put to the rule, nothing is skipped.  Nothing here
imports eld_amd.  int64 holds every intermediate (the widest, k2q (N - 1) V1, is below 2^62); site_loop recomputes one site in Python
integers and reports the widths it met."""
import numpy as np

from pairstats_ref import NB, bin_index


def reject_mask(x, k2q, min_dev):
    """x int64 (N, ...) -> bool (N, ...): the samples the leave-one-out rule rejects."""
    N = x.shape[0]
    if N < 4 or k2q <= 0:
        return np.zeros(x.shape, bool)
    S1 = x.sum(axis=0)
    S2 = (x * x).sum(axis=0)
    d = N * x - S1
    V1 = (N - 1) * (S2 - x * x) - (S1 - x) * (S1 - x)
    return (np.abs(d) > (N - 1) * min_dev) & (4 * d * d * (N - 2) > k2q * (N - 1) * V1)


def stack(frames, p, group, G, black, white, k2q, min_dev, mask=None):
    """frames uint16 (N,Hm,Wm); group, black: p*p values per cell (y % p) * p + x % p; mask: bool (Hm,Wm) of flagged sites.
    -> (mean uint16 (Hm,Wm), kept uint8 (Hm,Wm) with 256 written as 0, ptc int64 (G, NB, 4))."""
    x = np.asarray(frames).astype(np.int64)
    N, Hm, Wm = x.shape
    rej = reject_mask(x, k2q, min_dev)
    n = N - rej.sum(axis=0)
    S = np.where(rej, 0, x).sum(axis=0)
    mean = np.where(n > 0, (2 * S + n) // np.maximum(2 * n, 1), 0)
    S1 = x.sum(axis=0)
    V = N * (x * x).sum(axis=0) - S1 * S1
    cell = (np.arange(Hm)[:, None] % p) * p + np.arange(Wm)[None, :] % p
    g = np.asarray(group, np.int64).reshape(-1)[cell]
    blk = np.asarray(black, np.int64).reshape(-1)[cell]
    ok = (g >= 0) & (n == N) & (x.max(axis=0) < white) & (x.min(axis=0) > 0)
    if mask is not None:
        ok = ok & ~np.asarray(mask, bool)
    b = bin_index(mean, blk, white)
    ptc = np.zeros((G, NB, 4), np.int64)
    idx = (g[ok], b[ok])
    np.add.at(ptc[..., 0], idx, 1)
    np.add.at(ptc[..., 1], idx, S1[ok])
    np.add.at(ptc[..., 2], idx, V[ok] % (1 << 32))
    np.add.at(ptc[..., 3], idx, V[ok] >> 32)
    return mean.astype(np.uint16), (n % 256).astype(np.uint8), ptc


def site_loop(samples, k2q, min_dev):
    """One site in Python integers -> (mean, n, rejected flags, widths): widths maps every intermediate of the rule and of the outputs to the
    largest absolute value met."""
    xs = [int(v) for v in samples]
    N = len(xs)
    S1, S2 = sum(xs), sum(v * v for v in xs)
    widths = {'S1': S1, 'S2': S2, 'V': N * S2 - S1 * S1, 'd': 0, 'd2': 0, 'V1': 0, 'left': 0, 'right': 0}
    flags = []
    for v in xs:
        d = N * v - S1
        V1 = (N - 1) * (S2 - v * v) - (S1 - v) ** 2
        left, right = 4 * d * d * (N - 2), k2q * (N - 1) * V1
        assert V1 >= 0
        for k, q in (('d', abs(d)), ('d2', d * d), ('V1', V1), ('left', left), ('right', right)):
            widths[k] = max(widths[k], q)
        flags.append(N >= 4 and k2q > 0 and abs(d) > (N - 1) * min_dev and left > right)
    kept = [v for v, r in zip(xs, flags) if not r]
    n = len(kept)
    return ((2 * sum(kept) + n) // (2 * n) if n else 0), n, flags, widths


def points(ptc, N, black):
    """ptc int64 (G, NB, 4), black: one value per group -> (n, mu, var) float64 (G, NB), nan where a bin is empty; the halves of sum V are
    recombined in Python integers."""
    G = ptc.shape[0]
    n = ptc[..., 0].astype(np.float64)
    mu = np.full((G, NB), np.nan)
    var = np.full((G, NB), np.nan)
    for g in range(G):
        for b in range(NB):
            c = int(ptc[g, b, 0])
            if c:
                mu[g, b] = int(ptc[g, b, 1]) / (N * c) - float(black[g])
                var[g, b] = (int(ptc[g, b, 2]) + (int(ptc[g, b, 3]) << 32)) / (N * (N - 1) * c)
    return n, mu, var


def gain(pts, min_sites=64):
    """Weighted least squares var = K mu + c over the points of `pts` (a list of (n, mu, var)) with n >= min_sites outside bins 0 and NB - 1,
    weights n / var^2 -> (K, c)."""
    n = np.concatenate([q[0][:, 1:NB - 1].reshape(-1) for q in pts])
    mu = np.concatenate([q[1][:, 1:NB - 1].reshape(-1) for q in pts])
    var = np.concatenate([q[2][:, 1:NB - 1].reshape(-1) for q in pts])
    use = (n >= min_sites) & (var > 0)
    n, mu, var = n[use], mu[use], var[use]
    w = n / (var * var)
    mw = np.sum(w * mu) / np.sum(w)
    vw = np.sum(w * var) / np.sum(w)
    K = np.sum(w * (mu - mw) * (var - vw)) / np.sum(w * (mu - mw) ** 2)
    return float(K), float(vw - K * mw)


def scene_burst(seed, N=16, Hm=64, Wm=96, K=2.0, read=3.0, black=512, white=16383):
    """The statistical case: scene 5 + 6000 ((x + 0.37 y) / (W + 0.37 H))^2 DN, x = clip(rint(K Poisson(scene / K) + N(0, read) + black), 0, white)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:Hm, 0:Wm]
    scene = 5.0 + 6000.0 * ((xx + 0.37 * yy) / (Wm + 0.37 * Hm)) ** 2
    x = K * rng.poisson(scene / K, size=(N, Hm, Wm)) + rng.normal(0.0, read, size=(N, Hm, Wm)) + black
    return np.clip(np.rint(x), 0, white).astype(np.uint16)
