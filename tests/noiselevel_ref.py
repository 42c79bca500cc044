"""NumPy restatement of eld_tile_noise_sums_u16 (include/eld_amd.h, "noise level from a single frame"): the bit-exact yardstick of
eld_amd/csrc/noiselevel.hip.  Written from the definition -- nine shifted views of the frame, one boolean per rule -- not from the
kernel's staging.  Nothing here imports eld_amd."""
import numpy as np

TILE = 16                   # a tile is TILE * stride sites on a side


def tiles_along(n, s):
    """Tiles that cover the sites s <= i < n - s."""
    return -(-(n - 2 * s) // (TILE * s)) if n > 2 * s else 0


def tile_sums_ref(frames, Hc, Wc, p, stride, group, G, black, white, mask=None):
    """frames uint16 (F,Hm,Wm) or (Hm,Wm); group, black: p*p values per cell (y % p) * p + x % p (group -1: not counted); mask: bool
    (Hm,Wm) of flagged sites.  -> int64 (F, nty, ntx, G, 4) = (n, sum S9, sum r^2, sum dx^2 + dy^2) per tile and group."""
    fr = np.asarray(frames)
    if fr.ndim == 2:
        fr = fr[None]
    fr = fr.astype(np.int64)
    F, Hm, Wm = fr.shape
    s = int(stride)
    assert 1 <= s <= p and p % s == 0 and 0 <= Hc <= Hm and 0 <= Wc <= Wm
    nty, ntx = tiles_along(Hc, s), tiles_along(Wc, s)
    out = np.zeros((F, nty, ntx, G, 4), np.int64)
    if nty == 0 or ntx == 0 or F == 0:
        return out
    cell = (np.arange(Hc)[:, None] % p) * p + np.arange(Wc)[None, :] % p
    grp = np.asarray(group, np.int64).reshape(-1)[cell]
    blk = np.asarray(black, np.int64).reshape(-1)[cell]
    flagged = np.zeros((Hc, Wc), bool) if mask is None else np.asarray(mask, bool)[:Hc, :Wc]
    h, w = Hc - 2 * s, Wc - 2 * s                           # the sites (y, x) = (s + i, s + j)

    def nine(a):
        """a (..., Hc, Wc) -> the views a[a_][b_] over the centre sites"""
        return [[a[..., ia * s:ia * s + h, ib * s:ib * s + w] for ib in range(3)] for ia in range(3)]

    g9, b9, m9 = nine(grp), nine(blk), nine(flagged)
    g = g9[1][1]
    static = g >= 0
    for ia in range(3):
        for ib in range(3):
            static = static & (g9[ia][ib] == g) & ~m9[ia][ib]
    black9 = sum(b9[ia][ib] for ia in range(3) for ib in range(3))
    ty = (np.arange(h) // (TILE * s))[:, None] + np.zeros((1, w), np.int64)
    tx = (np.arange(w) // (TILE * s))[None, :] + np.zeros((h, 1), np.int64)
    for f in range(F):
        v = nine(fr[f, :Hc, :Wc])
        ok = static.copy()
        for ia in range(3):
            for ib in range(3):
                ok &= (v[ia][ib] > 0) & (v[ia][ib] < white)
        r = (v[0][0] - 2 * v[0][1] + v[0][2] - 2 * v[1][0] + 4 * v[1][1] - 2 * v[1][2] + v[2][0] - 2 * v[2][1] + v[2][2])
        dx, dy = v[1][2] - v[1][0], v[2][1] - v[0][1]
        s9 = sum(v[ia][ib] for ia in range(3) for ib in range(3)) - black9
        idx = (ty[ok], tx[ok], g[ok])
        np.add.at(out[f, ..., 0], idx, 1)
        np.add.at(out[f, ..., 1], idx, s9[ok])
        np.add.at(out[f, ..., 2], idx, (r * r)[ok])
        np.add.at(out[f, ..., 3], idx, (dx * dx + dy * dy)[ok])
    return out
