"""NumPy restatement of eld_pair_level_stats_u16 (include/eld_amd.h, "error versus signal level"): the bit-exact yardstick of
eld_amd/csrc/pairstats.hip.  Written from the definition, not from the kernel's bit tricks.  Nothing here imports eld_amd."""
import numpy as np

NB = 61


def octave_loop(s):
    """floor(log2 s) of one positive integer, by counting."""
    o = 0
    while (1 << (o + 1)) <= s:
        o += 1
    return o


def bin_loop(ref, black, white):
    """The bin of one code, the slow way: the cross-check of bin_index."""
    s = ref - black
    if ref >= white:
        return NB - 1
    if s <= 0:
        return 0
    if s < 8:
        return s
    o = octave_loop(s)
    quarter = (4 * s) // (1 << o) - 4                 # which quarter of the octave [2^o, 2^(o+1)) holds s
    return 8 + 4 * (o - 3) + quarter


def bin_index(ref, black, white):
    """ref, black: integer arrays (broadcast) -> int64 bins in [0, NB)."""
    ref = np.asarray(ref, np.int64)
    s = ref - np.asarray(black, np.int64)
    ref, s = np.broadcast_arrays(ref, s)
    b = np.clip(s, 0, 7)
    big = s >= 8
    sb = s[big]
    o = np.floor(np.log2(sb.astype(np.float64))).astype(np.int64)
    b[big] = 8 + 4 * (o - 3) + (4 * sb) // (np.int64(1) << o) - 4
    b[ref >= white] = NB - 1
    return b


def pair_level_sums(est, ref, p, group, G, black, white, Hc=None, Wc=None, mask=None):
    """est, ref uint16 (F,Hm,Wm); group, black: p*p values per cell (y % p) * p + x % p (group -1: not counted); mask: bool (Hm,Wm) of
    flagged sites.  -> int64 (F, G, NB, 4) = (n, sum s, sum e, sum e^2), by np.add.at."""
    est = np.asarray(est).astype(np.int64)
    ref = np.asarray(ref).astype(np.int64)
    F, Hm, Wm = ref.shape
    Hc = Hm if Hc is None else Hc
    Wc = Wm if Wc is None else Wc
    cell = (np.arange(Hm)[:, None] % p) * p + np.arange(Wm)[None, :] % p
    g = np.asarray(group, np.int64).reshape(-1)[cell]
    blk = np.asarray(black, np.int64).reshape(-1)[cell]
    ok = (np.arange(Hm)[:, None] < Hc) & (np.arange(Wm)[None, :] < Wc) & (g >= 0)
    if mask is not None:
        ok = ok & ~np.asarray(mask, bool)
    out = np.zeros((F, G, NB, 4), np.int64)
    for f in range(F):
        s = ref[f] - blk
        e = est[f] - ref[f]
        b = bin_index(ref[f], blk, white)
        idx = (np.full(int(ok.sum()), f), g[ok], b[ok])
        np.add.at(out[..., 0], idx, 1)
        np.add.at(out[..., 1], idx, s[ok])
        np.add.at(out[..., 2], idx, e[ok])
        np.add.at(out[..., 3], idx, e[ok] * e[ok])
    return out
