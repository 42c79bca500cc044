"""NumPy int64 restatement of the defective-pixel contract (include/eld_amd.h "defective-pixel maps"): colour classes,
the same-class neighbourhood in a (2R + 1)^2 window clipped to the image, the lower median, the deviation of the stack sum, the flags,
the bitmap packing and the repair.  Brute force over the window offsets: nothing here knows the kernel's tap tables."""
import numpy as np

CODE_COLOUR = np.array([0, 1, 2, 1])              # rawpy colour code -> R 0, G 1, B 2
BAYER_R = 2
BIG = np.int64(1) << 40                           # sorts after every stack sum and every code


def class_map(Hm, Wm, cfa, raw_pattern):
    """(Hm,Wm) int64: Bayer the channel code raw_pattern[y&1][x&1]; X-Trans the colour of rawpy's 6x6 pattern (codes 1 and 3 both G)."""
    pat = np.asarray(raw_pattern, np.int64)
    if cfa == 'bayer':
        pat = pat.reshape(2, 2)
        return pat[np.arange(Hm)[:, None] & 1, np.arange(Wm)[None, :] & 1]
    pat = CODE_COLOUR[pat.reshape(6, 6)]
    return pat[np.arange(Hm)[:, None] % 6, np.arange(Wm)[None, :] % 6]


def lower_median(values):
    v = sorted(int(x) for x in values)
    return v[(len(v) - 1) // 2]


def neighbours(cls, y, x, R):
    """The sites of N(y, x), raster order."""
    Hm, Wm = cls.shape
    return [(yy, xx) for yy in range(max(0, y - R), min(Hm, y + R + 1)) for xx in range(max(0, x - R), min(Wm, x + R + 1))
            if (yy, xx) != (y, x) and cls[yy, xx] == cls[y, x]]


def _window_median(values, cls, allowed, R):
    """Per site: (lower median of `values` over the sites of N that are `allowed`, their number).  One pass per window offset."""
    Hm, Wm = cls.shape
    stack, valid = [], []
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            if dy == 0 and dx == 0:
                continue
            v = np.full((Hm, Wm), BIG, np.int64)
            ok = np.zeros((Hm, Wm), bool)
            ys, ye = max(0, -dy), min(Hm, Hm - dy)          # sites whose neighbour (y + dy, x + dx) lies inside the image
            xs, xe = max(0, -dx), min(Wm, Wm - dx)
            if ys < ye and xs < xe:
                here = (slice(ys, ye), slice(xs, xe))
                there = (slice(ys + dy, ye + dy), slice(xs + dx, xe + dx))
                ok[here] = (cls[there] == cls[here]) & allowed[there]
                v[here] = np.where(ok[here], values[there], BIG)
            stack.append(v)
            valid.append(ok)
    stack, m = np.sort(np.stack(stack), axis=0), np.sum(np.stack(valid), axis=0)
    rank = np.maximum(m - 1, 0) // 2
    return np.take_along_axis(stack, rank[None], axis=0)[0], m


def deviation(stack, cls, R):
    """stack (F,Hm,Wm) uint16 -> D (Hm,Wm) int64 = S - lower median of S over N; a site without neighbours gets 0."""
    S = np.asarray(stack).astype(np.int64).sum(axis=0)
    med, m = _window_median(S, cls, np.ones(cls.shape, bool), R)
    return np.where(m > 0, S - med, 0)


def flags(D, T_hi, T_lo):
    return (D > T_hi) | (-D > T_lo)


def pack_bitmap(mask):
    """bool (Hm,Wm) -> uint32 (Hm, ceil(Wm/32)), bit x & 31 of word [y][x >> 5], by loops."""
    Hm, Wm = mask.shape
    out = np.zeros((Hm, (Wm + 31) // 32), np.uint32)
    for y, x in np.argwhere(mask):
        out[y, x >> 5] |= np.uint32(1) << np.uint32(x & 31)
    return out


def repair(u, mask, cls, R):
    """u (Hm,Wm) or (N,Hm,Wm) uint16 -> repaired copy: a flagged site becomes the lower median of u over the unflagged sites of N; with
    none it keeps its code."""
    u = np.asarray(u)
    if u.ndim == 3:
        return np.stack([repair(f, mask, cls, R) for f in u])
    med, m = _window_median(u.astype(np.int64), cls, ~mask, R)
    return np.where(mask & (m > 0), med, u).astype(np.uint16)


def repair_loops(u, mask, cls, R):
    """The same, site by site (for the hand-made cases)."""
    out = np.array(u, copy=True)
    for y, x in np.argwhere(mask):
        vals = [u[yy, xx] for yy, xx in neighbours(cls, y, x, R) if not mask[yy, xx]]
        if vals:
            out[y, x] = lower_median(vals)
    return out


def xtrans_min_neighbours(raw_pattern, R, sides):
    """The fewest neighbours any site has, over mosaics of every (Hm, Wm) in sides x sides."""
    best = None
    for Hm in sides:
        for Wm in sides:
            cls = class_map(Hm, Wm, 'xtrans', raw_pattern)
            n = min(len(neighbours(cls, y, x, R)) for y in range(Hm) for x in range(Wm))
            best = n if best is None else min(best, n)
    return best
