"""NumPy restatement of eld_amd/validate.py's contracts: both binning rules, the group maps, the clean image of a flat
pair and the KL divergence.  Written from the contract, not from the kernels."""
import numpy as np

CODE_COLOUR = np.array([0, 1, 2, 1])                 # rawpy colour code -> colour R 0, G 1, B 2
XT_PLANE_COLOUR = np.array([0, 1, 2, 0, 2, 1, 1, 1, 1])
Q_LIM = 2.0 ** 29


def groups_u16(cfa, raw_pattern):
    """-> (p, (p,p) int array of groups, G): Bayer the packed channel of the cell, X-Trans the colour of its code."""
    pat = np.asarray(raw_pattern, np.int64)
    if cfa == 'xtrans':
        return 6, CODE_COLOUR[pat.reshape(6, 6)], 3
    return 2, pat.reshape(2, 2), 4


def groups_f32(cfa):
    return (XT_PLANE_COLOUR, 3) if cfa == 'xtrans' else (np.arange(4), 4)


def bincount_groups(d, g, G, R, keep=None):
    """d: integer deviations, g: group of each element (-1: not counted) -> (G, 2R+1) int64: bin = clamp(d + R, 0, 2R)."""
    b = np.clip(np.asarray(d, np.int64) + R, 0, 2 * R)
    ok = np.asarray(g) >= 0
    if keep is not None:
        ok = ok & keep
    return np.stack([np.bincount(b[ok & (g == k)], minlength=2 * R + 1) for k in range(G)]).astype(np.int64)


def hist_u16_ref(u, p, group, G, centre, R, v=None, mask=None):
    """u (F,Hm,Wm) uint16; group: p*p ints in [-1, G); centre: G ints (ignored with v); mask (Hm,Wm) bool: True = flagged, not counted."""
    u = np.asarray(u).astype(np.int64)
    F, Hm, Wm = u.shape
    gm = np.asarray(group, np.int64).reshape(p, p)[np.arange(Hm)[:, None] % p, np.arange(Wm)[None, :] % p]
    keep = None if mask is None else ~np.asarray(mask, bool)
    out = []
    for f in range(F):
        d = u[f] - (np.asarray(v[f]).astype(np.int64) if v is not None else np.asarray(centre, np.int64)[np.maximum(gm, 0)])
        out.append(bincount_groups(d, gm, G, R, keep))
    return np.stack(out)


def quant_ref(x, scale):
    """q(t) = rint(float32(t) * float32(scale)) in float32 (round half to even), saturated at +-2^29; also the NaN mask of the product."""
    with np.errstate(invalid='ignore', over='ignore'):
        p = (np.asarray(x, np.float32) * np.float32(scale)).astype(np.float32)
    nan = np.isnan(p)
    q = np.clip(np.rint(np.where(nan, np.float32(0), p)), -Q_LIM, Q_LIM).astype(np.int64)
    return q, nan


def hist_f32_ref(x, group, G, scale, R, x2=None):
    """x (N,C,H,W) float32; group: C ints in [-1, G); scale: N floats."""
    x = np.asarray(x, np.float32)
    N, C, H, W = x.shape
    gm = np.broadcast_to(np.asarray(group, np.int64).reshape(C, 1, 1), (C, H, W))
    out = []
    for n in range(N):
        q, nan = quant_ref(x[n], scale[n])
        if x2 is not None:
            q2, nan2 = quant_ref(x2[n], scale[n])
            q, nan = q - q2, nan | nan2
        out.append(bincount_groups(q, gm, G, R, ~nan))
    return np.stack(out)


def clean_from_flat_pair_ref(a, b, cfa, raw_pattern, black, color_bias, sat):
    """y = clip((((a + b) * 0.5 - black_c) - color_bias_c) / sat, 0, 1), every operation in float32, packed: Bayer plane c = the cells of
    packed channel c; X-Trans the 9 planes of oracle.noise_ref.pack_raw_xtrans with the black level / bias of the plane's colour."""
    F32 = np.float32
    m = ((np.asarray(a).astype(F32) + np.asarray(b).astype(F32)) * F32(0.5)).astype(F32)
    black = np.asarray(black, np.float64)
    if cfa == 'xtrans':
        from oracle import noise_ref as O
        planes = O.pack_raw_xtrans(m)
        bl, cb = black[XT_PLANE_COLOUR], np.asarray(color_bias, np.float64)[XT_PLANE_COLOUR]
    else:
        pat = np.asarray(raw_pattern).reshape(2, 2)
        planes = np.stack([m[np.argwhere(pat == c)[0][0]::2, np.argwhere(pat == c)[0][1]::2] for c in range(4)])
        bl, cb = black, np.asarray(color_bias, np.float64)
    t = ((planes - bl.astype(F32)[:, None, None]).astype(F32) - cb.astype(F32)[:, None, None]).astype(F32)
    return np.clip((t / F32(sat)).astype(F32), F32(0), F32(1))


def kl_ref(p_counts, q_counts, alpha=1.0):
    """sum p log(p / q), p = (n + alpha) / (sum n + alpha B), over the last axis, float64, term by term in Python."""
    p_counts, q_counts = np.asarray(p_counts, np.float64), np.asarray(q_counts, np.float64)
    B = p_counts.shape[-1]
    out = np.zeros(p_counts.shape[:-1])
    for idx in np.ndindex(*p_counts.shape[:-1]):
        n, m = p_counts[idx], q_counts[idx]
        s = 0.0
        for k in range(B):
            pk, qk = (n[k] + alpha) / (n.sum() + alpha * B), (m[k] + alpha) / (m.sum() + alpha * B)
            if pk > 0:
                s += pk * np.log(pk / qk)
        out[idx] = s
    return out
