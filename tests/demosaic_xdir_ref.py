"""NumPy restatement, operation by operation, of the directional X-Trans demosaic (csrc/demosaic_xdir.hip eld_render_xtrans_dir,
csrc/demosaic_xdir_dev.h; include/eld_amd.h and DESIGN.md sec. 33 state the same evaluation order).  Every stage is evaluated with full
windows on the mosaic v extended by 6 sites (one cell) with the colour-preserving mirror of `ext_index`:

    A  every site      G0 = v at G sites, else sum(w * v over the G sites of the 3x3 window, raster order, added to a zero) / sum(w),
                       w = [1 2 1] x [1 2 1]
    B  every site      d_h = |G0_W - G0_E| + |(2 G0 - G0_WW) - G0_EE|        d_v likewise with N, S
                       S_h, S_v = the sums of d_h, d_v over the 3x3 window, added to a zero in raster order
    C  R and B sites   per axis, by the pattern (`axis_maps`):
                         solitary (both neighbours and both second neighbours are G):
                             s1 = v(-1) + v(+1)    s2 = v(-2) + v(+2)    g = s1 * 0.5 + (s1 - s2) * (46/256)
                         paired (neighbour a is G, 2a the site's own colour, -2a is G):
                             g = (v(a) + (v(-2a) - v(a)) * (33/256)) + (v - v(2a)) * (92/256)
                       w_h = S_v*S_v + 1e-6          w_v = S_h*S_h + 1e-6
                       G^  = g_h + (g_v - g_h) * (w_v / (w_h + w_v));            G^ = v at G sites
    D  delta = v - G^ at R and B sites; colour k in {R, B}: v at its own sites, elsewhere
                       G^ + sum(w * delta over the k sites of the 5x5 window, raster order, added to a zero) / sum(w),
                       w = [1 2 3 2 1] x [1 2 3 2 1]

The two axis estimates are Markesteijn's (174, -46 and 223, 33, 92 in 256ths) written as a mean plus differences, so that a constant comes
back exact for every float32 value.  `dtype` lets the tests evaluate the same formulas in float64.  The helpers (mosaic, colour map, matrix,
quantiser) are tests/demosaic_ref.py's."""
import numpy as np

import demosaic_ref as D

F32 = np.float32
HALO = 6


def ext_index(i, L, axis):
    """index i of the extension of [0, L) into [0, L): rows (axis 0) mirror about lines = 0 (mod 3), columns (axis 1) about lines
    = 2 (mod 3), the only mirrors of the 6x6 cell; repeated until the index is inside (a 6-site side needs two rounds)"""
    i = int(i)
    while i < 0 or i >= L:
        if axis == 0:
            i = -i if i < 0 else 2 * (L - 3) - i
        else:
            i = 4 - i if i < 0 else 2 * (L - 1) - i
    return i


def ext_indices(L, axis, halo=HALO):
    return np.array([ext_index(i, L, axis) for i in range(-halo, L + halo)], np.int64)


def extend(m, halo=HALO):
    """(N,H,W) -> (N,H+2*halo,W+2*halo)"""
    _, H, W = m.shape
    return m[:, ext_indices(H, 0, halo)][:, :, ext_indices(W, 1, halo)]


def axis_maps(col):
    """For a periodic colour map: (a_h, a_v), int maps over the same sites.  0 at a G site and along the solitary axis of a non-G site;
    -1 / +1 along its paired axis: the side of the G neighbour."""
    out = []
    for axis in (1, 0):
        m1, p1 = np.roll(col, 1, axis), np.roll(col, -1, axis)
        out.append(np.where(col == 1, 0, np.where((m1 == 1) & (p1 == 1), 0, np.where(m1 == 1, -1, 1))))
    return out[0], out[1]


def _normfull(val, sel, wts, mo, ma, H, W):
    """sum(w * val over the selected sites of the full window) / sum(w) on the frame + mo; val and sel are known on the frame + ma"""
    t = val.dtype.type
    r = wts.shape[0] // 2
    o = ma - mo
    acc = np.zeros((val.shape[0], H + 2 * mo, W + 2 * mo), val.dtype)
    ws = np.zeros((H + 2 * mo, W + 2 * mo), np.int64)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ok = sel[o + dy:o + dy + H + 2 * mo, o + dx:o + dx + W + 2 * mo]
            v = val[:, o + dy:o + dy + H + 2 * mo, o + dx:o + dx + W + 2 * mo]
            wt = int(wts[dy + r, dx + r])
            acc = np.where(ok, acc + t(wt) * v, acc)
            ws = ws + wt * ok
    return acc, ws


def directional_xtrans(m):
    """m (N,H,W) X-Trans mosaic (whole 6x6 cells) -> (N,3,H,W) camera RGB in m's dtype."""
    t = m.dtype.type
    Nf, H, W = m.shape
    assert H % 6 == 0 and W % 6 == 0 and H >= 6 and W >= 6
    V = extend(m)
    colx = D.xtrans_colour_map(H + 12, W + 12)              # the colours of the frame + 6: the extension keeps the colour (a cell is 6 sites)
    a_h, a_v = axis_maps(colx)

    def at(A, ma, mo, dy, dx):
        """A, known on the frame and `ma` sites around it, at offset (dy, dx) from every site of the frame and `mo` sites around it"""
        o = ma - mo
        return A[..., o + dy:o + dy + H + 2 * mo, o + dx:o + dx + W + 2 * mo]

    # A, on the frame + 5
    acc, ws = _normfull(V, colx == 1, D.W3, 5, 6, H, W)
    col5 = at(colx, 6, 5, 0, 0)
    assert (ws[col5 != 1] > 0).all()
    G0 = np.where(col5 == 1, at(V, 6, 5, 0, 0), acc / np.maximum(ws, 1).astype(m.dtype))
    # B, gradients on the frame + 3, sums on the frame + 2
    c = at(G0, 5, 3, 0, 0)
    d_h = np.abs(at(G0, 5, 3, 0, -1) - at(G0, 5, 3, 0, 1)) + np.abs((t(2) * c - at(G0, 5, 3, 0, -2)) - at(G0, 5, 3, 0, 2))
    d_v = np.abs(at(G0, 5, 3, -1, 0) - at(G0, 5, 3, 1, 0)) + np.abs((t(2) * c - at(G0, 5, 3, -2, 0)) - at(G0, 5, 3, 2, 0))
    S_h = np.zeros((Nf, H + 4, W + 4), m.dtype)
    S_v = np.zeros((Nf, H + 4, W + 4), m.dtype)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            S_h = S_h + at(d_h, 3, 2, dy, dx)
            S_v = S_v + at(d_v, 3, 2, dy, dx)
    # C, on the frame + 2
    c2 = at(V, 6, 2, 0, 0)

    def axis_estimate(a, horizontal):
        def v(k):
            return at(V, 6, 2, 0, k) if horizontal else at(V, 6, 2, k, 0)
        s1, s2 = v(-1) + v(1), v(-2) + v(2)
        sol = s1 * t(0.5) + (s1 - s2) * t(46 / 256)
        pair = [(v(s) + (v(-2 * s) - v(s)) * t(33 / 256)) + (c2 - v(2 * s)) * t(92 / 256) for s in (-1, 1)]
        return np.where(a == 0, sol, np.where(a < 0, pair[0], pair[1]))
    g_h = axis_estimate(at(a_h, 6, 2, 0, 0), True)
    g_v = axis_estimate(at(a_v, 6, 2, 0, 0), False)
    w_h = S_v * S_v + t(1e-6)
    w_v = S_h * S_h + t(1e-6)
    col2 = at(colx, 6, 2, 0, 0)
    G = np.where(col2 == 1, c2, g_h + (g_v - g_h) * (w_v / (w_h + w_v)))
    delta = c2 - G
    # D, on the frame
    col = at(colx, 6, 0, 0, 0)
    v0, Gf = at(V, 6, 0, 0, 0), at(G, 2, 0, 0, 0)
    out = np.zeros((Nf, 3, H, W), m.dtype)
    out[:, 1] = Gf
    for k in (0, 2):
        acc, ws = _normfull(delta, col2 == k, D.W5, 0, 2, H, W)
        assert (ws > 0).all()
        out[:, k] = np.where(col == k, v0, Gf + acc / ws.astype(m.dtype))
    return out


def linear_xtrans_dir(packed, wbs, ccms=None, dtype=F32):
    rgb = directional_xtrans(D.mosaic_xtrans(packed, wbs, dtype))
    return rgb if ccms is None else D.apply_ccm(rgb, ccms)


def sample(img):
    """(3,H,W) picture, whole cells -> (1,9,H/3,W/3) packed planes"""
    _, H, W = img.shape
    rows, cols = D.O.xtrans_source_index(H // 3, W // 3)
    return np.stack([img[D.PLANE_COLOUR[k], rows[k], cols[k]] for k in range(9)])[None]
