"""NumPy restatement, operation by operation, of the edge-directed Bayer demosaic (csrc/demosaic_edge.hip eld_render_bayer_edge,
csrc/demosaic_edge_dev.h; include/eld_amd.h and DESIGN.md sec. 32 state the same evaluation order).  Every stage is evaluated on the mosaic
extended by np.pad(mode='reflect') (period 2(H - 1), the edge not repeated: CFA parity is kept), four sites deep:

    A  every site      a_h = (2c - WW) - EE          a_v = (2c - NN) - SS
                       d_h = |W - E| + |a_h|         d_v = |N - S| + |a_v|
    B  every site      S_h, S_v = the sums of d_h, d_v over the 3x3 window, added to a zero in raster order
    C  R and B sites   g_h = (W + E)*0.5 + a_h*0.25  g_v = (N + S)*0.5 + a_v*0.25
                       w_h = S_v*S_v + 1e-6          w_v = S_h*S_h + 1e-6
                       G^  = g_h + (g_v - g_h) * (w_v / (w_h + w_v));            G^ = c at G sites
    D  delta = c - G^ at R and B sites; colour k in {R, B}: c at its own sites, G^ + ((d_NW + d_NE) + (d_SW + d_SE))*0.25 at the other
       colour's, G^ + (d_W + d_E)*0.5 at a G site with k left and right, G^ + (d_N + d_S)*0.5 at a G site with k above and below.

`dtype` lets the tests evaluate the same formulas in float64.  The helpers (mosaic, colour map, matrix, quantiser) are tests/demosaic_ref.py's."""
import numpy as np

import demosaic_ref as D

F32 = np.float32


def edge_directed(m, raw_pattern):
    """m (N,H,W) Bayer mosaic -> (N,3,H,W) camera RGB in m's dtype."""
    t = m.dtype.type
    Nf, H, W = m.shape
    V = np.pad(m, ((0, 0), (4, 4), (4, 4)), mode='reflect')

    def at(A, ma, mo, dy, dx):
        """A, known on the frame and `ma` sites around it, at offset (dy, dx) from every site of the frame and `mo` sites around it"""
        o = ma - mo
        return A[:, o + dy:o + dy + H + 2 * mo, o + dx:o + dx + W + 2 * mo]

    def second(mo):
        """a_h, a_v on the frame + mo"""
        c = at(V, 4, mo, 0, 0)
        return (t(2) * c - at(V, 4, mo, 0, -2)) - at(V, 4, mo, 0, 2), (t(2) * c - at(V, 4, mo, -2, 0)) - at(V, 4, mo, 2, 0)

    # A, on the frame + 2
    a_h, a_v = second(2)
    d_h = np.abs(at(V, 4, 2, 0, -1) - at(V, 4, 2, 0, 1)) + np.abs(a_h)
    d_v = np.abs(at(V, 4, 2, -1, 0) - at(V, 4, 2, 1, 0)) + np.abs(a_v)
    # B, on the frame + 1
    S_h = np.zeros((Nf, H + 2, W + 2), m.dtype)
    S_v = np.zeros((Nf, H + 2, W + 2), m.dtype)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            S_h = S_h + at(d_h, 2, 1, dy, dx)
            S_v = S_v + at(d_v, 2, 1, dy, dx)
    # C, on the frame + 1
    a_h, a_v = second(1)
    c1 = at(V, 4, 1, 0, 0)
    g_h = (at(V, 4, 1, 0, -1) + at(V, 4, 1, 0, 1)) * t(0.5) + a_h * t(0.25)
    g_v = (at(V, 4, 1, -1, 0) + at(V, 4, 1, 1, 0)) * t(0.5) + a_v * t(0.25)
    w_h = S_v * S_v + t(1e-6)
    w_v = S_h * S_h + t(1e-6)
    col1 = D.bayer_colour_map(raw_pattern, H + 4, W + 4)[1:H + 3, 1:W + 3]       # the colours of the frame + 1: the extension keeps parity
    G = np.where(col1 == 1, c1, g_h + (g_v - g_h) * (w_v / (w_h + w_v)))
    delta = c1 - G
    # D, on the frame

    def d(dy, dx):
        return at(delta, 1, 0, dy, dx)
    c, G0 = at(V, 4, 0, 0, 0), at(G, 1, 0, 0, 0)
    diag = G0 + ((d(-1, -1) + d(-1, 1)) + (d(1, -1) + d(1, 1))) * t(0.25)
    hor = G0 + (d(0, -1) + d(0, 1)) * t(0.5)
    ver = G0 + (d(-1, 0) + d(1, 0)) * t(0.5)
    col = D.bayer_colour_map(raw_pattern, H, W)
    col_h = np.roll(col, 1, axis=1)                        # colour of the horizontal neighbours (period 2: either side)
    out = np.zeros((Nf, 3, H, W), m.dtype)
    for k in (0, 2):
        out[:, k] = np.where(col == k, c, np.where(col == 2 - k, diag, np.where(col_h == k, hor, ver)))
    out[:, 1] = G0
    return out


def linear_bayer_edge(packed, raw_pattern, wbs, ccms=None, dtype=F32):
    rgb = edge_directed(D.mosaic_bayer(packed, raw_pattern, wbs, dtype), raw_pattern)
    return rgb if ccms is None else D.apply_ccm(rgb, ccms)


def gratings(seed, H=192, W=256):
    """the quality scene of tests/test_demosaic_edge_cpu.py: fine oriented gratings, one luminance under three slowly varying tints"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    L = np.zeros((H, W))
    for by in range(0, H, 48):
        for bx in range(0, W, 64):
            th = rng.uniform(0, np.pi)
            per = rng.uniform(2.6, 9)
            y, x = yy[by:by + 48, bx:bx + 64], xx[by:by + 48, bx:bx + 64]
            s = np.sin((x * np.cos(th) + y * np.sin(th)) * 2 * np.pi / per)
            L[by:by + 48, bx:bx + 64] = 0.5 + 0.35 * np.sign(s) * np.minimum(1.0, 3 * np.abs(s))
    tint = (0.9, 1.0, 0.7)
    return np.stack([np.clip(L * tint[k] * (1 + 0.15 * np.sin(xx / 40 + k) * np.cos(yy / 37 + 2 * k)), 0.0, 1.0) for k in range(3)])


def sample(img, pat):
    """(3,H,W) picture -> (1,4,H/2,W/2) packed planes of raw_pattern `pat`"""
    _, H, W = img.shape
    p = np.zeros((1, 4, H // 2, W // 2))
    for k in range(4):
        (oy,), (ox,) = np.where(np.asarray(pat) == k)
        p[0, k] = img[D.CODE_COLOUR[k], oy::2, ox::2]
    return p
