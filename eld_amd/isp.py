"""Raw -> sRGB ISP on the device: the reference's util/process.py:52-68 `process` (gains, binning, CCM, gamma / camera
response, 8-bit quantisation) as one HBM-bound HIP kernel (csrc/eval.hip eld_isp_process).  Used by the sRGB training /
evaluation stages (train_syn.py:55-58, models/ELD_model.py:230-233), and its X-Trans counterpart (process_xtrans) for eld_amd.denoise.
render_bayer / render_xtrans are the same pipeline at MOSAIC resolution: a demosaic (csrc/demosaic.hip; for Bayer with demosaic='edge'
csrc/demosaic_edge.hip, for X-Trans with demosaic='directional' csrc/demosaic_xdir.hip) in place of the binning; with
`warp=` the demosaiced camera RGB is resampled by a DNG WarpRectilinear before the matrix and the tone curve (warp_rgb, csrc/warp.hip); with
`frame=` it is cropped, resized by an antialiasing filter and turned by a TIFF orientation there (Frame, frame_rgb, csrc/frame.hip)."""
import collections
import ctypes
import math

import numpy as np

from . import _lib as L


def _crf(CRF, dev):
    import torch
    if CRF is None:
        return None, None, 0
    E = torch.as_tensor(np.asarray(CRF[0].cpu() if hasattr(CRF[0], 'cpu') else CRF[0]), dtype=torch.float32, device=dev).contiguous()
    fs = torch.as_tensor(np.asarray(CRF[1].cpu() if hasattr(CRF[1], 'cpu') else CRF[1]), dtype=torch.float32, device=dev).contiguous()
    n = int(E.numel())
    assert fs.numel() == n and n >= 2
    return E, fs, n


def process(bayer_images, wbs, cam2rgbs, gamma=2.2, CRF=None):
    """Same signature and semantics as util/process.py:52-68.  bayer_images: CUDA (N,4,H,W) float32 RGBG; wbs (N,4);
    cam2rgbs (N,3,3); CRF: None or (E, fs) 1-D tensors/arrays (ascending E).  Returns CUDA (N,3,H,W) float32."""
    import torch
    assert bayer_images.is_cuda and bayer_images.dim() == 4 and bayer_images.shape[1] == 4
    dev = bayer_images.device
    x = bayer_images.contiguous().float()
    N, _, H, W = x.shape
    wbs = torch.as_tensor(wbs, dtype=torch.float32, device=dev).reshape(N, 4).contiguous()
    ccm = torch.as_tensor(cam2rgbs, dtype=torch.float32, device=dev).reshape(N, 9).contiguous()
    out = torch.empty((N, 3, H, W), dtype=torch.float32, device=dev)
    E, fs, n = _crf(CRF, dev)
    L.check(L.lib().eld_isp_process(L.dptr(x), L.dptr(wbs), L.dptr(ccm), L.dptr(out), N, H, W, float(gamma), L.dptr(E), L.dptr(fs), n,
                                    L.cur_stream()), 'eld_isp_process')
    return out


def process_xtrans(packed, wbs, cam2rgbs, gamma=2.2, CRF=None):
    """`process` on X-Trans (csrc/eval.hip eld_isp_process_xtrans): packed CUDA (N,9,H,W) float32 in RawPacker.pack_raw_xtrans's planes, one
    packed pixel = one 3x3 mosaic block; wbs (N,3) R, G, B gains; cam2rgbs (N,3,3).  Per colour the mean of its planes (R 0, 3; G 1, 5-8;
    B 2, 4) summed in ascending plane order in float32 -- the reference's `process` applied to X-Trans binning, not LibRaw's demosaic.
    Returns CUDA (N,3,H,W) float32 quantised to k/255."""
    import torch
    assert packed.is_cuda and packed.dim() == 4 and packed.shape[1] == 9
    dev = packed.device
    x = packed.contiguous().float()
    N, _, H, W = x.shape
    wbs = torch.as_tensor(wbs, dtype=torch.float32, device=dev).reshape(N, 3).contiguous()
    ccm = torch.as_tensor(cam2rgbs, dtype=torch.float32, device=dev).reshape(N, 9).contiguous()
    out = torch.empty((N, 3, H, W), dtype=torch.float32, device=dev)
    E, fs, n = _crf(CRF, dev)
    L.check(L.lib().eld_isp_process_xtrans(L.dptr(x), L.dptr(wbs), L.dptr(ccm), L.dptr(out), N, H, W, float(gamma), L.dptr(E), L.dptr(fs), n,
                                           L.cur_stream()), 'eld_isp_process_xtrans')
    return out


def _render_out(x, planes, wbs, cam2rgbs, linear, gains):
    import torch
    if not (x.is_cuda and x.dim() == 4 and x.shape[1] == planes):
        raise ValueError('packed must be a CUDA (N,%d,h,w) tensor, got %s on %s' % (planes, tuple(x.shape), x.device))
    dev = x.device
    x = x.contiguous().float()
    N, _, h, w = x.shape
    wbs = torch.as_tensor(wbs, dtype=torch.float32, device=dev).reshape(N, gains).contiguous()
    ccm = None if cam2rgbs is None else torch.as_tensor(cam2rgbs, dtype=torch.float32, device=dev).reshape(N, 9).contiguous()
    if ccm is None and not linear:
        raise ValueError('the sRGB render needs cam2rgbs (only linear=True renders camera RGB)')
    f = planes // 4 + 1                                      # mosaic sites per packed pixel and side: Bayer 2, X-Trans 3
    out = torch.empty((N, 3, f * h, f * w), dtype=torch.float32 if linear else torch.uint8, device=dev)
    return x, wbs, ccm, out, L.RENDER_LINEAR_F32 if linear else L.RENDER_SRGB8


WARP_LDS_BYTES = -1                      # LDS a workgroup of eld_warp_rgb_f32 may stage source boxes in (< 0: the library's default, 0: none); tests set 65536


def warp_rgb(rgb, warp, cam2rgbs=None, gamma=2.2, CRF=None, linear=False):
    """DNG WarpRectilinear on demosaiced camera RGB, then the tail of the renders (csrc/warp.hip eld_warp_rgb_f32).
    rgb: CUDA (N,3,Hm,Wm) float32 camera RGB, as render_bayer / render_xtrans return it with linear=True and cam2rgbs=None.  warp: an
    eld_amd.dng_opcodes.Warp.  Every output pixel of every plane is a Catmull-Rom sample of its plane at the coordinate the warp's polynomial
    gives (the edge replicated); the three samples then take cam2rgbs (N,3,3; None: no matrix) and, unless linear, the gamma or CRF and the
    8-bit quantiser.  Returns CUDA (N,3,Hm,Wm): uint8 codes, or with linear=True float32."""
    import torch
    from .dng_opcodes import Warp
    if not isinstance(warp, Warp):
        raise ValueError('warp must be an eld_amd.dng_opcodes.Warp, got %r' % (type(warp).__name__,))
    if not (hasattr(rgb, 'is_cuda') and rgb.is_cuda and rgb.dim() == 4 and rgb.shape[1] == 3):
        raise ValueError('rgb must be a CUDA (N,3,Hm,Wm) tensor, got %s' % (tuple(rgb.shape) if hasattr(rgb, 'shape') else type(rgb).__name__,))
    dev = rgb.device
    x = rgb.contiguous().float()
    N, _, Hm, Wm = x.shape
    rec = warp.record(Hm, Wm)
    ccm = None if cam2rgbs is None else torch.as_tensor(cam2rgbs, dtype=torch.float32, device=dev).reshape(N, 9).contiguous()
    out = torch.empty((N, 3, Hm, Wm), dtype=torch.float32 if linear else torch.uint8, device=dev)
    E, fs, n = _crf(CRF, dev)
    with torch.cuda.device(dev):
        L.check(L.lib().eld_warp_rgb_f32(L.dptr(x), L.dptr(out), L.RENDER_LINEAR_F32 if linear else L.RENDER_SRGB8, N, Hm, Wm,
                                         ctypes.c_void_p(rec.ctypes.data), L.dptr(ccm), float(gamma), L.dptr(E), L.dptr(fs), n,
                                         int(WARP_LDS_BYTES), L.cur_stream()), 'eld_warp_rgb_f32')
    return out


def _warped(render, warp, cam2rgbs, gamma, CRF, linear):
    """the render with a warp: camera RGB (linear, no matrix) from `render`, then warp_rgb with the caller's matrix and tone curve"""
    if cam2rgbs is None and not linear:
        raise ValueError('the sRGB render needs cam2rgbs (only linear=True renders camera RGB)')
    return warp_rgb(render(), warp, cam2rgbs, gamma, CRF, linear)


# ---- the frame: crop, antialiased resize, orientation (csrc/frame.hip eld_frame_rgb_f32) ----------------------------------
FRAME_FILTERS = ('area', 'lanczos')
FRAME_MAX_TAPS = 4096
Taps = collections.namedtuple('Taps', 'ystart ycount yw xstart xcount xw')     # int32 (n,), int32 (n,), float32 (n,T) per axis: y over Hc, x over Wc


def _round_side(v):
    return max(1, int(math.floor(float(v) + 0.5)))


def _axis_taps(S, q, c, n, flt):
    """the tap table of one axis (the contract of DESIGN.md sec. 34, float64, every operation rounded on its own): source length S, crop origin q
    and length c, n outputs -> (start int32 (n,), count int32 (n,), weights float32 (n,T))"""
    F = np.float64
    i = np.arange(n, dtype=F)
    scale = F(c) / F(n)
    if flt == 'area':
        a = np.clip(F(q) + i * scale, F(0), F(S))
        b = np.clip(F(q) + (i + F(1)) * scale, F(0), F(S))
        lo, hi = np.floor(a).astype(np.int64), np.ceil(b).astype(np.int64)
    else:
        fs = max(scale, F(1))
        centre = F(q) + (i + F(0.5)) * scale
        lo = np.maximum(0, np.floor(centre - F(3) * fs + F(0.5)).astype(np.int64))
        hi = np.minimum(S, np.floor(centre + F(3) * fs + F(0.5)).astype(np.int64))
    count = hi - lo
    if count.min() < 1:
        raise ValueError('an output of the frame has no source tap: the crop does not lie inside the %d source pixels' % S)
    T = int(count.max())
    if T > FRAME_MAX_TAPS:
        raise ValueError('the frame reduces %g source pixels to %d: %d taps per output, more than %d' % (c, n, T, FRAME_MAX_TAPS))
    k = lo[:, None] + np.arange(T, dtype=np.int64)[None, :]
    used = k < hi[:, None]
    kf = k.astype(F)
    if flt == 'area':
        w = np.minimum(b[:, None], kf + F(1)) - np.maximum(a[:, None], kf)
    else:
        x = ((kf + F(0.5)) - centre[:, None]) / fs
        with np.errstate(all='ignore'):
            px, px3 = F(np.pi) * x, (F(np.pi) * x) / F(3)
            w = np.where(x == 0, F(1), (np.sin(px) / px) * (np.sin(px3) / px3))
        w = np.where(np.abs(x) < F(3), w, F(0))
    w = np.where(used, w, F(0))
    total = w[:, 0].copy()
    for t in range(1, T):                                            # the ascending sum; the padding adds zeros behind the last tap
        total = total + w[:, t]
    w32 = np.where(used, (w / total[:, None]), F(0)).astype(np.float32)
    return lo.astype(np.int32), count.astype(np.int32), np.ascontiguousarray(w32)


class Frame:
    """How a render is framed: a crop rectangle of the demosaiced picture, the size it is resampled to, and the TIFF orientation it is turned by.
    crop: None (the whole picture) or (y0, x0, ch, cw), floats in pixel-edge coordinates of the source (pixel i covers [i, i + 1)), inside it.
    orientation: 1 .. 8 (TIFF / Exif Orientation: 1 upright as stored, 3 turned by 180 degrees, 6 and 8 the two portrait ways, the even
    ones and 5, 7 mirrored).  size: the UPRIGHT picture: None (the crop's own size, each side rounded to the nearest integer >= 1), an int
    (the long edge; the other side keeps the aspect, rounded, >= 1) or (Ho, Wo).  filter: 'area' (default: every output is the mean of the
    source area it covers, which is exact antialiasing when it reduces and nearest-like when it enlarges) or 'lanczos' (a = 3, the support
    stretched by the reduction, as Pillow builds it)."""
    def __init__(self, crop=None, orientation=1, size=None, filter='area'):
        if crop is not None:
            try:
                crop = tuple(float(v) for v in crop)
            except (TypeError, ValueError):
                raise ValueError('crop must be None or (y0, x0, ch, cw), got %r' % (crop,))
            if len(crop) != 4 or not all(math.isfinite(v) for v in crop) or crop[0] < 0 or crop[1] < 0 or crop[2] <= 0 or crop[3] <= 0:
                raise ValueError('crop must be None or (y0, x0, ch, cw) with y0, x0 >= 0 and ch, cw > 0, got %r' % (crop,))
        if isinstance(orientation, bool) or not isinstance(orientation, (int, np.integer)) or not 1 <= int(orientation) <= 8:
            raise ValueError('orientation must be a TIFF Orientation 1 .. 8, got %r' % (orientation,))
        if size is not None:
            if isinstance(size, (int, np.integer)) and not isinstance(size, bool):
                size = int(size)
                ok = size >= 1
            else:
                try:
                    size = tuple(int(v) for v in size)
                    ok = len(size) == 2 and min(size) >= 1
                except (TypeError, ValueError):
                    ok = False
            if not ok:
                raise ValueError('size must be None, a long edge >= 1 or (Ho, Wo) with both >= 1, got %r' % (size,))
        if filter not in FRAME_FILTERS:
            raise ValueError('filter must be one of %r, got %r' % (FRAME_FILTERS, filter))
        self.crop, self.orientation, self.size, self.filter = crop, int(orientation), size, filter

    def __repr__(self):
        return 'Frame(crop=%r, orientation=%d, size=%r, filter=%r)' % (self.crop, self.orientation, self.size, self.filter)

    def rect(self, Hs, Ws):
        """the crop inside an Hs x Ws source, as float64 (y0, x0, ch, cw); ValueError when it leaves the source"""
        y0, x0, ch, cw = self.crop if self.crop is not None else (0.0, 0.0, float(Hs), float(Ws))
        if y0 + ch > Hs or x0 + cw > Ws:
            raise ValueError('the crop %r does not lie inside the %d x %d picture' % (self.crop, Hs, Ws))
        return y0, x0, ch, cw

    def out_size(self, Hs, Ws):
        """(Ho, Wo) of the upright picture this frame makes of an Hs x Ws source"""
        _, _, ch, cw = self.rect(Hs, Ws)
        uh, uw = (cw, ch) if self.orientation >= 5 else (ch, cw)         # the crop's upright sides
        if self.size is None:
            return _round_side(uh), _round_side(uw)
        if isinstance(self.size, int):
            if uh >= uw:
                return self.size, _round_side(self.size * uw / uh)
            return _round_side(self.size * uh / uw), self.size
        return self.size

    def taps(self, Hs, Ws):
        """-> (Taps, (Ho, Wo)): the tap tables of the unoriented grid (y: Hc entries, x: Wc entries; Hc x Wc is Ho x Wo, swapped for
        orientation >= 5) as NumPy arrays, and the upright size."""
        Hs, Ws = int(Hs), int(Ws)
        if Hs < 1 or Ws < 1:
            raise ValueError('the source must be at least 1 x 1, got %d x %d' % (Hs, Ws))
        y0, x0, ch, cw = self.rect(Hs, Ws)
        Ho, Wo = self.out_size(Hs, Ws)
        Hc, Wc = (Wo, Ho) if self.orientation >= 5 else (Ho, Wo)
        ys, yc, yw = _axis_taps(Hs, y0, ch, Hc, self.filter)
        xs, xc, xw = _axis_taps(Ws, x0, cw, Wc, self.filter)
        return Taps(ys, yc, yw, xs, xc, xw), (Ho, Wo)

    @property
    def identity(self):
        """the frame changes nothing: the whole picture at its own size, upright, through 'area' (single taps of weight exactly 1.0; 'lanczos'
        at scale 1 is not that: sin(pi n) is not 0 in float64, so its side taps carry weights near 1e-17 and it still filters)"""
        return self.crop is None and self.orientation == 1 and self.size is None and self.filter == 'area'


def frame_tile():
    """(rows, columns) of unoriented outputs in the tile one workgroup of eld_frame_rgb_f32's column pass owns"""
    th, tw = ctypes.c_int(), ctypes.c_int()
    L.check(L.lib().eld_frame_rgb_tile(ctypes.byref(th), ctypes.byref(tw), None), 'eld_frame_rgb_tile')
    return th.value, tw.value


def frame_rgb(rgb, frame, cam2rgbs=None, gamma=2.2, CRF=None, linear=False, out=None, workspace=None):
    """Crop, resize and turn demosaiced camera RGB, then the tail of the renders (csrc/frame.hip eld_frame_rgb_f32).
    rgb: CUDA (N,3,Hs,Ws) float32 camera RGB, as render_bayer / render_xtrans return it with linear=True and cam2rgbs=None, or warp_rgb
    with the same.  frame: a Frame.  The crop is resampled in linear light by the frame's separable filter (horizontal sums, then vertical
    ones, float32 in ascending tap order); the three values of a pixel then take cam2rgbs (N,3,3; None: no matrix) and, unless linear, the
    gamma or CRF and the 8-bit quantiser; the result is stored upright.  Returns CUDA (N,3,Ho,Wo): uint8 codes, or with linear=True float32.
    out, workspace: buffers to use in place of fresh ones: out (N,3,Ho,Wo) of the output's type, workspace float32 with at least
    N * 3 * rows * Wc elements (rows: the source rows the vertical table uses)."""
    import torch
    if not isinstance(frame, Frame):
        raise ValueError('frame must be an eld_amd.isp.Frame, got %r' % (type(frame).__name__,))
    if not (hasattr(rgb, 'is_cuda') and rgb.is_cuda and rgb.dim() == 4 and rgb.shape[1] == 3):
        raise ValueError('rgb must be a CUDA (N,3,Hs,Ws) tensor, got %s' % (tuple(rgb.shape) if hasattr(rgb, 'shape') else type(rgb).__name__,))
    dev = rgb.device
    x = rgb.contiguous().float()
    N, _, Hs, Ws = x.shape
    t, (Ho, Wo) = frame.taps(Hs, Ws)
    Wc = Ho if frame.orientation >= 5 else Wo
    row0 = int(t.ystart.min())                                       # the source rows the vertical table uses: one contiguous range
    rows = int((t.ystart + t.ycount).max()) - row0
    ccm = None if cam2rgbs is None else torch.as_tensor(cam2rgbs, dtype=torch.float32, device=dev).reshape(N, 9).contiguous()
    dtype = torch.float32 if linear else torch.uint8
    if out is None:
        out = torch.empty((N, 3, Ho, Wo), dtype=dtype, device=dev)
    elif tuple(out.shape) != (N, 3, Ho, Wo) or out.dtype != dtype or out.device != dev or not out.is_contiguous():
        raise ValueError('out must be a contiguous %s (%d,3,%d,%d) tensor on %s' % (dtype, N, Ho, Wo, dev))
    need = N * 3 * rows * Wc
    if workspace is None:
        workspace = torch.empty((max(need, 1),), dtype=torch.float32, device=dev)
    elif workspace.dtype != torch.float32 or workspace.device != dev or not workspace.is_contiguous() or workspace.numel() < need:
        raise ValueError('workspace must be a contiguous float32 tensor of at least %d elements on %s' % (need, dev))
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    tabs = [up(t.ystart, np.int32), up(t.ycount, np.int32), up(t.yw, np.float32), up(t.xstart, np.int32), up(t.xcount, np.int32),
            up(t.xw.T, np.float32)]                               # the x weights tap-major: a wave of the row pass reads 64 consecutive floats per tap
    E, fs, n = _crf(CRF, dev)
    with torch.cuda.device(dev):
        L.check(L.lib().eld_frame_rgb_f32(L.dptr(x), L.dptr(out), L.RENDER_LINEAR_F32 if linear else L.RENDER_SRGB8, N, Hs, Ws, Ho, Wo,
                                          frame.orientation, L.dptr(tabs[0]), L.dptr(tabs[1]), L.dptr(tabs[2]), int(t.yw.shape[1]),
                                          L.dptr(tabs[3]), L.dptr(tabs[4]), L.dptr(tabs[5]), int(t.xw.shape[1]), row0, rows, L.dptr(workspace),
                                          workspace.numel() * 4, L.dptr(ccm), float(gamma), L.dptr(E), L.dptr(fs), n, L.cur_stream()),
                'eld_frame_rgb_f32')
    return out


def _framed(render, warp, frame, cam2rgbs, gamma, CRF, linear):
    """the render with a frame: camera RGB (linear, no matrix) from `render`, warped first when there is a warp, then frame_rgb with the
    caller's matrix and tone curve"""
    if cam2rgbs is None and not linear:
        raise ValueError('the sRGB render needs cam2rgbs (only linear=True renders camera RGB)')
    cam = render()
    if warp is not None:
        cam = warp_rgb(cam, warp, None, linear=True)
    return frame_rgb(cam, frame, cam2rgbs, gamma, CRF, linear)


# the renders' demosaic: 'mhc', the CFA's default (Bayer: Malvar-He-Cutler; X-Trans: the normalised convolution); 'edge', the edge-directed
# Bayer one (csrc/demosaic_edge.hip); 'directional', the directional X-Trans one (csrc/demosaic_xdir.hip)
DEMOSAICS = ('mhc', 'edge', 'directional')


def check_demosaic(demosaic, cfa='bayer', srgb_size='full'):
    """what every caller with a demosaic argument refuses before any device work"""
    if not isinstance(demosaic, str) or demosaic not in DEMOSAICS:
        raise ValueError('demosaic must be one of %r, got %r' % (DEMOSAICS, demosaic))
    if demosaic == 'edge' and cfa != 'bayer':
        raise ValueError("demosaic='edge' is a Bayer demosaic: cfa=%r renders with its own" % (cfa,))
    if demosaic == 'edge' and srgb_size != 'full':
        raise ValueError("demosaic='edge' belongs to the full-resolution render: it needs srgb_size='full', got %r" % (srgb_size,))
    if demosaic == 'directional' and cfa != 'xtrans':
        raise ValueError("demosaic='directional' is an X-Trans demosaic: cfa=%r renders with its own" % (cfa,))
    if demosaic == 'directional' and srgb_size != 'full':
        raise ValueError("demosaic='directional' belongs to the full-resolution render: it needs srgb_size='full', got %r" % (srgb_size,))


def edge_tile():
    """(rows, columns) of PACKED pixels in the tile one workgroup of eld_render_bayer_edge owns"""
    th, tw = ctypes.c_int(), ctypes.c_int()
    L.check(L.lib().eld_render_bayer_edge_tile(ctypes.byref(th), ctypes.byref(tw), None), 'eld_render_bayer_edge_tile')
    return th.value // 2, tw.value // 2


def render_bayer(bayer_images, raw_pattern, wbs, cam2rgbs, gamma=2.2, CRF=None, linear=False, warp=None, demosaic='mhc', frame=None):
    """`process` at mosaic resolution (csrc/demosaic.hip eld_render_bayer): gains and clamp, Malvar-He-Cutler demosaic with mirrored
    borders, then the CCM / gamma or CRF / quantiser of `process`.  bayer_images CUDA (N,4,h,w) float32 in the planes of raw_pattern (2x2
    rawpy codes, R 0, G1 1, B 2, G2 3, as the write-back takes it); wbs (N,4) by plane; cam2rgbs (N,3,3), or None with linear=True.
    Returns CUDA (N,3,2h,2w): uint8 codes, or with linear=True float32 linear RGB after the CCM (no clamp, no gamma).
    warp: None, or an eld_amd.dng_opcodes.Warp: the demosaiced camera RGB is resampled by it (warp_rgb) before the matrix and the tone curve.
    demosaic: 'mhc' (default), or 'edge': the edge-directed demosaic of csrc/demosaic_edge.hip eld_render_bayer_edge in
    place of Malvar-He-Cutler; everything around it is the same, and packed sides of 1 are allowed.
    frame: None, or a Frame: the demosaiced camera RGB (after the warp, when both are given) is cropped, resized and turned by it before the
    matrix and the tone curve (frame_rgb); the output then has the frame's upright size."""
    check_demosaic(demosaic)
    if frame is not None:
        return _framed(lambda: render_bayer(bayer_images, raw_pattern, wbs, None, linear=True, demosaic=demosaic), warp, frame, cam2rgbs, gamma, CRF,
                       linear)
    if warp is not None:
        return _warped(lambda: render_bayer(bayer_images, raw_pattern, wbs, None, linear=True, demosaic=demosaic), warp, cam2rgbs, gamma, CRF, linear)
    x, wbs, ccm, out, mode = _render_out(bayer_images, 4, wbs, cam2rgbs, linear, 4)
    pat = [int(v) for v in np.asarray(raw_pattern).reshape(-1)]
    if len(pat) != 4:
        raise ValueError('raw_pattern must hold 2x2 codes, got %r' % (raw_pattern,))
    E, fs, n = _crf(CRF, x.device)
    N, _, h, w = x.shape
    name = 'eld_render_bayer_edge' if demosaic == 'edge' else 'eld_render_bayer'
    L.check(getattr(L.lib(), name)(L.dptr(x), (ctypes.c_int * 4)(*pat), L.dptr(wbs), L.dptr(ccm), L.dptr(out), mode, N, h, w, float(gamma),
                                   L.dptr(E), L.dptr(fs), n, L.cur_stream()), name)
    return out


def xdir_tile():
    """(rows, columns) of PACKED pixels in the tile one workgroup of eld_render_xtrans_dir owns"""
    th, tw = ctypes.c_int(), ctypes.c_int()
    L.check(L.lib().eld_render_xtrans_dir_tile(ctypes.byref(th), ctypes.byref(tw), None), 'eld_render_xtrans_dir_tile')
    return th.value // 3, tw.value // 3


def render_xtrans(packed, wbs, cam2rgbs, gamma=2.2, CRF=None, linear=False, warp=None, demosaic='mhc', frame=None):
    """`process_xtrans` at mosaic resolution (csrc/demosaic.hip eld_render_xtrans): gains by plane colour and clamp, a two-stage normalised
    convolution on colour differences (G from the 3x3, R - G and B - G from the 5x5 neighbourhood, windows clipped to the image), then
    the tail of `process`.  packed CUDA (N,9,h,w) float32 with even h and w (whole 6x6 cells); wbs (N,3); cam2rgbs (N,3,3), or None with
    linear=True.  Returns CUDA (N,3,3h,3w): uint8 codes, or with linear=True float32 linear RGB after the CCM.  warp: as render_bayer's.
    demosaic: 'mhc' (default: the render above), or 'directional': the directional demosaic of csrc/demosaic_xdir.hip eld_render_xtrans_dir
     in place of the normalised convolution of green; everything around it is the same.  frame: as render_bayer's."""
    check_demosaic(demosaic, 'xtrans')
    if frame is not None:
        return _framed(lambda: render_xtrans(packed, wbs, None, linear=True, demosaic=demosaic), warp, frame, cam2rgbs, gamma, CRF, linear)
    if warp is not None:
        return _warped(lambda: render_xtrans(packed, wbs, None, linear=True, demosaic=demosaic), warp, cam2rgbs, gamma, CRF, linear)
    x, wbs, ccm, out, mode = _render_out(packed, 9, wbs, cam2rgbs, linear, 3)
    E, fs, n = _crf(CRF, x.device)
    N, _, h, w = x.shape
    name = 'eld_render_xtrans_dir' if demosaic == 'directional' else 'eld_render_xtrans'
    L.check(getattr(L.lib(), name)(L.dptr(x), L.dptr(wbs), L.dptr(ccm), L.dptr(out), mode, N, h, w, float(gamma), L.dptr(E), L.dptr(fs), n,
                                   L.cur_stream()), name)
    return out
