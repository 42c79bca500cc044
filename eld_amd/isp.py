"""Raw -> sRGB ISP on the device: the reference's util/process.py:52-68 `process` (gains, binning, CCM, gamma / camera
response, 8-bit quantisation) as one HBM-bound HIP kernel (csrc/eval.hip eld_isp_process).  Used by the sRGB training /
evaluation stages (train_syn.py:55-58, models/ELD_model.py:230-233), and its X-Trans counterpart (process_xtrans) for eld_amd.denoise.
render_bayer / render_xtrans are the same pipeline at MOSAIC resolution: a demosaic (csrc/demosaic.hip; for Bayer with demosaic='edge'
csrc/demosaic_edge.hip, for X-Trans with demosaic='directional' csrc/demosaic_xdir.hip) in place of the binning; with
`warp=` the demosaiced camera RGB is resampled by a DNG WarpRectilinear before the matrix and the tone curve (warp_rgb, csrc/warp.hip)."""
import ctypes

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


def render_bayer(bayer_images, raw_pattern, wbs, cam2rgbs, gamma=2.2, CRF=None, linear=False, warp=None, demosaic='mhc'):
    """`process` at mosaic resolution (csrc/demosaic.hip eld_render_bayer): gains and clamp, Malvar-He-Cutler demosaic with mirrored
    borders, then the CCM / gamma or CRF / quantiser of `process`.  bayer_images CUDA (N,4,h,w) float32 in the planes of raw_pattern (2x2
    rawpy codes, R 0, G1 1, B 2, G2 3, as the write-back takes it); wbs (N,4) by plane; cam2rgbs (N,3,3), or None with linear=True.
    Returns CUDA (N,3,2h,2w): uint8 codes, or with linear=True float32 linear RGB after the CCM (no clamp, no gamma).
    warp: None, or an eld_amd.dng_opcodes.Warp: the demosaiced camera RGB is resampled by it (warp_rgb) before the matrix and the tone curve.
    demosaic: 'mhc' (default), or 'edge': the edge-directed demosaic of csrc/demosaic_edge.hip eld_render_bayer_edge in
    place of Malvar-He-Cutler; everything around it is the same, and packed sides of 1 are allowed."""
    check_demosaic(demosaic)
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


def render_xtrans(packed, wbs, cam2rgbs, gamma=2.2, CRF=None, linear=False, warp=None, demosaic='mhc'):
    """`process_xtrans` at mosaic resolution (csrc/demosaic.hip eld_render_xtrans): gains by plane colour and clamp, a two-stage normalised
    convolution on colour differences (G from the 3x3, R - G and B - G from the 5x5 neighbourhood, windows clipped to the image), then
    the tail of `process`.  packed CUDA (N,9,h,w) float32 with even h and w (whole 6x6 cells); wbs (N,3); cam2rgbs (N,3,3), or None with
    linear=True.  Returns CUDA (N,3,3h,3w): uint8 codes, or with linear=True float32 linear RGB after the CCM.  warp: as render_bayer's.
    demosaic: 'mhc' (default: the render above), or 'directional': the directional demosaic of csrc/demosaic_xdir.hip eld_render_xtrans_dir
     in place of the normalised convolution of green; everything around it is the same."""
    check_demosaic(demosaic, 'xtrans')
    if warp is not None:
        return _warped(lambda: render_xtrans(packed, wbs, None, linear=True, demosaic=demosaic), warp, cam2rgbs, gamma, CRF, linear)
    x, wbs, ccm, out, mode = _render_out(packed, 9, wbs, cam2rgbs, linear, 3)
    E, fs, n = _crf(CRF, x.device)
    N, _, h, w = x.shape
    name = 'eld_render_xtrans_dir' if demosaic == 'directional' else 'eld_render_xtrans'
    L.check(getattr(L.lib(), name)(L.dptr(x), L.dptr(wbs), L.dptr(ccm), L.dptr(out), mode, N, h, w, float(gamma), L.dptr(E), L.dptr(fs), n,
                                   L.cur_stream()), name)
    return out
