"""Denoise raw frames end to end: a trained U-Net on a sensor's own uint16 mosaics, back to a uint16 mosaic (and, with a white
balance and a colour matrix, an 8-bit sRGB rendering).  The third step after calibrating a sensor (eld_amd.calibrate) and training a
denoiser for it (train_syn.py through the plugins).  Every device stage is a HIP kernel of libeld_amd:

    input stage   pack -> x ratio -> clip in one pass (eld_pack_raw_*_u16_gain; dataset/sid_dataset.py:398-409)
    network       the U-Net, whole frame when the packed sides are multiples of 16, else the reference's forward_chop tiles
    write-back    the packed output -> uint16 codes (eld_unpack_raw_*_u16; the mosaic half of postprocess_bayer / postprocess_xtrans,
                  models/ELD_model.py:41-129)
    sRGB          util/process.py `process` (eld_isp_process; X-Trans: eld_isp_process_xtrans, the same pipeline on X-Trans binning) at
                  packed resolution, or with srgb_size='full' the same pipeline behind a demosaic at mosaic resolution
                  (eld_render_bayer: Malvar-He-Cutler, or with demosaic='edge' eld_render_bayer_edge: edge-directed; eld_render_xtrans:
                  normalised convolution on colour differences, or with demosaic='directional' eld_render_xtrans_dir: directional)

Write-back rounding.  Per element v = float64(clip(x, 0, 1)) * (white - black) + black (exact).  rounding='reference' truncates as the
reference's assignment into the uint16 raw_image_visible does (Bayer: the float64 expression; X-Trans: the reference evaluates it in
float32, and so does this mode).  Under that truncation pack followed by write-back is NOT the identity on Bayer: of the 15872 codes in
[512, 16383], 7893 come back one DN low (7676 of 15360 for black 1024).  rounding='nearest' (the default) rounds half to even, and then
every code in [black, white] round-trips, for (black, white) = (512, 16383), (1024, 16383), (2048, 16383) and (0, 65535).

Raw files: a DNG input (.dng) is decoded on the device by eld_amd.dng (no rawpy) and its tags fill what the command line and the
sidecar leave open; every other format converts to DNG.  Mosaics also arrive as arrays (.npy, `raw.raw_image_visible`), with the values
rawpy reports (raw_pattern, black_level_per_channel, camera_whitebalance, rgb_camera_matrix[:3, :3]) as arguments or a JSON sidecar.
The sRGB output is the reference's `process`: at packed resolution by default, at mosaic resolution with --srgb-size full
(Bayer: Malvar-He-Cutler, or with --demosaic edge the edge-directed demosaic; X-Trans: normalised convolution, or with
--demosaic directional the directional demosaic).

    python -m eld_amd.denoise --ckpt model.pt --cfa xtrans --black 1024 --white 16383 --ratio 100 [--wb R G B] [--ccm 9 values] [--bf16] \\
        [--srgb-size full] in.npy [more.npy] -o outdir
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

from . import _lib as L
from .defects import as_defect_map, repair_device
from .flatfield import LENS_MODES, as_flat_field
from .isp import DEMOSAICS, FRAME_FILTERS, Frame, check_demosaic, frame_rgb, process, process_xtrans, render_bayer, render_xtrans, warp_rgb
from .mosaic import (DEFAULT_BLACK, DEFAULT_PATTERN, PLANES, as_u16 as _as_u16, check_cfa as _check_cfa,  # noqa: F401 (the names this module always had)
                     check_sides as _check_sides, levels as _levels)
from .shading import as_dark_shading

ROUNDING = ('nearest', 'reference')
SRGB_SIZES = ('packed', 'full')


# ---- the denoiser ---------------------------------------------------------------------------------------------------------------
class Denoiser:
    """A U-Net ready for inference: `net` (eld_amd.unet.UNetSeeInDark), the CFA it was trained for and its precision."""
    def __init__(self, net, cfa, precision):
        self.net, self.cfa, self.precision = net, cfa, precision

    @property
    def in_channels(self):
        return self.net.in_channels

    @property
    def out_channels(self):
        return self.net.out_channels


def load_denoiser(ckpt_or_model, cfa='bayer', precision='fp32', device=None):
    """ckpt_or_model: a checkpoint path, the reference's checkpoint dict ({'netG': state_dict, ...}, what ELDModel.save writes and
    ELDModel.load reads), a bare U-Net state_dict, an ELDModel or a U-Net instance.  Returns a Denoiser whose network runs in
    `precision` ('fp32' or 'bf16') on `device` (default: the current CUDA device)."""
    import torch
    from .unet import UNetSeeInDark
    _check_cfa(cfa)
    if precision not in ('fp32', 'bf16'):
        raise ValueError("precision must be 'fp32' or 'bf16', got %r" % (precision,))
    if isinstance(ckpt_or_model, (str, os.PathLike)):
        ckpt_or_model = torch.load(ckpt_or_model, map_location='cpu')
    if isinstance(ckpt_or_model, UNetSeeInDark):
        net = ckpt_or_model
    elif hasattr(ckpt_or_model, 'netG'):
        net = ckpt_or_model.netG
    elif isinstance(ckpt_or_model, dict):
        sd = ckpt_or_model.get('netG', ckpt_or_model)
        if 'conv1_1.weight' not in sd or 'conv10_1.weight' not in sd:
            raise ValueError('not a U-Net checkpoint: expected the reference dict {"netG": state_dict, ...} or a UNetSeeInDark state_dict')
        net = UNetSeeInDark(int(sd['conv1_1.weight'].shape[1]), int(sd['conv10_1.weight'].shape[0]))
        net.load_state_dict(sd)
    else:
        raise ValueError('cannot load a denoiser from %r' % (type(ckpt_or_model).__name__,))
    if device is None:
        device = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')
    net = net.to(device)
    net.requires_grad_(False)
    net.inference_precision = precision
    return Denoiser(net, cfa, precision)


# ---- argument checks (all before any device work; the mosaic's own are eld_amd.mosaic's) -----------------------------------------------
def _ratios(ratio, N):
    r = np.asarray(ratio, dtype=np.float64).reshape(-1)
    if r.size == 1:
        r = np.repeat(r, N)
    if r.size != N:
        raise ValueError('ratio takes one value or one per frame (%d), got %d' % (N, r.size))
    if not np.all(np.isfinite(r)) or np.any(r <= 0):
        raise ValueError('ratio must be finite and > 0, got %r' % (r.tolist(),))
    return r.astype(np.float32)


def _colour(cfa, wb, ccm, N):
    """-> (wbs float32 (N,4) Bayer RGBG / (N,3) X-Trans RGB, ccms float32 (N,3,3)) or (None, None)"""
    if wb is None and ccm is None:
        return None, None
    if wb is None or ccm is None:
        raise ValueError('the sRGB output needs both wb and ccm')
    w = np.asarray(wb, dtype=np.float64)
    if w.ndim == 1:
        w = np.broadcast_to(w, (N, w.size))
    if w.ndim != 2 or w.shape[0] != N or w.shape[1] not in (3, 4):
        raise ValueError('wb must hold 3 (R, G, B) or 4 (rawpy camera_whitebalance) values, per frame or for all, got shape %s'
                         % (np.shape(wb),))
    if w.shape[1] == 4:                       # raw2rgb_postprocess (util/process.py:111-121): wb /= wb[1]
        if np.any(w[:, 1] == 0):
            raise ValueError('camera_whitebalance with a zero green gain')
        w = w / w[:, 1:2]
    if cfa == 'bayer' and w.shape[1] == 3:
        w = np.concatenate([w, w[:, 1:2]], axis=1)          # R, G, B -> R, G1, B, G2
    if cfa == 'xtrans':
        w = w[:, :3]
    m = np.asarray(ccm, dtype=np.float64)
    if m.shape == (9,) or m.shape == (3, 3):
        m = np.broadcast_to(m.reshape(3, 3), (N, 3, 3))
    if m.shape != (N, 3, 3):
        raise ValueError('ccm must be 3x3 (9 values), per frame or for all, got shape %s' % (np.shape(ccm),))
    if not (np.all(np.isfinite(w)) and np.all(np.isfinite(m))):
        raise ValueError('wb and ccm must be finite')
    return np.ascontiguousarray(w, dtype=np.float32), np.ascontiguousarray(m, dtype=np.float32)


colour_args = _colour                                 # the public name (eld_amd.evaluate renders with it)


# ---- the device stages ------------------------------------------------------------------------------------------------------------
def pack_input(t, cfa, raw_pattern, black_level, white_point, ratios, shading=None, tval=None, flatfield=None):
    """CUDA int16-view codes (N,Hm,Wm) -> the network input (N,C,h,w) float32: pack, x ratio[n], clip -- one kernel.  shading (a
    DarkShading) with tval = shading.t(iso): the same kernel shape with the map a + b * tval subtracted in float32 between the black level
    and the division (eld_pack_raw_*_u16_shaded).  flatfield (a FlatField): the black- and shading-corrected value is multiplied by the
    map's PRNU plane before the division (eld_pack_raw_*_u16_flat), with or without a shading map."""
    import torch
    N, Hm, Wm = t.shape
    r = torch.as_tensor(np.asarray(ratios, np.float32), device=t.device)
    if cfa == 'bayer':
        out = torch.empty((N, 4, Hm // 2, Wm // 2), dtype=torch.float32, device=t.device)
        stem = 'eld_pack_raw_bayer_u16'
        head = (L.dptr(t), L.dptr(out), N, Hm // 2, Wm // 2, (ctypes.c_int * 4)(*raw_pattern), (ctypes.c_float * 4)(*black_level),
                float(white_point), L.dptr(r))
    else:
        out = torch.empty((N, 9, 2 * (Hm // 6), 2 * (Wm // 6)), dtype=torch.float32, device=t.device)
        stem = 'eld_pack_raw_xtrans_u16'
        head = (L.dptr(t), L.dptr(out), N, Hm, Wm, float(black_level[0]), float(white_point), L.dptr(r))
    ma, mb = shading.on(t.device) if shading is not None else (None, None)
    if flatfield is not None:
        gain = flatfield.on(t.device, 'prnu')
        name, planes = stem + '_flat', (L.dptr(ma), L.dptr(mb), float(tval) if shading is not None else 0.0, L.dptr(gain))
    elif shading is not None:
        name, planes = stem + '_shaded', (L.dptr(ma), L.dptr(mb), float(tval))
    else:
        name, planes = stem + '_gain', ()
    L.check(getattr(L.lib(), name)(*head, *planes, L.cur_stream()), name)
    return out


def write_back(packed, mosaic, cfa, raw_pattern, black_level, white_point, rounding='nearest'):
    """Packed output (N,C,h,w) float32 -> uint16 codes written INTO `mosaic` (CUDA int16/uint16 (N,Hm,Wm)).  Bayer writes every pixel;
    X-Trans writes the whole 6x6 cells and leaves the borders beyond them as they are."""
    packed = packed.contiguous().float()
    N = packed.shape[0]
    mode = {'nearest': L.ROUND_NEAREST, 'reference': L.ROUND_TRUNC if cfa == 'bayer' else L.ROUND_TRUNC_F32}[rounding]
    if cfa == 'bayer':
        pat = (ctypes.c_int * 4)(*raw_pattern)
        blk = (ctypes.c_float * 4)(*black_level)
        L.check(L.lib().eld_unpack_raw_bayer_u16(L.dptr(packed), L.dptr(mosaic), N, packed.shape[2], packed.shape[3], pat, blk, float(white_point),
                                                 mode, L.cur_stream()), 'eld_unpack_raw_bayer_u16')
    else:
        L.check(L.lib().eld_unpack_raw_xtrans_u16(L.dptr(packed), L.dptr(mosaic), N, mosaic.shape[1], mosaic.shape[2], float(black_level[0]),
                                                  float(white_point), mode, L.cur_stream()), 'eld_unpack_raw_xtrans_u16')
    return mosaic


def run_network(denoiser, x, chop=None):
    """x (N,C,h,w) CUDA float32 -> the network output.  chop None: whole frame when h and w are multiples of 16, else forward_chop."""
    import torch
    from .model import forward_chop
    h, w = x.shape[2:]
    if chop is None:
        chop = bool(h % 16 or w % 16)
    with torch.no_grad():
        return forward_chop(denoiser.net, x) if chop else denoiser.net(x)


def denoise_raw(denoiser, mosaic_u16, cfa, raw_pattern=None, black_level=None, white_point=16383, ratio=1.0, wb=None, ccm=None, CRF=None,
                chop=None, rounding='nearest', srgb_size='packed', linear=False, defects=None, shading=None, iso=None, flatfield=None,
                lens='srgb', warp=None, jpeg=None, demosaic='mhc', frame=None, preview_frame=None):
    """Denoise uint16 sensor mosaics with a trained U-Net -- or, given an eld_amd.classical.ClassicalDenoiser in place of a Denoiser, with the
    classical baseline (Anscombe transform, non-local means, unbiased inverse on the sensor's codes instead of the input stage and the
    network; `chop` is then ignored, and 'packed' is the baseline's output in the network's convention).

    mosaic_u16  NumPy uint16 array or CUDA uint16 / int16-view tensor, (Hm, Wm) or (N, Hm, Wm) -- rawpy's raw_image_visible.
    cfa         'bayer' (4 planes; raw_pattern: rawpy's 2x2 raw_pattern, default RGGB; black_level: 1 or 4 values, default 512) or
                'xtrans' (9 planes, RawPacker.pack_raw_xtrans's layout; one black level, default 1024).
    ratio       exposure ratio, one value or one per frame: the input is clip(pack(raw) * ratio, 0, 1) (dataset/sid_dataset.py:398-409).
    wb, ccm     with both, an sRGB rendering at packed resolution (util/process.py `process`): wb R, G, B, or rawpy's 4-value
                camera_whitebalance (divided by its green); ccm rawpy's rgb_camera_matrix[:3, :3].  CRF: None (gamma 2.2) or (E, fs).
    chop        None: whole frame when the packed sides are multiples of 16, else the reference's forward_chop; True / False force it.
    rounding    'nearest' (default: every code in [black, white] round-trips) or 'reference' (the reference's truncation, bit for bit).
    srgb_size   'packed' (default): the rendering above.  'full': the same gains, matrix and tone curve behind a demosaic, at mosaic
                resolution (N,3,Hm,Wm) -- X-Trans: the whole 6x6 cells, as the write-back; needs wb and ccm.
    linear      with srgb_size='full', also 'linear': float32 (N,3,Hm,Wm) linear RGB after the colour matrix (no clamp, no tone curve).
    defects     a DefectMap (eld_amd.defects) or the path of a saved one: the flagged sites of the input codes are repaired (the lower
                median of their unflagged same-colour neighbours) in one pass before the input stage -- the ratio would turn a warm pixel
                into a saturated dot.  X-Trans: the borders outside whole cells, which pass through to the output mosaic, are repaired
                too.  None (default): the codes are used as they are.
    shading, iso  a DarkShading (eld_amd.shading) or the path of a saved one, and the ISO the frames were shot at: after the defect
                repair the input stage subtracts the sensor's fixed pattern a + b * (iso - x0) in float32, fused into the pack
                (eld_pack_raw_*_u16_shaded) -- the ratio would otherwise multiply it into visible columns and blotches.  The write-back is
                unchanged: the network's output estimates the clean signal above the nominal black level.  shading without iso, a map
                of another shape, CFA or Bayer pattern, or an ISO outside the map's range is a ValueError.
    flatfield, lens  a FlatField (eld_amd.flatfield) or the path of a saved one.  The network input is multiplied by its PRNU plane only,
                fused into the input stage (eld_pack_raw_*_u16_flat): lens gain in front of the network would raise the corners' noise
                above what the noise model trained it on.  The lens plane multiplies the network's OUTPUT, before the clip the output
                stages apply: lens='srgb' (default) in the sRGB rendering only -- the mosaic written back stays a raw frame a converter
                may still lens-correct; 'all' in the write-back too; 'off' nowhere.  'packed' is the network's own output in every mode.

    warp        an eld_amd.dng_opcodes.Warp (a DNG WarpRectilinear: lens distortion and lateral chromatic aberration), with srgb_size='full'
                only: the demosaiced camera RGB is resampled by it before the colour matrix and the tone curve (eld_amd.isp.warp_rgb), in
                'srgb' and in 'linear'.  The mosaic written back is not warped: it stays a raw frame.

    jpeg        None (default), or a dict with any of quality (1..100, default 90) and subsampling ('444' / '420', default '420'): the sRGB
                rendering is also encoded as baseline JPEG on the device, before its copy to the host (eld_amd.jpeg.encode_jpeg), and the
                result gains 'jpeg': a list of bytes, one file per frame.  It needs the sRGB output (wb and ccm) and not linear=True.

    demosaic    'mhc' (default): the full-resolution render demosaics with its CFA's default (Bayer: Malvar-He-Cutler).  'edge': with the edge-directed demosaic
                (eld_amd.isp.render_bayer(..., demosaic='edge')), which keeps fine oriented detail free of zipper; Bayer and
                srgb_size='full' only.  'directional': the full-resolution X-Trans render demosaics with the directional demosaic
                (eld_amd.isp.render_xtrans(..., demosaic='directional')) in place of the isotropic normalised convolution;
                X-Trans and srgb_size='full' only.  warp, linear and jpeg take either's output as they take the default's.

    frame       an eld_amd.isp.Frame (crop, upright size, TIFF orientation, resampling filter), with srgb_size='full' only: the demosaiced
                camera RGB (after the warp, when there is one) is cropped, resampled in linear light and turned by it before the colour
                matrix and the tone curve (eld_amd.isp.frame_rgb).  It applies to 'srgb', to 'linear' and to what jpeg
                encodes, which then have the frame's upright shape.  The mosaic written back and 'packed' are untouched.
    preview_frame  a second Frame, with jpeg only: the result gains 'preview', a list of JPEG files of the sRGB rendering framed by it
                instead (a small preview beside the full picture, or an unturned one for a DNG whose Orientation tag does the turning),
                encoded with jpeg's quality and subsampling.

    Returns {'packed': (N,C,h,w) float32 network output, 'mosaic': codes of the input's shape, type and device, 'srgb': (N,3,h,w)
    uint8 or None}; NumPy in -> NumPy out, CUDA tensor in -> CUDA tensors out.  Bad arguments raise ValueError before any device work."""
    _check_cfa(cfa)
    if getattr(denoiser, 'cfa', cfa) != cfa:
        raise ValueError('the denoiser was loaded for cfa=%r, called with %r' % (denoiser.cfa, cfa))
    if rounding not in ROUNDING:
        raise ValueError('rounding must be one of %r, got %r' % (ROUNDING, rounding))
    if chop not in (None, True, False):
        raise ValueError('chop must be None, True or False, got %r' % (chop,))
    if not isinstance(srgb_size, str) or srgb_size not in SRGB_SIZES:
        raise ValueError('srgb_size must be one of %r, got %r' % (SRGB_SIZES, srgb_size))
    if srgb_size == 'full' and (wb is None or ccm is None):
        raise ValueError("srgb_size='full' renders sRGB: it needs both wb and ccm")
    if linear and srgb_size != 'full':
        raise ValueError("linear=True needs srgb_size='full'")
    check_demosaic(demosaic, cfa, srgb_size)
    if warp is not None:
        from .dng_opcodes import Warp
        if not isinstance(warp, Warp):
            raise ValueError('warp must be an eld_amd.dng_opcodes.Warp, got %r' % (type(warp).__name__,))
        if srgb_size != 'full':
            raise ValueError("warp resamples the full-resolution render: it needs srgb_size='full'")
    if jpeg is not None:
        from .jpeg import _check_args as check_jpeg_args
        if not isinstance(jpeg, dict) or set(jpeg) - {'quality', 'subsampling'}:
            raise ValueError('jpeg must be None or a dict with the keys quality and subsampling, got %r' % (jpeg,))
        check_jpeg_args(jpeg.get('quality', 90), jpeg.get('subsampling', '420'), 0, 0)
        if wb is None or ccm is None:
            raise ValueError('jpeg encodes the sRGB rendering: it needs both wb and ccm')
        if linear:
            raise ValueError('jpeg encodes the uint8 sRGB rendering: it does not go with linear=True')
    for name, f in (('frame', frame), ('preview_frame', preview_frame)):
        if f is None:
            continue
        if not isinstance(f, Frame):
            raise ValueError('%s must be an eld_amd.isp.Frame, got %r' % (name, type(f).__name__))
        if srgb_size != 'full':
            raise ValueError("%s frames the full-resolution render: it needs srgb_size='full'" % name)
    if preview_frame is not None and jpeg is None:
        raise ValueError('preview_frame makes a second JPEG: it needs jpeg (a dict, possibly empty)')
    kind, batched = _as_u16(mosaic_u16)
    shape = tuple(mosaic_u16.shape)
    N = shape[0] if batched else 1
    Hm, Wm = shape[-2:]
    if N < 1:
        raise ValueError('empty batch')
    _check_sides(Hm, Wm, cfa)
    for f in (frame, preview_frame):                                  # the render's rectangle: X-Trans renders whole 6 x 6 cells
        if f is not None:
            f.taps(*((Hm // 6 * 6, Wm // 6 * 6) if cfa == 'xtrans' else (Hm, Wm)))
    pat, blk, white = _levels(cfa, raw_pattern, black_level, white_point)
    ratios = _ratios(ratio, N)
    if denoiser.in_channels != PLANES[cfa]:
        raise ValueError('the network takes %d input planes, a %s frame packs to %d' % (denoiser.in_channels, cfa, PLANES[cfa]))
    if denoiser.out_channels != PLANES[cfa]:
        raise ValueError('the network writes %d planes, the %s write-back needs %d' % (denoiser.out_channels, cfa, PLANES[cfa]))
    wbs, ccms = _colour(cfa, wb, ccm, N)
    if defects is not None:
        defects = as_defect_map(defects)
        defects.check_frames((Hm, Wm), cfa, 'denoise_raw')
    tval = None
    if shading is not None:
        shading = as_dark_shading(shading)
        if iso is None:
            raise ValueError('shading needs iso: the ISO the frames were shot at')
        shading.check_frames((Hm, Wm), cfa, 'denoise_raw')
        shading.check_pattern(None if cfa == 'xtrans' else np.asarray(pat).reshape(2, 2), 'denoise_raw')
        tval = shading.t(iso)
    elif iso is not None:
        raise ValueError('iso is the abscissa of a dark-shading map: pass shading= with it')
    if not isinstance(lens, str) or lens not in LENS_MODES:
        raise ValueError('lens must be one of %r, got %r' % (LENS_MODES, lens))
    if flatfield is not None:
        flatfield = as_flat_field(flatfield)
        flatfield.check_frames((Hm, Wm), cfa, 'denoise_raw')
        flatfield.check_pattern(None if cfa == 'xtrans' else np.asarray(pat).reshape(2, 2), 'denoise_raw')
    if srgb_size == 'full' and cfa == 'bayer' and (pat[0] & 1) != (pat[3] & 1):
        raise ValueError('the full-size render needs a Bayer raw_pattern with its greens on a diagonal, got %r' % (raw_pattern,))

    import torch
    classical = getattr(denoiser, 'is_classical', False)          # eld_amd.classical.ClassicalDenoiser: no network, so no device of its own
    if classical:
        dev = mosaic_u16.device if kind == 'torch' else torch.device('cuda', torch.cuda.current_device())
    else:
        dev = next(denoiser.net.parameters()).device
    if dev.type != 'cuda':
        raise ValueError('the denoiser must live on a CUDA device (load_denoiser(..., device=...)), it is on %s' % dev)
    if kind == 'numpy':
        t = torch.from_numpy(np.ascontiguousarray(mosaic_u16).view(np.int16)).to(dev)
    else:
        t = mosaic_u16.contiguous()
        if t.device != dev:
            raise ValueError('the mosaic is on %s, the denoiser on %s' % (t.device, dev))
    t3 = t if batched else t.unsqueeze(0)
    if defects is not None:
        t3 = repair_device(t3, defects)
    if classical:                                                 # the sensor's codes, not the clipped input; chop has no meaning here
        with torch.cuda.device(dev):
            net_out = out = denoiser.denoise_codes(t3, pat, blk, white, ratios, shading, tval, flatfield)
    else:
        if flatfield is None:
            x = pack_input(t3, cfa, pat, blk, white, ratios, shading, tval)
        else:
            x = pack_input(t3, cfa, pat, blk, white, ratios, shading, tval, flatfield)
        net_out = out = run_network(denoiser, x, chop)
    mosaic = t3.clone()                   # X-Trans: the borders outside whole cells keep the input's codes
    if flatfield is not None and lens != 'off':
        out = net_out * flatfield.packed_lens(dev)             # what the sRGB stages below render; they and the write-back clip after it
        write_back(out if lens == 'all' else net_out, mosaic, cfa, pat, blk, white, rounding)
    else:
        write_back(out, mosaic, cfa, pat, blk, white, rounding)
    srgb = lin = preview = None
    if wbs is not None and srgb_size == 'full':
        wt, ct = torch.from_numpy(wbs).to(dev), torch.from_numpy(ccms).to(dev)
        if cfa == 'bayer':
            render = lambda c, **kw: render_bayer(out, pat, wt, c, demosaic=demosaic, **kw)
        else:
            render = lambda c, **kw: render_xtrans(out, wt, c, demosaic=demosaic, **kw)
        if warp is None and frame is None and preview_frame is None:
            srgb = render(ct, CRF=CRF)
            lin = render(ct, linear=True) if linear else None
        else:                                                     # one demosaic to camera RGB, resampled once per output
            cam = render(None, linear=True)
            if frame is not None or preview_frame is not None:    # the frames take the warped camera RGB
                warped = cam if warp is None else warp_rgb(cam, warp, None, linear=True)
            if frame is not None:
                srgb = frame_rgb(warped, frame, ct, CRF=CRF)
                lin = frame_rgb(warped, frame, ct, linear=True) if linear else None
            elif warp is not None:
                srgb = warp_rgb(cam, warp, ct, CRF=CRF)
                lin = warp_rgb(cam, warp, ct, linear=True) if linear else None
            else:                                                 # only the preview is framed
                srgb = render(ct, CRF=CRF)
                lin = render(ct, linear=True) if linear else None
            if preview_frame is not None:
                preview = frame_rgb(warped, preview_frame, ct, CRF=CRF)
    elif wbs is not None:
        fn = process if cfa == 'bayer' else process_xtrans
        rgb = fn(out, torch.from_numpy(wbs).to(dev), torch.from_numpy(ccms).to(dev), CRF=CRF)
        srgb = torch.round(rgb * 255.0).to(torch.uint8)          # k/255 -> k exactly
    files = previews = None
    if jpeg is not None:                                          # on the device, before the rendering's copy to the host
        from .jpeg import encode_jpeg
        with torch.cuda.device(dev):
            files = encode_jpeg(srgb, **jpeg)
            previews = None if preview is None else encode_jpeg(preview, **jpeg)
    if not batched:
        mosaic = mosaic[0]
    if kind == 'numpy':
        res = {'packed': net_out.cpu().numpy(), 'mosaic': mosaic.cpu().numpy().view(np.uint16),
               'srgb': None if srgb is None else srgb.cpu().numpy()}
        if lin is not None:
            res['linear'] = lin.cpu().numpy()
    else:
        res = {'packed': net_out, 'mosaic': mosaic, 'srgb': srgb}
        if lin is not None:
            res['linear'] = lin
    if files is not None:
        res['jpeg'] = files
        if previews is not None:
            res['preview'] = previews
    return res


# ---- command line -------------------------------------------------------------------------------------------------------------
SIDECAR_ALIASES = {'black_level_per_channel': 'black_level', 'white_level': 'white_point', 'camera_whitebalance': 'wb',
                   'rgb_camera_matrix': 'ccm', 'black': 'black_level', 'white': 'white_point'}
SIDECAR_KEYS = ('cfa', 'raw_pattern', 'black_level', 'white_point', 'ratio', 'wb', 'ccm', 'precision', 'rounding', 'chop', 'srgb_size', 'defects',
                'shading', 'iso', 'flatfield', 'lens', 'warp', 'demosaic', 'crop', 'orient', 'size', 'resample', 'dng_preview_size')


def read_sidecar(path):
    """JSON with denoise_raw's keys, or the names rawpy reports (raw_pattern, black_level_per_channel, white_level, camera_whitebalance,
    rgb_camera_matrix -- a 3x4 / 4x4 matrix is cut to [:3, :3])."""
    with open(path) as fh:
        d = json.load(fh)
    return sidecar_from_dict(d, path)


def sidecar_from_dict(d, path):
    """read_sidecar on an object already parsed from `path` (eld_amd.evaluate's manifest carries the same fields beside its pairs)."""
    if not isinstance(d, dict):
        raise ValueError('%s: the sidecar must be a JSON object' % path)
    out = {}
    for k, v in d.items():
        k = SIDECAR_ALIASES.get(k, k)
        if (k in ('defects', 'shading', 'flatfield') or (k == 'warp' and v != 'opcodes')) and isinstance(v, str):
            v = os.path.join(os.path.dirname(os.path.abspath(path)), v)      # a saved defect / dark-shading / flat-field map or a warp file, relative to the sidecar
        if k not in SIDECAR_KEYS:
            raise ValueError('%s: unknown key %r (known: %s)' % (path, k, ', '.join(SIDECAR_KEYS + tuple(SIDECAR_ALIASES))))
        if k == 'ccm':
            m = np.asarray(v, dtype=np.float64)
            if m.ndim == 2 and m.shape[0] >= 3 and m.shape[1] >= 3:
                m = m[:3, :3]
            v = m.reshape(-1).tolist()
        out[k] = v
    return out


def build_parser():
    p = argparse.ArgumentParser(prog='python -m eld_amd.denoise', description='Denoise uint16 raw mosaics (.npy) with a trained ELD U-Net.')
    p.add_argument('inputs', nargs='+', help='uint16 mosaics (.npy, raw_image_visible) or DNG files (.dng; their tags fill what is not given)')
    p.add_argument('-o', '--out', required=True, help='output directory')
    p.add_argument('--ckpt', required=True, help='checkpoint (.pt): the reference dict {"netG": ...} or a U-Net state_dict')
    p.add_argument('--meta', help='JSON sidecar: cfa, raw_pattern, black_level, white_point, ratio, wb, ccm (or rawpy names)')
    p.add_argument('--cfa', choices=sorted(PLANES))
    p.add_argument('--raw-pattern', type=int, nargs=4, metavar='CODE', help='Bayer 2x2 raw_pattern, row-major')
    p.add_argument('--black', type=float, nargs='+', help='black level(s): 1 or 4 (Bayer), 1 (X-Trans)')
    p.add_argument('--white', type=float, help='white point (default 16383)')
    p.add_argument('--ratio', type=float, help='exposure ratio (default 1)')
    p.add_argument('--wb', type=float, nargs='+', help='white balance: R G B, or the 4 camera_whitebalance values')
    p.add_argument('--ccm', type=float, nargs=9, help='3x3 camera -> sRGB matrix, row-major')
    p.add_argument('--bf16', action='store_true', help='run the network in bf16')
    p.add_argument('--chop', choices=('auto', 'on', 'off'), help='forward_chop tiles (default auto)')
    p.add_argument('--rounding', choices=ROUNDING, help="write-back rounding (default 'nearest')")
    p.add_argument('--defects', metavar='PATH', help='a defect map written by eld_amd.defects (.npz): its sites are repaired before the network')
    p.add_argument('--shading', metavar='FILE', help='a dark-shading map written by eld_amd.shading (.npz): subtracted in the input stage; needs --iso')
    p.add_argument('--iso', type=float, help='the ISO the frames were shot at (the abscissa of --shading)')
    p.add_argument('--flatfield', metavar='FILE', help='a flat-field map written by eld_amd.flatfield (.npz): PRNU in the input stage, lens gain on the output')
    p.add_argument('--lens', choices=LENS_MODES, help="where the lens plane of --flatfield applies: the sRGB rendering ('srgb', the default), the written-back mosaic too ('all'), nowhere ('off')")
    p.add_argument('--opcodes', choices=('ignore', 'apply'), default='ignore',
                   help="the OpcodeList tags of .dng inputs: 'ignore' (the default), or 'apply': list 1's bad pixels join --defects, the gain "
                        'opcodes of lists 2 and 3 become the lens plane --lens places (not together with --flatfield)')
    p.add_argument('--warp', metavar='opcodes|FILE.json',
                   help="with --srgb-size full: resample the demosaiced picture by a DNG WarpRectilinear (lens distortion, lateral CA) before the colour "
                        "matrix: 'opcodes' takes the one in OpcodeList3 of each .dng input, FILE.json holds {\"sets\": [[kr0, kr1, kr2, kr3, kt0, kt1], ...], "
                        '"cx": ..., "cy": ...} with one set or three (R, G, B).  The written-back mosaic and --dng stay unwarped raw frames')
    p.add_argument('--crop', metavar='default|Y0,X0,H,W',
                   help="with --srgb-size full: render this rectangle of the demosaiced picture only (pixel-edge coordinates, fractions allowed); "
                        "'default' takes DefaultCropOrigin / DefaultCropSize of each .dng input.  The written-back mosaic and --dng keep the whole frame")
    p.add_argument('--orient', metavar='auto|1..8',
                   help="with --srgb-size full: turn the rendered picture upright by this TIFF Orientation; 'auto' takes the Orientation tag of each .dng input")
    p.add_argument('--size', metavar='N|HxW', help='with --srgb-size full: resample the rendered picture to a long edge of N pixels (aspect kept) or to H x W, in linear light')
    p.add_argument('--resample', choices=FRAME_FILTERS, help="the filter of --size and of a fractional --crop: 'area' (default) or 'lanczos'")
    p.add_argument('--dng-preview-size', type=int, metavar='N', help='of --dng-preview: the long edge of the preview (default: the size of the cropped picture)')
    p.add_argument('--dng', action='store_true', help='also write <name>_denoised.dng (uncompressed 16-bit unless --dng-compression says otherwise; the tags of a .dng input are copied)')
    p.add_argument('--dng-compression', choices=('none', 'ljpeg'), default='none', help="of --dng: 'none' (uncompressed strips, the default) or 'ljpeg' (lossless-JPEG tiles, encoded on the device)")
    p.add_argument('--dng-preview', action='store_true', help='of --dng: the sRGB rendering, encoded as JPEG on the device (the settings of --jpeg, or its defaults), becomes the preview in IFD0 and the mosaic moves to a SubIFD')
    p.add_argument('--jpeg', type=int, nargs='?', const=90, metavar='Q', help='also write <name>_srgb.jpg: the sRGB rendering as baseline JPEG of quality Q (1..100, default 90), encoded on the device')
    p.add_argument('--jpeg-subsampling', choices=('444', '420'), help="chroma subsampling of --jpeg and --dng-preview (default '420')")
    p.add_argument('--srgb-size', choices=SRGB_SIZES, help="sRGB at packed resolution (default) or demosaiced at mosaic resolution ('full')")
    p.add_argument('--demosaic', choices=DEMOSAICS, help="of --srgb-size full: the CFA's default ('mhc': Bayer Malvar-He-Cutler, X-Trans normalised convolution), the edge-directed demosaic ('edge', Bayer only) or the directional one ('directional', X-Trans only)")
    return p


def parse_args(argv):
    """-> (inputs, outdir, ckpt, options for load_denoiser / denoise_raw).  Command-line values override the sidecar's."""
    return options_from(build_parser().parse_args(argv))


def options_from(a):
    """parse_args on a namespace already parsed by build_parser() or a parser that extends it (eld_amd.classical)."""
    o = read_sidecar(a.meta) if a.meta else {}
    cli = {'cfa': a.cfa, 'raw_pattern': a.raw_pattern, 'black_level': a.black, 'white_point': a.white, 'ratio': a.ratio, 'wb': a.wb,
           'ccm': a.ccm, 'rounding': a.rounding, 'srgb_size': a.srgb_size, 'defects': a.defects, 'shading': a.shading, 'iso': a.iso, 'flatfield': a.flatfield, 'lens': a.lens, 'warp': getattr(a, 'warp', None), 'demosaic': getattr(a, 'demosaic', None), 'crop': getattr(a, 'crop', None), 'orient': getattr(a, 'orient', None), 'size': getattr(a, 'size', None), 'resample': getattr(a, 'resample', None), 'dng_preview_size': getattr(a, 'dng_preview_size', None), 'precision': 'bf16' if a.bf16 else None,
           'chop': None if a.chop is None else {'auto': 'auto', 'on': True, 'off': False}[a.chop]}
    o.update({k: v for k, v in cli.items() if v is not None})
    # below the command line and the sidecar, above the defaults: the tags of the first .dng input (all .dng inputs must agree on the sensor keys)
    from .dng import fill_from_tags
    tags = fill_from_tags(o, getattr(a, 'inputs', None) or [])
    if tags is not None:
        if o.get('wb') is None and o.get('ccm') is None and tags.get('wb') is not None and tags.get('ccm') is not None:
            o['wb'], o['ccm'] = tags['wb'], tags['ccm']
        if o.get('shading') is not None and o.get('iso') is None and tags.get('iso') is not None:
            o['iso'] = tags['iso']
    if getattr(a, 'dng', False):
        o['dng'] = True
    if getattr(a, 'dng_compression', 'none') != 'none':
        if not o.get('dng'):
            raise ValueError('--dng-compression goes with --dng')
        o['dng_compression'] = a.dng_compression
    if getattr(a, 'dng_preview', False):
        if not o.get('dng'):
            raise ValueError('--dng-preview goes with --dng')
        o['dng_preview'] = True
    if getattr(a, 'jpeg', None) is not None:
        o['jpeg_out'] = True
    if o.get('jpeg_out') or o.get('dng_preview'):
        from .jpeg import _check_args as check_jpeg_args
        o['jpeg'] = {'quality': 90 if getattr(a, 'jpeg', None) is None else a.jpeg, 'subsampling': getattr(a, 'jpeg_subsampling', None) or '420'}
        check_jpeg_args(o['jpeg']['quality'], o['jpeg']['subsampling'], 0, 0)
        if o.get('wb') is None or o.get('ccm') is None:
            raise ValueError('--jpeg and --dng-preview encode the sRGB rendering: they need --wb and --ccm')
    elif getattr(a, 'jpeg_subsampling', None) is not None:
        raise ValueError('--jpeg-subsampling goes with --jpeg or --dng-preview')
    o.setdefault('cfa', 'bayer')
    o.setdefault('white_point', 16383)
    o.setdefault('ratio', 1.0)
    o.setdefault('precision', 'fp32')
    o.setdefault('rounding', 'nearest')
    o.setdefault('srgb_size', 'packed')
    if o['srgb_size'] not in SRGB_SIZES:
        raise ValueError('srgb_size must be one of %r, got %r' % (SRGB_SIZES, o['srgb_size']))
    if o.get('chop') == 'auto':
        o['chop'] = None
    _check_cfa(o['cfa'])
    if o.get('demosaic') is not None:
        check_demosaic(o['demosaic'], o['cfa'], o['srgb_size'])
    if o.get('raw_pattern') is not None:
        o['raw_pattern'] = np.asarray(o['raw_pattern']).reshape(2, 2).tolist()
    if o.get('black_level') is not None:
        b = np.asarray(o['black_level'], dtype=np.float64).reshape(-1)
        o['black_level'] = b.tolist() if b.size > 1 else float(b[0])
    if o.get('ccm') is not None:
        o['ccm'] = np.asarray(o['ccm'], dtype=np.float64).reshape(3, 3).tolist()
    if (o.get('wb') is None) != (o.get('ccm') is None):
        raise ValueError('the sRGB output needs both --wb and --ccm')
    if o['srgb_size'] == 'full' and o.get('wb') is None:
        raise ValueError('--srgb-size full needs --wb and --ccm')
    if o.get('shading') is not None and o.get('iso') is None:
        raise ValueError('--shading needs --iso')
    if o.get('lens') is not None and o['lens'] not in LENS_MODES:
        raise ValueError('lens must be one of %r, got %r' % (LENS_MODES, o['lens']))
    if getattr(a, 'opcodes', 'ignore') == 'apply':
        o['opcodes'] = 'apply'
        if o.get('flatfield') is not None:
            raise ValueError('--opcodes apply together with --flatfield would correct the lens twice: give one of them')
    if o.get('lens') is not None and o.get('flatfield') is None and o.get('opcodes') != 'apply':
        raise ValueError('--lens needs --flatfield')
    if o.get('warp') is not None:
        if o['srgb_size'] != 'full':
            raise ValueError('--warp resamples the full-resolution render: it needs --srgb-size full')
        if o['warp'] == 'opcodes':
            from .dng import is_dng
            for path in getattr(a, 'inputs', None) or []:
                if not is_dng(path):
                    raise ValueError("%s: --warp opcodes reads OpcodeList3 of .dng inputs (a .json file gives a warp to any input)" % path)
        elif not isinstance(o['warp'], str):
            raise ValueError("warp must be 'opcodes' or the path of a .json file, got %r" % (o['warp'],))
    check_frame_options(o, getattr(a, 'inputs', None) or [])
    return a.inputs, a.out, a.ckpt, o


FRAME_OPTIONS = (('crop', '--crop'), ('orient', '--orient'), ('size', '--size'), ('resample', '--resample'), ('dng_preview_size', '--dng-preview-size'))


def check_frame_options(o, inputs):
    """The frame's options (command line or sidecar) parsed in place: crop -> 'default' or (y0, x0, h, w) floats; orient -> 'auto' or 1 .. 8; size ->
    an int or (H, W); every ValueError they can raise without reading a pixel."""
    from .dng import is_dng
    for key, flag in FRAME_OPTIONS:
        if o.get(key) is not None and o['srgb_size'] != 'full':
            raise ValueError('%s frames the full-resolution render: it needs --srgb-size full' % flag)
    v = o.get('crop')
    if v is not None and v != 'default':
        try:
            v = tuple(float(x) for x in (v.split(',') if isinstance(v, str) else v))
            Frame(crop=v)
        except (TypeError, ValueError):
            raise ValueError("--crop takes 'default' or Y0,X0,H,W with Y0, X0 >= 0 and H, W > 0, got %r" % (o['crop'],))
        o['crop'] = v
    v = o.get('orient')
    if v is not None and v != 'auto':
        try:
            v = int(v)
            Frame(orientation=v)
        except (TypeError, ValueError):
            raise ValueError("--orient takes 'auto' or a TIFF Orientation 1 .. 8, got %r" % (o['orient'],))
        o['orient'] = v
    v = o.get('size')
    if v is not None:
        try:
            if isinstance(v, str):
                v = tuple(int(x) for x in v.lower().split('x')) if 'x' in v.lower() else int(v)
            elif not isinstance(v, int):
                v = tuple(int(x) for x in v)
            Frame(size=v)
        except (TypeError, ValueError):
            raise ValueError('--size takes a long edge N >= 1 or HxW, got %r' % (o['size'],))
        o['size'] = v
    if o.get('resample') is not None and o['resample'] not in FRAME_FILTERS:
        raise ValueError('resample must be one of %r, got %r' % (FRAME_FILTERS, o['resample']))
    v = o.get('dng_preview_size')
    if v is not None:
        if not o.get('dng_preview'):
            raise ValueError('--dng-preview-size goes with --dng-preview')
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError('--dng-preview-size takes a long edge N >= 1, got %r' % (v,))
    for key, word, flag in (('crop', 'default', '--crop default reads DefaultCropOrigin / DefaultCropSize'), ('orient', 'auto', '--orient auto reads the Orientation tag')):
        if o.get(key) == word:
            for path in inputs:
                if not is_dng(path):
                    raise ValueError('%s: %s of .dng inputs' % (path, flag))


def frame_option(path, raw, o):
    """The frame's options for one input -> (Frame or None for the sRGB outputs, Frame or None for the DNG preview).  The render's rectangle is the
    visible mosaic (X-Trans: its whole 6 x 6 cells); a crop is intersected with it, with a line when that clips it, and an empty
    intersection is a ValueError.  The DNG preview takes the same crop, --dng-preview-size and orientation 1: the DNG's Orientation tag turns
    the preview as it turns the raw image."""
    if all(o.get(k) is None for k, _ in FRAME_OPTIONS):
        return None, None
    Hm, Wm = (int(v) for v in raw.shape[-2:])
    if o['cfa'] == 'xtrans':
        Hm, Wm = Hm // 6 * 6, Wm // 6 * 6
    crop, orient = o.get('crop'), o.get('orient') or 1
    if crop == 'default' or orient == 'auto':
        from .dng import dng_meta
        meta = dng_meta(path)
        if crop == 'default':
            crop = meta.get('default_crop')
            if crop is None:
                print('%s: no DefaultCropSize: --crop default changes nothing for this file' % path)
        if orient == 'auto':
            orient = meta.get('orientation', 1)
    if crop is not None:
        y0, x0, ch, cw = (float(v) for v in crop)
        y1, x1 = min(y0 + ch, float(Hm)), min(x0 + cw, float(Wm))
        if y1 <= y0 or x1 <= x0:
            raise ValueError('%s: the crop (y0, x0, h, w) = %r lies outside the %d x %d picture' % (path, tuple(crop), Hm, Wm))
        if (y1 - y0, x1 - x0) != (ch, cw):
            print('%s: the crop %r is clipped to the %d x %d picture: (%g, %g, %g, %g)' % (path, tuple(crop), Hm, Wm, y0, x0, y1 - y0, x1 - x0))
        crop = (y0, x0, y1 - y0, x1 - x0)
    flt = o.get('resample') or 'area'
    frame = Frame(crop, orient, o.get('size'), flt)
    preview = None
    if o.get('dng_preview') and (orient != 1 or o.get('size') is not None or o.get('dng_preview_size') is not None):
        preview = Frame(crop, 1, o.get('dng_preview_size'), flt)
    return (None if frame.identity else frame), preview


def save_png(path, hwc):
    try:
        from PIL import Image
    except ImportError:
        return False
    Image.fromarray(hwc).save(path)
    return True


def main(argv=None):
    inputs, outdir, ckpt, o = parse_args(sys.argv[1:] if argv is None else argv)
    den = load_denoiser(ckpt, cfa=o['cfa'], precision=o['precision'])
    return run_frames(den, inputs, outdir, o)


def opcode_options(path, raw, kw, o):
    """--opcodes apply for one .dng input: denoise_raw's keywords with the file's own corrections in them, and the opcode tags --dng carries
    into the written file.  List 1's bad pixels are OR-ed into the --defects map; the gain opcodes of lists 2 and 3 become a FlatField whose
    lens plane goes where --flatfield's would, under --lens (default 'srgb').  A list-2 opcode that is no gain (MapTable, MapPolynomial,
    DeltaPerRow, DeltaPerColumn) would change the network's input and is not applied there: mandatory, it is a ValueError that names it.
    Carried: lists 2 and 3 as the source has them -- with lens='all', where the gains are already in the written mosaic, without their gain
    opcodes; never list 1 (its pixels are repaired, and the written mosaic is the active area only)."""
    from . import dng_opcodes as O
    from .dng import dng_meta, is_dng
    if not is_dng(path):
        raise ValueError('%s: --opcodes apply reads the opcode lists of .dng inputs' % path)
    lists, meta = O.read_opcodes(path), dng_meta(path)
    Hm, Wm = (int(v) for v in raw.shape[-2:])
    kw = dict(kw)
    dmap = O.defects_from_opcodes(lists[0], raw, meta, lists.linearization)
    if dmap.count:
        kw['defects'] = O.merge_defects(kw.get('defects'), dmap)
    for i, op in enumerate(lists[1]):
        if O.disposition(op, 2) == 'apply' and op.id in O.NOT_GAIN_IDS_2:
            if not op.optional:
                raise ValueError('%s: OpcodeList2[%d] %s is mandatory and changes the pixel values in front of the network: it is not applied '
                                 'there (python -m eld_amd.dng --opcodes apply --linear-out applies it)' % (path, i, op.name))
            print('%s: OpcodeList2[%d] %s skipped because optional' % (path, i, op.name))
    lens = o.get('lens') or 'srgb'
    prog = O.gain_program(lists[1], lists[2], Hm, Wm)
    if len(prog):
        pattern = o.get('raw_pattern') if o['cfa'] == 'bayer' else meta['raw_pattern']
        kw['flatfield'] = O.lens_from_opcodes(lists[1], lists[2], Hm, Wm, o['cfa'], pattern, min(int(o['white_point']), 65535))
        kw['lens'] = lens
    carried = {}
    for no, name in ((2, 'OpcodeList2'), (3, 'OpcodeList3')):
        if name not in lists.raw:
            continue
        if lens == 'all':
            rest = O.without_gains(lists[no - 1], no)
            if rest:
                carried[name] = O.pack_opcode_list(rest)
        else:
            carried[name] = lists.raw[name]
    return kw, carried


def read_warp(path):
    """A warp file: JSON {"sets": [[kr0, kr1, kr2, kr3, kt0, kt1], ...] (one set or three: R, G, B), "cx": ..., "cy": ...} -> Warp."""
    from .dng_opcodes import Warp
    with open(path) as fh:
        d = json.load(fh)
    if not isinstance(d, dict) or set(d) != {'sets', 'cx', 'cy'}:
        raise ValueError('%s: a warp file is a JSON object with the keys sets, cx, cy' % path)
    try:
        return Warp(d['sets'], d['cx'], d['cy'])
    except (TypeError, ValueError) as e:
        raise ValueError('%s: %s' % (path, e))


def warp_option(path, raw, o, carried):
    """--warp for one input -> (Warp or None, the opcode tags --dng carries).  'opcodes': list 3's WarpRectilinear of the .dng input (None, with a
    line saying so, when the list has none); the written mosaic is not warped, so --dng carries the source's lists 2 and 3 -- as --opcodes apply
    already decided them when it is given too."""
    if o['warp'] != 'opcodes':
        return read_warp(o['warp']), carried
    from . import dng_opcodes as O
    lists = O.read_opcodes(path)
    Hm, Wm = (int(v) for v in raw.shape[-2:])
    warp = O.warp_from_opcodes(lists[2], Hm, Wm, '%s: OpcodeList3' % path)
    if warp is None:
        print('%s: OpcodeList3 holds no WarpRectilinear: --warp opcodes changes nothing for this file' % path)
    if carried is None:
        carried = {name: lists.raw[name] for name in ('OpcodeList2', 'OpcodeList3') if name in lists.raw}
    return warp, carried


def run_frames(den, inputs, outdir, o):
    """The command line's loop: denoise every input with `den` (a Denoiser or a ClassicalDenoiser) under the options `o`, write the outputs."""
    os.makedirs(outdir, exist_ok=True)
    kw = {k: o.get(k) for k in ('raw_pattern', 'black_level', 'white_point', 'ratio', 'wb', 'ccm', 'chop', 'rounding', 'srgb_size')}
    if o.get('defects') is not None:
        kw['defects'] = as_defect_map(o['defects'], '--defects')
    if o.get('shading') is not None:
        kw['shading'], kw['iso'] = as_dark_shading(o['shading'], '--shading'), o['iso']
    if o.get('flatfield') is not None:
        kw['flatfield'], kw['lens'] = as_flat_field(o['flatfield'], '--flatfield'), o.get('lens') or 'srgb'
    if o.get('jpeg') is not None:
        kw['jpeg'] = dict(o['jpeg'])
    if o.get('demosaic') is not None:
        kw['demosaic'] = o['demosaic']
    from .dng import COMPRESSION_CHOICES, is_dng, load_frame, write_dng
    dng_kw = {'compression': COMPRESSION_CHOICES[o.get('dng_compression') or 'none']}
    for path in inputs:
        raw = load_frame(path)
        fkw, carried = kw, None
        if o.get('opcodes') == 'apply':
            fkw, carried = opcode_options(path, raw, kw, o)
        if o.get('warp') is not None:
            warp, carried = warp_option(path, raw, o, carried)
            fkw = dict(fkw, warp=warp)
        frame, preview_frame = frame_option(path, raw, o)
        if frame is not None or preview_frame is not None:
            fkw = dict(fkw, frame=frame, preview_frame=preview_frame)
        res = denoise_raw(den, raw, o['cfa'], **fkw)
        name = os.path.splitext(os.path.basename(path))[0]
        np.save(os.path.join(outdir, name + '_denoised.npy'), res['mosaic'])
        line = '%s -> %s_denoised.npy' % (path, name)
        if o.get('dng'):
            if raw.ndim != 2:
                raise ValueError('%s: --dng writes one frame per file, the input holds a stack of %d' % (path, raw.shape[0]))
            if o.get('dng_preview'):
                dng_kw = dict(dng_kw, preview=(res['preview'] if preview_frame is not None else res['jpeg'])[0])
            if is_dng(path):
                write_dng(os.path.join(outdir, name + '_denoised.dng'), res['mosaic'], like=path, opcodes=carried, **dng_kw)
            else:
                write_dng(os.path.join(outdir, name + '_denoised.dng'), res['mosaic'],
                          meta={k: o.get(k) for k in ('cfa', 'raw_pattern', 'black_level', 'white_point', 'wb', 'ccm', 'iso')}, **dng_kw)
            line += ', %s_denoised.dng' % name
        if res['srgb'] is not None:
            hwc = np.ascontiguousarray(np.moveaxis(res['srgb'], 1, -1))          # (N,h,w,3); one frame: (h,w,3)
            hwc = hwc if raw.ndim == 3 else hwc[0]
            np.save(os.path.join(outdir, name + '_srgb.npy'), hwc)
            line += ', %s_srgb.npy' % name
            if hwc.ndim == 3 and save_png(os.path.join(outdir, name + '_srgb.png'), hwc):
                line += ', %s_srgb.png' % name
            if o.get('jpeg_out'):
                for i, data in enumerate(res['jpeg']):
                    jname = name + ('_srgb.jpg' if raw.ndim == 2 else '_srgb_%d.jpg' % i)
                    with open(os.path.join(outdir, jname), 'wb') as fh:
                        fh.write(data)
                    line += ', %s' % jname
        print(line)
    return 0


if __name__ == '__main__':
    sys.exit(main())
