"""NumPy restatements the denoise tests share: the dataset pack (float32, as the pack kernels evaluate it), the exposure gain, the
write-back to uint16 codes in its three roundings and the X-Trans sRGB binning (on top of oracle/isp_ref.py)."""
import numpy as np

from oracle import isp_ref as I
from oracle import noise_ref as O
from xtrans_ref import PLANE_COLOUR

F32 = np.float32


def bayer_offsets(raw_pattern):
    """colour code k -> (row, col) of the 2x2 cell (np.where(raw_pattern == k))"""
    pat = np.asarray(raw_pattern).reshape(2, 2)
    return [tuple(int(v[0]) for v in np.where(pat == k)) for k in range(4)]


def pack_bayer(u, raw_pattern, black, white):
    """(N,2h,2w) uint16 -> (N,4,h,w) float32: clip((float32(u) - b_k) / (white - b_k), 0, 1)."""
    u = np.asarray(u)
    out = []
    for k, (oy, ox) in enumerate(bayer_offsets(raw_pattern)):
        b = F32(black[k])
        out.append(np.clip((u[:, oy::2, ox::2].astype(F32) - b) / (F32(white) - b), F32(0), F32(1)))
    return np.stack(out, axis=1)


def pack_xtrans(u, black, white):
    """(N,Hm,Wm) uint16 -> (N,9,2*(Hm//6),2*(Wm//6)) float32."""
    u = np.asarray(u)
    h, w = 2 * (u.shape[1] // 6), 2 * (u.shape[2] // 6)
    rows, cols = O.xtrans_source_index(h, w)
    b = F32(black)
    return np.clip((u[:, rows, cols].astype(F32) - b) / (F32(white) - b), F32(0), F32(1))


def gain(p, ratios):
    """The evaluation input stage (dataset/sid_dataset.py:398-409): np.maximum(np.minimum(p * float32(ratio), 1), 0) per image."""
    r = np.asarray(ratios, F32).reshape(-1, 1, 1, 1)
    return np.maximum(np.minimum(p * r, F32(1)), F32(0))


def codes(x, black, white, rounding):
    """The write-back of float32 values x with one (black, white): 'trunc' (the reference's float64 expression + uint16 assignment),
    'nearest' (the same value rounded half to even) or 'trunc_f32' (the reference's X-Trans float32 expression, truncated)."""
    c = np.clip(np.asarray(x, F32), F32(0), F32(1))
    if rounding == 'trunc_f32':
        return (c * F32(white - black) + F32(black)).astype(np.uint16)
    v = c.astype(np.float64) * (float(white) - float(black)) + float(black)
    return (np.rint(v) if rounding == 'nearest' else v).astype(np.uint16)


def unpack_bayer(p, raw_pattern, black, white, rounding):
    """(N,4,h,w) -> (N,2h,2w) uint16 (postprocess_bayer's assignment, models/ELD_model.py:41-70)."""
    N, _, h, w = p.shape
    out = np.zeros((N, 2 * h, 2 * w), np.uint16)
    for k, (oy, ox) in enumerate(bayer_offsets(raw_pattern)):
        out[:, oy::2, ox::2] = codes(p[:, k], black[k], white, rounding)
    return out


def unpack_xtrans(p, mosaic, black, white, rounding):
    """(N,9,h,w) written into a copy of `mosaic` (N,Hm,Wm): the whole 6x6 cells only (postprocess_xtrans, models/ELD_model.py:73-129)."""
    out = np.array(mosaic, dtype=np.uint16, copy=True)
    rows, cols = O.xtrans_source_index(p.shape[2], p.shape[3])
    out[:, rows, cols] = codes(p, black, white, rounding)
    return out


def xtrans_binning(x):
    """(N,9,h,w) clamped planes -> (N,3,h,w): per colour its planes summed in ascending plane order in float32, / plane count."""
    out = []
    for col in range(3):
        planes = [k for k in range(9) if PLANE_COLOUR[k] == col]
        s = x[:, planes[0]]
        for k in planes[1:]:
            s = s + x[:, k]
        out.append(s / F32(len(planes)))
    return np.stack(out, axis=1)


def isp_xtrans(packed, wbs, ccms, gamma=2.2, CRF=None):
    """eld_isp_process_xtrans restated: wbs (N,3), ccms (N,3,3)."""
    packed = np.asarray(packed, F32)
    wb9 = np.asarray(wbs, F32)[:, PLANE_COLOUR]
    x = np.clip(packed * wb9[:, :, None, None], F32(0), F32(1)).astype(F32)
    img = np.clip(I.apply_ccms(xtrans_binning(x), np.asarray(ccms, F32)), 0.0, 1.0).astype(F32)
    if CRF is None:
        return I.gamma_compression(img, gamma)
    return I.camera_response_function(img, CRF[0], CRF[1])
