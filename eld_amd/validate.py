"""Validate a calibrated noise table against the sensor's own frames: does noise synthesised from the table look like the sensor's?

The check of the ELD paper's Table 1, per colour group: the discrete KL divergence between the histogram of real bias frames (and of
the difference of real flat pairs) and the histogram of the sampler's synthesis under each noise model named, next to the divergence of
two synthetic draws from each other (the sampling floor).  It is a test of MARGINAL distributions: the spatial structure of row noise is
seen only through its effect on the marginal.  structure=True (--structure) adds the report of that structure: row, column and
fixed-pattern variance components of the real frames next to those of each model's synthesis (eld_amd/structure.py).

    report = validate_camera(sessions, raw_pattern, black_level, white_level, models=('Pg', 'PG', 'PGR', 'PGRB'))
    report['best']                                  # the model with the lowest mean bias-frame kl
    report['sessions'][0]['frames'][0]['models']['PG']   # {'kl', 'floor', 'kl_groups', 'floor_groups'}

The histograms are exact integer counts built on the device (eld_amd/csrc/hist.hip: eld_hist_u16 for sensor codes, eld_hist_f32 for
sampler output); the binning contract is DESIGN.md sec. 15.  kl_divergence runs in float64 on the host.

Command line: python -m eld_amd.validate manifest.json [--camera TABLE.npy] [--models Pg,PG,PGR,PGRB] [--source frames|table]
[--defects PATH|auto] [--radius N] [--seed S] [--out report.json] [--hist hist.npz] [--structure [--lags L]] (the manifest is calibrate's).
"""
import argparse
import ctypes
import json
import sys

import numpy as np

from . import _lib as L
from . import calibrate as CAL
from . import mosaic as M
from . import structure as ST
from .defects import as_defect_map, check_defects, find_defects
from .noise import NoiseParams, model_flags, table_cfa

MODEL_LETTERS = 'PpgGRUBDC'
DARK_EXCLUDES = 'gGRBC'                           # the terms a dark frame already holds: not next to D
MAX_RADIUS = 32767
XT_PLANE_COLOUR = (0, 1, 2, 0, 2, 1, 1, 1, 1)     # packed X-Trans plane -> colour (R 0, G 1, B 2): planes 0, 3 R; 1, 5-8 G; 2, 4 B
ID_BASE = 1 << 62                                 # validation streams lie far from the sample ids a training run counts up from 0


# ---- argument checks (host only) -------------------------------------------------------------------------------------------------------
def _radius(radius, what='radius'):
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or radius < 1 or radius > MAX_RADIUS:
        raise ValueError('%s must be an integer in [1, %d], got %r' % (what, MAX_RADIUS, radius))
    return int(radius)


def _models(models):
    if isinstance(models, str):
        models = [m for m in models.split(',') if m]
    models = list(models)
    if not models:
        raise ValueError('no noise model named')
    for m in models:
        if not isinstance(m, str) or not m or any(ch not in MODEL_LETTERS for ch in m):
            raise ValueError('unknown noise model %r: the letters are %s' % (m, ', '.join(MODEL_LETTERS)))
        if 'D' in m and any(ch in m for ch in DARK_EXCLUDES):
            raise ValueError("noise model %r: D takes the signal-independent noise from the sensor's dark frames and excludes %s"
                             % (m, ', '.join(DARK_EXCLUDES)))
    if len(set(models)) != len(models):
        raise ValueError('a noise model is named twice: %r' % (models,))
    return models


def group_map_u16(cfa, raw_pattern):
    """-> (period, groups: p*p ints, G).  Bayer: cell (r, c) -> the packed channel raw_pattern[r][c] (R, G1, B, G2), G = 4;
    X-Trans: cell -> the colour (R 0, G 1, B 2) of its colour code, G = 3."""
    lay = M.CfaLayout(cfa, raw_pattern)
    return lay.period, list(lay.group), lay.G


def group_map_f32(cfa):
    """-> (C, groups: C ints, G).  Bayer: plane c -> group c; X-Trans: planes 0, 3 -> R, 1, 5-8 -> G, 2, 4 -> B."""
    if M.check_cfa(cfa) == 'xtrans':
        return 9, list(XT_PLANE_COLOUR), 3
    return 4, [0, 1, 2, 3], 4


def group_black(cfa, black_level):
    """The integer centre of each histogram group: rint(black) of the packed channel (Bayer) or of the colour (X-Trans, whose two green
    codes must share one rounded black level: a group has one centre)."""
    b = np.rint(M.black_levels(black_level)).astype(np.int64)
    if cfa == 'xtrans':
        if b[1] != b[3]:
            raise ValueError('X-Trans: the two green colour codes have black levels %d and %d; a histogram group has one centre' % (b[1], b[3]))
        return b[:3]
    return b


def sample_id(session, frame, model_index, draw):
    """The sampler stream of one synthetic frame: 2^62 + session * 2^40 + frame * 2^8 + model_index * 2 + draw.
    session < 2^20, frame < 2^32 (bias frames count from 0, flat pairs follow them), model_index < 128, draw 0 or 1."""
    session, frame, model_index, draw = int(session), int(frame), int(model_index), int(draw)
    if not (0 <= session < 1 << 20 and 0 <= frame < 1 << 32 and 0 <= model_index < 128 and draw in (0, 1)):
        raise ValueError('sample_id(%d, %d, %d, %d): out of range' % (session, frame, model_index, draw))
    return ID_BASE + (session << 40) + (frame << 8) + (model_index << 1) + draw


# ---- KL divergence (host, float64) -----------------------------------------------------------------------------------------------------
def kl_divergence(p_counts, q_counts, alpha=1.0):
    """Discrete KL(p || q) over the last axis, float64: p = (n + alpha) / (sum n + alpha B), q likewise, sum p log(p / q).
    alpha (additive smoothing) is an interface default that nothing pins: 1.0 is add-one smoothing; report the value with the numbers.
    alpha = 0 uses the raw frequencies (0 log 0 = 0).  ValueError when alpha < 0, when a histogram is empty at alpha = 0, or when
    alpha <= 0 and some q bin is empty where the p bin is not (the divergence is infinite)."""
    p = np.asarray(p_counts, dtype=np.float64)
    q = np.asarray(q_counts, dtype=np.float64)
    if p.shape[-1:] != q.shape[-1:] or p.ndim == 0:
        raise ValueError('histograms must share their last axis, got %s and %s' % (p.shape, q.shape))
    if not (alpha >= 0):
        raise ValueError('alpha must be >= 0, got %r' % (alpha,))
    if np.any(p < 0) or np.any(q < 0):
        raise ValueError('negative counts')
    p, q = np.broadcast_arrays(p, q)
    if alpha <= 0:
        if np.any((q == 0) & (p > 0)):
            raise ValueError('alpha <= 0 and a q bin is empty where the p bin is not: the divergence is infinite')
        if np.any(p.sum(axis=-1) == 0) or np.any(q.sum(axis=-1) == 0):
            raise ValueError('alpha <= 0 and an empty histogram')
    B = p.shape[-1]
    pp = (p + alpha) / (p.sum(axis=-1, keepdims=True) + alpha * B)
    qq = (q + alpha) / (q.sum(axis=-1, keepdims=True) + alpha * B)
    with np.errstate(divide='ignore', invalid='ignore'):
        t = np.where(pp > 0, pp * np.log(pp / qq), 0.0)
    return t.sum(axis=-1)


# ---- histograms (device) ---------------------------------------------------------------------------------------------------------------
def histogram_u16(frames, cfa, raw_pattern, centre, radius, subtract=None, defects=None):
    """Exact histograms of sensor codes.  frames (F,Hm,Wm) uint16 [ndarray or CUDA int16/uint16 tensor] -> int64 ndarray (F, G, 2R+1):
    per colour group (group_map_u16) the counts of clamp(u - centre[g] + R, 0, 2R), or of clamp(u - v + R, 0, 2R) with subtract=v (same
    shape; centre is then ignored and may be None).  defects: a DefectMap whose flagged sites are not counted."""
    R = _radius(radius)
    lay = M.CfaLayout(cfa, raw_pattern)
    p, G = lay.period, lay.G
    F, Hm, Wm = M.check_mosaics(frames, 3, 'frames', None)
    if subtract is not None:
        if M.check_mosaics(subtract, 3, 'subtract', None) != (F, Hm, Wm):
            raise ValueError('subtract has shape %s, the frames %s' % (M.shape_of(subtract), (F, Hm, Wm)))
        cen = None
    else:
        c = np.asarray(centre if centre is not None else [], dtype=np.float64).reshape(-1)
        if c.size != G or not np.all(c == np.rint(c)) or np.any(np.abs(c) > 1 << 30):
            raise ValueError('centre must hold %d integers (one per group), got %r' % (G, centre))
        cen = (ctypes.c_int32 * G)(*[int(v) for v in c])
    if defects is not None:
        defects = check_defects(defects, cfa, (Hm, Wm), raw_pattern if cfa == 'xtrans' else None)
        if isinstance(defects, str):
            raise ValueError("histogram_u16 takes a DefectMap, not 'auto'")
    import torch
    u = M.device_u16(frames)
    v = None if subtract is None else M.device_u16(subtract)
    counts = torch.empty((F, G, 2 * R + 1), dtype=torch.int64, device=u.device)
    bm = None if defects is None else defects.bitmap_on(u.device)
    L.check(L.lib().eld_hist_u16(L.dptr(u), L.dptr(v), F, Hm, Wm, p, lay.c_group(), G, cen, R, L.dptr(bm), L.dptr(counts),
                                 L.cur_stream()), 'eld_hist_u16')
    return counts.cpu().numpy()


def histogram_f32(x, scale, radius, cfa, subtract=None):
    """Exact histograms of sampler output.  x: CUDA float32 (N,C,H,W) (C = 4 Bayer, 9 X-Trans); scale: N floats (or one for all);
    -> int64 ndarray (N, G, 2R+1): per colour group (group_map_f32) the counts of clamp(q(x) + R, 0, 2R), q(t) = rint(float32(t * scale[n]))
    saturated at +-2^29, or of clamp(q(x) - q(x2) + R, 0, 2R) with subtract=x2.  An element whose product is NaN is not counted."""
    R = _radius(radius)
    C, groups, G = group_map_f32(cfa)
    import torch
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4:
        raise ValueError('x must be a CUDA float32 tensor (N, C, H, W)')
    if x.shape[1] != C:
        raise ValueError('cfa=%r input has %d planes, got %d' % (cfa, C, x.shape[1]))
    if subtract is not None and (not isinstance(subtract, torch.Tensor) or not subtract.is_cuda or subtract.dtype != torch.float32
                                 or subtract.shape != x.shape):
        raise ValueError('subtract must be a CUDA float32 tensor of the shape of x')
    N, _, H, W = (int(v) for v in x.shape)
    sc = np.asarray(scale, dtype=np.float32).reshape(-1)
    if sc.size == 1:
        sc = np.repeat(sc, N)
    if sc.size != N:
        raise ValueError('scale must hold one value per image (%d), got %d' % (N, sc.size))
    x = x.contiguous()
    x2 = None if subtract is None else subtract.contiguous()
    scd = torch.from_numpy(np.ascontiguousarray(sc)).to(x.device)
    counts = torch.empty((N, G, 2 * R + 1), dtype=torch.int64, device=x.device)
    L.check(L.lib().eld_hist_f32(L.dptr(x), L.dptr(x2), N, C, H, W, (ctypes.c_int * C)(*groups), G, L.dptr(scd), R, L.dptr(counts),
                                 L.cur_stream()), 'eld_hist_f32')
    return counts.cpu().numpy()


# ---- synthesis -------------------------------------------------------------------------------------------------------------------------
def _noise_params(p, sat):
    """Any parameter record -> the one validation samples with: ratio = 1, saturation = sat, q_step = 1."""
    if isinstance(p, dict):
        p = NoiseParams(p.get('K', 1.0), p.get('g_scale', 0.0), sat, 1.0, p.get('tl_lambda', 0.0), p.get('tl_scale', 0.0), p.get('row_scale', 0.0),
                        1.0, tuple(p.get('color_bias', (0.0,) * 4)), col_scale=p.get('col_scale', 0.0))
    p = NoiseParams.coerce(p)
    cb = tuple(float(v) for v in p.color_bias) + (0.0,) * (4 - len(p.color_bias))
    return NoiseParams(float(p[0]), float(p[1]), float(sat), 1.0, float(p.tl_lambda), float(p.tl_scale), float(p.row_scale), 1.0, cb,
                       col_scale=float(p.col_scale))


def _sample(clean, params, model, cfa, seed, ids, dark=None, dark_table=None):
    """The sampler on clean (N,C,h,w) float32 CUDA with one parameter record and N sample ids -> float32 (N,C,h,w).  dark, dark_table:
    the DarkPool and the frame table of a model with D (sample_noise_records)."""
    from .noise import make_records, sample_noise_records
    return sample_noise_records(clean, make_records([params] * len(ids), ids), model_flags(model, cfa), seed, dark=dark, dark_table=dark_table)


def _leave_one_out(pool, first, count, omit):
    """The frame table of one session without its frame `omit`, on the pool's device -> ((tensor, count - 1), (0, count - 1)): the table
    argument of the sampler and the range a record names in it."""
    import torch
    rows = np.delete(pool.pool.frames[first:first + count], omit)
    return (torch.from_numpy(rows.view(np.uint8).copy()).to(pool.pool.device), len(rows)), (0, len(rows))


def _disjoint_halves(pool, first, count, omit):
    """The leave-one-out frames of one session in two disjoint tables (every other frame each), as _leave_one_out returns them: two draws
    that read one table each never read the same dark frame, whatever the seed.  Needs count >= 3."""
    import torch
    rows = np.delete(pool.pool.frames[first:first + count], omit)
    out = []
    for half in (rows[0::2], rows[1::2]):
        out.append(((torch.from_numpy(half.view(np.uint8).copy()).to(pool.pool.device), len(half)), (0, len(half))))
    return out


def synthesize_codes(clean, params, model, cfa, seed, sample_id, white, black, shape=None):
    """What a sensor would have stored for one frame: the sampler's output x on `clean` under `model`, as a uint16 mosaic
    clip(rint(x * sat) + rint(black_c), 0, 65535), unpacked (CUDA uint16 (Hm, Wm); Bayer planes land in the layout [[0, 1], [3, 2]] of
    RawPacker.unpack_raw_bayer).  x * sat is one float32 multiply and rint rounds half to even: eld_hist_f32's q.
    clean: packed float32 (C,h,w) [ndarray or CUDA tensor], or None for a dark frame -- zeros of the packed `shape` (C,h,w).
    params: a NoiseParams / dict (K, g_scale, tl_lambda, tl_scale, row_scale, col_scale, color_bias, in DN); the sampler runs with ratio = 1,
    saturation = white - max(black) and q_step = 1.  black: per packed channel (Bayer) or per colour code (X-Trans)."""
    import torch
    M.check_cfa(cfa)
    _models([model])
    b = np.rint(M.black_levels(black))
    sat = float(white) - float(np.max(M.black_levels(black)))
    if not sat > 0:
        raise ValueError('white level %r does not exceed the black level' % (white,))
    C = group_map_f32(cfa)[0]
    if clean is None:
        if shape is None or len(shape) != 3 or int(shape[0]) != C:
            raise ValueError('a dark frame needs shape=(%d, h, w), got %r' % (C, shape))
        y = torch.zeros((1,) + tuple(int(v) for v in shape), dtype=torch.float32, device='cuda')
    else:
        y = (torch.from_numpy(np.ascontiguousarray(clean, dtype=np.float32)).cuda() if isinstance(clean, np.ndarray) else clean.float()).contiguous()
        if y.dim() != 3 or y.shape[0] != C:
            raise ValueError('clean must be packed (%d, h, w), got %s' % (C, tuple(y.shape)))
        y = y.unsqueeze(0)
    x = _sample(y, _noise_params(params, sat), model, cfa, seed, [int(sample_id)])
    return _stored_codes(x, cfa, b, sat)[0]


def _stored_codes(x, cfa, b, sat):
    """Sampler output x (N,C,h,w) -> the stored codes (N,Hm,Wm) uint16 of synthesize_codes; b = rint(black) per packed channel / colour code."""
    import torch
    from .noise import RawPacker
    C = x.shape[1]
    plane_black = b[list(XT_PLANE_COLOUR)] if cfa == 'xtrans' else b
    codes = torch.round(x * np.float32(sat)) + torch.from_numpy(plane_black.astype(np.float32)).to(x.device).view(1, C, 1, 1)
    mos = RawPacker(cfa).unpack_raw(torch.clamp(codes, 0, 65535))
    return mos.to(torch.int32).to(torch.uint16)


def clean_from_flat_pair(a, b, cfa, raw_pattern, black_level, color_bias, sat):
    """The clean image a flat pair stands for, packed float32 (C,h,w) on the device:
        y = clip((((a + b) * 0.5 - black_c) - color_bias_c) / sat, 0, 1)
    every operation in float32 ((a + b) * 0.5 is exact), black_c / color_bias_c those of the plane's packed channel (Bayer) or colour
    (X-Trans: black of the colour code R 0, G 1, B 2); a, b: CUDA int16/uint16 (Hm,Wm)."""
    import torch
    from .noise import RawPacker
    m = ((a.to(torch.int32) & 0xffff).float() + (b.to(torch.int32) & 0xffff).float()) * 0.5
    blk = M.black_levels(black_level)
    if cfa == 'xtrans':
        planes = RawPacker('xtrans').pack_raw_xtrans(m)
        col = list(XT_PLANE_COLOUR)
        bl, cb = blk[col], np.asarray(color_bias, np.float64).reshape(-1)[:3][col]
    else:
        pat = M.bayer_pattern(raw_pattern)
        pos = [np.argwhere(pat == c)[0] for c in range(4)]
        planes = torch.stack([m[int(r)::2, int(q)::2] for r, q in pos]).contiguous()
        bl, cb = blk, np.asarray(color_bias, np.float64).reshape(-1)[:4]
    C = planes.shape[0]
    dev = planes.device
    t = (planes - torch.from_numpy(bl.astype(np.float32)).to(dev).view(C, 1, 1)) - torch.from_numpy(cb.astype(np.float32)).to(dev).view(C, 1, 1)
    return torch.clamp(t / np.float32(sat), 0.0, 1.0).contiguous()


# ---- the validation --------------------------------------------------------------------------------------------------------------------
def _table_params(table, K, ncb):
    """source='table': the regression means at log K (no sigma scatter), the median G_shape, the mean colour-bias row."""
    prof = table[CAL.PROFILE]
    lk = float(np.log(K))
    reg = {k: float(np.exp(float(prof[k]['slope']) * lk + float(prof[k]['bias']))) for k in CAL.SIGMA_KEYS}
    cb = np.asarray(table['color_bias'], np.float64).reshape(len(table['G_shape']), -1).mean(axis=0)
    out = {'K': float(K), 'g_scale': reg['g_scale'], 'tl_scale': reg['G_scale'], 'row_scale': reg['R_scale'],
           'tl_lambda': float(np.median(np.asarray(table['G_shape'], np.float64))), 'color_bias': [float(v) for v in cb[:ncb]]}
    if CAL.COLUMN_KEY in prof:                       # a table of calibrate --column
        out['col_scale'] = float(np.exp(float(prof[CAL.COLUMN_KEY]['slope']) * lk + float(prof[CAL.COLUMN_KEY]['bias'])))
    return out


def _frame_params(fr, ncb):
    out = {'K': float(fr['K']), 'g_scale': float(fr['g_scale']), 'tl_scale': float(fr['G_scale']), 'row_scale': float(fr['R_scale']),
           'tl_lambda': float(fr['lambda']), 'color_bias': [float(v) for v in np.asarray(fr['color_bias']).reshape(-1)[:ncb]]}
    if CAL.COLUMN_KEY in fr:                         # a diag of calibrate_camera(column=True): the frame's own column-noise sample
        out['col_scale'] = float(fr[CAL.COLUMN_KEY])
    return out


def _mean_params(ps):
    out = {k: float(np.mean([p[k] for p in ps])) for k in ('K', 'g_scale', 'tl_scale', 'row_scale')}
    if all('col_scale' in p for p in ps):
        out['col_scale'] = float(np.mean([p['col_scale'] for p in ps]))
    out['tl_lambda'] = float(np.median([p['tl_lambda'] for p in ps]))
    out['color_bias'] = [float(v) for v in np.mean([p['color_bias'] for p in ps], axis=0)]
    return out


def _check_session_shapes(sessions, cfa):
    """calibrate's per-session checks without the counts its log-linear fits need: with a diag given nothing is fitted here."""
    if not isinstance(sessions, (list, tuple)) or len(sessions) == 0:
        raise ValueError('sessions must be a non-empty list of {"iso", "bias", "flats"}')
    shape = None
    for i, s in enumerate(sessions):
        for k in ('bias', 'flats'):
            if k not in s:
                raise ValueError('session %d has no %r' % (i, k))
        F, Hm, Wm = M.check_mosaics(s['bias'], 3, 'session %d bias' % i, cfa)
        P = M.check_mosaics(s['flats'], 4, 'session %d flats' % i, cfa)[0]
        shape = shape or (Hm, Wm)
        if (Hm, Wm) != shape or M.shape_of(s['flats'])[-2:] != shape:
            raise ValueError('session %d: mosaic shapes differ' % i)
        if F == 0 or P == 0:
            raise ValueError('session %d: needs at least one bias frame and one flat pair' % i)


def validate_camera(sessions, raw_pattern, black_level, white_level, table=None, diag=None, models=('Pg', 'PG', 'PGR', 'PGRB'), source='frames',
                    cfa='bayer', defects=None, radius=256, flat_radius=1024, seed=2018, alpha=1.0, keep_hist=False, structure=False, lags=8, shading=None):
    """Sessions (calibrate_camera's) -> a report dict: how far the sampler's synthesis under each model lies from the real frames.

    Parameters of a bias frame: source='frames' -- that frame's own estimates, diag['frames'] of calibrate_camera (run here when neither
    table nor diag is given); source='table' -- the table's regression means at log K of the session (diag['K']), without sigma scatter,
    the median G_shape and the mean colour-bias row.  Flat pairs use the session's mean parameters.
    Bias frame f of session s, model m (index i): real = histogram of u - rint(black_g); syn_d = histogram of q(x_d), x_d the sampler's dark
    frame at sample_id(s, f, i, d); kl = KL(real || syn_0), floor = KL(syn_0 || syn_1), each the mean over the colour groups ('kl_groups',
    'floor_groups' hold the G values).  Flat pair j: real = histogram of a - b; syn = histogram of q(x_0) - q(x_1) on the clean image
    clean_from_flat_pair, ids sample_id(s, F + j, i, d); kl_flat = KL(real || syn).  A defects map masks the real side only (synthetic
    frames have no defects; probabilities are normalised).
    A model with the letter D (e.g. 'PD', 'PDU') takes its signal-independent noise from the sensor's own frames: for bias frame f the draws
    read the session's OTHER bias frames (leave-one-out: the frame table handed to the sampler omits f; with defects the pooled frames are
    repaired), the clean image is zero and K the frame's.  Such rows carry 'dark': 'leave-one-out'; they apply to bias frames only (kl_flat
    is None) and every session needs at least two bias frames (ValueError).  A model with the letter C (e.g. 'PGRC') adds the
    per-sensor-column term: its scale is the frame's 'C_scale' of a diag of calibrate_camera(column=True) (the calibration that runs here
    without a diag is run that way) or, with source='table', the table's 'C_scale' law; a diag or table without it is a ValueError.  kl of 'PD' against its floor is how close two real frames of
    the sensor are to each other: the yardstick the parametric rows are read against.  best = the model of lowest mean bias-frame kl, lowest index on a tie.
    This is a check of marginal distributions per colour group; the spatial structure of the noise is a separate report:
    structure=True adds report['structure'] (eld_amd/structure.py).  Per session: 'real' -- the components of the bias
    frames (pairs = all frame pairs of the session; the defects map applies); per model 'synthetic' -- the same components of two synthetic
    dark frames per real frame, stored as codes the way synthesize_codes stores them, drawn with the sample ids of the histogram pass
    (pair = the two draws; for a model with D the two draws are repeated for this report with the leave-one-out frames dealt into two
    disjoint tables, so that they never read the same dark frame), averaged over the frames -- and 'log_ratio' = log(synthetic / real)
    where both are positive.  Each component is
    the mean over frames (pairs) and colour groups; row_acf1 / col_acf1 are the lag-1 autocorrelations.  A model with D in a session of
    fewer than 3 bias frames draws both frames from the same real frame: its fixed / temporal split is None and 'split' says why.  No
    best model is chosen from these numbers.  Without structure=True the report is what it was.
    shading: a DarkShading (eld_amd.shading) or its path: the REAL bias frames are corrected at their session's ISO (the integer path,
    eld_shading_apply_u16; flagged sites pass through) before the histograms and the structure sums, and the dark frames a model with D
    draws from are corrected the same way, so the report shows the fixed components with the correction applied, next to the models.  The
    flats, and the calibration that runs here without a diag, see the frames as they are.  Every session then needs an 'iso' inside the
    map's range (ValueError).  report['shading'] records x0 and the ISO range."""
    cfa = M.check_cfa(cfa)
    models = _models(models)
    R, RF = _radius(radius), _radius(flat_radius, 'flat_radius')
    if source not in ('frames', 'table'):
        raise ValueError("source must be 'frames' or 'table', got %r" % (source,))
    if not (alpha >= 0):
        raise ValueError('alpha must be >= 0, got %r' % (alpha,))
    if structure:
        lags = ST.check_lags(lags)
    if table is not None and any('B' in m for m in models) and table_cfa(table) != cfa:
        raise ValueError('the table is for cfa=%r, the frames are %r: its colour bias does not apply (model with B)' % (table_cfa(table), cfa))
    M.xtrans_pattern(raw_pattern) if cfa == 'xtrans' else M.bayer_pattern(raw_pattern)
    black = M.black_levels(black_level)
    check_defects(defects, cfa, raw_pattern=raw_pattern)
    if diag is None:
        M.check_sessions(sessions, cfa)                 # a calibration runs here: its session and frame counts apply
    else:
        _check_session_shapes(sessions, cfa)
    if len(sessions) >= 1 << 20:
        raise ValueError('too many sessions')
    with_dark = any('D' in m for m in models)
    with_col = any('C' in m for m in models)
    if with_dark:
        for i, s in enumerate(sessions):
            if M.shape_of(s['bias'])[0] < 2:
                raise ValueError('session %d has a single bias frame: a model with D draws from the OTHER bias frames of the session' % i)
    centre = group_black(cfa, black)
    sat = float(white_level) - float(black.max())
    if not sat > 0:
        raise ValueError('white level %r does not exceed the black level' % (white_level,))
    if defects is not None and not isinstance(defects, str):
        defects.check_frames(M.shape_of(sessions[0]['bias']), cfa, 'validation')
    if shading is not None:
        from .shading import as_dark_shading
        shading = as_dark_shading(shading)
        shading.check_pattern(None if cfa == 'xtrans' else raw_pattern, 'validation')
        for i, s in enumerate(sessions):
            shading.check_frames(M.shape_of(s['bias']), cfa, 'session %d bias' % i)
            if s.get('iso') is None:
                raise ValueError("session %d has no 'iso': the dark-shading map is subtracted at the session's ISO" % i)
            shading.t(s['iso'])

    import torch
    if diag is None:
        table_c, diag = CAL.calibrate_camera(sessions, raw_pattern, black_level, white_level, cfa=cfa, defects=defects, column=with_col)
        if table is None:
            table = table_c
    if defects == 'auto':
        defects = diag.get('defects')
        if defects is None:
            defects = find_defects(sessions[0]['bias'], cfa, raw_pattern)[0]
    C, _, G = group_map_f32(cfa)
    ncb = 3 if cfa == 'xtrans' else 4
    if source == 'table':
        if table is None or 'K' not in diag:
            raise ValueError("source='table' needs a table and the session gains diag['K']")
        if len(diag['K']) != len(sessions):
            raise ValueError("diag['K'] holds %d gains for %d sessions" % (len(diag['K']), len(sessions)))
    else:
        nb = sum(M.shape_of(s['bias'])[0] for s in sessions)
        if 'frames' not in diag or len(diag['frames']) != nb:
            raise ValueError("source='frames' needs diag['frames'] with one record per bias frame (%d)" % nb)

    dpool = None
    if with_dark:
        from .darkpool import DarkPool
        dpool = DarkPool([{'bias': s['bias'], 'iso': s.get('iso')} for s in sessions], cfa=cfa, raw_pattern=None if cfa == 'xtrans' else raw_pattern,
                         black_level=black, white_level=white_level, defects=defects, shading=shading)
    report = {'models': models, 'source': source, 'cfa': cfa, 'groups': G, 'radius': R, 'flat_radius': RF, 'alpha': float(alpha), 'seed': int(seed),
              'sessions': []}
    hists = {}
    if shading is not None:
        report['shading'] = {'x0': shading.x0, 'iso_min': shading.iso_min, 'iso_max': shading.iso_max, 'centred': shading.centred}
    if structure:
        report['structure'] = {'lags': lags, 'sessions': []}
        cells = ST.cell_centres(cfa, raw_pattern, black)
        bl = np.rint(black)
    j0 = 0
    for si, s in enumerate(sessions):
        bias = M.device_u16(s['bias'])
        if shading is not None:
            bias = shading.apply_device(bias, shading.t(s['iso']), None if isinstance(defects, str) else defects)
        flats = M.device_u16(s['flats'])
        F, Hm, Wm = M.shape_of(bias)
        P = M.shape_of(flats)[0]
        h, w = (2 * (Hm // 6), 2 * (Wm // 6)) if cfa == 'xtrans' else (Hm // 2, Wm // 2)
        if source == 'table':
            fparams = [_table_params(table, float(diag['K'][si]), ncb)] * F
        else:
            fparams = [_frame_params(fr, ncb) for fr in diag['frames'][j0:j0 + F]]
        j0 += F
        if with_col and not all('col_scale' in p for p in fparams):
            raise ValueError("a model with C needs the column-noise scale: %s has no 'C_scale'; calibrate with `python -m eld_amd.calibrate --column` "
                             "(calibrate_camera(..., column=True))" % ("the table's 'Profile-1'" if source == 'table' else "diag['frames']"))
        sparams = _mean_params(fparams)
        real = histogram_u16(bias, cfa, raw_pattern, centre, R, defects=defects)
        dark = torch.zeros((2, C, h, w), dtype=torch.float32, device=bias.device)
        srep = {'iso': s.get('iso'), 'K': sparams['K'], 'params': sparams, 'frames': [], 'flats': []}
        if structure:
            rst = ST.structure_stats(ST.structure_sums(bias, cfa, raw_pattern, cells, defects=defects,
                                                       pairs=[(a, b) for a in range(F) for b in range(a + 1, F)]), cfa, raw_pattern, lags)
            syn_parts = {m: [] for m in models}
        for f in range(F):
            frep = {'params': fparams[f], 'models': {}}
            prm = _noise_params(fparams[f], sat)
            if dpool is not None:
                loo_table, loo_range = _leave_one_out(dpool, dpool.ranges[si][0], F, f)
                dprm = NoiseParams(prm[0], prm[1], prm[2], prm[3], q_step=1.0, dark=loo_range)
                if structure and F >= 3:
                    halves = _disjoint_halves(dpool, dpool.ranges[si][0], F, f)
            for mi, m in enumerate(models):
                ids = [sample_id(si, f, mi, 0), sample_id(si, f, mi, 1)]
                if 'D' in m:
                    x = _sample(dark, dprm, m, cfa, seed, ids, dark=dpool, dark_table=loo_table)
                else:
                    x = _sample(dark, prm, m, cfa, seed, ids)
                syn = histogram_f32(x, sat, R, cfa)
                if structure:
                    if 'D' in m and F >= 3:                    # the two draws of the histogram pass may have read the same dark frame
                        x = torch.cat([_sample(dark[d:d + 1], NoiseParams(prm[0], prm[1], prm[2], prm[3], q_step=1.0, dark=rng_), m, cfa, seed,
                                               ids[d:d + 1], dark=dpool, dark_table=tab) for d, (tab, rng_) in enumerate(halves)])
                    sst = ST.structure_stats(ST.structure_sums(_stored_codes(x, cfa, bl, sat), cfa, raw_pattern, cells, pairs=[(0, 1)]),
                                             cfa, raw_pattern, lags)
                    syn_parts[m].append(ST.summarise(sst, with_pairs=not ('D' in m and F < 3)))
                klg, flg = kl_divergence(real[f], syn[0], alpha), kl_divergence(syn[0], syn[1], alpha)
                frep['models'][m] = {'kl': float(klg.mean()), 'floor': float(flg.mean()), 'kl_groups': klg.tolist(), 'floor_groups': flg.tolist()}
                if 'D' in m:
                    frep['models'][m]['dark'] = 'leave-one-out'
                if keep_hist:
                    hists['s%d_f%d_%s' % (si, f, m)] = syn
            srep['frames'].append(frep)
        if keep_hist:
            hists['s%d_real' % si] = real
        a, b = flats[:, 0].contiguous(), flats[:, 1].contiguous()
        realf = histogram_u16(a, cfa, raw_pattern, None, RF, subtract=b, defects=defects)
        prm = _noise_params(sparams, sat)
        for j in range(P):
            y = clean_from_flat_pair(a[j], b[j], cfa, raw_pattern, black, sparams['color_bias'], sat)
            y2 = torch.stack([y, y])
            prep = {'models': {}}
            for mi, m in enumerate(models):
                if 'D' in m:                                   # dark frames stand for the noise of bias frames only
                    prep['models'][m] = {'kl_flat': None, 'kl_flat_groups': None, 'dark': 'leave-one-out'}
                    continue
                x = _sample(y2, prm, m, cfa, seed, [sample_id(si, F + j, mi, 0), sample_id(si, F + j, mi, 1)])
                syn = histogram_f32(x[:1], sat, RF, cfa, subtract=x[1:])
                klg = kl_divergence(realf[j], syn[0], alpha)
                prep['models'][m] = {'kl_flat': float(klg.mean()), 'kl_flat_groups': klg.tolist()}
                if keep_hist:
                    hists['s%d_p%d_%s' % (si, j, m)] = syn[0]
            srep['flats'].append(prep)
        if keep_hist:
            hists['s%d_real_flats' % si] = realf
        srep['means'] = {m: {'kl': float(np.mean([fr['models'][m]['kl'] for fr in srep['frames']])),
                             'floor': float(np.mean([fr['models'][m]['floor'] for fr in srep['frames']])),
                             'kl_flat': None if 'D' in m else float(np.mean([pr['models'][m]['kl_flat'] for pr in srep['flats']]))} for m in models}
        report['sessions'].append(srep)
        if structure:
            real = ST.summarise(rst)
            strep = {'iso': s.get('iso'), 'real': real, 'real_frames': _finite(rst['frames']), 'real_pairs': _finite(rst['pairs']), 'models': {}}
            for m in models:
                synm = {}
                for k in ST.COMPONENTS:
                    vals = [q[k] for q in syn_parts[m] if q[k] is not None]
                    synm[k] = float(np.mean(vals)) if vals else None
                strep['models'][m] = {'synthetic': synm, 'log_ratio': ST.log_ratio(real, synm)}
                if 'D' in m:
                    strep['models'][m]['dark'] = 'leave-one-out'
                    if F < 3:
                        strep['models'][m]['split'] = 'fewer than 3 bias frames: both draws read the same dark frame, no fixed / temporal split'
            report['structure']['sessions'].append(strep)
    report['means'] = {m: {k: float(np.mean([fr['models'][m][k] for s in report['sessions'] for fr in s['frames']])) for k in ('kl', 'floor')}
                       for m in models}
    for m in models:
        report['means'][m]['kl_flat'] = None if 'D' in m else float(np.mean([pr['models'][m]['kl_flat'] for s in report['sessions'] for pr in s['flats']]))
        if 'D' in m:
            report['means'][m]['dark'] = 'leave-one-out'
    report['best'] = models[int(np.argmin([report['means'][m]['kl'] for m in models]))]      # argmin: the lowest index on a tie
    if keep_hist:
        report['hist'] = hists
    return report


def _finite(x):
    """Nested lists / dicts of floats with nan (a moment without data) -> the same with None."""
    if isinstance(x, dict):
        return {k: _finite(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_finite(v) for v in x]
    if isinstance(x, float) and not np.isfinite(x):
        return None
    return x


def _sigma(v):
    """A variance component as a signed sigma for the table: sign(v) sqrt(|v|); '-' where undefined."""
    return '      -' if v is None else '%7.3f' % (np.sign(v) * np.sqrt(abs(v)))


def structure_lines(rep):
    """The printed structure table: one line per session and model, real | synthetic."""
    out = ['structure (sigma in DN, negative = none detected): sigma_row (sensor), sigma_col, sigma_pix fixed, row_acf[1]; real | synthetic']
    for si, s in enumerate(rep['structure']['sessions']):
        for m in rep['models']:
            r, y = s['real'], s['models'][m]['synthetic']

            def acf(v):
                return '      -' if v is None else '%7.3f' % v
            out.append('session %d iso %-6s %-6s row %s | %s  col %s | %s  fixed %s | %s  acf1 %s | %s'
                       % (si, s['iso'], m, _sigma(r['row_var_sensor']), _sigma(y['row_var_sensor']), _sigma(r['col_var_sensor']),
                          _sigma(y['col_var_sensor']), _sigma(r['pix_fixed_var']), _sigma(y['pix_fixed_var']), acf(r['row_acf1']), acf(y['row_acf1'])))
    return out


# ---- command line ----------------------------------------------------------------------------------------------------------------------
def to_jsonable(x):
    """NumPy scalars and arrays -> Python numbers and lists, recursively (the report as JSON: no pickle)."""
    if isinstance(x, dict):
        return {str(k): to_jsonable(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [to_jsonable(v) for v in x]
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, np.generic):
        return x.item()
    return x


def parser():
    ap = argparse.ArgumentParser(prog='python -m eld_amd.validate', description=__doc__.split('\n')[0])
    ap.add_argument('manifest', help="calibrate's manifest JSON")
    ap.add_argument('--camera', help='a table written by eld_amd.calibrate (<camera>_params.npy); default: calibrate here')
    ap.add_argument('--models', default='Pg,PG,PGR,PGRB', type=_models_arg)
    ap.add_argument('--source', default='frames', choices=('frames', 'table'))
    ap.add_argument('--defects', help="a defect map (.npz) or 'auto'; overrides the manifest's \"defects\"")
    ap.add_argument('--radius', type=_radius_arg, default=256)
    ap.add_argument('--seed', type=int, default=2018)
    ap.add_argument('--out', help='write the report here as JSON')
    ap.add_argument('--hist', help='write the histograms here (.npz)')
    ap.add_argument('--structure', action='store_true', help='add the spatial-structure report: row, column and fixed-pattern components')
    ap.add_argument('--shading', metavar='FILE', help='a dark-shading map written by eld_amd.shading (.npz): the real bias frames are corrected first')
    ap.add_argument('--lags', type=_lags_arg, default=8, help='autocorrelation lags of the structure report')
    return ap


def _lags_arg(s):
    try:
        return ST.check_lags(int(s))
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def _models_arg(s):
    try:
        return _models(s)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def _radius_arg(s):
    try:
        return _radius(int(s))
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def main(argv=None):
    a = parser().parse_args(argv)
    sessions, pattern, black, white, cfa = CAL.load_manifest(a.manifest, with_cfa=True)
    defects = a.defects if a.defects is not None else CAL.manifest_defects(a.manifest)
    if defects is not None and defects != 'auto':
        defects = as_defect_map(defects, '--defects')
    table = None if a.camera is None else np.load(a.camera, allow_pickle=True).item()
    rep = validate_camera(sessions, pattern, black, white, table=table, models=a.models, source=a.source, cfa=cfa, defects=defects,
                          radius=a.radius, seed=a.seed, keep_hist=a.hist is not None, structure=a.structure, lags=a.lags,
                          shading=a.shading)
    hists = rep.pop('hist', None)
    for si, s in enumerate(rep['sessions']):
        for m in rep['models']:
            mm = s['means'][m]
            flat = 'kl_flat %.5f' % mm['kl_flat'] if mm['kl_flat'] is not None else 'dark frames, leave-one-out'
            print('session %d iso %-6s %-6s kl %.5f  floor %.5f  %s' % (si, s['iso'], m, mm['kl'], mm['floor'], flat))
    print('best model: %s (alpha %g, radius %d, seed %d)' % (rep['best'], rep['alpha'], rep['radius'], rep['seed']))
    if a.structure:
        print('\n'.join(structure_lines(rep)))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(to_jsonable(rep), f, indent=1)
        print('wrote', a.out)
    if a.hist:
        np.savez(a.hist, **hists)
        print('wrote', a.hist)
    return 0


if __name__ == '__main__':
    sys.exit(main())
