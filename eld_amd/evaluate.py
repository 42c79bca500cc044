"""Evaluate a denoiser on captured short/long pairs: PSNR / SSIM per ISO and exposure ratio, and error as a function of signal level.

    rep = evaluate_pairs(denoiser, pairs, 'bayer', raw_pattern, black_level, white_point)     # pairs: [{'short', 'long', 'ratio', 'iso'}, ...]
    rep['table']                                    # means per (iso, ratio): the layout of the paper's tables
    rep['pairs'][0]['curves']['output']['bias']     # (G, NB): mean error per colour group and signal bin, in DN

The numbers are the reference's evaluation (test_ELD.py / test_SID.py: ELDEvalDataset -> ELDModel.eval(correct=True)) composed from this
package's public pieces: the input stage clip(pack x ratio) (denoise.pack_input, dataset/sid_dataset.py:397-410), an optional centre crop
(crop_center), the network (denoise.run_network), the illuminance correction (metrics.illuminance_correct, models/ELD_model.py:138-169)
and PSNR / SSIM (metrics.quality_assess_frames, util/index.py:76-81) of the output and of the input against the long exposure.

PSNR and SSIM hide the typical failure at ratios of 100-300, a signal-dependent bias in the shadows (lifted or crushed blacks, a colour
cast).  With levels=True the corrected output and the clipped input are written back to uint16 codes and compared with the long exposure's
codes per CFA colour and signal bin: exact integer sums from one HIP pass (csrc/pairstats.hip: eld_pair_level_stats_u16), turned into
bias and RMSE curves on the host in float64 (level_curves).  The contract, the bin function and how to read the lowest bins are DESIGN.md
sec. 19.

Command line: python -m eld_amd.evaluate pairs.json --ckpt net.pt [--meta sensor.json] [--bf16] [--no-correct] [--crop N] [--defects F]
[--shading F] [--json OUT] [--save DIR] [--baseline-K K (--baseline-sigma S | --baseline-camera TABLE) [--baseline-method bm3d]]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

from . import _lib as L
from . import mosaic as M
from .defects import as_defect_map, pack_bitmap, repair_device

NB = L.PAIRSTATS_BINS
STATS = ('n', 'sum_s', 'sum_e', 'sum_e2')
GROUP_NAMES = {'bayer': ('R', 'G1', 'B', 'G2'), 'xtrans': ('R', 'G', 'B')}
METRICS = ('psnr', 'ssim', 'psnr_in', 'ssim_in')
BASELINE_METRICS = ('psnr_nlm', 'ssim_nlm')                # added by evaluate_pairs(..., baseline=ClassicalDenoiser); '_bm3d' with method='bm3d'


# ---- the bins (host) --------------------------------------------------------------------------------------------------------------------
def bin_lower_edges():
    """The smallest signal s = ref - black of bins 1 .. NB - 2, int64 (NB,): entry 0 is 0 (bin 0 holds every s <= 0) and the last entry
    -1 (the saturated bin is chosen by ref >= white, not by s)."""
    e = np.zeros(NB, np.int64)
    e[1:8] = np.arange(1, 8)
    for o in range(3, 16):
        for q in range(4):
            e[8 + 4 * (o - 3) + q] = (4 + q) << (o - 2)
    e[NB - 1] = -1
    return e


# ---- the kernel's wrapper ---------------------------------------------------------------------------------------------------------------
def _level_sums(est, ref, lay, white, Hc, Wc, bitmap=None):
    """eld_pair_level_stats_u16 on CUDA code tensors (F,Hm,Wm) -> int64 ndarray (F, G, NB, 4); lay: the CfaLayout of the cut; bitmap: the
    device words of a defect map."""
    import torch
    F, Hm, Wm = (int(v) for v in ref.shape)
    lib = L.lib()
    with torch.cuda.device(ref.device):
        out = torch.empty((F, lay.G, NB, 4), dtype=torch.int64, device=ref.device)
        need = lib.eld_pair_level_stats_workspace_bytes(F, Hm, Wm)
        ws = M.workspace(need, ref.device)
        L.check(lib.eld_pair_level_stats_u16(L.dptr(est), L.dptr(ref), F, Hm, Wm, Hc, Wc, lay.period, lay.c_group(), lay.G, lay.c_black(), white,
                                             L.dptr(bitmap), L.dptr(out), L.dptr(ws), need, L.cur_stream()), 'eld_pair_level_stats_u16')
    return out.cpu().numpy()


def pair_level_stats(est_u16, ref_u16, cfa, raw_pattern, black_level, white_point, defects=None):
    """Exact error-versus-signal sums of an estimate against a reference.  est_u16, ref_u16: uint16 mosaics (Hm,Wm) or (F,Hm,Wm), NumPy or
    CUDA int16/uint16 tensors, of one shape.  -> int64 ndarray (F, G, NB, 4): per frame, colour group (validate.group_map_u16: Bayer R, G1,
    B, G2; X-Trans R, G, B) and signal bin (NB = 61, the last bin holds ref >= white_point) the sums STATS =
    (n, sum s, sum e, sum e^2) with s = ref - black and e = est - ref.  X-Trans counts the whole 6x6 cells only (the borders beyond them
    pass through the write-back untouched); defects: a DefectMap whose flagged sites are not counted."""
    lay = M.CfaLayout.for_codes(cfa, raw_pattern, black_level)
    white = M.check_white(white_point)
    se, sr = M.check_stack(est_u16, 'est_u16'), M.check_stack(ref_u16, 'ref_u16')
    if se != sr:
        raise ValueError('est_u16 has shape %s, ref_u16 %s' % (se, sr))
    F, Hm, Wm = sr
    M.check_site_count(Hm, Wm)
    if defects is not None:
        defects = as_defect_map(defects)
        defects.check_frames((Hm, Wm), cfa, 'pair_level_stats')
    Hc, Wc = lay.whole_cells(Hm, Wm)
    est = M.device_u16(est_u16).reshape(F, Hm, Wm)
    ref = M.device_u16(ref_u16).reshape(F, Hm, Wm)
    if ref.device != est.device:
        raise ValueError('est_u16 is on %s, ref_u16 on %s' % (est.device, ref.device))
    return _level_sums(est, ref, lay, white, Hc, Wc, None if defects is None else defects.bitmap_on(ref.device))


# ---- curves (host, float64) -------------------------------------------------------------------------------------------------------------
def level_curves(sums, span=None):
    """sums: int64 (..., G, NB, 4) from pair_level_stats (sum over frames first to pool them).  -> dict of float64 arrays:
        'n' (..., G, NB) int64      sites per bin
        'signal', 'bias', 'rmse' (..., G, NB)      sum s / n, sum e / n, sqrt(sum e^2 / n) in DN; nan where the bin is empty
        'mse_codes' (..., G)        sum e^2 / n over all bins but the saturated one
        'psnr_codes' (..., G)       10 log10(span^2 / mse_codes), span = white - black of the group (one value or G); nan without span,
                                    inf for a zero error
    Nothing divides by zero on the way: an empty bin or group is nan."""
    s = np.asarray(sums)
    if s.dtype.kind not in 'iu' or s.ndim < 3 or s.shape[-2:] != (NB, 4):
        raise ValueError('sums must be an integer array (..., G, %d, 4), got %s %s' % (NB, s.dtype, s.shape))
    n = s[..., 0].astype(np.int64)
    nf = n.astype(np.float64)
    has = n > 0
    den = np.where(has, nf, 1.0)

    def per_n(v):
        return np.where(has, v.astype(np.float64) / den, np.nan)

    out = {'n': n, 'signal': per_n(s[..., 1]), 'bias': per_n(s[..., 2]), 'rmse': np.sqrt(per_n(s[..., 3]))}
    # the totals as Python integers: sum e^2 of a whole frame may exceed 2^53, the quotient is rounded once
    tn = n[..., :NB - 1].sum(axis=-1)
    tq = s[..., :NB - 1, 3].astype(object).sum(axis=-1)
    mse = np.full(tn.shape, np.nan)
    for i in np.ndindex(tn.shape):
        if tn[i] > 0:
            mse[i] = int(np.asarray(tq)[i]) / int(tn[i])
    out['mse_codes'] = mse
    psnr = np.full(tn.shape, np.nan)
    if span is not None:
        sp = np.broadcast_to(np.asarray(span, np.float64), tn.shape)
        if np.any(sp <= 0):
            raise ValueError('span (white - black) must be positive, got %r' % (span,))
        pos = mse > 0
        psnr[pos] = 10.0 * np.log10(sp[pos] * sp[pos] / mse[pos])
        psnr[mse == 0] = np.inf
    out['psnr_codes'] = psnr
    return out


# ---- the evaluation ---------------------------------------------------------------------------------------------------------------------
def pair_ratio(pair, what='pair'):
    """The exposure ratio of one pair: its 'ratio', or long_iso * long_exposure / (iso * exposure) (dataset/sid_dataset.py:397-401)."""
    if pair.get('ratio') is not None:
        r = float(pair['ratio'])
    else:
        miss = [k for k in ('iso', 'exposure', 'long_iso', 'long_exposure') if pair.get(k) is None]
        if miss:
            raise ValueError("%s: needs 'ratio' or all of iso, exposure, long_iso, long_exposure (missing: %s)" % (what, ', '.join(miss)))
        short = float(pair['iso']) * float(pair['exposure'])
        if not (short > 0 and math.isfinite(short)):
            raise ValueError('%s: iso * exposure must be finite and > 0, got %r' % (what, short))
        r = float(pair['long_iso']) * float(pair['long_exposure']) / short
    if not (math.isfinite(r) and r > 0):
        raise ValueError('%s: the ratio must be finite and > 0, got %r' % (what, r))
    return r


def _crop_box(h, w, crop):
    """crop_center (dataset/sid_dataset.py:37-41) on a packed h x w frame -> (y0, x0)"""
    return h // 2 - crop // 2, w // 2 - crop // 2


def _check_pairs(pairs, cfa, crop, shading):
    """Everything the host can see -> [(kind, (Hm, Wm), ratio, iso)]"""
    if not isinstance(pairs, (list, tuple)) or not pairs:
        raise ValueError('pairs must be a non-empty list of dicts')
    info = []
    for i, pr in enumerate(pairs):
        what = 'pair %d' % i
        if not isinstance(pr, dict) or 'short' not in pr or 'long' not in pr:
            raise ValueError("%s: a pair is a dict with 'short' and 'long' mosaics" % what)
        kinds = []
        for k in ('short', 'long'):
            try:
                kind, batched = M.as_u16(pr[k])
            except ValueError as e:
                raise ValueError('%s: %s: %s' % (what, k, e))
            if batched:
                raise ValueError('%s: %s must be one (Hm, Wm) mosaic, got shape %s' % (what, k, tuple(pr[k].shape)))
            kinds.append(kind)
        ss, sl = tuple(int(v) for v in pr['short'].shape), tuple(int(v) for v in pr['long'].shape)
        if ss != sl:
            raise ValueError('%s: short is %d x %d, long %d x %d' % ((what,) + ss + sl))
        M.check_sides(ss[0], ss[1], cfa)
        ratio = pair_ratio(pr, what)
        iso = pr.get('iso')
        if iso is not None and not (math.isfinite(float(iso)) and float(iso) > 0):
            raise ValueError('%s: iso must be finite and > 0, got %r' % (what, iso))
        if shading is not None and iso is None:
            raise ValueError('%s: shading needs iso: the ISO the short exposure was shot at' % what)
        h, w = (ss[0] // 2, ss[1] // 2) if M.PLANES[cfa] == 4 else (2 * (ss[0] // 6), 2 * (ss[1] // 6))
        if crop is not None and (crop > h or crop > w):
            raise ValueError('%s: crop %d exceeds the packed frame %d x %d' % (what, crop, h, w))
        info.append((kinds, ss, ratio, None if iso is None else float(iso)))
    return info


def _to_device(m, dev):
    import torch
    if isinstance(m, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(m).view(np.int16)).to(dev).unsqueeze(0)
    if m.device != dev:
        raise ValueError('a mosaic is on %s, the denoiser on %s' % (m.device, dev))
    return m.contiguous().unsqueeze(0)


def _codes(packed, y0, x0, long3, cfa, pat, blk, white):
    """A packed frame (1,C,n,m) that was cut at (y0, x0) of the packed long exposure -> its uint16 codes (rounding='nearest') and the long
    exposure's, both cut to the sites the packed frame covers: (est, ref, phase of the cut in the CFA cell)."""
    import torch
    from .denoise import write_back
    C, n, m = packed.shape[1:]
    step = 2 if cfa == 'bayer' else 3                              # mosaic sites per packed pixel and axis
    Hm, Wm = long3.shape[1:]
    hp, wp = (Hm // 2, Wm // 2) if cfa == 'bayer' else (2 * (Hm // 6), 2 * (Wm // 6))
    full = packed
    if (n, m) != (hp, wp):                                         # written back inside a whole frame: a cut may start in the middle of a cell
        full = torch.zeros((1, C, hp, wp), dtype=torch.float32, device=packed.device)
        full[:, :, y0:y0 + n, x0:x0 + m] = packed
    est = write_back(full, long3.clone(), cfa, pat, blk, white, 'nearest')
    ys, xs = step * y0, step * x0
    box = (slice(None), slice(ys, ys + step * n), slice(xs, xs + step * m))
    return est[box].contiguous(), long3[box].contiguous(), (ys, xs)


def _rolled_pattern(cfa, raw_pattern, phase):
    """The CFA cell as seen from a cut that starts at mosaic site `phase`."""
    pat = np.asarray(M.default_pattern(cfa, raw_pattern))
    if cfa == 'xtrans':
        return np.roll(pat, (-(phase[0] % 6), -(phase[1] % 6)), axis=(0, 1))
    return pat.reshape(2, 2)                                       # a Bayer cut starts on an even site


def _cut_bitmap(defects, phase, shape, dev):
    """The device bitmap of the cut of `shape` that starts at mosaic site `phase` (None without a map)."""
    if defects is None:
        return None
    if tuple(shape) == defects.shape:
        return defects.bitmap_on(dev)
    import torch
    m = defects.mask[phase[0]:phase[0] + shape[0], phase[1]:phase[1] + shape[1]]
    return torch.from_numpy(pack_bitmap(m).view(np.int32).copy()).to(dev)


def table_by_iso_ratio(rows, metrics=METRICS):
    """Means of the metrics over the rows that share (iso, ratio), sorted by iso (rows without one last) then ratio: the paper's layout."""
    keys = sorted({(r['iso'], r['ratio']) for r in rows}, key=lambda k: (k[0] is None, k[0] or 0.0, k[1]))
    table = []
    for iso, ratio in keys:
        sel = [r for r in rows if r['iso'] == iso and r['ratio'] == ratio]
        row = {'iso': iso, 'ratio': ratio, 'count': len(sel)}
        for k in metrics:
            row[k] = float(np.mean([r[k] for r in sel]))
        table.append(row)
    return table


def evaluate_pairs(denoiser, pairs, cfa, raw_pattern=None, black_level=None, white_point=16383, correct=True, crop=None, chop=None, defects=None,
                   shading=None, levels=True, on_pair=None, flatfield=None, baseline=None):
    """Evaluate `denoiser` (denoise.load_denoiser) on captured pairs, as the reference's test scripts do.

    pairs     a list of dicts: 'short' and 'long' (uint16 mosaics (Hm,Wm): NumPy, or CUDA uint16 / int16-view tensors) and either 'ratio' or
              'iso', 'exposure', 'long_iso', 'long_exposure' (ratio = long_iso * long_exposure / (iso * exposure)).  'iso' also groups the
              table and is the abscissa of `shading`; 'name' is carried into the row.
    correct   apply metrics.illuminance_correct(output, target) before the metrics (ELDModel.eval(correct=True)).
    crop      None, or N: the centre crop of N x N packed pixels the reference's evaluation takes (512), input and target alike.
    chop      as denoise_raw: None = whole frame when the packed sides are multiples of 16, else forward_chop.
    defects, shading   as denoise_raw: both mosaics are repaired with the map; the dark shading is subtracted from the short exposure only.
    flatfield a FlatField (eld_amd.flatfield) or the path of a saved one: its PRNU plane multiplies the short exposure in the input stage
              (as denoise_raw) and the long exposure through the integer path (FlatField.apply(part='prnu')), after the repair.
    levels    also the error-versus-signal sums (pair_level_stats) of the corrected output and of the clipped input, both written back to
              codes with rounding='nearest', against the long exposure's codes.
    on_pair   called as on_pair(index, row, {'input', 'output', 'target'}) with the packed CUDA tensors of each pair (the command line's --save).
    baseline  None, or a ClassicalDenoiser (eld_amd.classical): the short exposure's codes also go through the classical baseline (the same
              repair, shading and flat-field maps, the same crop and illuminance correction), and every row gains psnr_nlm and ssim_nlm
              (psnr_bm3d and ssim_bm3d with a method='bm3d' baseline: the keys take its `label`), the table and the mean their means, and with levels 'sums', 'curves' and 'pooled' a third set 'baseline'; the tensors handed to
              on_pair gain 'baseline'.  A pair's 'K' (its gain in DN per electron: ISO changes it) replaces the baseline's for that pair
              (ClassicalDenoiser.with_gain).  With None every key and number of the report is what it was without this argument.

    Returns {'pairs': rows, 'table': means per (iso, ratio), 'mean': the means over all pairs, 'groups': the colour groups' names,
    'pooled': {'output', 'input'} curves over all pairs (None without levels)}.  A row holds psnr, ssim (output against target), psnr_in,
    ssim_in (input against target), ratio, iso, name and with levels 'sums' {'output', 'input'} (int64 (G, NB, 4)), 'curves' (level_curves
    of them) and psnr_codes (the output's, per group).  Bad arguments raise ValueError before any device work."""
    from .denoise import pack_input, run_network
    M.check_cfa(cfa)
    if getattr(denoiser, 'cfa', cfa) != cfa:
        raise ValueError('the denoiser was loaded for cfa=%r, called with %r' % (denoiser.cfa, cfa))
    if chop not in (None, True, False):
        raise ValueError('chop must be None, True or False, got %r' % (chop,))
    if crop is not None and (isinstance(crop, bool) or not isinstance(crop, (int, np.integer)) or crop < 1):
        raise ValueError('crop must be None or a positive integer (packed pixels), got %r' % (crop,))
    if crop is not None and cfa == 'xtrans' and crop % 2:
        raise ValueError('an X-Trans crop must be even (two packed pixels span one 6x6 cell), got %d' % crop)
    pat, blk, white = M.levels(cfa, raw_pattern, black_level, white_point)
    if denoiser.in_channels != M.PLANES[cfa] or denoiser.out_channels != M.PLANES[cfa]:
        raise ValueError('the network maps %d to %d planes, a %s frame packs to %d' % (denoiser.in_channels, denoiser.out_channels, cfa, M.PLANES[cfa]))
    if shading is not None:
        from .shading import as_dark_shading
        shading = as_dark_shading(shading)
    if defects is not None:
        defects = as_defect_map(defects)
    if flatfield is not None:
        from .flatfield import as_flat_field
        flatfield = as_flat_field(flatfield)
        flatfield.check_pattern(None if cfa == 'xtrans' else np.asarray(pat).reshape(2, 2), 'evaluate_pairs')
    info = _check_pairs(pairs, cfa, crop, shading)
    if baseline is not None:
        if not getattr(baseline, 'is_classical', False):
            raise ValueError('baseline must be a ClassicalDenoiser (eld_amd.classical) or None, got %r' % (type(baseline).__name__,))
        if baseline.cfa != cfa:
            raise ValueError('the baseline was made for cfa=%r, called with %r' % (baseline.cfa, cfa))
        baselines = [baseline if pr.get('K') is None else baseline.with_gain(pr['K']) for pr in pairs]
    label = getattr(baseline, 'label', 'nlm')                  # the denoiser's method names its keys and columns
    bkeys = ('psnr_' + label, 'ssim_' + label)
    metrics = METRICS + (bkeys if baseline is not None else ())
    for i, (_, shape, _, iso) in enumerate(info):
        if flatfield is not None:
            flatfield.check_frames(shape, cfa, 'pair %d' % i)
        if defects is not None:
            defects.check_frames(shape, cfa, 'pair %d' % i)
        if shading is not None:
            shading.check_frames(shape, cfa, 'pair %d' % i)
            shading.check_pattern(None if cfa == 'xtrans' else np.asarray(pat).reshape(2, 2), 'pair %d' % i)
            shading.t(iso)

    import torch
    from .metrics import illuminance_correct, quality_assess_frames
    dev = next(denoiser.net.parameters()).device
    if dev.type != 'cuda':
        raise ValueError('the denoiser must live on a CUDA device (load_denoiser(..., device=...)), it is on %s' % dev)
    span = [white - b for b in blk] if cfa == 'bayer' else white - blk[0]
    rows = []
    pooled = {'output': 0, 'input': 0}
    if baseline is not None:
        pooled['baseline'] = 0
    with torch.cuda.device(dev):
        for i, (pr, (_, shape, ratio, iso)) in enumerate(zip(pairs, info)):
            short, long_ = _to_device(pr['short'], dev), _to_device(pr['long'], dev)
            if defects is not None:
                short, long_ = repair_device(short, defects), repair_device(long_, defects)
            if flatfield is not None:
                x = pack_input(short, cfa, pat, blk, white, [ratio], shading, None if shading is None else shading.t(iso), flatfield)
                long_ = flatfield.apply(long_, part='prnu', black_level=blk, defects=defects)
            else:
                x = pack_input(short, cfa, pat, blk, white, [ratio], shading, None if shading is None else shading.t(iso))
            target = pack_input(long_, cfa, pat, blk, white, [1.0])
            y0 = x0 = 0
            if crop is not None:
                y0, x0 = _crop_box(x.shape[2], x.shape[3], crop)
                x = x[:, :, y0:y0 + crop, x0:x0 + crop].contiguous()
                target = target[:, :, y0:y0 + crop, x0:x0 + crop].contiguous()
            out = run_network(denoiser, x, chop)
            if correct:
                out = illuminance_correct(out, target)
            q = quality_assess_frames(out, target)[0].tolist()
            qi = quality_assess_frames(x, target)[0].tolist()
            row = {'name': pr.get('name'), 'ratio': ratio, 'iso': iso, 'psnr': q[0], 'ssim': q[1], 'psnr_in': qi[0], 'ssim_in': qi[1]}
            sets = (('output', out), ('input', x))
            if baseline is not None:
                nlm = baselines[i].denoise_codes(short, pat, blk, white, [ratio], shading, None if shading is None else shading.t(iso), flatfield)
                if crop is not None:
                    nlm = nlm[:, :, y0:y0 + crop, x0:x0 + crop].contiguous()
                if correct:
                    nlm = illuminance_correct(nlm, target)
                qn = quality_assess_frames(nlm, target)[0].tolist()
                row[bkeys[0]], row[bkeys[1]] = qn[0], qn[1]
                sets += (('baseline', nlm),)
            if levels:
                sums = {}
                for k, t in sets:
                    est, ref, phase = _codes(t, y0, x0, long_, cfa, pat, blk, white)
                    lay = M.CfaLayout.for_codes(cfa, _rolled_pattern(cfa, raw_pattern, phase), blk)
                    cut = tuple(int(v) for v in est.shape[1:])
                    sums[k] = _level_sums(est, ref, lay, int(white), cut[0], cut[1], _cut_bitmap(defects, phase, cut, dev))[0]
                    pooled[k] = pooled[k] + sums[k]
                row['sums'] = sums
                row['curves'] = {k: level_curves(v, span) for k, v in sums.items()}
                row['psnr_codes'] = row['curves']['output']['psnr_codes']
            rows.append(row)
            if on_pair is not None:
                tensors = {'input': x, 'output': out, 'target': target}
                if baseline is not None:
                    tensors['baseline'] = nlm
                on_pair(i, row, tensors)
    mean = {k: float(np.mean([r[k] for r in rows])) for k in metrics}
    return {'pairs': rows, 'table': table_by_iso_ratio(rows, metrics), 'mean': mean, 'groups': list(GROUP_NAMES[cfa]), 'bin_lower_edges': bin_lower_edges(),
            'pooled': {k: level_curves(v, span) for k, v in pooled.items()} if levels else None}


# ---- reports ----------------------------------------------------------------------------------------------------------------------------
def baseline_label(row):
    """The label of the baseline whose columns a table row or a pair's row carries ('nlm', 'bm3d'), or None."""
    for label in ('nlm', 'bm3d'):
        if 'psnr_' + label in row:
            return label
    return None


def table_lines(table):
    lines = ['%8s %8s %5s %9s %8s %9s %8s' % ('iso', 'ratio', 'n', 'PSNR', 'SSIM', 'PSNR in', 'SSIM in')]
    nlm = baseline_label(table[0]) if table else None              # evaluate_pairs(..., baseline=...): two more columns
    if nlm:
        lines[0] += ' %9s %8s' % ('PSNR ' + nlm, 'SSIM ' + nlm)
    for r in table:
        lines.append('%8s %8.4g %5d %9.3f %8.4f %9.3f %8.4f' % ('-' if r['iso'] is None else '%g' % r['iso'], r['ratio'], r['count'], r['psnr'], r['ssim'],
                                                               r['psnr_in'], r['ssim_in']))
        if nlm:
            lines[-1] += ' %9.3f %8.4f' % (r['psnr_' + nlm], r['ssim_' + nlm])
    return lines


def curve_lines(pooled, groups, label='nlm'):
    """Per colour group the populated bins: lower edge of the bin (DN above black), sites, mean signal, then bias and RMSE of the output
    next to the input's; label: the baseline's, for the headings of its two columns."""
    edges = bin_lower_edges()
    lines = []
    b_ = pooled.get('baseline')                                   # evaluate_pairs(..., baseline=...): the baseline's bias and RMSE, appended
    for g, name in enumerate(groups):
        lines.append('%s: %8s %10s %10s | %10s %10s | %10s %10s' % (name, 's >=', 'sites', 'signal', 'bias out', 'bias in', 'rmse out', 'rmse in'))
        if b_ is not None:
            lines[-1] += ' | %10s %10s' % ('bias ' + label, 'rmse ' + label)
        o, i = pooled['output'], pooled['input']
        for b in range(NB):
            if o['n'][g, b] == 0:
                continue
            lines.append('%s  %8s %10d %10.2f | %+10.3f %+10.3f | %10.3f %10.3f' % (' ' * len(name), 'sat' if b == NB - 1 else '%d' % edges[b], o['n'][g, b],
                                                                                  o['signal'][g, b], o['bias'][g, b], i['bias'][g, b], o['rmse'][g, b],
                                                                                  i['rmse'][g, b]))
            if b_ is not None:
                lines[-1] += ' | %+10.3f %10.3f' % (b_['bias'][g, b], b_['rmse'][g, b])
    return lines


# ---- command line -----------------------------------------------------------------------------------------------------------------------
PAIR_KEYS = ('short', 'long', 'ratio', 'iso', 'exposure', 'long_iso', 'long_exposure', 'name', 'K')
OPTION_KEYS = ('cfa', 'raw_pattern', 'black_level', 'white_point', 'wb', 'ccm', 'precision', 'chop', 'defects', 'shading', 'flatfield')


def read_manifest(path):
    """pairs.json -> (options, pairs): the sidecar fields denoise.read_sidecar knows (cfa, raw_pattern, black_level, white_point, wb, ccm,
    precision, chop, defects, shading, or rawpy's names) and 'pairs', a list of {'short': 'a.npy', 'long': 'b.npy', 'ratio': 100, 'iso':
    1600, ...}; file names are relative to the manifest.  The mosaics are not loaded here."""
    from .denoise import sidecar_from_dict
    if not os.path.exists(path):
        raise ValueError('no such manifest: %s' % path)
    with open(path) as fh:
        d = json.load(fh)
    if not isinstance(d, dict) or not isinstance(d.get('pairs'), list) or not d['pairs']:
        raise ValueError("%s: the manifest is a JSON object with a non-empty list 'pairs'" % path)
    opts = sidecar_from_dict({k: v for k, v in d.items() if k != 'pairs'}, path)
    for k in ('ratio', 'iso'):
        if k in opts:
            raise ValueError('%s: %r belongs to each pair, not to the manifest' % (path, k))
    base = os.path.dirname(os.path.abspath(path))
    pairs = []
    for i, pr in enumerate(d['pairs']):
        if not isinstance(pr, dict):
            raise ValueError('%s: pair %d is not an object' % (path, i))
        unknown = [k for k in pr if k not in PAIR_KEYS]
        if unknown:
            raise ValueError('%s: pair %d: unknown key %r (known: %s)' % (path, i, unknown[0], ', '.join(PAIR_KEYS)))
        for k in ('short', 'long'):
            if not isinstance(pr.get(k), str):
                raise ValueError('%s: pair %d: %r must name a .npy file' % (path, i, k))
        q = dict(pr)
        q['short'], q['long'] = os.path.join(base, pr['short']), os.path.join(base, pr['long'])
        q.setdefault('name', os.path.splitext(os.path.basename(pr['short']))[0])
        pair_ratio(q, '%s: pair %d' % (path, i))
        pairs.append(q)
    return opts, pairs


def load_pairs(pairs):
    """The manifest's pairs with their mosaics loaded (.npy: np.load; .dng: eld_amd.dng.read_dng)."""
    from .dng import load_frame
    out = []
    for pr in pairs:
        q = dict(pr)
        for k in ('short', 'long'):
            if not os.path.exists(pr[k]):
                raise ValueError('no such file: %s' % pr[k])
            q[k] = load_frame(pr[k])
        out.append(q)
    return out


def build_parser():
    p = argparse.ArgumentParser(prog='python -m eld_amd.evaluate', description='Evaluate a trained ELD U-Net on captured short/long pairs of raw mosaics.')
    p.add_argument('manifest', help="pairs.json: sensor fields (cfa, raw_pattern, black_level, white_point, wb, ccm) and 'pairs'")
    p.add_argument('--ckpt', required=True, help='checkpoint (.pt): the reference dict {"netG": ...} or a U-Net state_dict')
    p.add_argument('--meta', help='JSON sidecar (eld_amd.denoise): its fields override the manifest\'s')
    p.add_argument('--bf16', action='store_true', help='run the network in bf16')
    p.add_argument('--no-correct', action='store_true', help='no illuminance correction before the metrics')
    p.add_argument('--crop', type=int, help='centre crop of N x N packed pixels (the reference evaluates 512)')
    p.add_argument('--defects', metavar='F', help='a defect map written by eld_amd.defects (.npz)')
    p.add_argument('--shading', metavar='F', help='a dark-shading map written by eld_amd.shading (.npz); every pair then needs iso')
    p.add_argument('--flatfield', metavar='F', help='a flat-field map written by eld_amd.flatfield (.npz): its PRNU plane corrects both exposures')
    p.add_argument('--json', metavar='OUT', help='write the whole report as JSON')
    p.add_argument('--save', metavar='DIR', help='write sRGB PNGs of input, output and target at packed resolution (needs wb and ccm)')
    p.add_argument('--baseline-K', type=float, metavar='K', help="also evaluate the classical baseline (eld_amd.classical) with this gain in DN per "
                                                                 "electron; a pair's own 'K' in the manifest replaces it for that pair")
    p.add_argument('--baseline-sigma', type=float, metavar='S', help='read noise of the baseline in DN (default: the g_scale line of --baseline-camera)')
    p.add_argument('--baseline-camera', metavar='TABLE', help='a calibrated table (a name or a _params.npy path) the baseline reads its read noise from')
    p.add_argument('--baseline-search', type=int, default=7, metavar='S', help='search radius of the baseline (default 7; bm3d: 12)')
    p.add_argument('--baseline-patch', type=int, default=2, metavar='P', help='patch radius of the baseline (default 2)')
    p.add_argument('--baseline-strength', type=float, default=0.5, metavar='H', help='filter strength of the baseline (default 0.5; bm3d: 1.0)')
    p.add_argument('--baseline-method', choices=('nlm', 'bm3d'), default='nlm', help='the baseline\'s filter (default nlm); it names the added '
                                                                                      'columns and keys: psnr_nlm or psnr_bm3d')
    p.add_argument('--baseline-step', type=int, default=3, metavar='N', help='bm3d: stride of the reference blocks (default 3)')
    p.add_argument('--baseline-group', type=int, default=16, metavar='G', help='bm3d: the largest group (default 16)')
    p.add_argument('--baseline-no-mix', action='store_true', help='bm3d: transform every plane alone')
    return p


def parse_args(argv):
    """-> (argparse namespace, options, pairs).  Precedence: the manifest's fields, then --meta's, then the command line's."""
    from .classical import parse_method_args
    from .denoise import read_sidecar
    a = parse_method_args(build_parser(), argv, 'baseline_method', 'baseline_')
    o, pairs = read_manifest(a.manifest)
    if a.meta:
        side = read_sidecar(a.meta)
        o.update({k: v for k, v in side.items() if k in OPTION_KEYS})
    cli = {'defects': a.defects, 'shading': a.shading, 'flatfield': a.flatfield, 'precision': 'bf16' if a.bf16 else None}
    o.update({k: v for k, v in cli.items() if v is not None})
    o = {k: v for k, v in o.items() if k in OPTION_KEYS}
    from .dng import fill_from_tags
    fill_from_tags(o, [pr[k] for pr in pairs for k in ('short', 'long') if os.path.exists(pr[k])])   # below the manifest and --meta, above the defaults
    o.setdefault('cfa', 'bayer')
    o.setdefault('white_point', 16383)
    o.setdefault('precision', 'fp32')
    if o.get('chop') == 'auto':
        o['chop'] = None
    if (o.get('wb') is None) != (o.get('ccm') is None):
        raise ValueError('the sRGB output needs both wb and ccm')
    if a.save and o.get('wb') is None:
        raise ValueError('--save renders sRGB: the manifest or --meta must hold wb and ccm')
    if o.get('shading') is not None and any(pr.get('iso') is None for pr in pairs):
        raise ValueError('--shading needs iso in every pair')
    if a.baseline_K is None and (a.baseline_sigma is not None or a.baseline_camera is not None):
        raise ValueError('--baseline-sigma and --baseline-camera belong to --baseline-K')
    if a.baseline_K is not None and a.baseline_sigma is None and a.baseline_camera is None:
        raise ValueError('--baseline-K needs --baseline-sigma or --baseline-camera')
    return a, o, pairs


def _saver(outdir, cfa, wb, ccm):
    """on_pair callback: packed-resolution sRGB PNGs through the ISP (util/process.py `process`)."""
    import torch
    from .denoise import colour_args, save_png
    from .isp import process, process_xtrans
    os.makedirs(outdir, exist_ok=True)
    wbs, ccms = colour_args(cfa, wb, ccm, 1)

    def save(i, row, tensors):
        for k, t in tensors.items():
            rgb = (process if cfa == 'bayer' else process_xtrans)(t, torch.from_numpy(wbs).to(t.device), torch.from_numpy(ccms).to(t.device))
            hwc = torch.round(rgb * 255.0).to(torch.uint8)[0].permute(1, 2, 0).contiguous().cpu().numpy()
            save_png(os.path.join(outdir, '%s_%s.png' % (row['name'] or 'pair%03d' % i, k)), hwc)
    return save


def main(argv=None):
    from .denoise import load_denoiser
    from .validate import to_jsonable
    a, o, pairs = parse_args(sys.argv[1:] if argv is None else argv)
    den = load_denoiser(a.ckpt, cfa=o['cfa'], precision=o['precision'])
    base = None
    if a.baseline_K is not None:
        from .classical import ClassicalDenoiser
        base = ClassicalDenoiser(o['cfa'], a.baseline_K, sigma=a.baseline_sigma, camera=a.baseline_camera, search=a.baseline_search,
                                 patch=a.baseline_patch, strength=a.baseline_strength, method=a.baseline_method, step=a.baseline_step,
                                 group=a.baseline_group, mix=False if a.baseline_no_mix else None)
    rep = evaluate_pairs(den, load_pairs(pairs), o['cfa'], raw_pattern=o.get('raw_pattern'), black_level=o.get('black_level'),
                         white_point=o['white_point'], correct=not a.no_correct, crop=a.crop, chop=o.get('chop'), defects=o.get('defects'),
                         shading=o.get('shading'), flatfield=o.get('flatfield'), on_pair=_saver(a.save, o['cfa'], o['wb'], o['ccm']) if a.save else None,
                         baseline=base)
    for line in table_lines(rep['table']):
        print(line)
    print('mean over %d pairs: PSNR %.3f SSIM %.4f (input: %.3f %.4f)' % (len(rep['pairs']), rep['mean']['psnr'], rep['mean']['ssim'],
                                                                          rep['mean']['psnr_in'], rep['mean']['ssim_in']))
    if base is not None and base.label == 'nlm':
        print('classical baseline (search %d, patch %d, strength %g): PSNR %.3f SSIM %.4f' % (base.search, base.patch, base.strength,
                                                                                              rep['mean']['psnr_nlm'], rep['mean']['ssim_nlm']))
    elif base is not None:
        print('classical baseline bm3d (search %d, step %d, group %d, %s, strength %g): PSNR %.3f SSIM %.4f' % (
            base.search, base.step, base.group, 'across the planes' if base.mix else 'every plane alone', base.strength,
            rep['mean']['psnr_bm3d'], rep['mean']['ssim_bm3d']))
    for line in curve_lines(rep['pooled'], rep['groups'], 'nlm' if base is None else base.label):
        print(line)
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(to_jsonable(rep), fh, indent=1)
        print('wrote %s' % a.json)
    return 0


if __name__ == '__main__':
    sys.exit(main())
