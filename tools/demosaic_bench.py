"""GPU time of the full-resolution renders (csrc/demosaic.hip) on the two frames of DESIGN.md sec. 11 -- Bayer 4 x 2016 x 3024 and
X-Trans 9 x 1386 x 2080 -- next to the packed-resolution ISP kernels (eld_isp_process / eld_isp_process_xtrans) on the same frames in
the same process, and the share of a denoise call spent outside the U-Net with srgb_size='full'.  Event-timed, median of --reps runs,
spread (min, max) reported.  Writes profiles/demosaic_bench.json and prints it.

    python tools/demosaic_bench.py [--reps 10] [--peak-tbs 8.0] [--no-unet]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from eld_amd import load_library                    # noqa: E402
from eld_amd.denoise import Denoiser, pack_input, run_network, write_back    # noqa: E402
from eld_amd.isp import process, process_xtrans, render_bayer, render_xtrans    # noqa: E402
from eld_amd.unet import UNetSeeInDark             # noqa: E402


def timed(fn, reps):
    """(median, min, max) GPU milliseconds of fn() over reps runs (events on the current stream), after two warm-up runs"""
    fn()
    fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def entry(t, nbytes, peak):
    return {'ms': round(t[0], 4), 'ms_min': round(t[1], 4), 'ms_max': round(t[2], 4), 'bytes': int(nbytes),
            'hbm_frac': round(nbytes / (t[0] * 1e-3) / (peak * 1e12), 3)}


def case(cfa, packed_shape, reps, peak, unet):
    torch.manual_seed(0)
    C, h, w = packed_shape
    f = 2 if cfa == 'bayer' else 3
    out = torch.rand(1, C, h, w, device='cuda') * 1.2 - 0.1
    wb = torch.tensor([[2.0, 1.0, 1.5, 1.0]] if cfa == 'bayer' else [[2.0, 1.0, 1.5]], device='cuda')
    ccm = torch.tensor([[1.6, -0.4, -0.2], [-0.2, 1.5, -0.3], [0.0, -0.5, 1.5]], device='cuda').reshape(1, 3, 3)
    pat = [0, 1, 3, 2]
    if cfa == 'bayer':
        full = lambda **kw: render_bayer(out, pat, wb, ccm, **kw)             # noqa: E731
        base = lambda: process(out, wb, ccm)                                  # noqa: E731
    else:
        full = lambda **kw: render_xtrans(out, wb, ccm, **kw)                 # noqa: E731
        base = lambda: process_xtrans(out, wb, ccm)                           # noqa: E731
    sites = f * f * h * w
    res = {'cfa': cfa, 'packed': [C, h, w], 'render': [3, f * h, f * w],
           'full_srgb8': entry(timed(full, reps), C * h * w * 4 + 3 * sites, peak),
           'full_linear_f32': entry(timed(lambda: full(linear=True), reps), C * h * w * 4 + 12 * sites, peak),
           'packed_isp': entry(timed(base, reps), C * h * w * 4 + 12 * h * w, peak)}
    res['full_srgb8_vs_packed_isp_frac'] = round(res['full_srgb8']['hbm_frac'] / res['packed_isp']['hbm_frac'], 3)
    if unet:
        den = Denoiser(UNetSeeInDark(C, C).cuda().requires_grad_(False), cfa, 'fp32')
        blk = [512.0] * 4 if cfa == 'bayer' else [1024.0]
        u = torch.from_numpy(np.random.default_rng(0).integers(512, 2048, size=(1, f * h, f * w), dtype=np.uint16).view(np.int16)).cuda()
        mosaic = u.clone()
        share = {}
        for prec in ('fp32', 'bf16'):
            den.precision = den.net.inference_precision = prec
            x = pack_input(u, cfa, pat if cfa == 'bayer' else None, blk, 16383.0, [100.0])
            t_net = timed(lambda: run_network(den, x), max(3, reps // 3))[0]
            t_in = timed(lambda: pack_input(u, cfa, pat if cfa == 'bayer' else None, blk, 16383.0, [100.0]), reps)[0]
            t_wb = timed(lambda: write_back(out, mosaic, cfa, pat if cfa == 'bayer' else None, blk, 16383.0, 'nearest'), reps)[0]
            rest = t_in + t_wb + res['full_srgb8']['ms']
            share[prec] = {'unet_ms': round(t_net, 3), 'input_ms': round(t_in, 4), 'write_back_ms': round(t_wb, 4),
                           'outside_unet_share_full': round(rest / (rest + t_net), 4)}
        res['denoise'] = share
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--peak-tbs', type=float, default=8.0, help='HBM peak, TB/s (MI355X: 8.0)')
    ap.add_argument('--no-unet', action='store_true', help='kernels only: skip the U-Net timing of the denoise share')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'demosaic_bench.json'))
    a = ap.parse_args()
    load_library()
    res = {'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'peak_tbs': a.peak_tbs,
           'cases': [case('bayer', (4, 2016, 3024), a.reps, a.peak_tbs, not a.no_unet),
                     case('xtrans', (9, 1386, 2080), a.reps, a.peak_tbs, not a.no_unet)]}
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
