"""Per-stage GPU time of eld_amd.denoise on one frame: input stage (pack x ratio clip), U-Net, write-back, sRGB -- a 24 MP Bayer frame
(4032 x 6048, packed 2016 x 3024: whole frame) and a 26 MP X-Trans frame (4160 x 6240, packed 9 x 1386 x 2080: forward_chop), fp32 and
bf16, random-init weights.  Prints one JSON line per case: median milliseconds per stage, the HBM fraction of the write-back and ISP
kernels (their compulsory bytes / time / peak) and the share of the end-to-end time spent outside the U-Net.

    python tools/denoise_bench.py [--reps 10] [--peak-tbs 8.0]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eld_amd import load_library                    # noqa: E402
from eld_amd.denoise import Denoiser, pack_input, run_network, write_back    # noqa: E402
from eld_amd.isp import process, process_xtrans    # noqa: E402
from eld_amd.unet import UNetSeeInDark             # noqa: E402


def timed(fn, reps):
    """median GPU milliseconds of fn() over reps runs (events on the current stream), after one warm-up run"""
    fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def case(cfa, shape, precision, reps, peak):
    torch.manual_seed(0)
    C = 4 if cfa == 'bayer' else 9
    den = Denoiser(UNetSeeInDark(C, C).cuda().requires_grad_(False), cfa, precision)
    den.net.inference_precision = precision
    rng = np.random.default_rng(0)
    u = torch.from_numpy(rng.integers(512, 2048, size=(1,) + shape, dtype=np.uint16).view(np.int16)).cuda()
    pat, blk = ([0, 1, 3, 2], [512.0] * 4) if cfa == 'bayer' else (None, [1024.0])
    ratios = [100.0]
    x = pack_input(u, cfa, pat, blk, 16383.0, ratios)
    out = run_network(den, x)
    mosaic = u.clone()
    wb = torch.tensor([[2.0, 1.0, 1.5, 1.0]] if cfa == 'bayer' else [[2.0, 1.0, 1.5]], device='cuda')
    ccm = torch.eye(3, device='cuda').reshape(1, 3, 3)
    isp = (lambda: process(out, wb, ccm)) if cfa == 'bayer' else (lambda: process_xtrans(out, wb, ccm))
    t_in = timed(lambda: pack_input(u, cfa, pat, blk, 16383.0, ratios), reps)
    t_net = timed(lambda: run_network(den, x), max(3, reps // 3))
    t_wb = timed(lambda: write_back(out, mosaic, cfa, pat, blk, 16383.0, 'nearest'), reps)
    t_isp = timed(isp, reps)
    h, w = out.shape[2:]
    px = shape[0] * shape[1]
    b_in = px * 2 + C * h * w * 4 + 4
    b_wb = C * h * w * 4 + C * h * w * 2                     # every packed value read once, one code written per value
    b_isp = C * h * w * 4 + 3 * h * w * 4
    rest = t_in + t_wb + t_isp
    return {'cfa': cfa, 'mosaic': list(shape), 'packed': [C, h, w], 'precision': precision, 'chop': bool(h % 16 or w % 16),
            'ms': {'input': round(t_in, 4), 'unet': round(t_net, 3), 'write_back': round(t_wb, 4), 'srgb': round(t_isp, 4)},
            'hbm_frac': {'input': round(b_in / (t_in * 1e-3) / (peak * 1e12), 3), 'write_back': round(b_wb / (t_wb * 1e-3) / (peak * 1e12), 3),
                         'srgb': round(b_isp / (t_isp * 1e-3) / (peak * 1e12), 3)},
            'outside_unet_share': round(rest / (rest + t_net), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--peak-tbs', type=float, default=8.0, help='HBM peak, TB/s (MI355X: 8.0)')
    a = ap.parse_args()
    load_library()
    for cfa, shape in (('bayer', (4032, 6048)), ('xtrans', (4160, 6240))):
        for prec in ('fp32', 'bf16'):
            print(json.dumps(case(cfa, shape, prec, a.reps, a.peak_tbs)), flush=True)


if __name__ == '__main__':
    main()
