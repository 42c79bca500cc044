"""GPU time of the defective-pixel kernels (csrc/defect.hip) next to the streaming yardstick eld_unpack_raw_bayer_u16 (4 B in, 2 B out
per site) on the same frame, interleaved in one process: the repair at a defect density of 1e-4 and at zero, out of
place and in place, and the deviation and flag kernels at F = 4.  Frames: Bayer 4032 x 6048, X-Trans 4160 x 6240, and a batch of 8 Bayer
frames (390 MB of codes, beyond the 256 MB Infinity Cache -- the single frames are not).  Event-timed, median of --reps runs, (min, max)
reported.  HBM fraction = compulsory bytes / time / peak.  Writes profiles/defect_bench.json and prints it.

    python tools/defect_bench.py [--reps 10] [--peak-tbs 8.0] [--no-unet]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from eld_amd import _lib as L                       # noqa: E402
from eld_amd import defects as DF                   # noqa: E402
from eld_amd.denoise import Denoiser, pack_input, run_network, write_back    # noqa: E402
from eld_amd.unet import UNetSeeInDark             # noqa: E402


def interleaved(fns, reps):
    """{name: (median, min, max) ms}: every round times each function once, in turn, after two warm-up rounds"""
    for _ in range(2):
        for fn in fns.values():
            fn()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b))
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in ts.items()}


def entry(t, nbytes, peak):
    """nbytes None: time only (the in-place repair touches the flagged groups only: its compulsory traffic depends on the map)"""
    e = {'ms': round(t[0], 4), 'ms_min': round(t[1], 4), 'ms_max': round(t[2], 4)}
    if nbytes is not None:
        e.update(bytes=int(nbytes), hbm_frac=round(nbytes / (t[0] * 1e-3) / (peak * 1e12), 3))
    return e


def case(cfa, N, Hm, Wm, reps, peak, unet):
    rng = np.random.default_rng(0)
    sites = Hm * Wm
    u = torch.from_numpy(rng.integers(400, 700, size=(N, Hm, Wm), dtype=np.uint16).view(np.int16)).cuda()
    out = torch.empty_like(u)
    idx = rng.choice(sites, sites // 10000, replace=False)
    dm = DF.DefectMap.from_sites(np.stack([idx // Wm, idx % Wm], axis=1), (Hm, Wm), cfa)
    empty = DF.DefectMap.from_sites([], (Hm, Wm), cfa)
    packed = torch.rand(N, 4, Hm // 2, Wm // 2, device='cuda')
    pat, blk = (ctypes.c_int * 4)(0, 1, 3, 2), (ctypes.c_float * 4)(512, 512, 512, 512)

    def yard():
        L.check(L.lib().eld_unpack_raw_bayer_u16(L.dptr(packed), L.dptr(out), N, Hm // 2, Wm // 2, pat, blk, 16383.0, L.ROUND_NEAREST, L.cur_stream()))
    fns = {'yardstick_unpack_raw_bayer_u16': yard,
           'repair_1e-4': lambda: DF.repair_device(u, dm, out), 'repair_0': lambda: DF.repair_device(u, empty, out),
           'repair_1e-4_in_place': lambda: DF.repair_device(u, dm, u), 'repair_0_in_place': lambda: DF.repair_device(u, empty, u)}
    bm_bytes = dm.words.nbytes
    nbytes = {'yardstick_unpack_raw_bayer_u16': 6 * N * sites, 'repair_1e-4': 4 * N * sites + bm_bytes, 'repair_0': 4 * N * sites + bm_bytes,
              'repair_1e-4_in_place': None, 'repair_0_in_place': None}
    D = bmap = None
    if N == 1:
        F = 4
        stack = torch.from_numpy(rng.integers(480, 560, size=(F, Hm, Wm), dtype=np.uint16).view(np.int16)).cuda()
        D = DF.deviation(stack, cfa)
        fns['deviation_F4'] = lambda: DF.deviation(stack, cfa)
        fns['flags'] = lambda: DF.flag_bitmap(D, 400, 400)
        nbytes['deviation_F4'] = (2 * F + 4 + 4 + 4) * sites          # stack in, S out, S in (once: the taps come from cache), D out
        nbytes['flags'] = 4 * sites + bm_bytes
    t = interleaved(fns, reps)
    res = {'cfa': cfa, 'frames': N, 'mosaic': [Hm, Wm], 'codes_mb': round(2 * N * sites / 1e6, 1), 'defects': dm.count,
           'infinity_cache_resident': 2 * 2 * N * sites <= 256e6}
    for k in fns:
        res[k] = entry(t[k], nbytes[k], peak)
    expected = t['yardstick_unpack_raw_bayer_u16'][0] * (4 * N * sites + bm_bytes) / (6 * N * sites)
    res['repair_expected_ms'] = round(expected, 4)
    res['repair_1e-4_measured_over_expected'] = round(t['repair_1e-4'][0] / expected, 3)
    res['repair_0_measured_over_expected'] = round(t['repair_0'][0] / expected, 3)
    if unet and N == 1:
        f = 2 if cfa == 'bayer' else 3
        C = 4 if cfa == 'bayer' else 9
        net = UNetSeeInDark(C, C).cuda().requires_grad_(False)
        b = [512.0] * 4 if cfa == 'bayer' else [1024.0]
        p = [0, 1, 3, 2] if cfa == 'bayer' else None
        hw = (Hm // 2 // 16 * 16, Wm // 2 // 16 * 16) if cfa == 'bayer' else (2 * (Hm // 6) // 16 * 16, 2 * (Wm // 6) // 16 * 16)
        v = u[:, :hw[0] * f, :hw[1] * f].contiguous()          # whole-frame U-Net: packed sides cut to multiples of 16
        dmv = DF.DefectMap.from_sites(dm.sites[(dm.sites[:, 0] < v.shape[1]) & (dm.sites[:, 1] < v.shape[2])], tuple(v.shape[1:]), cfa)
        mosaic = v.clone()
        share = {}
        for prec in ('fp32', 'bf16'):
            net.inference_precision = prec                    # what load_denoiser sets: the network reads it per call
            den = Denoiser(net, cfa, prec)
            x = pack_input(v, cfa, p, b, 16383.0, [100.0])
            with torch.no_grad():
                o = run_network(den, x)
            tt = interleaved({'net': lambda: run_network(den, x), 'input': lambda: pack_input(v, cfa, p, b, 16383.0, [100.0]),
                              'write_back': lambda: write_back(o, mosaic, cfa, p, b, 16383.0, 'nearest'),
                              'repair': lambda: DF.repair_device(v, dmv)}, max(3, reps // 3))
            rest = tt['input'][0] + tt['write_back'][0] + tt['repair'][0]
            share[prec] = {'unet_ms': round(tt['net'][0], 3), 'input_ms': round(tt['input'][0], 4), 'write_back_ms': round(tt['write_back'][0], 4),
                           'repair_ms': round(tt['repair'][0], 4), 'outside_unet_share_with_defects': round(rest / (rest + tt['net'][0]), 4)}
        res['denoise'] = share
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--peak-tbs', type=float, default=8.0, help='HBM peak, TB/s (MI355X: 8.0)')
    ap.add_argument('--no-unet', action='store_true', help='kernels only: skip the U-Net timing of the denoise share')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'defect_bench.json'))
    a = ap.parse_args()
    L.load_library()
    if not torch.cuda.is_available():
        raise SystemExit('tools/defect_bench.py measures on a GPU: none found')
    res = {'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'peak_tbs': a.peak_tbs,
           'cases': [case('bayer', 1, 4032, 6048, a.reps, a.peak_tbs, not a.no_unet), case('xtrans', 1, 4160, 6240, a.reps, a.peak_tbs, not a.no_unet),
                     case('bayer', 8, 4032, 6048, a.reps, a.peak_tbs, False)]}
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
