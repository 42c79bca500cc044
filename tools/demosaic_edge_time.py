"""GPU time of the edge-directed Bayer render (csrc/demosaic_edge.hip eld_render_bayer_edge) on the Bayer frame of
DESIGN.md sec. 11, 4 x 2016 x 3024 packed = 4032 x 6048 mosaic sites, next to its yardsticks in the same process: eld_render_bayer
(Malvar-He-Cutler) in both output modes and a device-to-device copy of the packed frame.  The calls alternate; each is timed with device
events around one call that goes straight to the library with arguments prepared beforehand; median of --reps runs after --warmup, spread
(min, max) reported.  `hbm_frac` is the compulsory traffic (the packed frame read once, the output written once) over the time, as a fraction
of --peak-tbs.  Unless --no-unet, the share of one `denoise --srgb-size full` call (input stage, U-Net, write-back, render) that the render
takes, for both demosaics.  Writes profiles/demosaic_edge_bench.json and prints it.

    python tools/demosaic_edge_time.py [--reps 10] [--warmup 3] [--peak-tbs 8.0] [--no-unet] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 2016, 3024                        # packed


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--peak-tbs', type=float, default=8.0, help='HBM peak, TB/s (MI355X: 8.0)')
    ap.add_argument('--no-unet', action='store_true', help='kernels only: skip the share of a denoise call')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'demosaic_edge_bench.json'))
    a = ap.parse_args(argv)
    import torch
    import eld_amd
    from eld_amd import _lib as L
    eld_amd.load_library()
    if not torch.cuda.is_available():
        raise RuntimeError('tools/demosaic_edge_time.py measures on a GPU: there is none')
    g = torch.Generator(device='cuda').manual_seed(1)
    packed = torch.rand((1, 4, H, W), device='cuda', generator=g) * 1.2 - 0.1
    wbs = torch.tensor([[2.0, 1.0, 1.5, 1.0]], device='cuda')
    ccm = torch.tensor([[1.6, -0.4, -0.2, -0.2, 1.5, -0.3, 0.0, -0.5, 1.5]], device='cuda')
    out8 = torch.empty((1, 3, 2 * H, 2 * W), dtype=torch.uint8, device='cuda')
    out32 = torch.empty((1, 3, 2 * H, 2 * W), dtype=torch.float32, device='cuda')
    dst = torch.empty_like(packed)
    lib, st = L.lib(), L.cur_stream()
    pat = (ctypes.c_int * 4)(0, 1, 3, 2)

    def render(name, o, mode):
        fn = getattr(lib, name)
        return lambda: L.check(fn(L.dptr(packed), pat, L.dptr(wbs), L.dptr(ccm), L.dptr(o), mode, 1, H, W, 2.2, None, None, 0, st), name)
    sites = 4 * H * W
    calls = {'edge_srgb8': (render('eld_render_bayer_edge', out8, L.RENDER_SRGB8), 4 * sites + 3 * sites),
             'edge_linear_f32': (render('eld_render_bayer_edge', out32, L.RENDER_LINEAR_F32), 4 * sites + 12 * sites),
             'mhc_srgb8': (render('eld_render_bayer', out8, L.RENDER_SRGB8), 4 * sites + 3 * sites),
             'mhc_linear_f32': (render('eld_render_bayer', out32, L.RENDER_LINEAR_F32), 4 * sites + 12 * sites),
             'copy_packed': (lambda: dst.copy_(packed), 8 * sites)}
    times = {k: [] for k in calls}
    for i in range(a.warmup + a.reps):
        for kind, (fn, _) in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                times[kind].append(e0.elapsed_time(e1) * 1e3)
    res = {'device': torch.cuda.get_device_name(0), 'src': L.build_src_hash(), 'reps': a.reps, 'warmup': a.warmup, 'peak_tbs': a.peak_tbs,
           'packed': [4, H, W], 'render': [3, 2 * H, 2 * W]}
    tile = [ctypes.c_int(), ctypes.c_int(), ctypes.c_int()]
    L.check(lib.eld_render_bayer_edge_tile(*[ctypes.byref(t) for t in tile]), 'eld_render_bayer_edge_tile')
    res['tile'], res['lds_bytes'] = [tile[0].value, tile[1].value], tile[2].value
    for kind, (_, nbytes) in calls.items():
        t = np.asarray(times[kind])
        res[kind] = {'median_us': round(float(np.median(t)), 2), 'min_us': round(float(t.min()), 2), 'max_us': round(float(t.max()), 2),
                     'bytes': nbytes, 'hbm_frac': round(nbytes / (float(np.median(t)) * 1e-6) / (a.peak_tbs * 1e12), 3)}
    res['ratios'] = {'edge_srgb8_over_mhc_srgb8': round(res['edge_srgb8']['median_us'] / res['mhc_srgb8']['median_us'], 3),
                     'edge_linear_over_mhc_linear': round(res['edge_linear_f32']['median_us'] / res['mhc_linear_f32']['median_us'], 3),
                     'edge_srgb8_over_copy': round(res['edge_srgb8']['median_us'] / res['copy_packed']['median_us'], 3),
                     'edge_linear_over_copy': round(res['edge_linear_f32']['median_us'] / res['copy_packed']['median_us'], 3),
                     'mhc_srgb8_over_copy': round(res['mhc_srgb8']['median_us'] / res['copy_packed']['median_us'], 3)}
    if not a.no_unet:
        from eld_amd.denoise import Denoiser, pack_input, run_network, write_back
        from eld_amd.unet import UNetSeeInDark
        den = Denoiser(UNetSeeInDark(4, 4).cuda().requires_grad_(False), 'bayer', 'fp32')
        u = torch.from_numpy(np.random.default_rng(0).integers(512, 2048, size=(1, 2 * H, 2 * W), dtype=np.uint16).view(np.int16)).cuda()
        mosaic = u.clone()
        p4, blk = [0, 1, 3, 2], [512.0] * 4

        def timed(fn, reps):
            fn()
            ts = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3)
            return float(np.median(ts))
        share = {}
        for prec in ('fp32', 'bf16'):
            den.precision = den.net.inference_precision = prec
            x = pack_input(u, 'bayer', p4, blk, 16383.0, [100.0])
            t_net = timed(lambda: run_network(den, x), 3)
            t_in = timed(lambda: pack_input(u, 'bayer', p4, blk, 16383.0, [100.0]), a.reps)
            t_wb = timed(lambda: write_back(packed, mosaic, 'bayer', p4, blk, 16383.0, 'nearest'), a.reps)
            rest = t_net + t_in + t_wb
            share[prec] = {'unet_us': round(t_net, 1), 'input_us': round(t_in, 1), 'write_back_us': round(t_wb, 1),
                           'render_share_edge': round(res['edge_srgb8']['median_us'] / (rest + res['edge_srgb8']['median_us']), 5),
                           'render_share_mhc': round(res['mhc_srgb8']['median_us'] / (rest + res['mhc_srgb8']['median_us']), 5)}
        res['denoise_full'] = share
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))
    return 0


if __name__ == '__main__':
    sys.exit(main())
