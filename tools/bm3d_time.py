"""Time eld_bm3d_vst_f32 on the two frames of tools/nlm_time.py -- one Bayer frame (4 x 1424 x 2128 packed planes, grouped
across the planes) and one 9-plane frame (9 x 1328 x 2000, every plane alone) -- at the defaults of ClassicalDenoiser(method='bm3d'): S = 12,
step 3, groups of up to 16.  Step 1 and step 2 are timed apart, next to non-local means at its defaults, the U-Net fp32 forward of the same
frame and a device-to-device copy of it, all in one process: calls alternate, each is timed with device events, medians and the 10th to
90th percentile are printed.

    python tools/bm3d_time.py [--reps 10] [--warmup 3] [--out result.json]

Counts per reference block (op_counts below), with n = (2S + 1)^2 candidates away from the edges, C planes, sets of M planes, L = 64 M G
values per set and G = 16 (an upper bound: smaller groups do less):
    matching     n 64 C differences: 2 LDS reads (16-bit) and 4 vector operations (subtract, clamp, multiply, add) each
    transforms   2 per set in step 1 and 3 in step 2, log2(L) / 2 radix-4 passes each: 2 L LDS accesses and 2 L additions per pass
    atomics      G 64 (C + C / M) 64-bit adds of 8 bytes: numerators of every plane, one denominator per set
The frame is the noisy ramp of tools/nlm_time.py, generated on the device from a seed."""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FRAMES = (('bayer', 4, 1424, 2128), ('xtrans', 9, 1328, 2000))


def grid_count(n, step):
    return (n - 8) // step + 1 + ((n - 8) % step != 0)


def op_counts(C, h, w, S, step, G, mix, wiener):
    """-> counts over the whole frame: reference blocks, matching differences, transform butterfly values, atomic adds and their bytes"""
    blocks = grid_count(h, step) * grid_count(w, step)
    M = C if mix else 1
    sets = C // M
    L = 64 * M * G
    passes = math.ceil(math.log2(L) / 2.0)
    transforms = 3 if wiener else 2
    atomics = G * 64 * (C + sets)
    return {'blocks': blocks, 'match_differences': blocks * (2 * S + 1) ** 2 * 64 * C, 'transform_values': blocks * sets * transforms * passes * L,
            'atomic_adds': blocks * atomics, 'atomic_bytes': blocks * atomics * 8}


def make_frame(torch, C, h, w, seed):
    """codes / 65535 of a ramp of 1 to 60 DN above black 512 with K = 2 shot noise (Gaussian of the Poisson variance) and 3 DN of read noise"""
    g = torch.Generator(device='cuda').manual_seed(seed)
    yy = torch.arange(h, device='cuda', dtype=torch.float32)[:, None]
    xx = torch.arange(w, device='cuda', dtype=torch.float32)[None, :]
    scene = (1.0 + 59.0 * ((xx + 0.37 * yy) / (w + 0.37 * h)) ** 2).expand(1, C, h, w)
    z = scene + torch.sqrt(2.0 * scene) * torch.randn((1, C, h, w), device='cuda', generator=g) + 3.0 * torch.randn((1, C, h, w), device='cuda', generator=g)
    return (torch.clamp(torch.round(z + 512.0), 0, 16383) / 65535.0).contiguous()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out')
    a = ap.parse_args(argv)
    import torch
    import eld_amd
    from eld_amd import _lib as L
    from eld_amd import classical as Cl
    from eld_amd.denoise import load_denoiser, run_network
    from eld_amd.unet import UNetSeeInDark
    eld_amd.load_library()
    if not torch.cuda.is_available():
        raise RuntimeError('tools/bm3d_time.py measures on a GPU: there is none')
    res = {'reps': a.reps, 'warmup': a.warmup, 'device': torch.cuda.get_device_name(0), 'src': L.build_src_hash(), 'frames': {}}
    for cfa, C, h, w in FRAMES:
        x = make_frame(torch, C, h, w, C)
        fwd = torch.from_numpy(Cl.vst_tables(2.0, 3.0, [512] * C).view(np.int16)).cuda()
        bm = Cl.ClassicalDenoiser(cfa, 2.0, sigma=3.0, method='bm3d')
        nl = Cl.ClassicalDenoiser(cfa, 2.0, sigma=3.0)
        tau1, thr, tau2, s2, win = bm.tables
        first = torch.empty((1, C, h, w), dtype=torch.int32, device='cuda')
        out = torch.empty_like(first)
        dst = torch.empty_like(x)
        torch.manual_seed(1)
        den = load_denoiser(UNetSeeInDark(C, C), cfa=cfa)
        calls = [('bm3d_step1', lambda: Cl.bm3d_vst(x, 65535.0, fwd, None, bm.search, bm.step, bm.group, bm.mix, tau1, thr, win, Cl.FRAC, out=first)),
                 ('bm3d_step2', lambda: Cl.bm3d_vst(x, 65535.0, fwd, first, bm.search, bm.step, bm.group, bm.mix, tau2, s2, win, Cl.FRAC, out=out)),
                 ('nlm_defaults', lambda: Cl.nlm_vst(x, 65535.0, fwd, nl.search, nl.patch, nl.sh, nl.wtab, Cl.FRAC, out=out)),
                 ('unet_fp32_forward', lambda: run_network(den, x, chop=False)),
                 ('copy', lambda: dst.copy_(x))]
        times = {k: [] for k, _ in calls}
        for i in range(a.warmup + a.reps):
            for name, fn in calls:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if i >= a.warmup:
                    times[name].append(e0.elapsed_time(e1) * 1e-3)
        row = {'C': C, 'h': h, 'w': w, 'sites': h * w, 'search': bm.search, 'step': bm.step, 'group': bm.group, 'mix': bm.mix}
        for name, _ in calls:
            t = float(np.median(times[name]))
            row[name] = {'median_s': t, 'p10_s': float(np.percentile(times[name], 10)), 'p90_s': float(np.percentile(times[name], 90))}
        for name, wiener in (('bm3d_step1', False), ('bm3d_step2', True)):
            k = row[name]
            k.update(op_counts(C, h, w, bm.search, bm.step, bm.group, bm.mix, wiener))
            k['us_per_block'] = k['median_s'] * 1e6 / k['blocks']
            k['atomic_GBps_at_most'] = k['atomic_bytes'] / k['median_s'] * 1e-9
            k['atomic_Gadds_per_s_at_most'] = k['atomic_adds'] / k['median_s'] * 1e-9
        row['bm3d_both_steps_s'] = row['bm3d_step1']['median_s'] + row['bm3d_step2']['median_s']
        row['copy']['rate_GBps'] = 8.0 * C * h * w / row['copy']['median_s'] * 1e-9               # 4 bytes read and 4 written per value
        res['frames'][cfa] = row
        del x, fwd, first, out, dst, den
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
