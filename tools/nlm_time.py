"""Time eld_nlm_vst_f32 on one Bayer frame (4 x 1424 x 2128 packed planes) and one 9-plane frame (9 x 1328 x 2000) at
(S, P) = (7, 1), (7, 2), (7, 3) and (10, 2), next to the U-Net fp32 forward of the same frame and a device-to-device copy of it, all in one
process: calls alternate, each is timed with device events, medians are printed.

    python tools/nlm_time.py [--reps 10] [--warmup 3] [--out result.json]

The kernel's integer work is derived from its three passes (op_counts below): per site and offset, with r = 1 + 2P / 32 the side of the
tile extended by the patch radius over the side of the tile,
    vector ALU   3 C r^2 (subtract, clamp, multiply-add of pass 1) + 2P r (row sums) + (2P + 6) / 4 (running column sum)
                 + 4 (shift, min, candidate mask, denominator) + C (numerators)
    LDS          2 C r^2 + r^2 (pass 1) + (2P + 2) r (pass 2) + (2P + 7) / 4 + 1 + C (pass 3) reads and writes of one lane
The bounds are those counts over the chip's rates: 256 CUs x 4 SIMDs x 32 lanes per clock for the vector ALU and 32 lanes per clock and CU
for 16- and 32-bit LDS accesses, at 2.4 GHz.  The frame is a noisy ramp generated on the device from a seed."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = ((7, 1), (7, 2), (7, 3), (10, 2))
FRAMES = (('bayer', 4, 1424, 2128), ('xtrans', 9, 1328, 2000))
CLOCK_HZ, CUS = 2.4e9, 256
VALU_LANES_PER_S = CUS * 4 * 32 * CLOCK_HZ
LDS_LANES_PER_S = CUS * 32 * CLOCK_HZ


def op_counts(C, S, P):
    """-> (vector-ALU operations, LDS accesses) of one lane per site, all offsets"""
    r = 1.0 + 2.0 * P / 32.0
    valu = 3 * C * r * r + 2 * P * r + (2 * P + 6) / 4.0 + 4 + C
    lds = 2 * C * r * r + r * r + (2 * P + 2) * r + (2 * P + 7) / 4.0 + 1 + C
    n = (2 * S + 1) ** 2
    return valu * n, lds * n


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
        raise RuntimeError('tools/nlm_time.py measures on a GPU: there is none')
    res = {'reps': a.reps, 'warmup': a.warmup, 'device': torch.cuda.get_device_name(0), 'src': L.build_src_hash(), 'frames': {}}
    for cfa, C, h, w in FRAMES:
        x = make_frame(torch, C, h, w, C)
        fwd = torch.from_numpy(Cl.vst_tables(2.0, 3.0, [512] * C).view(np.int16)).cuda()
        out = torch.empty((1, C, h, w), dtype=torch.int32, device='cuda')
        dst = torch.empty_like(x)
        torch.manual_seed(1)
        den = load_denoiser(UNetSeeInDark(C, C), cfa=cfa)

        def nlm(S, P):
            sh, wtab = Cl.nlm_weight_table(C, P, 0.5)
            return lambda: Cl.nlm_vst(x, 65535.0, fwd, S, P, sh, wtab, Cl.FRAC, out=out)

        def unet():
            return run_network(den, x, chop=False)

        calls = [('nlm_S%d_P%d' % sp, nlm(*sp)) for sp in CONFIGS] + [('unet_fp32_forward', unet), ('copy', lambda: dst.copy_(x))]
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
        sites = h * w
        row = {'C': C, 'h': h, 'w': w, 'sites': sites}
        for name, _ in calls:
            t = float(np.median(times[name]))
            row[name] = {'median_s': t, 'p10_s': float(np.percentile(times[name], 10)), 'p90_s': float(np.percentile(times[name], 90))}
        for S, P in CONFIGS:
            k = row['nlm_S%d_P%d' % (S, P)]
            valu, lds = op_counts(C, S, P)
            k['valu_ops_per_site'], k['lds_ops_per_site'] = valu, lds
            k['valu_bound_s'], k['lds_bound_s'] = valu * sites / VALU_LANES_PER_S, lds * sites / LDS_LANES_PER_S
            k['valu_bound_fraction'] = k['valu_bound_s'] / k['median_s']
            k['lds_bound_fraction'] = k['lds_bound_s'] / k['median_s']
            k['ns_per_site_offset'] = k['median_s'] * 1e9 / (sites * (2 * S + 1) ** 2)
        row['P3_over_P1'] = {'measured': row['nlm_S7_P3']['median_s'] / row['nlm_S7_P1']['median_s'],
                             'from_valu_count': op_counts(C, 7, 3)[0] / op_counts(C, 7, 1)[0],
                             'from_lds_count': op_counts(C, 7, 3)[1] / op_counts(C, 7, 1)[1],
                             'of_re_summing_the_patch': 49.0 / 9.0}
        row['copy']['rate_GBps'] = 8.0 * C * sites / row['copy']['median_s'] * 1e-9            # 4 bytes read and 4 written per value
        res['frames'][cfa] = row
        del x, fwd, out, dst, den
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
