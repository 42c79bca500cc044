"""Time eld_tile_noise_sums_u16 on one 24 MP Bayer frame (4000 x 6000, stride 2, four groups) and one 26 MP X-Trans
frame (4160 x 6240, the greens at stride 3), on a synthetic raw frame (a signal ramp with Poisson-Gaussian noise).  Next to each time stand
two yardsticks: the 2 bytes per site the pass must read over the HBM peak, and a device-to-device copy of the same frame (which moves 4
bytes per site, 2 read and 2 written), timed in the same process.

    python tools/noiselevel_time.py [--reps 30] [--warmup 5] [--out result.json]

The calls alternate inside one process; each is timed with device events around one call.  Prints the median, the 10th and 90th
percentile per call, and the ratio of the medians."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12      # bytes / s, MI355X
XT_COLOUR = [0, 2, 1, 2, 0, 1, 1, 1, 0, 1, 1, 2, 1, 1, 2, 1, 1, 0, 2, 0, 1, 0, 2, 1, 1, 1, 2, 1, 1, 0, 1, 1, 0, 1, 1, 2]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out')
    a = ap.parse_args(argv)
    import torch
    import eld_amd
    from eld_amd import _lib as L
    from eld_amd.noiselevel import TILE, tiles_along
    lib = eld_amd.load_library()
    if not torch.cuda.is_available():
        raise RuntimeError('tools/noiselevel_time.py measures on a GPU: there is none')
    g = torch.Generator(device='cuda').manual_seed(1)
    st = L.cur_stream()
    calls = []
    for cfa, Hm, Wm, p, s, group, G, black in (('bayer', 4000, 6000, 2, 2, [0, 1, 3, 2], 4, 512),
                                               ('xtrans', 4160, 6240, 6, 3, [c if c == 1 else -1 for c in XT_COLOUR], 3, 1024)):
        ramp = 4.0 * 1500.0 ** (torch.arange(Wm, device='cuda', dtype=torch.float32) / (Wm - 1))                # electrons, 4 -> 6000
        e = ramp[None, :].expand(Hm, Wm)
        u = 2.0 * (e + e.sqrt() * torch.randn((Hm, Wm), device='cuda', generator=g)) + 3.0 * torch.randn((Hm, Wm), device='cuda', generator=g) + black
        frame = u.round().clamp(0, 16383).to(torch.int32).to(torch.int16).reshape(1, Hm, Wm).contiguous()
        del u, e
        Hc, Wc = Hm // p * p, Wm // p * p
        out = torch.empty((1, tiles_along(Hc, s), tiles_along(Wc, s), G, 4), dtype=torch.int64, device='cuda')
        dst = torch.empty_like(frame)
        grp = (ctypes.c_int * (p * p))(*group)
        blk = (ctypes.c_int32 * (p * p))(*([black] * (p * p)))

        def sums(frame=frame, Hm=Hm, Wm=Wm, Hc=Hc, Wc=Wc, p=p, s=s, grp=grp, G=G, blk=blk, out=out):
            L.check(lib.eld_tile_noise_sums_u16(L.dptr(frame), 1, Hm, Wm, Hc, Wc, p, s, grp, G, blk, 16383, None, L.dptr(out), None, 0, st),
                    'eld_tile_noise_sums_u16')

        def copy(frame=frame, dst=dst):
            dst.copy_(frame)

        calls.append((cfa, sums, copy, Hm * Wm, out, s))
    times = {}
    for i in range(a.warmup + a.reps):
        for name, sums, copy, _, _, _ in calls:
            for kind, fn in (('sums', sums), ('copy', copy)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if i >= a.warmup:
                    times.setdefault((name, kind), []).append(e0.elapsed_time(e1) * 1e3)
    res = {'reps': a.reps, 'warmup': a.warmup, 'hbm_peak': HBM_PEAK, 'device': torch.cuda.get_device_name(0), 'src': L.build_src_hash()}
    for name, _, _, sites, out, s in calls:
        n = int(out[..., 0].sum())
        assert n > 0
        row = {'sites': sites, 'stride': s, 'tile': TILE * s, 'tiles': int(out.shape[1] * out.shape[2]), 'eligible_sites': n,
               'hbm_bound_us': 2.0 * sites / HBM_PEAK * 1e6}
        for kind in ('sums', 'copy'):
            t = np.asarray(times[(name, kind)])
            row[kind] = {'median_us': float(np.median(t)), 'p10_us': float(np.percentile(t, 10)), 'p90_us': float(np.percentile(t, 90))}
        row['sums_over_copy'] = row['sums']['median_us'] / row['copy']['median_us']
        row['sums_over_bound'] = row['sums']['median_us'] / row['hbm_bound_us']
        res[name] = row
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
