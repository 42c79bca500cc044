"""Time eld_burst_stack_u16 on a 24 MP Bayer burst (4000 x 6000) at N = 8, 16 and 64, next to a device-to-device copy
of the same stack timed in the same process: the copy is the yardstick the kernel's rate is read against.

    python tools/burst_time.py [--reps 20] [--warmup 3] [--frames 8,16,64] [--out result.json]

The kernel's rate counts 2 N + 3 bytes per site (N codes read, the mean and the kept count written); the copy's rate counts the 2 N bytes
it reads per site (it writes as many again).  The burst is a static scene with shot and read noise (about 0.4 % of the sites lose a
sample at N = 16), generated on the device from a seed.  Calls alternate; each is timed with device events; medians are printed."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_burst(torch, N, Hm, Wm, seed):
    """scene 5 + 6000 u^2 DN (u rising along the diagonal), K = 2, read noise 3 DN, black 512, clipped to [0, 16383]: uint16 codes as int16"""
    g = torch.Generator(device='cuda').manual_seed(seed)
    yy = torch.arange(Hm, device='cuda', dtype=torch.float32)[:, None]
    xx = torch.arange(Wm, device='cuda', dtype=torch.float32)[None, :]
    scene = 5.0 + 6000.0 * ((xx + 0.37 * yy) / (Wm + 0.37 * Hm)) ** 2
    out = torch.empty((N, Hm, Wm), dtype=torch.int16, device='cuda')
    for f in range(N):                                             # Gaussian shot noise of the Poisson variance: the timing does not need the tails
        z = scene + torch.sqrt(2.0 * scene) * torch.randn((Hm, Wm), device='cuda', generator=g) + 3.0 * torch.randn((Hm, Wm), device='cuda', generator=g)
        out[f] = torch.clamp(torch.round(z + 512.0), 0, 16383).to(torch.int16)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--frames', default='8,16,64')
    ap.add_argument('--size', default='4000x6000')
    ap.add_argument('--out')
    a = ap.parse_args(argv)
    import torch
    import eld_amd
    from eld_amd import _lib as L
    lib = eld_amd.load_library()
    if not torch.cuda.is_available():
        raise RuntimeError('tools/burst_time.py measures on a GPU: there is none')
    Hm, Wm = (int(v) for v in a.size.split('x'))
    st = L.cur_stream()
    grp, blk = (ctypes.c_int * 4)(0, 1, 3, 2), (ctypes.c_int32 * 4)(512, 512, 512, 512)
    res = {'reps': a.reps, 'warmup': a.warmup, 'device': torch.cuda.get_device_name(0), 'src': L.build_src_hash(), 'Hm': Hm, 'Wm': Wm, 'runs': {}}
    for N in [int(v) for v in a.frames.split(',')]:
        fr = make_burst(torch, N, Hm, Wm, N)
        dst = torch.empty_like(fr)
        mean = torch.empty((Hm, Wm), dtype=torch.int16, device='cuda')
        kept = torch.empty((Hm, Wm), dtype=torch.uint8, device='cuda')
        ptc = torch.empty((4, L.PAIRSTATS_BINS, 4), dtype=torch.int64, device='cuda')

        def stack(k2q=100):
            L.check(lib.eld_burst_stack_u16(L.dptr(fr), N, Hm, Wm, 2, grp, 4, blk, 16383, None, k2q, 2, L.dptr(mean), L.dptr(kept), L.dptr(ptc), None, 0, st),
                    'eld_burst_stack_u16')

        calls = (('stack', stack), ('stack_no_rule', lambda: stack(0)), ('copy', lambda: dst.copy_(fr)))
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
        stack()
        torch.cuda.synchronize()
        sites = Hm * Wm
        row = {'sites': sites, 'rejected_share': float((kept != (N % 256)).float().mean()), 'eligible_sites': int(ptc[..., 0].sum())}
        for name, _ in calls:
            t = float(np.median(times[name]))
            nbytes = 2 * N * sites if name == 'copy' else (2 * N + 3) * sites
            row[name] = {'median_s': t, 'p10_s': float(np.percentile(times[name], 10)), 'p90_s': float(np.percentile(times[name], 90)),
                         'bytes': nbytes, 'rate_GBps': nbytes / t * 1e-9}
        row['stack_read_rate_over_copy_read_rate'] = (2 * N * sites / row['stack']['median_s']) / (2 * N * sites / row['copy']['median_s'])
        res['runs'][str(N)] = row
        del fr, dst
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
