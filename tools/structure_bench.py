"""Time eld_struct_sums_u16 against eld_hist_u16 (R = 256) on one stack: 3 Bayer frames of 3000 x 4000 by default.

    python tools/structure_bench.py [--frames 3] [--height 3000] [--width 4000] [--reps 50] [--warmup 10] [--out result.json]

The two calls alternate inside one process; each is timed with device events around one call (its zeroing kernels included).  Prints the
median, the 10th and 90th percentile and the bytes read over the median as a share of the HBM peak."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12      # bytes / s, MI355X


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--frames', type=int, default=3)
    ap.add_argument('--height', type=int, default=3000)
    ap.add_argument('--width', type=int, default=4000)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--out')
    a = ap.parse_args(argv)
    import torch
    import eld_amd
    from eld_amd import _lib as L
    lib = eld_amd.load_library()
    F, Hm, Wm, R, p = a.frames, a.height, a.width, 256, 2
    g = torch.Generator(device='cuda').manual_seed(1)
    u = (512 + 6 * torch.randn((F, Hm, Wm), device='cuda', generator=g)).round().clamp(0, 65535).to(torch.int32).to(torch.uint16)
    cen = (ctypes.c_int32 * 4)(512, 512, 512, 512)
    grp = (ctypes.c_int * 4)(0, 1, 3, 2)
    row = torch.empty((F, Hm, p, 2), dtype=torch.int64, device='cuda')
    col = torch.empty((F, Wm, p, 2), dtype=torch.int64, device='cuda')
    cell = torch.empty((F, p * p, 3), dtype=torch.int64, device='cuda')
    counts = torch.empty((F, 4, 2 * R + 1), dtype=torch.int64, device='cuda')
    s = L.cur_stream()

    def sums():
        L.check(lib.eld_struct_sums_u16(L.dptr(u), F, Hm, Wm, p, cen, None, L.dptr(row), L.dptr(col), L.dptr(cell), s), 'eld_struct_sums_u16')

    def hist():
        L.check(lib.eld_hist_u16(L.dptr(u), None, F, Hm, Wm, p, grp, 4, cen, R, None, L.dptr(counts), s), 'eld_hist_u16')

    times = {'struct_sums': [], 'hist_u16': []}
    for i in range(a.warmup + a.reps):
        for name, fn in (('struct_sums', sums), ('hist_u16', hist)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    assert int(cell[:, :, 0].sum()) == F * Hm * Wm and int(counts.sum()) == F * Hm * Wm
    nbytes = 2.0 * F * Hm * Wm
    res = {'frames': F, 'height': Hm, 'width': Wm, 'radius': R, 'reps': a.reps, 'bytes_read': nbytes}
    for name, t in times.items():
        t = np.asarray(t)
        med = float(np.median(t))
        res[name] = {'median_us': med, 'p10_us': float(np.percentile(t, 10)), 'p90_us': float(np.percentile(t, 90)),
                     'hbm_share': nbytes / (med * 1e-6) / HBM_PEAK}
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
