"""Time eld_pair_level_stats_u16 on one 24 MP Bayer frame (4000 x 6000) and one 26 MP X-Trans frame (4160 x 6240), for
two contents: uniform-random codes, and a dark frame with every site within +-4 DN of black (nearly all sites of a wave in one or two
bins: the contention case).  Next to each time stand two yardsticks: the 4 bytes per site the kernel reads over the HBM peak, and
eld_hist_u16 (the existing kernel of the same kind: one LDS add per site, 2 bytes read) on the reference frame, timed in the same process.

    python tools/pairstats_bench.py [--reps 30] [--warmup 5] [--out result.json]

The calls alternate inside one process; each is timed with device events around one call.  Prints the median, the 10th and 90th
percentile per call."""
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
    lib = eld_amd.load_library()
    if not torch.cuda.is_available():
        raise RuntimeError('tools/pairstats_bench.py measures on a GPU: there is none')
    g = torch.Generator(device='cuda').manual_seed(1)
    st = L.cur_stream()
    NB = L.PAIRSTATS_BINS
    calls = []
    for cfa, Hm, Wm, p, group, G, black in (('bayer', 4000, 6000, 2, [0, 1, 3, 2], 4, 512), ('xtrans', 4160, 6240, 6, XT_COLOUR, 3, 1024)):
        for content in ('random', 'dark'):
            if content == 'random':
                ref = torch.randint(0, 65536, (1, Hm, Wm), device='cuda', generator=g, dtype=torch.int32)
                white = 65535
            else:
                ref = black + torch.randint(-4, 5, (1, Hm, Wm), device='cuda', generator=g, dtype=torch.int32)
                white = 16383
            est = (ref + torch.randint(-3, 4, (1, Hm, Wm), device='cuda', generator=g, dtype=torch.int32)).clamp(0, 65535)
            ref, est = ref.to(torch.int16), est.to(torch.int16)                    # the low 16 bits: the codes
            out = torch.empty((1, G, NB, 4), dtype=torch.int64, device='cuda')
            counts = torch.empty((1, G, 2 * 1024 + 1), dtype=torch.int64, device='cuda')
            grp = (ctypes.c_int * (p * p))(*group)
            blk = (ctypes.c_int32 * (p * p))(*([black] * (p * p)))
            cen = (ctypes.c_int32 * G)(*([black] * G))

            def stats(est=est, ref=ref, Hm=Hm, Wm=Wm, p=p, grp=grp, G=G, blk=blk, white=white, out=out):
                L.check(lib.eld_pair_level_stats_u16(L.dptr(est), L.dptr(ref), 1, Hm, Wm, Hm // p * p, Wm // p * p, p, grp, G, blk, white, None, L.dptr(out),
                                                     None, 0, st), 'eld_pair_level_stats_u16')

            def hist(ref=ref, Hm=Hm, Wm=Wm, p=p, grp=grp, G=G, cen=cen, counts=counts):
                L.check(lib.eld_hist_u16(L.dptr(ref), None, 1, Hm, Wm, p, grp, G, cen, 1024, None, L.dptr(counts), st), 'eld_hist_u16')

            calls.append(('%s_%s' % (cfa, content), stats, hist, Hm * Wm, out))
    times = {}
    for i in range(a.warmup + a.reps):
        for name, stats, hist, _, _ in calls:
            for kind, fn in (('stats', stats), ('hist', hist)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if i >= a.warmup:
                    times.setdefault((name, kind), []).append(e0.elapsed_time(e1) * 1e3)
    res = {'reps': a.reps, 'warmup': a.warmup, 'hbm_peak': HBM_PEAK, 'device': torch.cuda.get_device_name(0), 'src': L.build_src_hash()}
    for name, _, _, sites, out in calls:
        assert int(out[..., 0].sum()) > 0
        row = {'sites': sites, 'hbm_bound_us': 4.0 * sites / HBM_PEAK * 1e6}
        for kind in ('stats', 'hist'):
            t = np.asarray(times[(name, kind)])
            row[kind] = {'median_us': float(np.median(t)), 'p10_us': float(np.percentile(t, 10)), 'p90_us': float(np.percentile(t, 90))}
        row['stats_over_bound'] = row['stats']['median_us'] / row['hbm_bound_us']
        row['stats_over_hist'] = row['stats']['median_us'] / row['hist']['median_us']
        res[name] = row
    for cfa in ('bayer', 'xtrans'):
        res['%s_dark_over_random' % cfa] = res[cfa + '_dark']['stats']['median_us'] / res[cfa + '_random']['stats']['median_us']
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
