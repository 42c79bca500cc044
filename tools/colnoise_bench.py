"""Time the sampler under 'PGU', 'PGRU' and 'PGRCU' on one batch: what the row term and the column term cost per element.

    python tools/colnoise_bench.py [--batch 8] [--height 512] [--width 512] [--cfa bayer] [--reps 50] [--warmup 10] [--out result.json]

The three launches alternate inside one process; each is timed with device events around one call.  Prints the median, the 10th and 90th
percentile per model in ns per element, the cost of the row term t(PGRU) - t(PGU), of the column term t(PGRCU) - t(PGRU), and the run's
spread (the widest p90 - p10 of the three).  The packed width decides the column path: 2 * width sensor columns per block (Bayer; one parity,
`width`, for a block inside one plane) are staged in LDS up to MAX_LDS_COLS = 512, beyond that every element draws its own column normal."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--height', type=int, default=512)
    ap.add_argument('--width', type=int, default=512)
    ap.add_argument('--cfa', default='bayer', choices=('bayer', 'xtrans'))
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--out')
    a = ap.parse_args(argv)
    import torch
    import eld_amd
    from eld_amd import _lib as L
    from eld_amd.noise import NoiseParams, make_records, model_flags, sample_noise_records
    eld_amd.load_library()
    N, C, H, W = a.batch, 9 if a.cfa == 'xtrans' else 4, a.height, a.width
    g = torch.Generator(device='cuda').manual_seed(1)
    y = (torch.rand((N, C, H, W), device='cuda', generator=g) ** 2.2).contiguous()
    out = torch.empty_like(y)
    p = NoiseParams(2.288, 6.451, 15583, 208.98, tl_lambda=-0.14285714, tl_scale=3.3, row_scale=0.9, col_scale=0.7)
    recs = make_records([p] * N, list(range(N)))
    models = ('PGU', 'PGRU', 'PGRCU')
    flags = {m: model_flags(m, a.cfa) | L.CLIP for m in models}
    times = {m: [] for m in models}
    for i in range(a.warmup + a.reps):
        for m in models:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            sample_noise_records(y, recs, flags[m], 2018, out=out)
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                times[m].append(e0.elapsed_time(e1) * 1e6 / y.numel())          # ns per element
    assert bool(torch.isfinite(out).all())
    res = {'batch': N, 'planes': C, 'height': H, 'width': W, 'cfa': a.cfa, 'reps': a.reps, 'unit': 'ns per element'}
    for m in models:
        t = np.asarray(times[m])
        res[m] = {'median': float(np.median(t)), 'p10': float(np.percentile(t, 10)), 'p90': float(np.percentile(t, 90))}
    res['row_term'] = res['PGRU']['median'] - res['PGU']['median']
    res['col_term'] = res['PGRCU']['median'] - res['PGRU']['median']
    res['spread'] = max(res[m]['p90'] - res[m]['p10'] for m in models)
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
