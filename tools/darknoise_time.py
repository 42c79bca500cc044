"""GPU time of the sampler with the dark-frame term (PDU|CLIP, eld_noise_forward_dark) next to PGRU|CLIP and PU|CLIP at bench.py's shape:
8 x 4x1424x2128 float32 in, a pool of eight 2848x4256 frames in two sessions.  HIP events around the whole call (record upload included), three
warm runs, REPS launches (environment, default 20), one process; prints one JSON line and writes it to $DARK_BENCH_OUT when set.

    python tools/darknoise_time.py
    REPS=10 rocprofv3 --kernel-trace --stats -d prof -o dark -- python tools/darknoise_time.py      # kernel times alone, a run of its own
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eld_amd import _lib as L
from eld_amd.darkpool import DarkPool
from eld_amd.noise import NoiseParams, model_flags, sample_noise

REPS = int(os.environ.get('REPS', '20'))
dev = torch.device('cuda', 0)
g = torch.Generator(device=dev)
g.manual_seed(1)
frames = [(512 + torch.randn((2848, 4256), device=dev, generator=g) * 4).round().clamp(0, 16383).to(torch.int32).to(torch.uint16) for _ in range(8)]
pool = DarkPool([{'bias': frames[:4]}, {'bias': frames[4:]}], raw_pattern=[[0, 1], [3, 2]], black_level=[512] * 4, white_level=16383, K=[2.0, 4.0], device=dev)
y = (torch.rand((8, 4, 1424, 2128), device=dev, generator=g) ** 2.2).contiguous()
out = torch.empty_like(y)
res = {'device': torch.cuda.get_device_name(0), 'shape': list(y.shape), 'pool': '8 x 2848x4256 uint16', 'reps': REPS}
for name, prm in (('PDU', [NoiseParams(2.288, 6.451, pool.saturation, 208.98, dark=pool.ranges[i % 2]) for i in range(8)]),
                  ('PGRU', [NoiseParams(2.288, 6.451, 15583, 208.98, tl_lambda=-0.14285714, tl_scale=3.3, row_scale=0.9)] * 8),
                  ('PU', [NoiseParams(2.288, 6.451, 15583, 208.98)] * 8)):
    flags = model_flags(name) | L.CLIP
    kw = {'dark': pool} if name == 'PDU' else {}
    for _ in range(3):
        sample_noise(y, prm, flags, 2018, list(range(8)), out=out, **kw)
    torch.cuda.synchronize()
    ts = []
    for r in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        sample_noise(y, prm, flags, 2018, [8 * r + i for i in range(8)], out=out, **kw)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts = np.array(ts)
    res[name] = {'us_median': float(np.median(ts)), 'us_min': float(ts.min()), 'us_max': float(ts.max()),
                 'GB_per_s_algorithmic': float(y.numel() * (10 if name == 'PDU' else 8) / np.median(ts) / 1e3)}
    assert torch.isfinite(out).all()
print(json.dumps(res))
if os.environ.get('DARK_BENCH_OUT'):
    with open(os.environ['DARK_BENCH_OUT'], 'w') as f:
        json.dump(res, f, indent=1)
