"""GPU time of the histogram kernels (csrc/hist.hip) on one 4000 x 6000 frame, next to eld_calib_bias_stats on the same frame (it reads the
same bytes: the yardstick).  eld_hist_u16 under three laws -- a constant frame, rint(N(512, 3)) and uniform over all codes -- and eld_hist_f32
on the packed equivalent (4 x 2000 x 3000 float32).  HIP events, two warm runs, the minimum of --reps (>= 5) runs, one process.
Writes profiles/validate_hist.md and prints it.

    python tools/validate_time.py [--reps 10] [--radius 256]
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from eld_amd import _lib as L                       # noqa: E402

LAYOUT = 'replicated LDS: 512-thread workgroups, min(16, 72 KiB / table) copies by thread index, copy stride 1 mod 32 words, 64-bit global flush'


def timed(fn, reps):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--radius', type=int, default=256)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'validate_hist.md'))
    a = ap.parse_args()
    reps, R = max(5, a.reps), a.radius
    L.load_library()
    if not torch.cuda.is_available():
        raise SystemExit('tools/validate_time.py measures on a GPU: none found')
    Hm, Wm = 4000, 6000
    rng = np.random.default_rng(0)
    frames = {'constant': np.full((1, Hm, Wm), 512, np.uint16),
              'normal(512, 3)': np.clip(np.rint(rng.normal(512, 3, (1, Hm, Wm))), 0, 65535).astype(np.uint16),
              'uniform': rng.integers(0, 65536, (1, Hm, Wm)).astype(np.uint16)}
    pat = (ctypes.c_int * 4)(0, 1, 3, 2)
    cen = (ctypes.c_int32 * 4)(512, 512, 512, 512)
    counts = torch.empty((1, 4, 2 * R + 1), dtype=torch.int64, device='cuda')
    rows = []
    yard = None
    for name, u in frames.items():
        ud = torch.from_numpy(u.view(np.int16)).cuda()
        if yard is None:
            cs = torch.empty((1, 4, 2), dtype=torch.int64, device='cuda')
            rs = torch.empty((1, Hm, 2), dtype=torch.int64, device='cuda')
            ws = torch.empty(max(1, L.lib().eld_calib_bias_stats_workspace_bytes(1, Hm)), dtype=torch.uint8, device='cuda')
            yard = timed(lambda: L.check(L.lib().eld_calib_bias_stats(L.dptr(ud), 1, Hm, Wm, pat, L.dptr(cs), L.dptr(rs), L.dptr(ws), ws.numel(),
                                                                    L.cur_stream())), reps)
            rows.append(('eld_calib_bias_stats (yardstick)', 'constant', 2 * Hm * Wm, yard))
        t = timed(lambda: L.check(L.lib().eld_hist_u16(L.dptr(ud), None, 1, Hm, Wm, 2, pat, 4, cen, R, None, L.dptr(counts), L.cur_stream())), reps)
        rows.append(('eld_hist_u16', name, 2 * Hm * Wm, t))
        x = ((torch.stack([ud[0, 0::2, 0::2], ud[0, 0::2, 1::2], ud[0, 1::2, 1::2], ud[0, 1::2, 0::2]]).to(torch.int32) & 0xffff).float() - 512.0)[None]
        x = x.contiguous()
        sc = torch.ones(1, device='cuda')
        grp = (ctypes.c_int * 4)(0, 1, 2, 3)
        t = timed(lambda: L.check(L.lib().eld_hist_f32(L.dptr(x), None, 1, 4, Hm // 2, Wm // 2, grp, 4, L.dptr(sc), R, L.dptr(counts), L.cur_stream())), reps)
        rows.append(('eld_hist_f32', name, 4 * Hm * Wm, t))
        del ud, x
    lines = ['# Histogram kernels on one %d x %d frame (R = %d, G = 4)' % (Hm, Wm, R), '',
             'Device: %s.  HIP events, min of %d runs after 2 warm runs.  LDS layout: %s.' % (torch.cuda.get_device_name(0), reps, LAYOUT), '',
             '| kernel | law | bytes read | ms | TB/s | time / yardstick |', '|---|---|---|---|---|---|']
    for k, law, nb, t in rows:
        lines.append('| %s | %s | %d | %.4f | %.2f | %.2f |' % (k, law, nb, t, nb / (t * 1e-3) / 1e12, t / yard))
    text = '\n'.join(lines) + '\n'
    with open(a.out, 'w') as fh:
        fh.write(text)
    print(text)


if __name__ == '__main__':
    main()
