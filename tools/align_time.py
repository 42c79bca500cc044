"""Time the burst alignment on a 24 MP Bayer burst (4000 x 6000) at N = 8 and 16: the luma pyramid, the search per level,
the stack through the field it finds, eld_burst_stack_u16 on the same burst and a device-to-device copy of it, alternating in one process.

    python tools/align_time.py [--reps 20] [--warmup 3] [--frames 8,16] [--out profiles/align_time.json]

The burst is a textured scene (block noise at 1, 2, 4, 8 and 64 pixels) with shot and read noise, every frame rolled by its own whole
number of CFA periods within +-24 (hand-held motion; the wrap-around of the roll is a border effect the timing does not see).  Each call is
timed with device events; medians and the 10th and 90th percentiles are reported.  The library runs all levels in one call, so the search of
level l is the difference of the medians of align(levels = l + 1) and align(levels = l) less the same difference of the pyramid calls (the
level's tiles and candidates do not depend on how many levels lie above it); level 0 is align(1) - pyramid(1).  Next to each level stands
its VALU bound: h w 81 absolute-difference-adds per frame, two per v_sad_u16 lane-operation."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T = 16


def make_burst(torch, N, Hm, Wm, seed, span=24):
    g = torch.Generator(device='cuda').manual_seed(seed)
    a = torch.rand((Hm, Wm), device='cuda', generator=g)
    for k in (1, 2, 4, 8, 64):
        u = torch.rand((-(-Hm // k), -(-Wm // k)), device='cuda', generator=g)
        a += k * u.repeat_interleave(k, 0).repeat_interleave(k, 1)[:Hm, :Wm]
    a = (a - a.min()) / (a.max() - a.min())
    scene = 600.0 + 5000.0 * a * a
    shifts = torch.randint(-span, span + 1, (N, 2), generator=torch.Generator().manual_seed(seed))
    shifts[0] = 0
    out = torch.empty((N, Hm, Wm), dtype=torch.int16, device='cuda')
    for f in range(N):
        s = torch.roll(scene, (2 * int(shifts[f, 0]), 2 * int(shifts[f, 1])), (0, 1))
        z = s + torch.sqrt(2.0 * s) * torch.randn((Hm, Wm), device='cuda', generator=g) + 3.0 * torch.randn((Hm, Wm), device='cuda', generator=g)
        out[f] = torch.clamp(torch.round(z + 512.0), 0, 16383).to(torch.int16)
    return out, shifts.numpy()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--frames', default='8,16')
    ap.add_argument('--size', default='4000x6000')
    ap.add_argument('--out')
    a = ap.parse_args(argv)
    import torch
    import eld_amd
    from eld_amd import _lib as L
    from eld_amd.burst import align_levels
    lib = eld_amd.load_library()
    if not torch.cuda.is_available():
        raise RuntimeError('tools/align_time.py measures on a GPU: there is none')
    Hm, Wm = (int(v) for v in a.size.split('x'))
    st = L.cur_stream()
    grp, blk = (ctypes.c_int * 4)(0, 1, 3, 2), (ctypes.c_int32 * 4)(512, 512, 512, 512)
    levels = align_levels(Hm, Wm, 2)
    TY, TX = -(-(Hm // 2) // T), -(-(Wm // 2) // T)
    res = {'reps': a.reps, 'warmup': a.warmup, 'device': torch.cuda.get_device_name(0), 'src': L.build_src_hash(), 'Hm': Hm, 'Wm': Wm,
           'levels': levels, 'runs': {}}
    for N in [int(v) for v in a.frames.split(',')]:
        fr, shifts = make_burst(torch, N, Hm, Wm, N)
        dst = torch.empty_like(fr)
        mean = torch.empty((Hm, Wm), dtype=torch.int16, device='cuda')
        kept = torch.empty((Hm, Wm), dtype=torch.uint8, device='cuda')
        present = torch.empty((Hm, Wm), dtype=torch.uint8, device='cuda')
        ptc = torch.empty((4, L.PAIRSTATS_BINS, 4), dtype=torch.int64, device='cuda')
        disp = torch.empty((N, TY, TX, 2), dtype=torch.int16, device='cuda')
        cost = torch.empty((N, TY, TX), dtype=torch.int32, device='cuda')
        pyr = torch.empty(lib.eld_burst_luma_pyramid_elems(N, Hm, Wm, 2, levels), dtype=torch.int16, device='cuda')
        need = lib.eld_burst_align_workspace_bytes(N, Hm, Wm, 2, levels)
        ws = torch.empty(need, dtype=torch.uint8, device='cuda')

        def align(lv):
            L.check(lib.eld_burst_align_u16(L.dptr(fr), N, Hm, Wm, 2, 0, lv, L.dptr(disp), L.dptr(cost), L.dptr(ws), need, st), 'eld_burst_align_u16')

        def pyramid(lv):
            L.check(lib.eld_burst_luma_pyramid_u16(L.dptr(fr), N, Hm, Wm, 2, lv, L.dptr(pyr), st), 'eld_burst_luma_pyramid_u16')

        def aligned():
            L.check(lib.eld_burst_stack_aligned_u16(L.dptr(fr), N, Hm, Wm, 2, grp, 4, blk, 16383, None, 100, 2, L.dptr(disp), TY, TX, L.dptr(mean),
                                                    L.dptr(kept), L.dptr(present), L.dptr(ptc), L.dptr(ws), need, st), 'eld_burst_stack_aligned_u16')

        def stack():
            L.check(lib.eld_burst_stack_u16(L.dptr(fr), N, Hm, Wm, 2, grp, 4, blk, 16383, None, 100, 2, L.dptr(mean), L.dptr(kept), L.dptr(ptc), None, 0, st),
                    'eld_burst_stack_u16')

        align(levels)                                              # the field the aligned stack is timed with
        torch.cuda.synchronize()
        d = disp.cpu().numpy().astype(np.int64)
        found = float(np.mean((d == shifts[:, None, None, :]).all(axis=3)))     # a frame rolled by +a shows ref's (y, x) at (y + a, x + b)
        calls = [('align_%d' % lv, (lambda lv=lv: align(lv))) for lv in range(1, levels + 1)]
        calls += [('pyramid_%d' % lv, (lambda lv=lv: pyramid(lv))) for lv in range(1, levels + 1)]
        calls += [('stack_aligned', aligned), ('stack', stack), ('copy', lambda: dst.copy_(fr))]
        times = {k: [] for k, _ in calls}
        for i in range(a.warmup + a.reps):
            for name, fn in calls:
                if name == 'stack_aligned':
                    align(levels)                                  # the narrower align calls before it overwrote the field
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if i >= a.warmup:
                    times[name].append(e0.elapsed_time(e1) * 1e-3)
        aligned()
        torch.cuda.synchronize()
        sites = Hm * Wm
        row = {'sites': sites, 'tiles_with_the_frame_shift': found, 'absent_share': float((present != (N % 256)).float().mean()),
               'rejected_share': float((kept != present).float().mean())}
        for name, _ in calls:
            row[name] = {'median_s': float(np.median(times[name])), 'p10_s': float(np.percentile(times[name], 10)),
                         'p90_s': float(np.percentile(times[name], 90))}
        med = lambda k: row[k]['median_s'] if k in row else 0.0
        h, w = Hm // 2, Wm // 2
        row['search'] = {}
        for lv in range(levels):
            t = (med('align_%d' % (lv + 1)) - med('align_%d' % lv)) - (med('pyramid_%d' % (lv + 1)) - med('pyramid_%d' % lv))
            sads = h * w * 81 * (N - 1)
            row['search'][str(lv)] = {'h': h, 'w': w, 'tiles': -(-h // T) * -(-w // T), 'seconds': t, 'abs_diff_adds': sads,
                                      'abs_diff_adds_per_s': sads / t if t > 0 else None}
            h, w = (h + 1) // 2, (w + 1) // 2
        for name, nbytes in (('stack_aligned', (2 * N + 4) * sites), ('stack', (2 * N + 3) * sites), ('copy', 2 * N * sites)):
            row[name]['bytes'] = nbytes
            row[name]['rate_GBps'] = nbytes / row[name]['median_s'] * 1e-9
        res['runs'][str(N)] = row
        del fr, dst, ws, pyr
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
