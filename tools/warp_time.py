"""Time eld_warp_rgb_f32 on one 24 MP picture (3 x 4000 x 6000 float32 camera RGB) for the three lenses of sec. 30's table
and for the identity, writing 8-bit sRGB codes (gamma 2.2, with a matrix) and float32 linear RGB, with the source boxes staged in LDS (the
given budget) and with every tap read from global memory (lds_bytes = 0).  The yardsticks, timed in the same process: a device-to-device copy
of the same three planes (288 MB read, 288 MB written) and eld_render_bayer of the same frame (the demosaic that produces those planes).

    python tools/warp_time.py [--reps 20] [--warmup 3] [--lds -1] [--out result.json]

The calls alternate inside one process; each is timed with device events around one call, and goes straight to the library with arguments
prepared beforehand.  Prints the median, the 10th and 90th percentile per call, the ratio of the medians to the copy's, and per call the time
of ten back-to-back launches divided by ten (`train10_us`: what is left when no host gap separates the launches).  The staged and the direct
result of every lens are compared bit for bit after the timing (tests/test_warp_gpu.py pins both to the restatement on small shapes)."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HM, WM = 4000, 6000
LENSES = {'barrel_kr1_0.05': ((1.0, 0.05, 0.0, 0.0, 0.0, 0.0), 0.5, 0.5),
          'mixed': ((0.96, 0.06, -0.01, 0.002, 0.001, -0.001), 0.5, 0.5),
          'pincushion_kr1_-0.08': ((1.0, -0.08, 0.02, 0.0, 0.0, 0.0), 0.5, 0.5),
          'identity': ((1.0, 0.0, 0.0, 0.0, 0.0, 0.0), 0.5, 0.5),
          'three_sets_ca': (((1.0008, 0.05, 0.0, 0.0, 0.0, 0.0), (1.0, 0.05, 0.0, 0.0, 0.0, 0.0), (0.9992, 0.05, 0.0, 0.0, 0.0, 0.0)), 0.5, 0.5)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--lds', type=int, default=-1, help='lds_bytes of the staged calls (default -1: the library\'s default)')
    ap.add_argument('--out')
    a = ap.parse_args(argv)
    import torch
    import eld_amd
    from eld_amd import _lib as L
    from eld_amd.dng_opcodes import Warp
    eld_amd.load_library()
    if not torch.cuda.is_available():
        raise RuntimeError('tools/warp_time.py measures on a GPU: there is none')
    g = torch.Generator(device='cuda').manual_seed(1)
    packed = torch.rand((1, 4, HM // 2, WM // 2), device='cuda', generator=g)
    wbs = torch.tensor([[2.0, 1.0, 1.5, 1.0]], device='cuda')
    ccm = torch.tensor([[1.6, -0.4, -0.2, -0.2, 1.5, -0.3, 0.0, -0.5, 1.5]], device='cuda')
    rgb = torch.empty((1, 3, HM, WM), dtype=torch.float32, device='cuda')
    out8 = torch.empty((1, 3, HM, WM), dtype=torch.uint8, device='cuda')
    out32, dst = torch.empty_like(rgb), torch.empty_like(rgb)
    lib, st = L.lib(), L.cur_stream()
    pat = (ctypes.c_int * 4)(0, 1, 3, 2)

    def render(dst_, mode):
        return lambda: L.check(lib.eld_render_bayer(L.dptr(packed), pat, L.dptr(wbs), None if dst_ is rgb else L.dptr(ccm), L.dptr(dst_), mode, 1, HM // 2,
                                                    WM // 2, 2.2, None, None, 0, st), 'eld_render_bayer')
    render(rgb, L.RENDER_LINEAR_F32)()                               # the camera RGB every warp call reads
    records = {name: Warp(*lens).record(HM, WM) for name, lens in LENSES.items()}

    def warp(name, linear, budget):
        rec = ctypes.c_void_p(records[name].ctypes.data)
        o, mode = (out32, L.RENDER_LINEAR_F32) if linear else (out8, L.RENDER_SRGB8)
        return lambda: L.check(lib.eld_warp_rgb_f32(L.dptr(rgb), L.dptr(o), mode, 1, HM, WM, rec, L.dptr(ccm), 2.2, None, None, 0, budget, st),
                               'eld_warp_rgb_f32')

    def copy():
        dst.copy_(rgb)
    calls = [('copy', copy), ('render_bayer_srgb8', render(out8, L.RENDER_SRGB8))]
    for name in LENSES:
        for linear in (False, True):
            for tag, budget in (('lds', a.lds), ('direct', 0)):
                calls += [('%s/%s/%s' % (name, 'linear' if linear else 'srgb8', tag), warp(name, linear, budget)), ('copy', copy)]
    times = {}
    for i in range(a.warmup + a.reps):
        for kind, fn in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                times.setdefault(kind, []).append(e0.elapsed_time(e1) * 1e3)
    train = {}
    for kind, fn in dict(calls).items():                             # ten launches back to back between one pair of events
        t = []
        for i in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                fn()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1) * 100.0)
        train[kind] = float(np.median(t))
    for name in LENSES:                                              # the two paths wrote the same bits
        for linear in (False, True):
            o = out32 if linear else out8
            warp(name, linear, a.lds)()
            staged = o.clone()
            warp(name, linear, 0)()
            torch.cuda.synchronize()
            assert torch.equal(staged.view(torch.uint8), o.view(torch.uint8)), (name, linear)
    res = {'reps': a.reps, 'warmup': a.warmup, 'lds_bytes': a.lds, 'device': torch.cuda.get_device_name(0), 'src': L.build_src_hash(), 'pixels': HM * WM}
    for kind in times:
        t = np.asarray(times[kind])
        res[kind] = {'median_us': float(np.median(t)), 'p10_us': float(np.percentile(t, 10)), 'p90_us': float(np.percentile(t, 90)),
                     'train10_us': train[kind]}
    for kind in times:
        if kind != 'copy':
            res[kind]['over_copy'] = res[kind]['median_us'] / res['copy']['median_us']
            res[kind]['train10_over_copy'] = res[kind]['train10_us'] / res['copy']['train10_us']
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
