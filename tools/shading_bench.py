"""Time the dark-shading kernels: the fit on 3 sessions x 8 Bayer frames of 2848 x 4256, the apply pass on 8 such
frames, and the shaded input stage against the plain one (eld_pack_raw_bayer_u16_gain) on the same 8 frames.

    python tools/shading_bench.py [--height 2848] [--width 4256] [--sessions 3] [--frames 8] [--reps 30] [--warmup 5] [--out result.json]

All calls alternate inside one process; each is timed with device events around one call.  Prints the median, the 10th and 90th
percentile, and the bytes the algorithm moves over the median, as a rate and as a share of the HBM peak:
    fit   2 * (frames of all sessions) + 8 bytes per site          apply   4 + 8 bytes per site and frame (the map is read per call, once)
    shaded pack   2 + 8 + 4 = 14 bytes per site and frame          plain pack   2 + 4 = 6
(the shaded pack's map is shared by the frames of a call and may be served from cache: the count is what one frame needs)."""
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
    ap.add_argument('--height', type=int, default=2848)
    ap.add_argument('--width', type=int, default=4256)
    ap.add_argument('--sessions', type=int, default=3)
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out')
    a = ap.parse_args(argv)
    import torch
    import eld_amd
    from eld_amd import _lib as L
    lib = eld_amd.load_library()
    if not torch.cuda.is_available():
        raise RuntimeError('tools/shading_bench.py measures on a GPU: there is none')
    Hm, Wm, S, F = a.height, a.width, a.sessions, a.frames
    sites = Hm * Wm
    g = torch.Generator(device='cuda').manual_seed(1)
    step = -(-sites // 8) * 8
    pool = (512 + 4 * torch.randn(S * F * step, device='cuda', generator=g)).round().clamp(0, 65535).to(torch.int32).to(torch.int16)
    table = np.zeros(S * F, L.POOL_FRAME_DTYPE)
    for i in range(S * F):
        table[i] = (i * step, Hm, Wm)
    tab = torch.from_numpy(table.view(np.uint8).copy()).cuda()
    ses = (ctypes.c_int32 * (2 * S))(*[v for s in range(S) for v in (s * F, F)])
    from eld_amd.shading import fit_coefficients
    _, alpha, beta = fit_coefficients([800 * 2 ** s for s in range(S)], [F] * S)
    al, be = (ctypes.c_double * S)(*alpha), (ctypes.c_double * S)(*beta)
    cen = (ctypes.c_int32 * 4)(512, 512, 512, 512)
    ma = torch.empty((Hm, Wm), dtype=torch.float32, device='cuda')
    mb = torch.empty((Hm, Wm), dtype=torch.float32, device='cuda')
    frames = pool[:F * step].view(F, step)[:, :sites].contiguous().view(F, Hm, Wm)
    out_u = torch.empty_like(frames)
    packed = torch.empty((F, 4, Hm // 2, Wm // 2), dtype=torch.float32, device='cuda')
    packed2 = torch.empty_like(packed)
    ratios = torch.full((F,), 100.0, dtype=torch.float32, device='cuda')
    pat, blk = (ctypes.c_int * 4)(0, 1, 3, 2), (ctypes.c_float * 4)(512, 512, 512, 512)
    st = L.cur_stream()

    def fit():
        L.check(lib.eld_shading_fit_u16(L.dptr(pool), pool.numel(), L.dptr(tab), S * F, Hm, Wm, ses, S, al, be, cen, 2, None, L.dptr(ma), L.dptr(mb),
                                        st), 'eld_shading_fit_u16')

    def apply():
        L.check(lib.eld_shading_apply_u16(L.dptr(frames), L.dptr(out_u), F, Hm, Wm, L.dptr(ma), L.dptr(mb), 100.0, None, st), 'eld_shading_apply_u16')

    def pack_shaded():
        L.check(lib.eld_pack_raw_bayer_u16_shaded(L.dptr(frames), L.dptr(packed), F, Hm // 2, Wm // 2, pat, blk, 16383.0, L.dptr(ratios), L.dptr(ma),
                                                  L.dptr(mb), 100.0, st), 'eld_pack_raw_bayer_u16_shaded')

    def pack_plain():
        L.check(lib.eld_pack_raw_bayer_u16_gain(L.dptr(frames), L.dptr(packed2), F, Hm // 2, Wm // 2, pat, blk, 16383.0, L.dptr(ratios), st),
                'eld_pack_raw_bayer_u16_gain')

    calls = (('fit', fit, (2.0 * S * F + 8.0) * sites), ('apply', apply, (4.0 * F + 8.0) * sites), ('pack_shaded', pack_shaded, 14.0 * F * sites),
             ('pack_plain', pack_plain, 6.0 * F * sites))
    times = {name: [] for name, _, _ in calls}
    for i in range(a.warmup + a.reps):
        for name, fn, _ in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    res = {'height': Hm, 'width': Wm, 'sessions': S, 'frames': F, 'reps': a.reps, 'hbm_peak': HBM_PEAK}
    for name, _, nbytes in calls:
        t = np.asarray(times[name])
        med = float(np.median(t))
        res[name] = {'median_us': med, 'p10_us': float(np.percentile(t, 10)), 'p90_us': float(np.percentile(t, 90)), 'bytes': nbytes,
                     'bytes_per_s': nbytes / (med * 1e-6), 'hbm_share': nbytes / (med * 1e-6) / HBM_PEAK}
    res['pack_shaded_over_plain'] = res['pack_shaded']['median_us'] / res['pack_plain']['median_us']
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
