"""Time eld_frame_rgb_f32 on one 24 MP picture (3 x 4000 x 6000 float32 camera RGB): the whole picture to a long edge of 1024
and of 256, with both filters ('area', 'lanczos'), upright as stored (orientation 1) and turned (orientation 6, the LDS transpose), writing
8-bit sRGB codes (gamma 2.2, with a matrix) and float32 linear RGB; and the crop-and-turn-only case at full size (an integer crop at its own
size: single taps of weight 1).  The yardsticks, timed in the same process: per case a device-to-device copy that moves the bytes the call
must read and write (the crop's three planes in, the output out: a copy of half their sum reads and writes that many together), and
torch.nn.functional.interpolate(mode='bilinear', antialias=True) of the same planes to the same size, which runs no tail and no transpose.

    python tools/frame_time.py [--reps 20] [--warmup 3] [--cases TEXT] [--out FILE]      (default: profiles/frame_time.json)

The calls alternate inside one process; each is timed with device events around one call and goes straight to the library with tables,
workspace and output prepared beforehand.  Prints the median, the 10th and 90th percentile per call and the ratios of the medians to the
case's copy and to torch's resize.  After the timing every frame call's output is compared with eld_amd.isp.frame_rgb's."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HS, WS = 4000, 6000
FULL_CROP = (8, 12, 3984, 5976)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--cases', help='time only the cases whose name contains this text (for a kernel trace of one case)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'frame_time.json'), help='where the result goes (default: profiles/frame_time.json)')
    a = ap.parse_args(argv)
    import torch
    import torch.nn.functional as F
    import eld_amd
    from eld_amd import _lib as L
    from eld_amd import isp
    eld_amd.load_library()
    if not torch.cuda.is_available():
        raise RuntimeError('tools/frame_time.py measures on a GPU: there is none')
    g = torch.Generator(device='cuda').manual_seed(1)
    rgb = torch.rand((1, 3, HS, WS), device='cuda', generator=g)
    ccm = torch.tensor([[1.6, -0.4, -0.2, -0.2, 1.5, -0.3, 0.0, -0.5, 1.5]], device='cuda')
    lib, st = L.lib(), L.cur_stream()
    up = lambda arr, dt: torch.from_numpy(np.ascontiguousarray(arr, dtype=dt)).cuda()

    def prepare(frame, linear):
        """-> (the call, its output tensor, the bytes it must read and write)"""
        t, (Ho, Wo) = frame.taps(HS, WS)
        Wc = Ho if frame.orientation >= 5 else Wo
        row0, rows = int(t.ystart.min()), int((t.ystart + t.ycount).max()) - int(t.ystart.min())
        tabs = [up(t.ystart, np.int32), up(t.ycount, np.int32), up(t.yw, np.float32), up(t.xstart, np.int32), up(t.xcount, np.int32), up(t.xw.T, np.float32)]
        out = torch.empty((1, 3, Ho, Wo), dtype=torch.float32 if linear else torch.uint8, device='cuda')
        ws = torch.empty((3 * rows * Wc,), dtype=torch.float32, device='cuda')
        mode = L.RENDER_LINEAR_F32 if linear else L.RENDER_SRGB8
        cols = int((t.xstart + t.xcount).max()) - int(t.xstart.min())

        def call():
            L.check(lib.eld_frame_rgb_f32(L.dptr(rgb), L.dptr(out), mode, 1, HS, WS, Ho, Wo, frame.orientation, L.dptr(tabs[0]), L.dptr(tabs[1]),
                                          L.dptr(tabs[2]), int(t.yw.shape[1]), L.dptr(tabs[3]), L.dptr(tabs[4]), L.dptr(tabs[5]), int(t.xw.shape[1]), row0,
                                          rows, L.dptr(ws), ws.numel() * 4, L.dptr(ccm), 2.2, None, None, 0, st), 'eld_frame_rgb_f32')
        call.keep = (tabs, ws)
        return call, out, 3 * rows * cols * 4 + out.numel() * out.element_size(), 3 * rows * Wc * 4

    cases = {}
    for size in (1024, 256):
        for flt in ('area', 'lanczos'):
            for o in (1, 6):
                for linear in (False, True):
                    cases['size%d/%s/o%d/%s' % (size, flt, o, 'linear' if linear else 'srgb8')] = (isp.Frame(None, o, size, flt), linear, size)
    for o in (1, 6):
        for linear in (False, True):
            cases['full_crop/o%d/%s' % (o, 'linear' if linear else 'srgb8')] = (isp.Frame(FULL_CROP, o, None, 'area'), linear, None)
    if a.cases:
        cases = {k: v for k, v in cases.items() if a.cases in k}
    calls, outs, info, copies, resizes = {}, {}, {}, {}, {}                    # calls: every case and every yardstick once per round, in this order
    for name, (frame, linear, size) in cases.items():
        fn, out, nbytes, wsbytes = prepare(frame, linear)
        outs[name] = (out, frame, linear)
        info[name] = {'bytes_in_and_out': nbytes, 'workspace_bytes': wsbytes, 'out_shape': list(out.shape[2:])}
        cname = 'copy/%d' % nbytes
        if cname not in copies:
            src, dst = torch.empty((nbytes // 2,), dtype=torch.uint8, device='cuda'), torch.empty((nbytes // 2,), dtype=torch.uint8, device='cuda')
            copies[cname] = (lambda s=src, d=dst: d.copy_(s))
        rname = None
        if size is not None:
            Hc, Wc = isp.Frame(None, 1, size, 'area').out_size(HS, WS)
            rname = 'torch_bilinear_antialias/%dx%d' % (Hc, Wc)
            if rname not in resizes:
                resizes[rname] = (lambda hw=(Hc, Wc): F.interpolate(rgb, size=hw, mode='bilinear', antialias=True))
        info[name].update(copy=cname, torch=rname)
        calls[name] = fn
        calls.setdefault(cname, copies[cname])
        if rname:
            calls.setdefault(rname, resizes[rname])
    times = {}
    for i in range(a.warmup + a.reps):
        for kind, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                times.setdefault(kind, []).append(e0.elapsed_time(e1) * 1e3)
    for name, (out, frame, linear) in outs.items():                  # the prepared calls wrote what the package's own path writes
        want = isp.frame_rgb(rgb, frame, ccm, linear=linear)
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.uint8), want.view(torch.uint8)), name
    res = {'reps': a.reps, 'warmup': a.warmup, 'device': torch.cuda.get_device_name(0), 'src': L.build_src_hash(), 'source': [3, HS, WS]}
    for kind, t in times.items():
        t = np.asarray(t)
        res[kind] = {'median_us': float(np.median(t)), 'p10_us': float(np.percentile(t, 10)), 'p90_us': float(np.percentile(t, 90))}
    for name in cases:
        res[name].update(info[name])
        res[name]['over_copy'] = res[name]['median_us'] / res[info[name]['copy']]['median_us']
        if info[name]['torch']:
            res[name]['over_torch'] = res[name]['median_us'] / res[info[name]['torch']]['median_us']
    print(json.dumps(res))
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
