"""Time the baseline-JPEG encoder on one 24 MP sRGB render (4000 x 6000, a synthetic scene: smooth gradients, texture and
noise) at quality 90, 4:2:0 and 4:4:4: each kernel behind eld_amd.jpeg.encode_jpeg, their sum next to a device-to-device copy of the three
planes, the whole encode_jpeg call by the host's clock (host planning, the synchronisations and the copy of the compressed bytes included),
and, in the same run on the same machine's CPU, what it replaces: the device-to-host copy plus Image.save as PNG, and Image.save as JPEG at
the same settings with optimize=True.

    python tools/jpeg_time.py [--reps 20] [--warmup 3] [--cpu-reps 2] [--segment 0] [--chunk 0] [--out result.json]

The device calls alternate inside one process; each is timed with device events around one call.  Prints the median, the 10th and 90th
percentile per call.  Nothing is gated on the times.  The one condition is correctness at this size: Pillow decodes the device's file to the
pixels it decodes from its own file at the same settings (equal coefficients and tables); exit status 1 otherwise."""
import argparse
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, QUALITY = 4000, 6000, 90
KERNELS = ('coef', 'hist', 'pack', 'ffcount', 'cumsum', 'stuff')


def scene(torch):
    """(3, H, W) uint8 on the device"""
    g = torch.Generator(device='cuda').manual_seed(1)
    y = torch.arange(H, device='cuda', dtype=torch.float32)[:, None] / H
    x = torch.arange(W, device='cuda', dtype=torch.float32)[None, :] / W
    planes = []
    for c in range(3):
        p = 0.5 + 0.35 * torch.sin(6.0 * x + c) * torch.cos(4.0 * y - c) + 0.1 * torch.sin(300.0 * x * (1 + y)) * (x > 0.5)
        p = p + 0.02 * torch.randn((H, W), device='cuda', generator=g)
        planes.append((p.clamp(0, 1) * 255).round().to(torch.uint8))
    return torch.stack(planes).contiguous()


def stats(v):
    v = np.asarray(v)
    return {'median_us': float(np.median(v)), 'p10_us': float(np.percentile(v, 10)), 'p90_us': float(np.percentile(v, 90))}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--cpu-reps', type=int, default=2)
    ap.add_argument('--segment', type=int, default=0, help='blocks per segment (0: the default)')
    ap.add_argument('--chunk', type=int, default=0, help='bytes per stuffing chunk (0: the default)')
    ap.add_argument('--out')
    a = ap.parse_args(argv)
    import torch
    from PIL import Image
    import eld_amd
    from eld_amd import _lib as L
    from eld_amd import jpeg as J
    eld_amd.load_library()
    if not torch.cuda.is_available():
        raise RuntimeError('tools/jpeg_time.py measures on a GPU: there is none')
    rgb = scene(torch)
    dst = torch.empty_like(rgb)

    def copy():
        dst.copy_(rgb)

    props = torch.cuda.get_device_properties(0)
    res = {'reps': a.reps, 'warmup': a.warmup, 'device': torch.cuda.get_device_name(0), 'src': L.build_src_hash(), 'H': H, 'W': W, 'quality': QUALITY,
           'cus': props.multi_processor_count}
    ok = True
    for sub in ('420', '444'):
        enc = J.Encoder(rgb, QUALITY, sub, a.segment, a.chunk)
        enc.run()

        def cumsum():
            cum = torch.cumsum(enc.d_count, 0, dtype=torch.int64)
            enc.d_before = (cum - enc.d_count).to(torch.int32).contiguous()

        steps = {'coef': enc.coef, 'hist': enc.hist, 'pack': enc.pack, 'ffcount': enc.ffcount, 'cumsum': cumsum, 'stuff': enc.stuff, 'copy': copy}
        order = ('coef', 'copy', 'hist', 'pack', 'copy', 'ffcount', 'cumsum', 'stuff')
        times = {}
        for i in range(a.warmup + a.reps):
            for kind in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                steps[kind]()
                e1.record()
                e1.synchronize()
                if i >= a.warmup:
                    times.setdefault(kind, []).append(e0.elapsed_time(e1) * 1e3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            data = J.encode_jpeg(rgb, QUALITY, sub, a.segment, a.chunk)
            t1 = time.perf_counter()
            if i >= a.warmup:
                times.setdefault('encode_jpeg', []).append((t1 - t0) * 1e6)
        assert data == enc.data()                                    # the timed steps left the same bytes
        r = {'segment': enc.segment, 'segments': enc.nseg, 'blocks': enc.nblocks, 'chunk': enc.chunk, 'chunks': enc.nchunks, 'raw_bytes': enc.nraw,
             'file_bytes': len(data), 'coef_bytes': enc.nblocks * 128}
        for kind in KERNELS + ('copy', 'encode_jpeg'):
            r[kind] = stats(times[kind])
        r['encode_device_us'] = sum(r[k]['median_us'] for k in KERNELS)
        r['encode_over_copy'] = r['encode_device_us'] / r['copy']['median_us']
        r['encode_mpixels_per_s'] = H * W / r['encode_device_us']
        # the CPU path it replaces, and the check
        cpu = {'png': [], 'jpeg': []}
        for _ in range(a.cpu_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hwc = np.ascontiguousarray(np.moveaxis(rgb.cpu().numpy(), 0, -1))
            if sub == '420':                                         # the PNG does not depend on the subsampling: once
                Image.fromarray(hwc).save(io.BytesIO(), 'PNG')
                cpu['png'].append((time.perf_counter() - t0) * 1e6)
            t0 = time.perf_counter()
            buf = io.BytesIO()
            Image.fromarray(hwc).save(buf, 'JPEG', quality=QUALITY, subsampling=J.SUBSAMPLING[sub], optimize=True)
            cpu['jpeg'].append((time.perf_counter() - t0) * 1e6)
        if cpu['png']:
            res['cpu_d2h_png'] = stats(cpu['png'])
        if cpu['jpeg']:                                              # --cpu-reps 0: the device times alone (a run that compares segment lengths)
            r['cpu_pillow_jpeg'] = stats(cpu['jpeg'])
            r['pillow_file_bytes'] = len(buf.getvalue())
            ours = np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))
            theirs = np.asarray(Image.open(buf).convert('RGB'))
            r['decodes_like_pillows'] = bool(np.array_equal(ours, theirs))
            ok = ok and r['decodes_like_pillows']
        res[sub] = r
        del enc
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    if not ok:
        print("Pillow decodes the device's file to other pixels than its own: something is wrong", file=sys.stderr)
        return 1
    return 0


if __name__ == '__main__':
    sys.exit(main())
