"""Training-step time of the X-Trans network (9 -> 9) beside the Bayer one (4 -> 4) at the same packed pixel count (dev tool, not bench.py).

Default shape 8 x 1344 x 2000 packed pixels: a Fuji X-T2 frame (4032 x 6032 sensor) packed to 9 planes at 1344 x 2010, cut to multiples of
16.  For each (planes, precision) the tool builds ELDModel (opt.channels = planes, fused head), feeds one fixed noisy input, runs `--warmup`
steps, then times `--steps` calls of optimize_parameters (forward, loss, backward, Adam) one by one with CUDA events, and prints ONE JSON line:
median / min ms per step and ms per packed megapixel for every configuration.

    python tools/xtrans_step.py [--steps 10 --warmup 3 --batch 8 --height 1344 --width 2000 --configs x9:fp32,x9:bf16,b4:fp32,b4:bf16]

Per-launch head figures: run one small case under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/xtrans_step.py --steps 3`, then
    python tools/xtrans_step.py --head-stats DIR/.../*kernel_stats.csv --batch 8 --height 1344 --width 2000 [--planes 9]
prints the head kernels' average time per launch and the HBM bandwidth their algorithmic bytes imply (the fused training head reads the
32-channel activation and the target and writes the output and the 32-channel gradient: (32 + OC + OC + 32) x element size bytes per pixel).
"""
import argparse
import csv
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_opt(planes, precision):
    return types.SimpleNamespace(gpu_ids=[0], isTrain=True, checkpoints_dir='/tmp', name='xtrans_step', netG='unet', channels=planes,
                                 stage_in='raw', stage_out='raw', lr=1e-4, beta1=0.9, wd=0.0, loss='l1', resume=False, chop=False,
                                 no_log=False, save_epoch_freq=2, model='eld_model', precision=precision)


def time_config(planes, precision, B, H, W, steps, warmup):
    import torch
    from eld_amd.model import ELDModel
    torch.manual_seed(2018)
    m = ELDModel()
    m.initialize(make_opt(planes, precision))
    g = torch.Generator(device='cuda').manual_seed(1)
    t = torch.rand(B, planes, H, W, device='cuda', generator=g)
    x = (t + 0.02 * torch.randn(B, planes, H, W, device='cuda', generator=g)).clamp_(0, 1)
    m.set_input({'input': x, 'target': t}, 'train')
    for _ in range(warmup):
        m.optimize_parameters()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for e0, e1 in ev:
        e0.record()
        m.optimize_parameters()
        e1.record()
    torch.cuda.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    med = ms[len(ms) // 2] if len(ms) % 2 else 0.5 * (ms[len(ms) // 2 - 1] + ms[len(ms) // 2])
    mpix = B * H * W / 1e6
    loss = m.get_current_errors()['Pixel']
    del m, x, t
    torch.cuda.empty_cache()
    return {'planes': planes, 'precision': precision, 'ms_median': round(med, 3), 'ms_min': round(ms[0], 3),
            'ms_per_packed_mpix': round(med / mpix, 4), 'loss': loss}


def head_kind(name):
    """(element size, mode) of a head kernel from its demangled (or mangled) name: mode 'fwd', 'bwd', 'train' or None (reductions)."""
    import re
    if 'reduce' in name or 'loss' in name:
        return None, None
    bf16 = 'unsigned short' in name or 'ItL' in name or 'ItE' in name or 'IDF16' in name      # every head kernel is a template on the element: <unsigned short> / It..E
    m = re.search(r'head_wide_kernel<[^,]+, *\d+, *(\d)>', name) or re.search(r'head_wide_kernel\w*?Li\d+ELi(\d)E', name)
    if m:
        return (2 if bf16 else 4), {'0': 'fwd', '3': 'bwd'}.get(m.group(1), 'train')
    if 'head_train' in name:
        return (2 if bf16 else 4), 'train'
    if 'head_bwd' in name:
        return (2 if bf16 else 4), 'bwd'
    return (2 if bf16 else 4), 'fwd'


def head_stats(path, B, H, W, oc):
    """Average time per launch of the head kernels in a rocprofv3 --stats CSV, and the bandwidth of their algorithmic bytes."""
    px = B * H * W
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get('Name') or r.get('KernelName') or ''
            if 'head_' not in name:
                continue
            avg_ns = float(r.get('AverageNs') or r.get('AverageNS') or r.get('Average') or 0)
            calls = int(float(r.get('Calls') or r.get('Count') or 0))
            es, mode = head_kind(name)
            per_px = {'train': (32 + 32) * (es or 4) + 2 * oc * 4, 'bwd': (32 + 32) * (es or 4) + oc * 4, 'fwd': 32 * (es or 4) + oc * 4}.get(mode)
            rows.append({'kernel': name[:100], 'calls': calls, 'avg_ms': round(avg_ns / 1e6, 4), 'bytes_per_px': per_px,
                         'GB_per_s': round(px * per_px / avg_ns, 1) if per_px and avg_ns else None})
    print(json.dumps({'head_kernels': rows, 'pixels': px, 'planes': oc}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--height', type=int, default=1344)
    ap.add_argument('--width', type=int, default=2000)
    ap.add_argument('--configs', default='x9:fp32,x9:bf16,b4:fp32,b4:bf16')
    ap.add_argument('--head-stats', default=None, help='rocprofv3 kernel_stats.csv to summarise instead of timing')
    ap.add_argument('--planes', type=int, default=9, help='--head-stats: output planes of the profiled head')
    a = ap.parse_args()
    if a.height % 16 or a.width % 16:
        ap.error('height and width must be multiples of 16')
    if a.head_stats:
        head_stats(a.head_stats, a.batch, a.height, a.width, a.planes)
        return
    import eld_amd
    eld_amd.load_library()
    res = {'tool': 'xtrans_step', 'shape': [a.batch, a.height, a.width], 'steps': a.steps, 'warmup': a.warmup, 'results': []}
    for c in a.configs.split(','):
        kind, prec = c.split(':')
        res['results'].append(time_config(9 if kind == 'x9' else 4, prec, a.batch, a.height, a.width, a.steps, a.warmup))
    by = {(r['planes'], r['precision']): r for r in res['results']}
    for prec in ('fp32', 'bf16'):
        if (9, prec) in by and (4, prec) in by:
            res['x9_over_b4_%s' % prec] = round(by[(9, prec)]['ms_median'] / by[(4, prec)]['ms_median'], 4)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
