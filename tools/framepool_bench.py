#!/usr/bin/env python3
"""Measurements of the frame pool (eld_amd/framepool.py, csrc/framepool.hip); DESIGN.md sec. 12 quotes them.

  whole_frame   eld_crop_pack_raw_bayer_u16 against the existing eld_pack_raw_bayer_u16_gain on the same 8 frames of 2848 x 4256, cut as
                8 whole-frame patches of 4 x 1424 x 2128: both read 2 B per sensor pixel, the crop writes 2 B where the pack writes 4 B.
                Both are the bare entry points (records uploaded and outputs allocated beforehand), event-timed over 5 launches back to
                back, the two alternating in one process, median of --reps; the spread is (max - min) / median of each.
  train_shape   8 patches of C x 512 x 512 at the loader's random offsets, Bayer and X-Trans: time per patches() call (host checks, record
                upload, one launch), per bare entry call with the records already on the device, and the share of patches that took the
                4-byte load path.  34 MB (76 MB X-Trans) per launch is a few
                microseconds at HBM speed: launch-bound, so no bandwidth fraction is quoted.
  rate          Engine.train from a FramePoolLoader against the DataLoader path of tools/dropin_rate.py (run as a child process on the
                same board, 8 workers) at 1 and 8 patches of 4 x 512 x 512 per step.

    python tools/framepool_bench.py [--reps 10] [--peak-tbs 8.0] [--out profiles/framepool_bench.json] [--skip-rate]
"""
import argparse
import contextlib
import ctypes
import io
import json
import os
import re
import subprocess
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from eld_amd import _lib as L                                  # noqa: E402
from eld_amd.framepool import Crops, FramePool, FramePoolLoader    # noqa: E402

PATTERN, BLACK, WHITE = [0, 1, 3, 2], [512.0] * 4, 16383.0


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    m = float(np.median(ts))
    return {'median_ms': round(m, 4), 'min_ms': round(float(min(ts)), 4), 'max_ms': round(float(max(ts)), 4), 'spread': round((max(ts) - min(ts)) / m, 4)}


def entry_call(pool, crops):
    """-> a function that calls eld_crop_pack_raw_*_u16 once on records that are already on the device, into one output tensor."""
    rec = torch.from_numpy(crops.records.view(np.uint8).copy()).cuda()
    out = torch.empty((len(crops), pool.C, crops.ph, crops.pw), dtype=torch.int16, device='cuda')
    head = (L.dptr(pool.buffer), pool.elems, L.dptr(pool._table_dev), len(pool), int(pool.extent[:, 0].max()), int(pool.extent[:, 1].max()),
            L.dptr(rec), len(crops), crops.ph, crops.pw)
    if pool.cfa == 'bayer':
        pat, blk = (ctypes.c_int * 4)(*pool.raw_pattern), (ctypes.c_float * 4)(*pool.black_level)
        args = head + (pat, blk, float(pool.white_point), L.dptr(out), None)
        fn = L.lib().eld_crop_pack_raw_bayer_u16
    else:
        args = head + (float(pool.black_level[0]), float(pool.white_point), L.dptr(out), None)
        fn = L.lib().eld_crop_pack_raw_xtrans_u16

    def call(keep=(rec, out)):
        L.check(fn(*args[:-1], L.cur_stream()))
    return call


def whole_frame(reps, peak):
    rng = np.random.default_rng(0)
    N, Hm, Wm = 8, 2848, 4256
    frames = [rng.integers(400, 4096, size=(Hm, Wm), dtype=np.uint16) for _ in range(N)]
    pool = FramePool(frames, raw_pattern=[[0, 1], [3, 2]], black_level=512)
    crops = pool.check(Crops.make(range(N), [0] * N, [0] * N, Hm // 2, Wm // 2, ratios=100.0))
    stack = torch.from_numpy(np.stack(frames).view(np.int16)).cuda()
    ratios = torch.full((N,), 100.0, device='cuda')
    out32 = torch.empty((N, 4, Hm // 2, Wm // 2), dtype=torch.float32, device='cuda')
    pat, blk = (ctypes.c_int * 4)(*PATTERN), (ctypes.c_float * 4)(*BLACK)

    def pack():
        L.check(L.lib().eld_pack_raw_bayer_u16_gain(L.dptr(stack), L.dptr(out32), N, Hm // 2, Wm // 2, pat, blk, WHITE, L.dptr(ratios), L.cur_stream()))

    crop = entry_call(pool, crops)                           # the bare entry point, as pack() is: records uploaded once, output allocated once
    for _ in range(2):
        pack(), crop()
    tp, tc = [], []
    for _ in range(reps):                                    # alternate the two; 5 launches back to back per timing, so the queue never runs dry
        tp.append(event_ms(lambda: [pack() for _ in range(5)]) / 5)
        tc.append(event_ms(lambda: [crop() for _ in range(5)]) / 5)
    px = N * Hm * Wm
    sp, sc = stats(tp), stats(tc)
    sp['hbm_frac'] = round(px * 6 / (sp['median_ms'] * 1e-3) / (peak * 1e12), 3)
    sc['hbm_frac'] = round(px * 4 / (sc['median_ms'] * 1e-3) / (peak * 1e12), 3)
    return {'frames': [N, Hm, Wm], 'pack_u16_gain': sp, 'crop_pack': sc, 'crop_over_pack': round(sc['median_ms'] / sp['median_ms'], 4),
            'wide_loads': bool(pool.wide_loads(crops).all())}


def train_shape(cfa, reps):
    rng = np.random.default_rng(1)
    shape = (2848, 4256) if cfa == 'bayer' else (4160, 6240)
    pool = FramePool([rng.integers(400, 4096, size=shape, dtype=np.uint16) for _ in range(4)], cfa=cfa)
    nm = types.SimpleNamespace(_sample_params=lambda: (1.0, 1.0, 15583, 100.0))
    loader = FramePoolLoader(pool, nm, 8, patch=512, augment=False)
    np.random.seed(0)
    draws = [loader.draw()[0] for _ in range(200)]
    narrow = float(np.mean([1.0 - pool.wide_loads(c).mean() for c in draws]))
    for c in draws[:3]:
        pool.patches(c)
    ts, tk = [], []
    for r in range(reps):
        batch = draws[20 * r % 200:20 * r % 200 + 20]
        ts.append(event_ms(lambda: [pool.patches(c) for c in batch]) / len(batch))
        calls = [entry_call(pool, pool.check(c)) for c in batch]
        calls[0]()
        tk.append(event_ms(lambda: [f() for f in calls]) / len(calls))
    s = stats(ts)
    s['entry_only'] = stats(tk)                               # the launches alone, back to back: records already on the device
    return dict(s, cfa=cfa, patches=[8, pool.C, 512, 512], mbytes_per_launch=round(8 * pool.C * 512 * 512 * 4 / 1e6, 1), share_4byte_path=round(narrow, 4),
                note='launch-bound: time per patches() call (record upload + one launch), median over %d runs of 20 calls' % reps)


def rate_pool(batch, steps):
    from eld_amd.engine import Engine
    from eld_amd.noise import NoiseModel
    rng = np.random.default_rng(2)
    pool = FramePool([rng.integers(400, 4096, size=(2848, 4256), dtype=np.uint16) for _ in range(8)], raw_pattern=[[0, 1], [3, 2]], black_level=512)
    np.random.seed(2018)
    torch.manual_seed(2018)
    tmp = tempfile.mkdtemp()
    with contextlib.redirect_stdout(io.StringIO()):
        nm = NoiseModel(model='PGRU', include=4)
        loader = FramePoolLoader(pool, nm, batch, patch=512, steps_per_epoch=steps)
        opt = types.SimpleNamespace(gpu_ids=[0], isTrain=True, checkpoints_dir=tmp, name='t', netG='unet', channels=4, stage_in='raw', stage_out='raw',
                                    lr=1e-4, beta1=0.9, wd=0.0, loss='l1', resume=False, chop=False, no_log=True, save_epoch_freq=10 ** 6, model='eld_model',
                                    seed=2018)
        eng = Engine(opt)
        eng.train(loader)                                    # warm-up epoch
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.train(loader)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    return {'batch': batch, 'iterations': steps, 'ms_per_iteration': round(dt / steps * 1e3, 3), 'it_per_s': round(steps / dt, 1)}


def rate_dataloader(batch, patches):
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'dropin_rate.py'), str(batch), '8', str(patches)], capture_output=True, text=True,
                         timeout=600)
    m = re.search(r'(\d+) iterations in ([\d.]+) s = ([\d.]+) it/s = ([\d.]+) ms per iteration', out.stdout)
    if out.returncode != 0 or not m:
        raise RuntimeError('tools/dropin_rate.py failed (%d):\n%s\n%s' % (out.returncode, out.stdout[-2000:], out.stderr[-2000:]))
    return {'batch': batch, 'iterations': int(m.group(1)), 'ms_per_iteration': float(m.group(4)), 'it_per_s': float(m.group(3)), 'workers': 8}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--peak-tbs', type=float, default=8.0, help='HBM peak, TB/s (MI355X: 8.0)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'framepool_bench.json'))
    ap.add_argument('--skip-rate', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('framepool_bench.py needs a GPU: nothing is measured without one')
    L.load_library()
    res = {'device': torch.cuda.get_device_name(0), 'library_src_hash': L.build_src_hash(), 'reps': a.reps, 'peak_tbs': a.peak_tbs}
    res['whole_frame'] = whole_frame(a.reps, a.peak_tbs)
    print(json.dumps(res['whole_frame']), flush=True)
    res['train_shape'] = [train_shape(cfa, a.reps) for cfa in ('bayer', 'xtrans')]
    print(json.dumps(res['train_shape']), flush=True)
    if not a.skip_rate:
        res['rate'] = []
        for batch, patches in ((1, 256), (8, 256)):
            steps = patches // batch
            row = {'pool': rate_pool(batch, steps), 'dataloader': rate_dataloader(batch, patches)}
            res['rate'].append(row)
            print(json.dumps(row), flush=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
