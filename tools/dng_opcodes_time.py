"""Time the DNG opcode kernels on one 24 MP frame (4000 x 6000 float32) with the phone program: four GainMaps of
13 x 17 points, pitch 2, offsets (0,0) (0,1) (1,0) (1,1).  eld_dng_opcodes_apply_f32 (4 B read and 4 B written per site), out of place and in
place, and eld_dng_opcodes_gain_f32 (4 B written per site) stand next to a device-to-device copy of the same frame (4 B read and 4 B
written), timed in the same process; the apply and the gain plane are also timed with the maps read from the blob instead of LDS.

    python tools/dng_opcodes_time.py [--reps 20] [--warmup 3] [--out result.json]

The calls alternate inside one process; each is timed with device events around one call, and goes straight to the library with arguments
prepared beforehand (the Python wrappers' argument checks take longer than the kernels run and would be what the events see).  Prints the
median, the 10th and 90th percentile per call, the ratio of the medians to the copy's, the bytes per second each call moves, and per call
the time of ten back-to-back launches divided by ten (`train10_us`: what is left when no host gap separates the launches)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

HM, WM = 4000, 6000


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out')
    a = ap.parse_args(argv)
    import torch
    import dng_opcodes_cases as C
    import dng_opcodes_ref as R
    import eld_amd
    from eld_amd import _lib as L
    from eld_amd import dng_opcodes as O
    eld_amd.load_library()
    if not torch.cuda.is_available():
        raise RuntimeError('tools/dng_opcodes_time.py measures on a GPU: there is none')
    specs = C.phone_program(HM, WM)
    ops = C.to_opcodes(specs)
    prog, gprog = O.OpcodeProgram(ops, HM, WM), O.gain_program(ops, [], HM, WM)
    g = torch.Generator(device='cuda').manual_seed(1)
    frame = torch.rand((HM, WM), device='cuda', generator=g)
    out, plane, dst, work = torch.empty_like(frame), torch.empty_like(frame), torch.empty_like(frame), frame.clone()

    lib, st = L.lib(), L.cur_stream()
    blob, nb = prog.blob_on(frame.device), int(prog.blob.size)
    recs, grecs = prog.c_records(), gprog.c_records()
    p_frame, p_out, p_work, p_plane, p_blob = (L.dptr(t) for t in (frame, out, work, plane, blob))

    def apply(src, dst_, budget):
        return lambda: L.check(lib.eld_dng_opcodes_apply_f32(src, dst_, 1, HM, WM, recs, len(prog), p_blob, nb, budget, st), 'eld_dng_opcodes_apply_f32')

    def gain(budget):
        return lambda: L.check(lib.eld_dng_opcodes_gain_f32(p_plane, HM, WM, grecs, len(gprog), p_blob, nb, budget, st), 'eld_dng_opcodes_gain_f32')

    def copy():
        dst.copy_(frame)
    calls = (('apply', apply(p_frame, p_out, -1)), ('copy', copy), ('apply_in_place', apply(p_work, p_work, -1)), ('copy', copy),
             ('gain', gain(-1)), ('copy', copy), ('apply_maps_from_blob', apply(p_frame, p_out, 0)), ('copy', copy),
             ('gain_maps_from_blob', gain(0)), ('copy', copy))
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
    apply(p_frame, p_out, -1)()
    gain(-1)()
    torch.cuda.synchronize()
    # the timed calls computed the restatement's values (a band of rows: the NumPy side of 24 MP takes a while)
    rows = slice(1000, 1064)
    x = frame[rows].cpu().numpy()
    full = R.gain_plane(specs, [], HM, WM, rows)                      # every site is addressed by one of the four maps: apply = clip(x * gain)
    assert np.array_equal(plane[rows].cpu().numpy().view(np.uint32), full.view(np.uint32))
    clipped = np.where(x * full > 1, np.float32(1), x * full).astype(np.float32)
    assert np.array_equal(out[rows].cpu().numpy().view(np.uint32), clipped.view(np.uint32))
    res = {'reps': a.reps, 'warmup': a.warmup, 'device': torch.cuda.get_device_name(0), 'src': L.build_src_hash(), 'sites': HM * WM,
           'operations': len(prog), 'blob_bytes': int(prog.blob.size)}
    nbytes = {'gain': 4 * HM * WM, 'gain_maps_from_blob': 4 * HM * WM}
    for kind in sorted(times):
        t = np.asarray(times[kind])
        res[kind] = {'median_us': float(np.median(t)), 'p10_us': float(np.percentile(t, 10)), 'p90_us': float(np.percentile(t, 90)),
                     'tb_per_s': nbytes.get(kind, 8 * HM * WM) / float(np.median(t)) * 1e-6, 'train10_us': train[kind],
                     'train10_tb_per_s': nbytes.get(kind, 8 * HM * WM) / train[kind] * 1e-6}
    for kind in sorted(times):
        if kind != 'copy':
            res[kind + '_over_copy'] = res[kind]['median_us'] / res['copy']['median_us']
            res[kind + '_train10_over_copy'] = res[kind]['train10_us'] / res['copy']['train10_us']
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
