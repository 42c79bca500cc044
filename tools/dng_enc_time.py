"""Time the lossless-JPEG encoder on one 24 MP Bayer frame (4000 x 6000, 14 bits, tiles of 256 x 256): each of the four
kernels behind eld_amd.dng.encode_ljpeg, the whole encode_ljpeg call (host planning, the synchronisations and the copy of the compressed
bytes included), and next to them, in the same run, a device-to-device copy of the frame and eld_dng_ljpeg_u16 decoding the file that
write_dng(compression=7) has just written.  The scene is tools/dng_time.py's: a signal ramp with Poisson-Gaussian noise.

    python tools/dng_enc_time.py [--reps 20] [--warmup 3] [--segment 0] [--chunk 0] [--out result.json]

The calls alternate inside one process; each is timed with device events around one call (the whole encode_ljpeg by the host's clock, since it
synchronises).  Prints the median, the 10th and 90th percentile per call, the sum of the kernels' medians (the encode's device time), its ratio
to the copy and to the decode.  The one condition: the encode's device time is below the decode's; exit status 1 otherwise."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HM, WM, P, TILE = 4000, 6000, 14, 256
KERNELS = ('hist', 'pack', 'ffcount', 'cumsum', 'stuff')


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--segment', type=int, default=0, help='samples per segment (0: the default)')
    ap.add_argument('--chunk', type=int, default=0, help='bytes per stuffing chunk (0: the default)')
    ap.add_argument('--out')
    a = ap.parse_args(argv)
    import torch
    import eld_amd
    from eld_amd import _lib as L
    from eld_amd import dng as D
    lib = eld_amd.load_library()
    if not torch.cuda.is_available():
        raise RuntimeError('tools/dng_enc_time.py measures on a GPU: there is none')
    dev = torch.device('cuda', torch.cuda.current_device())
    g = torch.Generator(device='cuda').manual_seed(1)
    ramp = 4.0 * 1500.0 ** (torch.arange(WM, device='cuda', dtype=torch.float32) / (WM - 1))                    # electrons, 4 -> 6000
    e = ramp[None, :].expand(HM, WM)
    u = 2.0 * (e + e.sqrt() * torch.randn((HM, WM), device='cuda', generator=g)) + 3.0 * torch.randn((HM, WM), device='cuda', generator=g) + 512
    frame = u.round().clamp(0, 16383).to(torch.int16).contiguous()
    del u, e

    # ---- the file, and the decode of it as eld_amd.dng.read_dng sets it up
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, 'frame.dng')
    D.write_dng(path, frame, meta={'cfa': 'bayer', 'white_point': 16383}, compression=7, tile=(TILE, TILE), bits=P)
    file_bytes = os.path.getsize(path)
    t, buf, lay, meta, (lo, hi), recs, huff, ws_elems, lin = D._plan(path)
    host = np.zeros(hi - lo + D.PAD, dtype=np.uint8)
    host[:hi - lo] = np.frombuffer(buf, dtype=np.uint8, count=hi - lo, offset=lo)
    d_blob = torch.from_numpy(host).to(dev)
    d_recs = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).to(dev)
    d_huff = torch.from_numpy(huff.view(np.uint8).reshape(-1).copy()).to(dev)
    out_lj = torch.zeros((HM, WM), dtype=torch.int16, device=dev)
    st_lj = torch.zeros(len(recs), dtype=torch.int32, device=dev)
    st = L.cur_stream()

    def decode():
        L.check(lib.eld_dng_ljpeg_u16(L.dptr(d_blob), hi - lo, L.dptr(d_recs), len(recs), L.dptr(d_huff), len(huff), HM, WM, 0, 0, HM, WM, None, 0,
                                      None, 0, 0, L.dptr(out_lj), L.dptr(st_lj), st), 'eld_dng_ljpeg_u16')

    dst = torch.empty_like(frame)

    def copy():
        dst.copy_(frame)

    # ---- the encoder's steps on one planned encode
    enc = D.Encoder(frame, (TILE, TILE), P, a.segment, a.chunk)
    enc.hist()
    enc.plan()
    enc.pack()
    enc.ffcount()
    enc.sizes()
    enc.stuff()

    def cumsum():
        cum = torch.cumsum(enc.d_count, 0, dtype=torch.int32)
        enc.d_before = (cum - enc.d_count).contiguous()

    steps = {'hist': enc.hist, 'pack': enc.pack, 'ffcount': enc.ffcount, 'cumsum': cumsum, 'stuff': enc.stuff, 'copy': copy, 'decode': decode}
    order = ('hist', 'copy', 'pack', 'decode', 'ffcount', 'copy', 'cumsum', 'stuff', 'decode')
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
        streams = D.encode_ljpeg(frame, (TILE, TILE), P, a.segment, a.chunk)
        t1 = time.perf_counter()
        if i >= a.warmup:
            times.setdefault('encode_ljpeg', []).append((t1 - t0) * 1e6)
    assert int(st_lj.abs().sum()) == 0 and torch.equal(out_lj, frame)            # the file decodes to the frame
    assert streams == enc.streams()                                              # the timed steps left the same bytes
    props = torch.cuda.get_device_properties(0)
    res = {'reps': a.reps, 'warmup': a.warmup, 'device': torch.cuda.get_device_name(0), 'src': L.build_src_hash(), 'sites': HM * WM, 'tile': TILE,
           'bits': P, 'streams': enc.ns, 'segment': enc.segment, 'segments': enc.ns * enc.nseg, 'chunk': enc.chunk, 'chunks': enc.nchunks,
           'raw_bytes': int(enc.nraw.sum()), 'stuffed_bytes': enc.out_bytes, 'file_bytes': file_bytes, 'cus': props.multi_processor_count}
    for kind in KERNELS + ('copy', 'decode', 'encode_ljpeg'):
        v = np.asarray(times[kind])
        res[kind] = {'median_us': float(np.median(v)), 'p10_us': float(np.percentile(v, 10)), 'p90_us': float(np.percentile(v, 90))}
    res['encode_device_us'] = sum(res[k]['median_us'] for k in KERNELS)
    res['encode_over_copy'] = res['encode_device_us'] / res['copy']['median_us']
    res['encode_over_decode'] = res['encode_device_us'] / res['decode']['median_us']
    res['encode_msamples_per_s'] = HM * WM / res['encode_device_us']
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    os.remove(path)
    os.rmdir(tmp)
    if res['encode_device_us'] >= res['decode']['median_us']:
        print('the encode took longer on the device than the decode: something is wrong', file=sys.stderr)
        return 1
    return 0


if __name__ == '__main__':
    sys.exit(main())
