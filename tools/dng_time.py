"""Time the two DNG decoders on one 24 MP Bayer frame (4000 x 6000, 14 bits): eld_dng_ljpeg_u16 on lossless-JPEG tiles
of 256 x 256 with two components (the layout Adobe's converter writes) and eld_dng_unpack_u16 on the same frame as packed 14-bit rows.  Next
to each time stands a device-to-device copy of the decoded frame (2 bytes read and 2 written per site), timed in the same process.  The
scene is tools/noiselevel_time.py's: a signal ramp with Poisson-Gaussian noise.

    python tools/dng_time.py [--reps 20] [--warmup 3] [--distinct 16] [--out result.json]

Encoding 24 MP with the NumPy encoder of tests/dng_ref.py takes a while, so --distinct tiles of the scene are encoded (each with its own
Huffman table) and every tile position gets its own copy of one of those streams; --distinct 0 encodes all of them.  The calls alternate
inside one process; each is timed with device events around one call.  Prints the median, the 10th and 90th percentile per call, the ratio
of the medians to the copy's, and the occupancy of the one-lane-per-stream design (streams against the lanes of the device)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

HM, WM, P, TILE = 4000, 6000, 14, 256


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--distinct', type=int, default=16)
    ap.add_argument('--out')
    a = ap.parse_args(argv)
    import torch
    import dng_ref as R
    import eld_amd
    from eld_amd import _lib as L
    from eld_amd import dng as D
    lib = eld_amd.load_library()
    if not torch.cuda.is_available():
        raise RuntimeError('tools/dng_time.py measures on a GPU: there is none')
    dev = torch.device('cuda', torch.cuda.current_device())
    g = torch.Generator(device='cuda').manual_seed(1)
    ramp = 4.0 * 1500.0 ** (torch.arange(WM, device='cuda', dtype=torch.float32) / (WM - 1))                    # electrons, 4 -> 6000
    e = ramp[None, :].expand(HM, WM)
    u = 2.0 * (e + e.sqrt() * torch.randn((HM, WM), device='cuda', generator=g)) + 3.0 * torch.randn((HM, WM), device='cuda', generator=g) + 512
    frame = u.round().clamp(0, 16383).to(torch.int32).cpu().numpy().astype(np.uint16)
    del u, e
    st = L.cur_stream()
    ny, nx = -(-HM // TILE), -(-WM // TILE)

    # ---- lossless JPEG: records, tables and the blob, as eld_amd.dng._plan builds them from a file
    pos = [(ty, tx) for ty in range(ny) for tx in range(nx)]
    pick = pos if a.distinct <= 0 else [pos[(i * len(pos)) // a.distinct] for i in range(a.distinct)]
    enc = {}
    for ty, tx in pick:
        t = frame[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE]
        t = np.pad(t, ((0, TILE - t.shape[0]), (0, TILE - t.shape[1])), mode='edge')
        data, _ = R.ljpeg_encode(t.reshape(-1), P, TILE // 2, TILE, 2, pred=1)
        enc[(ty, tx)] = (data, t)
    keys = sorted(enc)
    recs = np.zeros(len(pos), dtype=L.DNG_STREAM_DTYPE)
    tables, index, blob, want = [], {}, bytearray(), np.zeros((HM, WM), dtype=np.uint16)
    for i, (ty, tx) in enumerate(pos):
        data, t = enc[(ty, tx)] if (ty, tx) in enc else enc[keys[i % len(keys)]]
        j = D.parse_ljpeg(data, 0, len(data), 'tile %d' % i)
        r = recs[i]
        r['x0'], r['y0'], r['tw'], r['th'] = tx * TILE, ty * TILE, TILE, TILE
        r['data_off'], r['data_len'] = len(blob) + j['data'][0], j['data'][1]
        r['P'], r['X'], r['Y'], r['Nf'], r['pred'] = j['P'], j['X'], j['Y'], j['Nf'], j['pred']
        for k, (counts, syms) in enumerate(j['tables']):
            key = (tuple(counts), tuple(syms))
            if key not in index:
                index[key] = len(tables)
                tables.append(D.huff_record(counts, syms, 'tile %d' % i))
            r['table'][k] = index[key]
        blob += data
        want[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE] = t[:HM - ty * TILE, :WM - tx * TILE]
    lj_bytes = len(blob)
    d_blob = torch.from_numpy(np.frombuffer(bytes(blob) + bytes(D.PAD), dtype=np.uint8).copy()).to(dev)
    d_recs = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).to(dev)
    d_huff = torch.from_numpy(np.array(tables, dtype=L.DNG_HUFF_DTYPE).view(np.uint8).reshape(-1).copy()).to(dev)
    out_lj = torch.zeros((HM, WM), dtype=torch.int16, device=dev)
    st_lj = torch.zeros(len(recs), dtype=torch.int32, device=dev)

    def ljpeg():
        L.check(lib.eld_dng_ljpeg_u16(L.dptr(d_blob), lj_bytes, L.dptr(d_recs), len(recs), L.dptr(d_huff), len(tables), HM, WM, 0, 0, HM, WM, None, 0,
                                      None, 0, 0, L.dptr(out_lj), L.dptr(st_lj), st), 'eld_dng_ljpeg_u16')

    # ---- packed 14-bit rows, one strip
    packed = b''.join(R.pack_rows(frame[r:r + 250], P) for r in range(0, HM, 250))        # rows are byte-aligned: chunks concatenate
    urec = np.zeros(1, dtype=L.DNG_STREAM_DTYPE)
    urec['data_len'], urec['tw'], urec['th'] = len(packed), WM, HM
    d_packed = torch.from_numpy(np.frombuffer(packed + bytes(D.PAD), dtype=np.uint8).copy()).to(dev)
    d_urec = torch.from_numpy(urec.view(np.uint8).reshape(-1).copy()).to(dev)
    out_un = torch.zeros((HM, WM), dtype=torch.int16, device=dev)
    st_un = torch.zeros(1, dtype=torch.int32, device=dev)

    def unpack():
        L.check(lib.eld_dng_unpack_u16(L.dptr(d_packed), len(packed), L.dptr(d_urec), 1, P, 0, HM, WM, 0, 0, HM, WM, None, 0, L.dptr(out_un),
                                       L.dptr(st_un), st), 'eld_dng_unpack_u16')

    dst = torch.empty_like(out_un)

    def copy():
        dst.copy_(out_un)

    times = {}
    for i in range(a.warmup + a.reps):
        for kind, fn in (('ljpeg', ljpeg), ('copy', copy), ('unpack', unpack), ('copy', copy)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                times.setdefault(kind, []).append(e0.elapsed_time(e1) * 1e3)
    assert int(st_lj.abs().sum()) == 0 and int(st_un.abs().sum()) == 0
    assert np.array_equal(out_lj.cpu().numpy().view(np.uint16), want) and np.array_equal(out_un.cpu().numpy().view(np.uint16), frame)
    props = torch.cuda.get_device_properties(0)
    lanes = props.multi_processor_count * 4 * 64
    res = {'reps': a.reps, 'warmup': a.warmup, 'device': torch.cuda.get_device_name(0), 'src': L.build_src_hash(), 'sites': HM * WM, 'tile': TILE,
           'streams': len(recs), 'distinct_streams': len(enc), 'tables': len(tables), 'ljpeg_bytes': lj_bytes, 'packed_bytes': len(packed),
           'simds': props.multi_processor_count * 4, 'lanes': lanes, 'lane_occupancy': len(recs) / lanes,
           'simd_occupancy': min(1.0, len(recs) / (props.multi_processor_count * 4))}
    for kind in ('ljpeg', 'unpack', 'copy'):
        t = np.asarray(times[kind])
        res[kind] = {'median_us': float(np.median(t)), 'p10_us': float(np.percentile(t, 10)), 'p90_us': float(np.percentile(t, 90))}
    res['ljpeg_over_copy'] = res['ljpeg']['median_us'] / res['copy']['median_us']
    res['unpack_over_copy'] = res['unpack']['median_us'] / res['copy']['median_us']
    res['ljpeg_msamples_per_s'] = HM * WM / res['ljpeg']['median_us']
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
