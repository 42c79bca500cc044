"""Stage timings of the calibration pipeline (eld_amd/calibrate.py) on synthetic frames: 9 ISOs x (2 bias frames + 8 flat pairs) of
4256 x 2848 mosaics, plus one 8288 x 5520 bias stack (Nikon D850 size).  Reports per stage the device time (hip events, median of
--reps), the stats kernels' GB/s against the measured 6.3 TB/s HBM ceiling, the PPCC's element*lambda/s against its VALU throughput
bound (ppcc_bound) and torch.sort's time.  One JSON line at the end (profiles/calib_bench.json is one such run).

    python tools/calib_bench.py [--reps 5] [--isos 9] [--out FILE]
    python tools/calib_bench.py --cfa xtrans | --cfa bayer2      (the cell passes against the Bayer entry points)
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eld_amd import _lib as L  # noqa: E402
from eld_amd import calibrate as CAL  # noqa: E402

HBM_BPS = 6.3e12                 # measured HBM ceiling of the MI355X (float4 copy)
CUS, SIMDS, CLOCK = 256, 4, 2.4e9   # 2.4 GHz: the peak shader clock, so the bound below is an upper bound

# PPCC VALU bound, a throughput model of ppcc_partial_kernel's inner loop (gfx950 ISA, 124 VGPRs: 4 waves per SIMD, enough to keep the
# vector unit issuing).  Cycles per wave64 instruction at throughput: fp32 2 (32 lanes per cycle), float64 FMA / add / mul / conversion
# 4 (half rate: 78.6 of 157.3 TF/s), transcendental 8 (quarter rate).  Per (wave, lambda):
CYC_HEAD = 2 * 2                 # x = lam g, the |x| < 1 test
CYC_DIRECT = 4 * 2 + 2 * 8       # |x| >= 1 in some lane: 2 mul, sub, mul by 1/lam; 2 exp2
CYC_POLY = 9 * 2 + 1 * 8         # |x| < 1 in some lane: x^2, 5-term Horner, lam h + 1, 2 mul; 1 exp2
CYC_ACC = 1 * 4 + 2 * 4          # M -> float64, 2 float64 FMAs
CYC_PAIR = 120                   # per wave and pair, shared by the block's 16 lambdas: the Filliben medians (float64), 2 log2, h, g,
                                 # the two loads -> dt, the t sums (~30 float64 / fp32 ops)
PP_LG = 16


def ppcc_bound(n, lambdas):
    """element*lambda/s the kernel could reach at these prices: every wave of 64 adjacent pairs runs the polynomial and / or the direct
    form for each lambda as its lanes need (a wave whose lanes disagree runs both)."""
    npairs = n // 2
    i = np.arange(npairs, dtype=np.float64)
    m = (i + 1 - 0.3175) / (n + 0.365)
    m[0] = 1 - 0.5 ** (1.0 / n)
    g = (np.log2(1 - m) - np.log2(m)) * (np.log(2) / 2)
    pad = (-npairs) % 64
    g = np.concatenate([g, np.full(pad, g[-1])]).reshape(-1, 64)
    gmin, gmax = g.min(axis=1), g.max(axis=1)
    cyc = 0.0
    for lam in np.abs(np.asarray(lambdas, np.float64)):
        poly = np.count_nonzero(lam * gmin < 1)
        direct = np.count_nonzero(lam * gmax >= 1)
        cyc += g.shape[0] * (CYC_HEAD + CYC_ACC + CYC_PAIR / PP_LG) + poly * CYC_POLY + direct * CYC_DIRECT
    return float(n) * len(lambdas) * CUS * SIMDS * CLOCK / cyc      # cyc: SIMD cycles of the whole launch, spread over every SIMD


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(ts))


def frames(F, Hm, Wm, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randint(480, 560, (F, Hm, Wm), generator=g, device='cuda', dtype=torch.int32)
    return x.to(torch.int16)


def bench_stack(u, reps, lam):
    F, Hm, Wm = u.shape
    n = Hm * Wm
    lib = L.lib()
    pat = (ctypes.c_int * 4)(0, 1, 3, 2)
    cs = torch.empty((F, 4, 2), dtype=torch.int64, device='cuda')
    rs = torch.empty((F, Hm, 2), dtype=torch.int64, device='cuda')
    ws = torch.empty(lib.eld_calib_bias_stats_workspace_bytes(F, Hm), dtype=torch.uint8, device='cuda')
    t_stats = timed(lambda: L.check(lib.eld_calib_bias_stats(L.dptr(u), F, Hm, Wm, pat, L.dptr(cs), L.dptr(rs), L.dptr(ws), ws.numel(),
                                                             L.cur_stream())), reps)
    st = CAL.bias_stats_from_sums(cs.cpu().numpy(), rs.cpu().numpy(), [[0, 1], [3, 2]], [512.0] * 4, Hm, Wm)
    cb = torch.from_numpy(st['color_bias']).cuda()
    rho = torch.from_numpy(st['row_offset']).cuda()
    t = torch.empty((F, n), dtype=torch.float32, device='cuda')
    blk = (ctypes.c_double * 4)(512.0, 512.0, 512.0, 512.0)
    t_res = timed(lambda: L.check(lib.eld_calib_bias_residual(L.dptr(u), F, Hm, Wm, pat, blk, L.dptr(cb), L.dptr(rho), L.dptr(t),
                                                              L.cur_stream())), reps)
    ts = {}
    t_sort = timed(lambda: ts.__setitem__('v', torch.sort(t, dim=1).values), reps)
    x = ts['v'].contiguous()
    lamd = torch.from_numpy(lam.astype(np.float32)).cuda()
    sums = torch.empty((F, lam.size, 2), dtype=torch.float64, device='cuda')
    tsums = torch.empty((F, 2), dtype=torch.float64, device='cuda')
    pws = torch.empty(lib.eld_calib_ppcc_workspace_bytes(F, n, lam.size), dtype=torch.uint8, device='cuda')
    t_ppcc = timed(lambda: L.check(lib.eld_calib_ppcc(L.dptr(x), F, n, L.dptr(lamd), lam.size, L.dptr(sums), L.dptr(tsums), L.dptr(pws),
                                                      pws.numel(), L.cur_stream())), reps)
    return {'frames': F, 'Hm': Hm, 'Wm': Wm,
            'bias_stats_s': t_stats, 'bias_stats_GBps': F * n * 2 / t_stats / 1e9,
            'residual_s': t_res, 'residual_GBps': F * n * 6 / t_res / 1e9,
            'sort_s': t_sort, 'ppcc_s': t_ppcc, 'ppcc_elem_lambda_per_s': F * n * lam.size / t_ppcc}


def bench_flats(ab, reps):
    P, _, Hm, Wm = ab.shape
    lib = L.lib()
    pat = (ctypes.c_int * 4)(0, 1, 3, 2)
    out = torch.empty((P, 4, 4), dtype=torch.int64, device='cuda')
    ws = torch.empty(lib.eld_calib_flat_stats_workspace_bytes(P, Hm), dtype=torch.uint8, device='cuda')
    t = timed(lambda: L.check(lib.eld_calib_flat_stats(L.dptr(ab), P, Hm, Wm, pat, 16383, L.dptr(out), L.dptr(ws), ws.numel(),
                                                       L.cur_stream())), reps)
    return {'pairs': P, 'flat_stats_s': t, 'flat_stats_GBps': P * 2 * Hm * Wm * 2 / t / 1e9}


def bench_cells(F, Hm, Wm, reps):
    """--cfa xtrans: the X-Trans cell statistics (p = 6) against the Bayer bias statistics on the same mosaics, and the flat pass."""
    lib = L.lib()
    u = frames(F, Hm, Wm, 7)
    pat = (ctypes.c_int * 4)(0, 1, 3, 2)
    cs = torch.empty((F, 4, 2), dtype=torch.int64, device='cuda')
    rs = torch.empty((F, Hm, 2), dtype=torch.int64, device='cuda')
    ws = torch.empty(lib.eld_calib_bias_stats_workspace_bytes(F, Hm), dtype=torch.uint8, device='cuda')
    xcs = torch.empty((F, 6, 6, 2), dtype=torch.int64, device='cuda')
    xrs = torch.empty((F, Hm, 6), dtype=torch.int64, device='cuda')
    xws = torch.empty(lib.eld_calib_cell_stats_workspace_bytes(F, Hm, 6), dtype=torch.uint8, device='cuda')
    bayer, xtrans = [], []
    for _ in range(3):                                   # interleaved A/B
        bayer.append(timed(lambda: L.check(lib.eld_calib_bias_stats(L.dptr(u), F, Hm, Wm, pat, L.dptr(cs), L.dptr(rs), L.dptr(ws), ws.numel(),
                                                                     L.cur_stream())), reps))
        xtrans.append(timed(lambda: L.check(lib.eld_calib_cell_stats(L.dptr(u), F, Hm, Wm, 6, L.dptr(xcs), L.dptr(xrs), L.dptr(xws),
                                                                      xws.numel(), L.cur_stream())), reps))
    tb, tx = float(np.median(bayer)), float(np.median(xtrans))
    ab = frames(4, Hm, Wm, 8).view(2, 2, Hm, Wm)
    out = torch.empty((2, 6, 6, 4), dtype=torch.int64, device='cuda')
    fws = torch.empty(lib.eld_calib_cell_flat_stats_workspace_bytes(2, Hm, 6), dtype=torch.uint8, device='cuda')
    tf = timed(lambda: L.check(lib.eld_calib_cell_flat_stats(L.dptr(ab), 2, Hm, Wm, 6, 16383, L.dptr(out), L.dptr(fws), fws.numel(),
                                                             L.cur_stream())), reps)
    byt = 2.0 * F * Hm * Wm
    res = {'mosaic': [F, Hm, Wm], 'bayer_bias_stats_ms': tb * 1e3, 'xtrans_cell_stats_ms': tx * 1e3, 'ratio': tx / tb,
           'bayer_GBps': byt / tb / 1e9, 'cell_stats_GBps': byt / tx / 1e9, 'cell_flat_stats_ms_2_pairs': tf * 1e3,
           'cell_flat_GBps': 2 * 2.0 * 2 * Hm * Wm / tf / 1e9}
    print(json.dumps(res))
    return res


BAYER_ENTRIES = ('eld_calib_bias_stats', 'eld_calib_bias_residual', 'eld_calib_flat_stats')


def bench_bayer2(F, Hm, Wm, P, reps, rounds=5, bayer=BAYER_ENTRIES):
    """--cfa bayer2: each pixel pass through its Bayer entry point and through the period-2 cell entry point on the same mosaics, `rounds`
    alternations of the median of `reps`.  Per pass: both medians, cell / bayer, and the spread (max / min) of the Bayer entry's own
    medians -- the margin inside which the two count as equal.  `bayer` names the three Bayer entries (a build that keeps other kernels
    under other names for an A/B passes them here; _lib's argument table must know them)."""
    lib = L.lib()
    f_stats, f_res, f_flat = (getattr(lib, n) for n in bayer)
    u = frames(F, Hm, Wm, 7)
    ab = frames(2 * P, Hm, Wm, 8).view(P, 2, Hm, Wm)
    pat = (ctypes.c_int * 4)(0, 1, 3, 2)
    blk4 = (ctypes.c_double * 4)(512.0, 511.0, 513.0, 510.0)
    blkc = (ctypes.c_double * 4)(512.0, 511.0, 510.0, 513.0)             # black_level[pattern[k]]
    i64 = lambda *shape: torch.empty(shape, dtype=torch.int64, device='cuda')   # noqa: E731
    cs, rs, fo = i64(F, 4, 2), i64(F, Hm, 2), i64(P, 4, 4)
    ws = torch.empty(lib.eld_calib_bias_stats_workspace_bytes(F, Hm), dtype=torch.uint8, device='cuda')
    fws = torch.empty(lib.eld_calib_flat_stats_workspace_bytes(P, Hm), dtype=torch.uint8, device='cuda')
    cb = torch.rand((F, 4), dtype=torch.float64, device='cuda')
    rho = torch.rand((F, Hm), dtype=torch.float64, device='cuda')
    t = torch.empty((F, Hm * Wm), dtype=torch.float32, device='cuda')
    st = L.cur_stream()
    calls = {
        'bias_stats': (lambda: L.check(f_stats(L.dptr(u), F, Hm, Wm, pat, L.dptr(cs), L.dptr(rs), L.dptr(ws), ws.numel(), st)),
                       lambda: L.check(lib.eld_calib_cell_stats(L.dptr(u), F, Hm, Wm, 2, L.dptr(cs), L.dptr(rs), L.dptr(ws), ws.numel(), st)),
                       2.0 * F * Hm * Wm),
        'residual': (lambda: L.check(f_res(L.dptr(u), F, Hm, Wm, pat, blk4, L.dptr(cb), L.dptr(rho), L.dptr(t), st)),
                     lambda: L.check(lib.eld_calib_cell_residual(L.dptr(u), F, Hm, Wm, 2, blkc, L.dptr(cb), L.dptr(rho), L.dptr(t), st)),
                     6.0 * F * Hm * Wm),
        'flat_stats': (lambda: L.check(f_flat(L.dptr(ab), P, Hm, Wm, pat, 16383, L.dptr(fo), L.dptr(fws), fws.numel(), st)),
                       lambda: L.check(lib.eld_calib_cell_flat_stats(L.dptr(ab), P, Hm, Wm, 2, 16383, L.dptr(fo), L.dptr(fws), fws.numel(), st)),
                       4.0 * P * Hm * Wm),
    }
    res = {'mosaic': [F, Hm, Wm], 'pairs': P, 'reps': reps, 'rounds': rounds, 'bayer_entries': list(bayer)}
    for name, (fa, fb, byt) in calls.items():
        fa(), fb()                                           # warm-up: code objects loaded
        ta, tb = [], []
        for _ in range(rounds):                              # interleaved A/B
            ta.append(timed(fa, reps))
            tb.append(timed(fb, reps))
        ma, mb = float(np.median(ta)), float(np.median(tb))
        res[name] = {'bayer_ms': ma * 1e3, 'cell2_ms': mb * 1e3, 'cell2_over_bayer': mb / ma, 'bayer_spread': max(ta) / min(ta),
                     'bayer_GBps': byt / ma / 1e9, 'cell2_GBps': byt / mb / 1e9,
                     'bayer_medians_ms': [1e3 * v for v in ta], 'cell2_medians_ms': [1e3 * v for v in tb]}
    print(json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cfa', choices=['bayer', 'xtrans', 'bayer2'], default='bayer',
                    help='xtrans: time the cell statistics (p = 6) against the Bayer bias statistics on 4 frames of 4158 x 6240; '
                         'bayer2: time each pass through its Bayer entry point against the period-2 cell entry point')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--isos', type=int, default=9)
    ap.add_argument('--out', help='also write the JSON result here')
    a = ap.parse_args()
    if a.cfa == 'xtrans':
        bench_cells(4, 4158, 6240, a.reps)
        return
    if a.cfa == 'bayer2':
        bench_bayer2(2, 2848, 4256, 8, a.reps)
        bench_bayer2(2, 5520, 8288, 2, a.reps)
        return
    L.load_library()
    lam = CAL.DEFAULT_LAMBDAS
    iso_rows = []
    for i in range(a.isos):
        bias = frames(2, 2848, 4256, 10 * i)
        flats = frames(16, 2848, 4256, 10 * i + 1).view(8, 2, 2848, 4256)
        r = bench_stack(bias, a.reps, lam)
        r.update(bench_flats(flats, a.reps))
        iso_rows.append(r)
        del bias, flats
    big = bench_stack(frames(2, 5520, 8288, 99), a.reps, lam)
    torch.cuda.synchronize()
    keys = ('bias_stats_s', 'residual_s', 'sort_s', 'ppcc_s', 'flat_stats_s')
    per_iso = {k: float(np.median([r[k] for r in iso_rows])) for k in keys}
    total = sum(sum(r[k] for k in keys) for r in iso_rows)
    res = {'isos': a.isos, 'per_iso_median_s': per_iso, 'session_total_s': total,
           'bias_stats_GBps': float(np.median([r['bias_stats_GBps'] for r in iso_rows])),
           'residual_GBps': float(np.median([r['residual_GBps'] for r in iso_rows])),
           'flat_stats_GBps': float(np.median([r['flat_stats_GBps'] for r in iso_rows])),
           'ppcc_elem_lambda_per_s': float(np.median([r['ppcc_elem_lambda_per_s'] for r in iso_rows])),
           'nikon_d850': big}
    res['frac_hbm'] = {k: res[k] * 1e9 / HBM_BPS for k in ('bias_stats_GBps', 'residual_GBps', 'flat_stats_GBps')}
    res['ppcc_valu_bound_elem_lambda_per_s'] = ppcc_bound(2848 * 4256, lam)
    res['ppcc_frac_valu'] = res['ppcc_elem_lambda_per_s'] / res['ppcc_valu_bound_elem_lambda_per_s']
    big['ppcc_valu_bound_elem_lambda_per_s'] = ppcc_bound(5520 * 8288, lam)
    big['ppcc_frac_valu'] = big['ppcc_elem_lambda_per_s'] / big['ppcc_valu_bound_elem_lambda_per_s']
    res['device'] = torch.cuda.get_device_name()
    res['library_src'] = L.build_src_hash()
    for r in iso_rows[:1] + [big]:
        print('%dx%dx%d: bias stats %.3f ms (%.0f GB/s)  residual %.3f ms (%.0f GB/s)  sort %.3f ms  ppcc %.3f ms (%.3g elem*lambda/s)'
              % (r['frames'], r['Hm'], r['Wm'], 1e3 * r['bias_stats_s'], r['bias_stats_GBps'], 1e3 * r['residual_s'], r['residual_GBps'],
                 1e3 * r['sort_s'], 1e3 * r['ppcc_s'], r['ppcc_elem_lambda_per_s']))
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
