"""GPU tests of the defective-pixel kernels (eld_amd/csrc/defect.hip) and their wiring (eld_amd/defects.py, calibrate, denoise, framepool):
the deviation, the bitmap and the repaired frames equal the NumPy restatement (tests/defects_ref.py) bit for bit; calibration over the
unflagged sites equals its CPU restatement and recovers the sampler's law where the unmasked run does not; denoise_raw and FramePool
with a map equal the same calls on repaired frames."""
import contextlib
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import defects_ref as R
from eld_amd import _lib as L
from eld_amd import calibrate as CAL
from eld_amd import defects as DF
from eld_amd.defects import DefectMap

from test_calib_cpu import PATTERNS, flat_sums_ref, ppcc_ref, sums_ref
from test_defects_cpu import XPAT, masked_bias_ref, masked_flat_ref, synthetic_bias_stack
from xtrans_ref import cell_flat_sums_ref, cell_sums_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def dev_u16(a):
    return _torch().from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def host_u16(t):
    return t.cpu().numpy().view(np.uint16)


def injected(rng, F, Hm, Wm, n=40):
    """A noisy dark stack with defects on every border and corner, a 2 x 2 cluster and n random sites (hot and dead)."""
    u = np.clip(np.round(rng.normal(512, 5, (F, Hm, Wm))), 0, 65535).astype(np.uint16)
    idx = rng.choice(Hm * Wm, n, replace=False)
    sites = [(0, 0), (0, Wm - 1), (Hm - 1, 0), (Hm - 1, Wm - 1), (0, Wm // 2), (Hm - 1, Wm // 2 + 1), (Hm // 2, 0), (Hm // 2 + 1, Wm - 1),
             (3, 3), (3, 4), (4, 3), (4, 4)] + [(int(i // Wm), int(i % Wm)) for i in idx]
    for k, (y, x) in enumerate(sites):
        u[:, y, x] = 0 if k % 3 == 2 else 3000 + 17 * k
    return u


CASES = [('bayer', p, s) for p in PATTERNS for s in ((34, 50), (66, 130))] + \
        [('bayer', PATTERNS[0], s) for s in ((2, 2), (4, 6), (130, 62), (40, 258))] + \
        [('xtrans', XPAT, s) for s in ((6, 6), (13, 20), (38, 70), (67, 130), (45, 262))]


@pytest.mark.parametrize('F', [1, 2, 8])
@pytest.mark.parametrize('cfa,pat,shape', CASES)
def test_deviation_bitmap_and_repair_equal_the_restatement(eld_lib, cfa, pat, shape, F):
    torch = _torch()
    Hm, Wm = shape
    rng = np.random.default_rng(1000 * Hm + Wm + F)
    u = injected(rng, F, Hm, Wm, n=min(40, Hm * Wm // 8)) if Hm * Wm >= 36 else rng.integers(0, 65536, (F, Hm, Wm)).astype(np.uint16)
    cls = R.class_map(Hm, Wm, cfa, pat)
    rad = 2 if cfa == 'bayer' else DF.xtrans_tables()['R']
    Dref = R.deviation(u, cls, rad)
    D = DF.deviation(u, cfa, pat)
    assert D.dtype == torch.int32 and np.array_equal(D.cpu().numpy().astype(np.int64), Dref)
    assert np.array_equal(DF.deviation(dev_u16(u), cfa, pat).cpu().numpy(), D.cpu().numpy())          # a CUDA view in, the same bits
    T_hi, T_lo = 200 * F, 150 * F
    mask = R.flags(Dref, T_hi, T_lo)
    pitch = (Wm + 31) // 32
    guard = torch.full((Hm * pitch + 2,), -1, dtype=torch.int32, device='cuda')                       # the words around the bitmap stay untouched
    bm = guard[1:1 + Hm * pitch].view(Hm, pitch)
    L.check(L.lib().eld_defect_flags(L.dptr(D), Hm, Wm, T_hi, T_lo, L.dptr(bm), L.cur_stream()))
    words = bm.cpu().numpy().view(np.uint32)
    assert np.array_equal(words, R.pack_bitmap(mask))                                                 # pad bits zero included
    assert int(guard[0]) == -1 and int(guard[-1]) == -1
    if len(DF.stranded_sites(mask, np.asarray(DF._class_pattern(cfa, pat)[1]), rad)):
        # Only frames too small to leave an unflagged neighbour take this exit, after the D and bitmap checks: Bayer (4, 6) (random codes
        # over the whole range: nearly every site is flagged) and X-Trans (6, 6) (12 injected defects among 36 sites).  Bayer (2, 2) has no
        # neighbours at all, so D = 0, nothing is flagged and it runs on.  The assert keeps any larger case from leaving here.
        assert Hm * Wm <= 36, shape
        return
    dm, diag = DF.find_defects(u, cfa, pat, thresholds=(T_hi, T_lo))
    assert np.array_equal(dm.words, words) and dm.count == int(mask.sum()) and diag['hot'] == int((Dref > T_hi).sum())
    assert np.array_equal(dm.sites, np.argwhere(mask))
    frames = np.concatenate([u, rng.integers(0, 65536, (2, Hm, Wm)).astype(np.uint16)])               # N > 1, the whole code range
    want = R.repair(frames, mask, cls, rad)
    got = DF.repair(frames, dm)
    assert got.dtype == np.uint16 and np.array_equal(got, want)
    assert np.array_equal(got[:, ~mask], frames[:, ~mask])                                            # unflagged sites are unchanged
    t = dev_u16(frames)
    out = DF.repair(t, dm)
    assert np.array_equal(host_u16(out), want) and np.array_equal(host_u16(t), frames)
    assert DF.repair(t, dm, out=t) is t and np.array_equal(host_u16(t), want)                         # in place: the same bits
    assert np.array_equal(DF.repair(frames[0], dm), want[0])
    empty = DefectMap.from_sites([], (Hm, Wm), cfa, pat)
    assert np.array_equal(DF.repair(frames, empty), frames)                                           # an empty map is the identity


@pytest.mark.parametrize('cfa,pat', [('bayer', PATTERNS[1]), ('xtrans', XPAT)])
def test_repair_from_odd_row_starts_and_every_alignment(eld_lib, cfa, pat):
    """Rows that start 2, 4, ... bytes off a 16-byte boundary (views into a larger buffer) and widths that are not multiples of 8 take
    the 4-byte and 2-byte forms: the same bits."""
    torch = _torch()
    rng = np.random.default_rng(9)
    rad = 2 if cfa == 'bayer' else 3
    for Hm, Wm in ((12, 22), (14, 36), (12, 70)):
        cls = R.class_map(Hm, Wm, cfa, pat)
        u = rng.integers(0, 65536, (2, Hm, Wm)).astype(np.uint16)
        dm = DefectMap.from_sites([[0, 0], [5, 7], [5, 9], [Hm - 1, Wm - 1], [6, Wm - 2]], (Hm, Wm), cfa, pat)
        want = R.repair(u, dm.mask, cls, rad)
        for off in (0, 1, 2, 3, 5):
            base = torch.zeros(2 * Hm * Wm + 16, dtype=torch.int16, device='cuda')
            view = base[off:off + 2 * Hm * Wm].view(2, Hm, Wm)
            view.copy_(dev_u16(u))
            assert np.array_equal(host_u16(DF.repair(view, dm)), want)
            DF.repair(view, dm, out=view)
            assert np.array_equal(host_u16(view), want)


def test_xtrans_tap_tables_equal_the_brute_force_scan(eld_lib):
    t = DF.xtrans_tables()
    rad = t['R']
    cls = R.class_map(30, 30, 'xtrans', XPAT)
    assert np.array_equal(t['colour'], cls[:6, :6])
    for py in range(6):
        for px in range(6):
            want = 0
            for yy, xx in R.neighbours(cls, 12 + py, 12 + px, rad):
                want |= 1 << ((yy - 12 - py + rad) * (2 * rad + 1) + xx - 12 - px + rad)
            assert int(t['mask'][py, px]) == want and int(t['count'][py, px]) == bin(want).count('1')


def test_find_defects_default_thresholds_on_the_synthetic_stack(eld_lib):
    """The device path equals the restatement that tests/test_defects_cpu.py scored (every injected site above the margin found)."""
    for cfa, pat, rad in (('bayer', [[0, 1], [3, 2]], 2), ('xtrans', XPAT, 3)):
        u, hot, amp, dead = synthetic_bias_stack(cfa)
        Hm, Wm = u.shape[1:]
        D = R.deviation(u, R.class_map(Hm, Wm, cfa, pat), rad)
        sigma = 1.4826 * float(np.sort(np.abs(D).reshape(-1))[(D.size - 1) // 2])
        T = max(int(np.ceil(8.0 * sigma)), 4 * 16)
        dm, diag = DF.find_defects(u, cfa, pat)
        assert diag['T_hi'] == diag['T_lo'] == T and abs(diag['sigma'] - sigma) < 1e-9
        assert np.array_equal(dm.mask, R.flags(D, T, T)) and diag['D_max'] == D.max() and diag['D_min'] == D.min()


# ---- calibration -------------------------------------------------------------------------------------------------------------------------
def _inject(rng, frames, sites, n_hot):
    """hot: +500 DN in every frame; the rest dead (0)."""
    out = np.array(frames, copy=True)
    ys, xs = sites[:, 0], sites[:, 1]
    out[..., ys[:n_hot], xs[:n_hot]] = np.clip(out[..., ys[:n_hot], xs[:n_hot]].astype(np.int64) + 500, 0, 65535).astype(np.uint16)
    out[..., ys[n_hot:], xs[n_hot:]] = 0
    return out


def _sites(rng, Hm, Wm, n):
    idx = rng.choice(Hm * Wm, n, replace=False)
    return np.stack([idx // Wm, idx % Wm], axis=1)


def test_bayer_calibration_over_the_unflagged_sites(eld_lib, tmp_path):
    """256 x 384 sessions from the sampler with 0.1 % defective sites: with the map the pipeline equals the CPU restatement over the
    unflagged pixels (exact sums, bit-equal residual, test_calib_gpu's PPCC bounds) and K comes back to 1 %; 'auto' finds the sites."""
    from test_calib_gpu import SAMPLER_PATTERN, make_sessions
    pattern, black, white = SAMPLER_PATTERN, [512.0] * 4, 16383
    rng = np.random.default_rng(4)
    sessions = make_sessions()
    Hm, Wm = sessions[0]['bias'].shape[1:]
    sites = _sites(rng, Hm, Wm, 98)
    for s in sessions:
        s['bias'], s['flats'] = _inject(rng, s['bias'], sites, 70), _inject(rng, s['flats'], sites, 70)
    dm = DefectMap.from_sites(sites, (Hm, Wm), 'bayer', pattern)
    keep = ~dm.mask
    ch = R.class_map(Hm, Wm, 'bayer', pattern)
    blk = np.asarray(black)[ch]
    clean = [{k: s[k] for k in ('iso', 'bias', 'flats')} for s in sessions]
    params, diag = CAL.calibrate_camera(clean, pattern, black, white, defects=dm)
    assert diag['defects'] is dm
    i = 0
    for s, K in zip(sessions, diag['K']):
        st = CAL.bias_frame_stats(s['bias'], pattern, black, residual=True, defects=dm)
        cs, rs = sums_ref(np.where(keep, s['bias'], 0), pattern)
        assert np.array_equal(st['chan_sums'], cs) and np.array_equal(st['row_sums'], rs)
        fl = CAL.flat_pair_stats(s['flats'], pattern, black, white, st['color_bias'].mean(axis=0), defects=dm)
        assert np.array_equal(fl['sums'], flat_sums_ref(np.where(keep, s['flats'], 0), pattern, white))
        t = st['t'].cpu().numpy()
        assert t.shape == (s['bias'].shape[0], Hm * Wm - dm.count)
        for f, u in enumerate(s['bias']):
            cb, rho, g, Rs, t32 = masked_bias_ref(u, ch, blk, keep)
            fr = diag['frames'][i]
            i += 1
            assert np.max(np.abs(fr['color_bias'] - cb)) <= 1e-9 and abs(fr['g_scale'] - g) <= 1e-9 and abs(fr['R_scale'] - Rs) <= 1e-9
            assert np.array_equal(t[f], t32)                                                    # bit-equal residual, flagged entries dropped
            r, slope = ppcc_ref(t32, CAL.DEFAULT_LAMBDAS)
            k = int(np.argmax(r))
            assert fr['lambda'] == CAL.DEFAULT_LAMBDAS[k] and abs(fr['G_scale'] - slope[k]) <= 1e-5 * slope[k]
        cbm = st['color_bias'].mean(axis=0)
        for p, pair in enumerate(s['flats']):
            mu, var, ok = masked_flat_ref(pair[0], pair[1], ch, blk, white, cbm, keep)
            np.testing.assert_allclose(fl['mu'][p], mu, rtol=0, atol=1e-9)
            np.testing.assert_allclose(fl['var'][p], var, rtol=1e-12)
            assert np.array_equal(fl['usable'][p], ok)
        assert abs(K / s['K'] - 1) < 0.01, (K, s['K'])
    # 'auto': the injected sites are found (500 DN and -512 DN per frame against a threshold of 16 DN per frame or 8 sigma)
    _, dauto = CAL.calibrate_camera(clean, pattern, black, white, defects='auto')
    found = dauto['defects'].mask
    assert found[sites[:, 0], sites[:, 1]].all() and int(found.sum()) <= len(sites) + 5
    # the command line writes the map beside the table
    man = {'raw_pattern': pattern, 'black_level': [512] * 4, 'white_level': white, 'defects': 'auto', 'sessions': []}
    for j, s in enumerate(sessions):
        e = {'iso': s['iso'], 'bias': [], 'flats': []}
        for q, u in enumerate(s['bias']):
            np.save(tmp_path / ('b%d_%d.npy' % (j, q)), u)
            e['bias'].append('b%d_%d.npy' % (j, q))
        for q, pr in enumerate(s['flats']):
            np.save(tmp_path / ('f%d_%da.npy' % (j, q)), pr[0])
            np.save(tmp_path / ('f%d_%db.npy' % (j, q)), pr[1])
            e['flats'].append(['f%d_%da.npy' % (j, q), 'f%d_%db.npy' % (j, q)])
        man['sessions'].append(e)
    (tmp_path / 'm.json').write_text(json.dumps(man))
    with contextlib.redirect_stdout(io.StringIO()):
        assert CAL.main([str(tmp_path / 'm.json'), '--camera', 'Cam', '--out', str(tmp_path / 'out')]) == 0
    assert np.array_equal(DefectMap.load(str(tmp_path / 'out' / 'Cam_defects.npz')).mask, found)


def test_bayer_closed_loop_with_the_map_and_negative_control_without(eld_lib):
    """Four Sony-size bias frames from the sampler (tl_scale 6, lambda 0, row 0.5 DN: var(e) = 36 * pi^2 / 3 + 0.25 + 1/12 = 118.8 DN^2)
    with 1 site in 10^4 hot by 500 DN and as many dead (-512 DN): unmasked they add 1e-4 * (500^2 + 512^2) = 51 DN^2, so g_scale comes
    out sqrt(170 / 118.8) = 1.20 times too large -- the negative control.  With the map the existing closed-loop bounds hold: lambda
    to one grid step, G_scale 3 %, R_scale 5 %, colour bias 0.05 DN, and g_scale within 3 % of the clean frames'."""
    from test_calib_gpu import SAMPLER_PATTERN, STEP, _bias_params, synth_mosaics
    torch = _torch()
    rng = np.random.default_rng(8)
    lam, tl_scale, row_scale, cb, F = 0.0, 6.0, 0.5, (1.5, -1.0, 0.75, 0.25), 4
    u = synth_mosaics(_bias_params(lam, tl_scale, row_scale, cb, F), L.READ_TL | L.ROW | L.CBIAS, [7000 + i for i in range(F)], 1424, 2128)
    Hm, Wm = 2848, 4256
    g_clean = CAL.bias_frame_stats(u, SAMPLER_PATTERN, [512.0] * 4)['g_scale']
    sites = _sites(rng, Hm, Wm, 2 * (Hm * Wm // 10000))
    ys, xs = torch.from_numpy(sites[:, 0]).cuda(), torch.from_numpy(sites[:, 1]).cuda()
    h = len(sites) // 2
    v = u.view(torch.int16)
    v[:, ys[:h], xs[:h]] = v[:, ys[:h], xs[:h]] + 500          # codes near 512: no wrap
    v[:, ys[h:], xs[h:]] = 0
    dm = DefectMap.from_sites(sites, (Hm, Wm), 'bayer', SAMPLER_PATTERN)
    st = CAL.bias_frame_stats(u, SAMPLER_PATTERN, [512.0] * 4, residual=True, defects=dm)
    pp = CAL.tukey_lambda_ppcc(st.pop('t'))
    assert np.all(np.abs(pp['lam_hat'] - lam) <= STEP + 1e-12), pp['lam_hat']
    assert abs(np.mean(pp['scale']) / tl_scale - 1) < 0.03, pp['scale']
    assert abs(np.mean(st['R_scale']) / row_scale - 1) < 0.05, st['R_scale']
    assert np.max(np.abs(st['color_bias'].mean(axis=0) - np.asarray(cb))) < 0.05, st['color_bias']
    assert np.all(np.abs(st['g_scale'] / g_clean - 1) < 0.03), (st['g_scale'], g_clean)
    bad = CAL.bias_frame_stats(u, SAMPLER_PATTERN, [512.0] * 4)
    print('g_scale clean', g_clean, 'masked', st['g_scale'], 'unmasked', bad['g_scale'])
    assert np.all(bad['g_scale'] / g_clean - 1 > 0.03), (bad['g_scale'], g_clean)                     # the negative control
    dauto, _ = DF.find_defects(u, 'bayer', SAMPLER_PATTERN)
    assert dauto.mask[sites[:, 0], sites[:, 1]].all()
    del u, v
    torch.cuda.empty_cache()


def test_xtrans_calibration_statistics_over_the_unflagged_sites(eld_lib):
    """X-Trans: with the map the device sums equal the exact sums over the unflagged pixels, the residual is bit-equal with the flagged
    entries dropped, and the statistics equal the float64 evaluation; without it g_scale is off by the injected 1e-3 * 500^2."""
    rng = np.random.default_rng(12)
    F, Hm, Wm, white = 2, 134, 200, 16383
    black = np.array([512.0, 510.0, 514.0, 510.0])
    u0 = np.clip(np.round(rng.normal(512, 3, (F, Hm, Wm)) + rng.normal(0, 1, (F, Hm, 1))), 0, 65535).astype(np.uint16)
    ab0 = np.clip(np.round(rng.normal(3000, 40, (3, 2, Hm, Wm))), 0, 65535).astype(np.uint16)
    sites = _sites(rng, Hm, Wm, 27)
    u, ab = _inject(rng, u0, sites, 20), _inject(rng, ab0, sites, 20)
    ab[:, :, sites[0, 0], sites[0, 1]] = white                          # a saturated defective site must not spoil its colour
    dm = DefectMap.from_sites(sites, (Hm, Wm), 'xtrans', XPAT)
    keep = ~dm.mask
    col = R.class_map(Hm, Wm, 'xtrans', XPAT)
    blackmap = black[XPAT[np.arange(Hm)[:, None] % 6, np.arange(Wm)[None, :] % 6]]
    st = CAL.xtrans_bias_frame_stats(u, XPAT, black, residual=True, defects=dm)
    cs, rs = cell_sums_ref(np.where(keep, u, 0), 6)
    assert np.array_equal(st['cell_sums'], cs) and np.array_equal(st['row_sums'], rs)
    t = st['t'].cpu().numpy()
    for f in range(F):
        cb, rho, g, Rs, t32 = masked_bias_ref(u[f], col, blackmap, keep)
        np.testing.assert_allclose(st['color_bias'][f], cb, rtol=0, atol=1e-9)
        np.testing.assert_allclose(st['row_offset'][f], rho, rtol=0, atol=1e-9)
        assert abs(st['g_scale'][f] - g) <= 1e-9 and abs(st['R_scale'][f] - Rs) <= 1e-9 and np.array_equal(t[f], t32)
    cbm = st['color_bias'].mean(axis=0)
    fl = CAL.xtrans_flat_pair_stats(ab, XPAT, black, white, cbm, defects=dm)
    assert np.array_equal(fl['sums'], cell_flat_sums_ref(np.where(keep, ab, 0), 6, white))
    for p in range(3):
        mu, var, ok = masked_flat_ref(ab[p, 0], ab[p, 1], col, blackmap, white, cbm, keep)
        np.testing.assert_allclose(fl['mu'][p], mu, rtol=0, atol=1e-9)
        np.testing.assert_allclose(fl['var'][p], var, rtol=1e-12)
        assert np.array_equal(fl['usable'][p], ok) and ok.all()
    g_clean = CAL.xtrans_bias_frame_stats(u0, XPAT, black)['g_scale']
    assert np.all(np.abs(st['g_scale'] / g_clean - 1) < 0.03)
    assert np.all(CAL.xtrans_bias_frame_stats(u, XPAT, black)['g_scale'] / g_clean - 1 > 0.03)        # negative control: 1e-3 * 500^2 = 250 DN^2 on 10
    assert not CAL.xtrans_flat_pair_stats(ab, XPAT, black, white, cbm)['usable'].all()
    dauto, _ = DF.find_defects(u, 'xtrans', XPAT)
    assert dauto.mask[sites[:, 0], sites[:, 1]].all()


def test_xtrans_closed_loop_with_the_map_and_negative_control_without(eld_lib):
    """The X-Trans twin of the Bayer closed loop, on test_xtrans_calib_gpu's set-up: four 4158 x 6240 frames from the sampler (tl_scale 6,
    lambda -0.2: var(TL) = 7.49, so var(e) = 36 * 7.49 + 0.25 + 1/12 = 270 DN^2), 1 site in 10^4 hot by 500 DN and as many dead (-512 DN).
    Unmasked they add 1e-4 * (500^2 + 512^2) = 51 DN^2: g_scale comes out sqrt(321 / 270) = 1.09 times too large, outside its 3 % -- the
    negative control.  With the map that file's closed-loop bounds hold: lambda to one grid step, G_scale 3 %, R_scale 5 %, colour bias
    0.05 DN, and g_scale within 3 % of the clean frames'."""
    from test_xtrans_calib_gpu import STEP, _bias_params, synth_xtrans
    torch = _torch()
    rng = np.random.default_rng(18)
    lam = float(CAL.DEFAULT_LAMBDAS[70 - 14])
    tl_scale, row_scale, cb, F = 6.0, 0.5, (1.5, -1.0, 0.75), 4
    u = synth_xtrans(_bias_params(lam, tl_scale, row_scale, cb, F), L.READ_TL | L.ROW | L.CBIAS, [8000 + i for i in range(F)], 1386, 2080)
    Hm, Wm = 4158, 6240
    assert tuple(u.shape) == (F, Hm, Wm)
    black = [512.0] * 4
    g_clean = CAL.xtrans_bias_frame_stats(u, XPAT, black)['g_scale']
    sites = _sites(rng, Hm, Wm, 2 * (Hm * Wm // 10000))
    ys, xs = torch.from_numpy(sites[:, 0]).cuda(), torch.from_numpy(sites[:, 1]).cuda()
    h = len(sites) // 2
    u[:, ys[:h], xs[:h]] = u[:, ys[:h], xs[:h]] + 500          # codes near 512: no wrap of the int16 view
    u[:, ys[h:], xs[h:]] = 0
    dm = DefectMap.from_sites(sites, (Hm, Wm), 'xtrans', XPAT)
    st = CAL.xtrans_bias_frame_stats(u, XPAT, black, residual=True, defects=dm)
    assert tuple(st['t'].shape) == (F, Hm * Wm - dm.count)
    pp = CAL.tukey_lambda_ppcc(st.pop('t'))
    assert np.all(np.abs(pp['lam_hat'] - lam) <= STEP + 1e-12), pp['lam_hat']
    assert abs(np.mean(pp['scale']) / tl_scale - 1) < 0.03, pp['scale']
    assert abs(np.mean(st['R_scale']) / row_scale - 1) < 0.05, st['R_scale']
    assert np.max(np.abs(st['color_bias'].mean(axis=0) - np.asarray(cb))) < 0.05, st['color_bias']
    assert np.all(np.abs(st['g_scale'] / g_clean - 1) < 0.03), (st['g_scale'], g_clean)
    bad = CAL.xtrans_bias_frame_stats(u, XPAT, black)
    print('xtrans g_scale clean', g_clean, 'masked', st['g_scale'], 'unmasked', bad['g_scale'])
    assert np.all(bad['g_scale'] / g_clean - 1 > 0.03), (bad['g_scale'], g_clean)                     # the negative control
    dauto, _ = DF.find_defects(u, 'xtrans', XPAT)
    assert dauto.mask[sites[:, 0], sites[:, 1]].all()
    del u
    torch.cuda.empty_cache()


def test_xtrans_sessions_through_calibrate_camera_with_a_map_and_auto(eld_lib, tmp_path):
    """Five 575 x 862 X-Trans sessions from the sampler (sides that are not multiples of 6) with 0.1 % defective sites in the bias and flat
    frames.  calibrate_camera(cfa='xtrans', defects=map) equals the CPU restatement over the unflagged pixels by test_calib_gpu's
    pipeline-versus-restatement criteria (statistics to 1e-9, a bit-equal residual, the lambda of ppcc_ref's arg-max, G_scale to 1e-5),
    K comes back to 1 % (18 photon-transfer points of 110 k (R, B) / 275 k (G) unflagged pixels: SE of the slope about 0.2 %), the
    colour bias within 6 SE as test_xtrans_calib_gpu bounds it at this size, and the unmasked g_scale misses by more than 3 %; 'auto'
    finds the injected sites and the command line writes the map."""
    from test_xtrans_calib_gpu import make_xtrans_sessions
    pattern, black, white = XPAT, [512.0] * 4, 16383
    rng = np.random.default_rng(14)
    sessions = make_xtrans_sessions(h=192, w=288, F=2, P=6, seed=2)
    Hm, Wm = sessions[0]['bias'].shape[1:]
    assert (Hm, Wm) == (575, 862)
    sites = _sites(rng, Hm, Wm, Hm * Wm // 1000)
    n_hot = 2 * len(sites) // 3
    for s in sessions:
        s['bias'], s['flats'] = _inject(rng, s['bias'], sites, n_hot), _inject(rng, s['flats'], sites, n_hot)
    dm = DefectMap.from_sites(sites, (Hm, Wm), 'xtrans', pattern)
    keep = ~dm.mask
    col = R.class_map(Hm, Wm, 'xtrans', pattern)
    blackmap = np.asarray(black)[np.asarray(pattern)[np.arange(Hm)[:, None] % 6, np.arange(Wm)[None, :] % 6]]
    given = [{k: s[k] for k in ('iso', 'bias', 'flats')} for s in sessions]
    params, diag = CAL.calibrate_camera(given, pattern, black, white, cfa='xtrans', defects=dm)
    assert diag['defects'] is dm and params['cfa'] == 'xtrans' and params['color_bias'].shape == (10, 3)
    i = 0
    for j, s in enumerate(sessions):
        st = CAL.xtrans_bias_frame_stats(s['bias'], pattern, black, residual=True, defects=dm)
        cs, rs = cell_sums_ref(np.where(keep, s['bias'], 0), 6)
        assert np.array_equal(st['cell_sums'], cs) and np.array_equal(st['row_sums'], rs)
        t = st['t'].cpu().numpy()
        cbs = []
        for f, u in enumerate(s['bias']):
            cb, rho, g, Rs, t32 = masked_bias_ref(u, col, blackmap, keep)
            cbs.append(cb)
            fr = diag['frames'][i]
            i += 1
            assert fr['session'] == j
            assert np.max(np.abs(fr['color_bias'] - cb)) <= 1e-9 and abs(fr['g_scale'] - g) <= 1e-9 and abs(fr['R_scale'] - Rs) <= 1e-9
            assert np.array_equal(t[f], t32)
            r, slope = ppcc_ref(t32, CAL.DEFAULT_LAMBDAS)
            k = int(np.argmax(r))
            assert fr['lambda'] == CAL.DEFAULT_LAMBDAS[k] and abs(fr['G_scale'] - slope[k]) <= 1e-5 * slope[k]
            se = np.sqrt(s['R'] ** 2 / Hm + (2.0 * s['G']) ** 2 / (Hm * Wm * 8 / 36))
            assert np.max(np.abs(fr['color_bias'] - np.asarray(s['cb']))) < 6 * se, (fr['color_bias'], s['cb'], se)
        cbm = np.mean(cbs, axis=0)
        pts = [masked_flat_ref(p[0], p[1], col, blackmap, white, cbm, keep) for p in s['flats']]
        assert all(p[2].all() for p in pts)
        K_ref = np.polyfit(np.concatenate([p[0] for p in pts]), np.concatenate([p[1] for p in pts]), 1)[0]
        assert abs(diag['K'][j] - K_ref) <= 1e-9 * K_ref
        assert abs(diag['K'][j] / s['K'] - 1) < 0.01, (diag['K'][j], s['K'])
        masked_g = np.array([fr['g_scale'] for fr in diag['frames'] if fr['session'] == j])
        unmasked_g = CAL.xtrans_bias_frame_stats(s['bias'], pattern, black)['g_scale']
        assert np.all(unmasked_g / masked_g - 1 > 0.03), (unmasked_g, masked_g)                      # 1e-3 * (2/3 * 500^2 + 1/3 * 512^2) = 254 DN^2 more
    _, dauto = CAL.calibrate_camera(given, pattern, black, white, cfa='xtrans', defects='auto')
    found = dauto['defects'].mask
    assert dauto['defects'].cfa == 'xtrans' and found[sites[:, 0], sites[:, 1]].all() and int(found.sum()) <= len(sites) + 5
    man = {'cfa': 'xtrans', 'raw_pattern': np.asarray(pattern).tolist(), 'black_level': [512] * 4, 'white_level': white, 'defects': 'auto',
           'sessions': []}
    for j, s in enumerate(sessions):
        e = {'iso': s['iso'], 'bias': [], 'flats': []}
        for q, u in enumerate(s['bias']):
            np.save(tmp_path / ('b%d_%d.npy' % (j, q)), u)
            e['bias'].append('b%d_%d.npy' % (j, q))
        for q, pr in enumerate(s['flats']):
            np.save(tmp_path / ('f%d_%da.npy' % (j, q)), pr[0])
            np.save(tmp_path / ('f%d_%db.npy' % (j, q)), pr[1])
            e['flats'].append(['f%d_%da.npy' % (j, q), 'f%d_%db.npy' % (j, q)])
        man['sessions'].append(e)
    (tmp_path / 'm.json').write_text(json.dumps(man))
    with contextlib.redirect_stdout(io.StringIO()):
        assert CAL.main([str(tmp_path / 'm.json'), '--camera', 'Fuji', '--out', str(tmp_path / 'out')]) == 0
    assert np.array_equal(DefectMap.load(str(tmp_path / 'out' / 'Fuji_defects.npz')).mask, found)
    with pytest.raises(ValueError, match='not the 6x6 cell'):                                          # another phase: documented, refused on the host
        CAL.calibrate_camera(given, np.roll(np.asarray(pattern), 1, axis=1), black, white, cfa='xtrans', defects='auto')
    with pytest.raises(ValueError, match='another X-Trans raw_pattern'):
        CAL.calibrate_camera(given, np.roll(np.asarray(pattern), 1, axis=1), black, white, cfa='xtrans', defects=dm)


# ---- denoise and the frame pool ---------------------------------------------------------------------------------------------------------
def _denoiser(cfa, precision):
    from eld_amd.denoise import load_denoiser
    from eld_amd.unet import UNetSeeInDark
    torch = _torch()
    torch.manual_seed(5)
    ch = 4 if cfa == 'bayer' else 9
    return load_denoiser(UNetSeeInDark(ch, ch), cfa=cfa, precision=precision)


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('cfa,shape', [('bayer', (64, 96)), ('xtrans', (52, 98))])
def test_denoise_with_a_map_equals_denoise_of_the_repaired_frame(eld_lib, tmp_path, cfa, shape, precision):
    from eld_amd.denoise import denoise_raw
    rng = np.random.default_rng(3)
    Hm, Wm = shape
    x = np.clip(np.round(rng.normal(560, 12, (2, Hm, Wm))), 0, 16383).astype(np.uint16)
    sites = np.concatenate([_sites(rng, Hm, Wm, 12), [[0, 0], [Hm - 1, Wm - 1], [Hm - 2, Wm - 3]]])     # X-Trans: the last rows / columns lie outside whole cells
    sites = np.unique(sites, axis=0)
    x[:, sites[:, 0], sites[:, 1]] = 9000
    m = DefectMap.from_sites(sites, (Hm, Wm), cfa)
    den = _denoiser(cfa, precision)
    kw = dict(black_level=512, ratio=100.0, wb=[2.0, 1.0, 1.5], ccm=np.eye(3))
    a = denoise_raw(den, x, cfa, defects=m, **kw)
    b = denoise_raw(den, DF.repair(x, m), cfa, **kw)
    for k in ('packed', 'mosaic', 'srgb'):
        assert np.array_equal(a[k], b[k]), k
    c = denoise_raw(den, x, cfa, defects=m.save(str(tmp_path / 'm.npz')), **kw)                        # a saved map by path
    assert np.array_equal(c['mosaic'], a['mosaic'])
    n0, n1 = denoise_raw(den, x, cfa, defects=None, **kw), denoise_raw(den, x, cfa, **kw)
    for k in ('packed', 'mosaic', 'srgb'):
        assert np.array_equal(n0[k], n1[k]), k
    assert not np.array_equal(n0['packed'], a['packed'])
    t = dev_u16(x)
    d = denoise_raw(den, t, cfa, defects=m, **kw)
    assert np.array_equal(host_u16(d['mosaic']), a['mosaic']) and np.array_equal(host_u16(t), x)      # the caller's tensor is not modified


@pytest.mark.parametrize('cfa', ['bayer', 'xtrans'])
def test_frame_pool_with_a_map_equals_a_pool_of_repaired_frames(eld_lib, cfa):
    from eld_amd.framepool import FramePool
    rng = np.random.default_rng(6)
    Hm, Wm = (160, 200) if cfa == 'bayer' else (156, 204)
    frames = [np.clip(np.round(rng.normal(900, 60, (Hm, Wm))), 0, 16383).astype(np.uint16) for _ in range(3)]
    sites = _sites(rng, Hm, Wm, 30)
    for f in frames:
        f[sites[:, 0], sites[:, 1]] = 12000
    m = DefectMap.from_sites(sites, (Hm, Wm), cfa)
    a = FramePool(frames, cfa=cfa, black_level=512, defects=m)
    b = FramePool([DF.repair(f, m) for f in frames], cfa=cfa, black_level=512)
    plain = FramePool(frames, cfa=cfa, black_level=512)
    assert np.array_equal(a.buffer.cpu().numpy(), b.buffer.cpu().numpy()) and not np.array_equal(a.buffer.cpu().numpy(), plain.buffer.cpu().numpy())
    C = a.C
    crops = a.grid((C, 32, 32), (C, 16, 16))
    assert np.array_equal(a.patches(crops, ratios=3.0).cpu().numpy(), b.patches(crops, ratios=3.0).cpu().numpy())


def test_one_training_step_is_bit_identical(eld_lib, tmp_path):
    from eld_amd.engine import Engine
    from eld_amd.framepool import FramePool, FramePoolLoader
    from test_framepool_gpu import make_opt, noise_model, train_losses
    torch = _torch()
    rng = np.random.default_rng(7)
    frames = [np.clip(np.round(rng.normal(900, 60, (200, 264))), 0, 16383).astype(np.uint16) for _ in range(2)]
    sites = _sites(rng, 200, 264, 40)
    for f in frames:
        f[sites[:, 0], sites[:, 1]] = 15000
    m = DefectMap.from_sites(sites, (200, 264))
    nm = noise_model()
    runs = []
    for pool in (FramePool(frames, raw_pattern=PATTERNS[0], black_level=512, defects=m),
                 FramePool([DF.repair(f, m) for f in frames], raw_pattern=PATTERNS[0], black_level=512)):
        loader = FramePoolLoader(pool, nm, 2, patch=64, steps_per_epoch=1)
        np.random.seed(11)
        batch = loader.batch(*loader.draw())
        torch.manual_seed(2018)
        with contextlib.redirect_stdout(io.StringIO()):
            engine = Engine(make_opt(tmp_path))
        engine.model.set_noise_model(nm)
        loss = train_losses(engine, [batch])
        runs.append((np.float64(loss[0]).tobytes(), engine.model.output.cpu().numpy().tobytes()))
    assert runs[0] == runs[1]


# ---- command lines, each a fresh child process ----------------------------------------------------------------------------------------------
def _run(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m'] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (args, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


def test_command_line_chain(eld_lib, tmp_path):
    """python -m eld_amd.defects -> calibrate --defects -> train_frames --defects -> denoise --defects on small frames."""
    from test_calib_gpu import SAMPLER_PATTERN, make_sessions
    rng = np.random.default_rng(2)
    sessions = make_sessions(h=64, w=96, F=2, P=4, seed=1)
    Hm, Wm = sessions[0]['bias'].shape[1:]
    sites = _sites(rng, Hm, Wm, 20)
    man = {'raw_pattern': SAMPLER_PATTERN, 'black_level': [512] * 4, 'white_level': 16383, 'sessions': []}
    for j, s in enumerate(sessions):
        bias, flats = _inject(rng, s['bias'], sites, 14), _inject(rng, s['flats'], sites, 14)
        e = {'iso': s['iso'], 'bias': [], 'flats': []}
        for q, u in enumerate(bias):
            np.save(tmp_path / ('b%d_%d.npy' % (j, q)), u)
            e['bias'].append('b%d_%d.npy' % (j, q))
        for q, pr in enumerate(flats):
            np.save(tmp_path / ('f%d_%da.npy' % (j, q)), pr[0])
            np.save(tmp_path / ('f%d_%db.npy' % (j, q)), pr[1])
            e['flats'].append(['f%d_%da.npy' % (j, q), 'f%d_%db.npy' % (j, q)])
        man['sessions'].append(e)
    (tmp_path / 'm.json').write_text(json.dumps(man))
    (tmp_path / 'sensor.json').write_text(json.dumps({'cfa': 'bayer', 'raw_pattern': SAMPLER_PATTERN, 'black_level': 512, 'white_point': 16383}))
    cwd = str(tmp_path)
    out = _run(['eld_amd.defects', 'm.json', '-o', 'defects.npz'], cwd)
    dm = DefectMap.load(str(tmp_path / 'defects.npz'))
    assert dm.mask[sites[:, 0], sites[:, 1]].all() and '%d defective sites' % dm.count in out
    out = _run(['eld_amd.calibrate', 'm.json', '--camera', 'Cam', '--out', 'tables', '--defects', 'defects.npz'], cwd)
    assert '%d defective sites kept out' % dm.count in out and os.path.exists(tmp_path / 'tables' / 'Cam_params.npy')
    long = np.clip(np.round(rng.normal(2000, 200, (Hm, Wm))), 0, 16383).astype(np.uint16)
    long[sites[:, 0], sites[:, 1]] = 16000
    np.save(tmp_path / 'long.npy', long)
    _run(['eld_amd.train_frames', 'long.npy', '--meta', 'sensor.json', '--camera', 'tables/Cam_params.npy', '--patch', '32', '--steps', '2',
          '--defects', 'defects.npz', '-o', 'cam.pt'], cwd)
    np.save(tmp_path / 'short.npy', (512 + (long.astype(np.int64) - 512) // 100).astype(np.uint16))
    _run(['eld_amd.denoise', '--ckpt', 'cam.pt', '--meta', 'sensor.json', '--ratio', '100', '--defects', 'defects.npz', 'short.npy', '-o', 'out'], cwd)
    assert np.load(tmp_path / 'out' / 'short_denoised.npy').shape == (Hm, Wm)
