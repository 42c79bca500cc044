"""GPU tests of the X-Trans calibration: the cell-statistics kernels (eld_calib_cell_*) against NumPy int64 / float64, a closed loop on the
sampler's own X-Trans noise, and the end-to-end path manifest -> CLI -> table -> NoiseModel('PGRUB', cfa='xtrans') -> ELDModel training."""
import ctypes
import json

import numpy as np
import pytest

from eld_amd import _lib as L
from eld_amd import calibrate as CAL

from test_calib_cpu import PATTERNS, flat_sums_ref, sums_ref
from xtrans_ref import CODE_COLOUR, cell_flat_sums_ref, cell_sums_ref, colour_map, fold_bayer, xtrans_pattern

pytestmark = pytest.mark.gpu

PAT = xtrans_pattern()
STEP = 2.0 / 140


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def cell_abi(u, p, white=None):
    """Raw ABI call on a CUDA int16 tensor: (F,Hm,Wm) bias -> (cell_sums, row_sums); (P,2,Hm,Wm) flats with white -> sums."""
    torch = _torch()
    if white is None:
        F, Hm, Wm = u.shape
        cs = torch.empty((F, p, p, 2), dtype=torch.int64, device='cuda')
        rs = torch.empty((F, Hm, p), dtype=torch.int64, device='cuda')
        ws = torch.empty(max(1, L.lib().eld_calib_cell_stats_workspace_bytes(F, Hm, p)), dtype=torch.uint8, device='cuda')
        L.check(L.lib().eld_calib_cell_stats(L.dptr(u), F, Hm, Wm, p, L.dptr(cs), L.dptr(rs), L.dptr(ws), ws.numel(), L.cur_stream()))
        return cs.cpu().numpy(), rs.cpu().numpy()
    P, _, Hm, Wm = u.shape
    out = torch.empty((P, p, p, 4), dtype=torch.int64, device='cuda')
    ws = torch.empty(max(1, L.lib().eld_calib_cell_flat_stats_workspace_bytes(P, Hm, p)), dtype=torch.uint8, device='cuda')
    L.check(L.lib().eld_calib_cell_flat_stats(L.dptr(u), P, Hm, Wm, p, int(white), L.dptr(out), L.dptr(ws), ws.numel(), L.cur_stream()))
    return out.cpu().numpy()


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


# ---- 4. exact sums and the residual --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1386, 2080), (130, 98), (37, 50), (67, 1000), (6, 6)])
def test_cell_sums_and_residual_equal_numpy(eld_lib, shape):
    # (1386, 2080): 16-byte path, Hm % 6 == 0; (130, 98): Wm % 8 != 0, Hm % 6 == 4; (37, 50) odd Hm; (67, 1000): 16-byte path with a
    # row tail (500 words, not a multiple of 12)
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    Hm, Wm = shape
    F = 2
    black = np.array([1024.0, 1023.0, 1025.5, 1021.0])
    u = rng.integers(0, 65536, (F, Hm, Wm), dtype=np.uint16)
    u[1] = np.clip(rng.normal(1030, 6, (Hm, Wm)), 0, 65535).astype(np.uint16)
    st = CAL.xtrans_bias_frame_stats(u, PAT, black, residual=True)
    cs, rs = cell_sums_ref(u, 6)
    assert np.array_equal(st['cell_sums'], cs) and np.array_equal(st['row_sums'], rs)
    code = colour_map(PAT, Hm, Wm)
    t_np = (((u.astype(np.float64) - black[code][None]) - st['color_bias'][:, CODE_COLOUR[code]]) - st['row_offset'][:, :, None]).astype(np.float32)
    assert np.array_equal(st['t'].cpu().numpy(), t_np.reshape(F, -1))
    white = 16383
    ab = rng.integers(0, 65536, (3, 2, Hm, Wm), dtype=np.uint16)
    ab[1] = rng.integers(400, 16383, (2, Hm, Wm), dtype=np.uint16)
    ab[2] = np.clip(rng.normal(3000, 50, (2, Hm, Wm)), 0, 65535).astype(np.uint16)
    ab[2, 0, 0, 0], ab[2, 1, -1, -1] = 16383, 65535
    assert np.array_equal(CAL.xtrans_flat_pair_stats(ab, PAT, black, white, [0.0] * 3)['sums'], cell_flat_sums_ref(ab, 6, white))
    # two calls: identical bits
    assert np.array_equal(CAL.xtrans_bias_frame_stats(u, PAT, black, residual=True)['t'].cpu().numpy(), st['t'].cpu().numpy())


def test_odd_element_view_gives_the_same_sums(eld_lib):
    torch = _torch()
    rng = np.random.default_rng(5)
    F, Hm, Wm = 2, 66, 98
    u = rng.integers(0, 65536, (F, Hm, Wm), dtype=np.uint16)
    buf = torch.zeros(u.size + 1, dtype=torch.int16, device='cuda')
    buf[1:] = _dev(u).reshape(-1)
    view = buf[1:].view(F, Hm, Wm)
    assert view.data_ptr() % 4 != 0
    st = CAL.xtrans_bias_frame_stats(view, PAT, [0.0] * 4)
    cs, rs = cell_sums_ref(u, 6)
    assert np.array_equal(st['cell_sums'], cs) and np.array_equal(st['row_sums'], rs)
    ab = rng.integers(0, 65536, (2, 2, Hm, Wm), dtype=np.uint16)
    fb = torch.zeros(ab.size + 1, dtype=torch.int16, device='cuda')
    fb[1:] = _dev(ab).reshape(-1)
    assert np.array_equal(CAL.xtrans_flat_pair_stats(fb[1:].view(2, 2, Hm, Wm), PAT, [0.0] * 4, 16383, [0.0] * 3)['sums'],
                          cell_flat_sums_ref(ab, 6, 16383))


def bayer_abi(u, pattern, white=None, residual=None):
    """The Bayer entry points, raw, on a CUDA int16 tensor: (F,Hm,Wm) bias -> (chan_sums, row_sums), or with residual=(black, cb, rho)
    the float32 residuals; (P,2,Hm,Wm) flats with white -> sums."""
    torch = _torch()
    lib, pat = L.lib(), (ctypes.c_int * 4)(*[int(v) for v in np.asarray(pattern).reshape(-1)])
    if white is not None:
        P, _, Hm, Wm = u.shape
        out = torch.empty((P, 4, 4), dtype=torch.int64, device='cuda')
        ws = torch.empty(max(1, lib.eld_calib_flat_stats_workspace_bytes(P, Hm)), dtype=torch.uint8, device='cuda')
        L.check(lib.eld_calib_flat_stats(L.dptr(u), P, Hm, Wm, pat, int(white), L.dptr(out), L.dptr(ws), ws.numel(), L.cur_stream()))
        return out.cpu().numpy()
    F, Hm, Wm = u.shape
    if residual is not None:
        black, cb, rho = residual
        t = torch.empty((F, Hm * Wm), dtype=torch.float32, device='cuda')
        cbd, rhod = torch.from_numpy(cb).cuda(), torch.from_numpy(rho).cuda()
        L.check(lib.eld_calib_bias_residual(L.dptr(u), F, Hm, Wm, pat, (ctypes.c_double * 4)(*black.tolist()), L.dptr(cbd), L.dptr(rhod),
                                            L.dptr(t), L.cur_stream()))
        return t.cpu().numpy()
    cs = torch.empty((F, 4, 2), dtype=torch.int64, device='cuda')
    rs = torch.empty((F, Hm, 2), dtype=torch.int64, device='cuda')
    ws = torch.empty(max(1, lib.eld_calib_bias_stats_workspace_bytes(F, Hm)), dtype=torch.uint8, device='cuda')
    L.check(lib.eld_calib_bias_stats(L.dptr(u), F, Hm, Wm, pat, L.dptr(cs), L.dptr(rs), L.dptr(ws), ws.numel(), L.cur_stream()))
    return cs.cpu().numpy(), rs.cpu().numpy()


@pytest.mark.parametrize('shape', [(2, 2), (130, 2), (66, 98), (64, 96), (130, 98)])
@pytest.mark.parametrize('pattern', PATTERNS)
def test_period_two_folds_to_the_bayer_passes(eld_lib, shape, pattern):
    # (2, 2): one word, tail lanes only; (66, 98) and (130, 98): the scalar path (Wm % 8 != 0); (64, 96): the 16-byte path, 12 groups.
    # Two frames / two pairs: the frame stride counts.  The Bayer entry points are called raw: the module no longer enters them.
    rng = np.random.default_rng(shape[0] + 1000 * PATTERNS.index(pattern))
    Hm, Wm = shape
    u = rng.integers(0, 65536, (2, Hm, Wm), dtype=np.uint16)
    cs, rs = cell_abi(_dev(u), 2)
    assert np.array_equal(cs, cell_sums_ref(u, 2)[0]) and np.array_equal(rs, cell_sums_ref(u, 2)[1])
    bs = CAL.bias_frame_stats(u, pattern, [0.0] * 4)
    assert np.array_equal(fold_bayer(cs, pattern), bs['chan_sums']) and np.array_equal(rs, bs['row_sums'])
    bcs, brs = bayer_abi(_dev(u), pattern)
    assert np.array_equal(bcs, sums_ref(u, pattern)[0]) and np.array_equal(brs, sums_ref(u, pattern)[1])
    white = 16383
    ab = rng.integers(0, 65536, (2, 2, Hm, Wm), dtype=np.uint16)
    ab[1] = np.clip(rng.normal(3000, 50, (2, Hm, Wm)), 0, 65535).astype(np.uint16)
    ab[1, 0, 0, 0], ab[1, 1, -1, -1] = 16383, 65535             # a saturated pixel; the largest code in the last pixel of the second frame
    fl = cell_abi(_dev(ab), 2, white=white)
    assert np.array_equal(fold_bayer(fl, pattern), CAL.flat_pair_stats(ab, pattern, [0.0] * 4, white, [0.0] * 4)['sums'])
    assert np.array_equal(bayer_abi(_dev(ab), pattern, white=white), flat_sums_ref(ab, pattern, white))
    black = np.array([512.0, 511.0, 513.5, 509.0])
    cb, rho = rng.normal(0.0, 2.0, (2, 4)), rng.normal(0.0, 1.0, (2, Hm))
    ch = np.asarray(pattern)[np.arange(Hm)[:, None] & 1, np.arange(Wm)[None, :] & 1]
    t_np = (((u.astype(np.float64) - black[ch][None]) - cb[:, ch]) - rho[:, :, None]).astype(np.float32)
    assert np.array_equal(bayer_abi(_dev(u), pattern, residual=(black, cb, rho)), t_np.reshape(2, -1))


# ---- 5. closed loop on the sampler -------------------------------------------------------------------------------------------
def synth_xtrans(params, flags, sample_ids, h, w, y=None, dn=1.0, black=512.0):
    """Sampler output on packed X-Trans (N,9,h,w), unpacked to the (3h,3w) mosaic, times dn, + black, rounded to uint16 (int16 view)."""
    from eld_amd.noise import RawPacker, sample_noise
    torch = _torch()
    N = len(params)
    if y is None:
        y = torch.zeros((N, 9, h, w), dtype=torch.float32, device='cuda')
    z = sample_noise(y, params, flags | L.CFA_XTRANS, 2018, sample_ids)
    mos = RawPacker('xtrans').unpack_raw_xtrans(z)
    del z
    return torch.clamp(torch.round(mos.double() * dn + black), 0, 65535).to(torch.int32).to(torch.int16)


def _bias_params(lam, tl_scale, row_scale, cb, N):
    from eld_amd.noise import NoiseParams
    return [NoiseParams(1.0, 0.0, 1.0, 1.0, tl_lambda=lam, tl_scale=tl_scale, row_scale=row_scale, color_bias=tuple(cb) + (0.0,))
            for _ in range(N)]


def test_closed_loop_bias_recovers_the_sampler_parameters(eld_lib):
    # Four frames of 9 x 1386 x 2080 packed = 4158 x 6240 mosaics (n = 25.9 M; R and B 5.8 M pixels each, G 14.4 M).  Every sensor row
    # holds all three colours, so the standard errors per frame are:
    #   colour bias: the row noise averaged over the Hm = 4158 rows: row_scale / sqrt(Hm) = 0.5 / 64.5 = 0.0078 DN, plus
    #     tl_scale * sd(TL) / sqrt(5.8 M) < 0.004 DN -> < 0.009 DN; the mean of 4 frames < 0.0045 DN: the 0.05 DN bound is > 10 SE;
    #   R_scale: sd(mean rho^2) / R^2 = sqrt(2 / Hm) (1 + s_t^2 / (Wm R^2)) <= 0.024 -> 1.2 % on R; mean of 4 frames 0.6 %: 5 % is 8 SE.
    #     A wrong row map mixes 2 or 3 sensor rows' normals into one mosaic row and shrinks R by 30 % or more;
    #   G_scale: the probplot slope over 25.9 M samples, SE < 0.1 %; the DN rounding adds < 0.1 %: 3 % is > 10 SE;
    #   lambda: the PPCC peak moves far less than a grid step at this n (the Bayer test finds it to one step from 12.1 M samples).
    torch = _torch()
    lam = float(CAL.DEFAULT_LAMBDAS[70 - 14])
    tl_scale, row_scale, cb = 6.0, 0.5, (1.5, -1.0, 0.75)
    F = 4
    u = synth_xtrans(_bias_params(lam, tl_scale, row_scale, cb, F), L.READ_TL | L.ROW | L.CBIAS, [3000 + i for i in range(F)], 1386, 2080)
    assert tuple(u.shape) == (F, 4158, 6240)
    st = CAL.xtrans_bias_frame_stats(u, PAT, [512.0] * 4, residual=True)
    pp = CAL.tukey_lambda_ppcc(st.pop('t'))
    assert np.all(np.abs(pp['lam_hat'] - lam) <= STEP + 1e-12), pp['lam_hat']
    assert abs(np.mean(pp['scale']) / tl_scale - 1) < 0.03, pp['scale']
    assert abs(np.mean(st['R_scale']) / row_scale - 1) < 0.05, st['R_scale']
    assert np.max(np.abs(st['color_bias'].mean(axis=0) - np.asarray(cb))) < 0.05, st['color_bias']
    del u
    torch.cuda.empty_cache()


def test_closed_loop_flats_recover_K(eld_lib):
    # Six levels, one pair each of 4158 x 6240 mosaics, K = 2.5, Gaussian read noise 3 DN.  var(a-b)/2 over the 5.8 M R (or B) pixels
    # has a relative SE of sqrt(2/5.8 M) = 0.06 % (G: 0.04 %); the OLS slope over 18 points spread over 400..8000 DN has SE < 0.05 %:
    # the 1 % bound is > 20 SE.  Rounding to DN adds a constant 1/12 to var(a-b)/2 (the intercept takes it).
    from eld_amd.noise import NoiseParams
    torch = _torch()
    K, S = 2.5, 16383.0 - 512.0
    levels = np.array([400.0, 1200, 2400, 4000, 6000, 8000])
    h, w = 1386, 2080
    y = torch.from_numpy(np.repeat(levels / S, 2).astype(np.float32)).cuda().view(-1, 1, 1, 1).expand(12, 9, h, w).contiguous()
    prm = [NoiseParams(K, 3.0, S, 1.0) for _ in range(12)]
    u = synth_xtrans(prm, L.SHOT_POISSON | L.READ_GAUSS, list(range(6000, 6012)), h, w, y=y, dn=S).view(6, 2, 3 * h, 3 * w)
    del y
    fl = CAL.xtrans_flat_pair_stats(u, PAT, [512.0] * 4, 16383, [0.0] * 3)
    assert fl['usable'].all()
    np.testing.assert_allclose(fl['mu'], levels[:, None].repeat(3, 1), rtol=2e-3)
    assert abs(CAL.ptc_gain(fl['mu'], fl['var'], fl['usable']) / K - 1) < 0.01
    del u
    torch.cuda.empty_cache()


# ---- 6. end to end: manifest -> CLI -> table -> NoiseModel -> ELDModel ----------------------------------------------------------
def _sony_law():
    from eld_amd.noise import load_camera_params
    return load_camera_params('SonyA7S2')['Profile-1']


def make_xtrans_sessions(h=64, w=96, F=2, P=4, seed=0):
    """Five sessions on the SonyA7S2 law, X-Trans: packed (9,h,w) synthesis unpacked to (3h,3w), then cropped by one row and two columns
    (sides that are not multiples of 6)."""
    from eld_amd.noise import NoiseParams
    torch = _torch()
    law = _sony_law()

    def f(name, K):
        return float(np.exp(law[name]['slope'] * np.log(K) + law[name]['bias']))
    sessions, sid = [], 20000 * (seed + 1)
    for s, K in enumerate([0.5, 1.0, 2.0, 4.0, 8.0]):
        lam = float(CAL.DEFAULT_LAMBDAS[70 + (4, 8, 10, 6, 9)[s]])
        cb = tuple(0.3 * np.sin(np.arange(3) + s))
        bias = synth_xtrans(_bias_params(lam, f('G_scale', K), f('R_scale', K), cb, F), L.READ_TL | L.ROW | L.CBIAS,
                            list(range(sid, sid + F)), h, w)[:, :-1, :-2]
        sid += F
        S = 16383.0 - 512.0
        levels = np.linspace(300.0, 0.5 * S, P)
        y = torch.from_numpy(np.repeat(levels / S, 2).astype(np.float32)).cuda().view(-1, 1, 1, 1).expand(2 * P, 9, h, w).contiguous()
        flats = synth_xtrans([NoiseParams(K, f('g_scale', K), S, 1.0) for _ in range(2 * P)], L.SHOT_POISSON | L.READ_GAUSS,
                             list(range(sid, sid + 2 * P)), h, w, y=y, dn=S).view(P, 2, 3 * h, 3 * w)[:, :, :-1, :-2]
        sid += 2 * P
        sessions.append({'iso': int(100 * K), 'bias': bias.cpu().numpy().view(np.uint16), 'flats': flats.cpu().numpy().view(np.uint16),
                         'K': K, 'cb': cb, 'G': f('G_scale', K), 'R': f('R_scale', K)})
    return sessions


def test_cli_table_drives_xtrans_training(eld_lib, tmp_path, monkeypatch, capsys):
    import types
    from eld_amd.model import ELDModel
    from eld_amd.noise import NoiseModel, load_camera_params
    torch = _torch()
    sessions = make_xtrans_sessions()
    man = {'cfa': 'xtrans', 'raw_pattern': PAT.tolist(), 'black_level': [512] * 4, 'white_level': 16383, 'sessions': []}
    for i, s in enumerate(sessions):
        e = {'iso': s['iso'], 'bias': [], 'flats': []}
        for j, u in enumerate(s['bias']):
            np.save(tmp_path / ('b%d_%d.npy' % (i, j)), u)
            e['bias'].append('b%d_%d.npy' % (i, j))
        for j, p in enumerate(s['flats']):
            np.save(tmp_path / ('f%d_%da.npy' % (i, j)), p[0])
            np.save(tmp_path / ('f%d_%db.npy' % (i, j)), p[1])
            e['flats'].append(['f%d_%da.npy' % (i, j), 'f%d_%db.npy' % (i, j)])
        man['sessions'].append(e)
    (tmp_path / 'm.json').write_text(json.dumps(man))
    rel = str(tmp_path / 'camera_params' / 'release')
    assert CAL.main([str(tmp_path / 'm.json'), '--camera', 'FujiSynth', '--out', rel]) == 0
    assert 'wrote' in capsys.readouterr().out
    tab = load_camera_params('FujiSynth', rel)
    assert tab['cfa'] == 'xtrans' and tab['color_bias'].shape == (10, 3) and tab['G_shape'].shape == (10,)
    # the table equals calibrate_camera on the same sessions; each session's K and colour bias come back
    params, diag = CAL.calibrate_camera([{k: s[k] for k in ('iso', 'bias', 'flats')} for s in sessions], PAT, [512] * 4, 16383, cfa='xtrans')
    assert np.array_equal(params['color_bias'], tab['color_bias']) and np.array_equal(params['G_shape'], tab['G_shape'])
    for s, K in zip(sessions, diag['K']):
        assert abs(K / s['K'] - 1) < 0.02, (K, s['K'])
    Hm, Wm = sessions[0]['bias'].shape[-2:]
    for fr in diag['frames']:
        s = sessions[fr['session']]
        # SE of a colour's mean: the row noise over Hm rows and the Tukey-lambda read noise (sd <= 2 x scale on this grid) over the
        # colour's 8/36 of the pixels; 6 SE
        se = np.sqrt(s['R'] ** 2 / Hm + (2.0 * s['G']) ** 2 / (Hm * Wm * 8 / 36))
        assert np.max(np.abs(fr['color_bias'] - np.asarray(s['cb']))) < 6 * se, (fr['color_bias'], s['cb'], se)

    monkeypatch.chdir(tmp_path)
    opt = types.SimpleNamespace(gpu_ids=[0], isTrain=True, checkpoints_dir=str(tmp_path), name='t', netG='unet', channels=9, stage_in='raw',
                                stage_out='raw', lr=1e-4, beta1=0.9, wd=0.0, loss='l1', resume=False, chop=False, no_log=True,
                                save_epoch_freq=2, model='eld_model')

    def train(prefetch):
        torch.manual_seed(2018)
        m = ELDModel()
        m.initialize(opt)
        nm = NoiseModel(model='PGRUB', cfa='xtrans', cameras=['FujiSynth'])
        assert nm.flags() & L.CFA_XTRANS
        m.set_noise_model(nm)
        np.random.seed(0)
        g = torch.Generator().manual_seed(1)
        data = [{'target': torch.floor(65535 * torch.rand(2, 9, 32, 48, generator=g) ** 2.2) / 65535} for _ in range(3)]
        xs = []
        for it, d in enumerate(data):
            if prefetch and it == 0:
                m.prefetch_input(d)
            m.set_input(d, 'train')
            if prefetch and it + 1 < len(data):
                m.prefetch_input(data[it + 1])
            x = m.input.detach().clone()
            assert bool(torch.isfinite(x).all()) and float(x.min()) >= 0 and float(x.max()) <= 1 and not torch.equal(x.cpu(), d['target'])
            xs.append(x)
            m.optimize_parameters()
            assert np.isfinite(m.get_current_errors()['Pixel'])
        torch.cuda.synchronize()
        return xs
    serial, pre = train(False), train(True)
    for a, b in zip(serial, pre):
        assert torch.equal(a, b)
