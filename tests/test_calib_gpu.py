"""GPU tests of the calibration kernels (eld_amd/csrc/calib.hip) and pipeline (eld_amd/calibrate.py): exact sums and bit-exact residuals
against NumPy, the PPCC against a float64 oracle, closed loops on the project's own sampler, and the end-to-end table against the CPU
restatement of tests/test_calib_cpu.py."""
import numpy as np
import pytest

from eld_amd import calibrate as CAL
from eld_amd import _lib as L
from eld_amd.noise import NoiseModel, NoiseParams, RawPacker, load_camera_params, sample_noise

from test_calib_cpu import PATTERNS, bias_ref, filliben, flat_ref, flat_sums_ref, ppcc_ref, sums_ref, tukey_quantile

pytestmark = pytest.mark.gpu

SAMPLER_PATTERN = [[0, 1], [3, 2]]          # the sampler's packing (R, G1 on even rows; G2, B on odd rows: noise.py:16-19)
STEP = 2.0 / 140                            # the default grid's spacing


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


# ---- 1. exact sums and the residual ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(2848, 4256), (130, 2), (2, 2), (66, 98)])
@pytest.mark.parametrize('pattern', PATTERNS)
def test_sums_and_residual_equal_numpy(eld_lib, shape, pattern):
    rng = np.random.default_rng(7 * shape[0] + shape[1] + 1000 * PATTERNS.index(pattern))
    Hm, Wm = shape
    F = 2
    black = np.array([512.0, 511.0, 513.5, 509.0])
    u = rng.integers(0, 65536, (F, Hm, Wm), dtype=np.uint16)          # the whole code range: exercises the uint32 squares
    u[1] = np.clip(rng.normal(512, 6, (Hm, Wm)), 0, 65535).astype(np.uint16)
    st = CAL.bias_frame_stats(u, pattern, black, residual=True)
    cs, rs = sums_ref(u, pattern)
    assert np.array_equal(st['chan_sums'], cs) and np.array_equal(st['row_sums'], rs)
    pat = np.asarray(pattern)
    ch = pat[np.arange(Hm)[:, None] & 1, np.arange(Wm)[None, :] & 1]
    t_np = (((u.astype(np.float64) - black[ch][None]) - st['color_bias'][:, ch]) - st['row_offset'][:, :, None]).astype(np.float32)
    assert np.array_equal(st['t'].cpu().numpy(), t_np.reshape(F, -1))
    # the same call on a CUDA uint16 view gives the same bits
    torch = _torch()
    st2 = CAL.bias_frame_stats(torch.from_numpy(u.view(np.int16)).cuda(), pattern, black)
    assert np.array_equal(st2['chan_sums'], cs)
    # flat pairs, with saturated pixels and extreme differences
    white = 16383
    ab = rng.integers(0, 65536, (3, 2, Hm, Wm), dtype=np.uint16)
    ab[1] = rng.integers(400, 16383, (2, Hm, Wm), dtype=np.uint16)
    ab[2] = np.clip(rng.normal(3000, 50, (2, Hm, Wm)), 0, 65535).astype(np.uint16)
    ab[2, 0, 0, 0], ab[2, 1, -1, -1] = 16383, 65535
    fl = CAL.flat_pair_stats(ab, pattern, black, white, [0.0] * 4)
    assert np.array_equal(fl['sums'], flat_sums_ref(ab, pattern, white))


def test_view_at_an_odd_element_gives_the_same_sums(eld_lib):
    """A uint16 view whose data starts 2 bytes into an allocation is copied to an aligned buffer by the module, not read misaligned."""
    torch = _torch()
    rng = np.random.default_rng(5)
    F, Hm, Wm = 2, 66, 98
    u = rng.integers(0, 65536, (F, Hm, Wm), dtype=np.uint16)
    base = torch.empty(F * Hm * Wm + 1, dtype=torch.int16, device='cuda')
    view = base[1:].view(F, Hm, Wm)
    view.copy_(torch.from_numpy(u.view(np.int16)).cuda())
    assert view.data_ptr() % 4 == 2
    cs, rs = sums_ref(u, PATTERNS[1])
    st = CAL.bias_frame_stats(view, PATTERNS[1], [0] * 4)
    assert np.array_equal(st['chan_sums'], cs) and np.array_equal(st['row_sums'], rs)
    ab = base[1:1 + 2 * 2 * 32 * Wm].view(2, 2, 32, Wm)                    # flat pairs take the same path
    assert np.array_equal(CAL.flat_pair_stats(ab, PATTERNS[1], [0] * 4, 16383, [0] * 4)['sums'],
                          flat_sums_ref(ab.cpu().numpy().view(np.uint16), PATTERNS[1], 16383))


# ---- 2. PPCC against the float64 oracle ----------------------------------------------------------------------------------------
def ppcc_oracle(t_sorted, lambdas):
    """float64 on the device through torch (an independent evaluation): M by expm1, no cancellation at small |lambda|."""
    torch = _torch()
    x = torch.as_tensor(t_sorted, dtype=torch.float64, device='cuda')
    n = x.numel()
    m = torch.from_numpy(filliben(n)).cuda()
    a, b = torch.log(m), torch.log1p(-m)
    xc = x - x.mean()
    sxx = float((xc * xc).sum())
    r, slope = np.empty(len(lambdas)), np.empty(len(lambdas))
    for k, lam in enumerate(lambdas):
        M = (a - b) if lam == 0 else torch.exp(lam * b) * torch.expm1(lam * (a - b)) / lam
        Mc = M - M.mean()
        sxm, smm = float((Mc * xc).sum()), float((Mc * Mc).sum())
        r[k], slope[k] = sxm / np.sqrt(smm * sxx), sxm / smm
    return r, slope


@pytest.mark.parametrize('n', [3, 1000, 100000, 12100000])
@pytest.mark.parametrize('lam_true', [-0.2, 0.0, 0.14])
def test_ppcc_matches_float64_oracle(eld_lib, n, lam_true):
    torch = _torch()
    rng = np.random.default_rng(n + int(100 * lam_true) + 100)
    u = rng.uniform(size=n)
    t = np.sort((3.0 * tukey_quantile(u, lam_true) - 1.25).astype(np.float32))
    lam = CAL.DEFAULT_LAMBDAS
    td = torch.from_numpy(t).cuda()
    got = CAL.tukey_lambda_ppcc(td, presorted=True)
    again = CAL.tukey_lambda_ppcc(td, presorted=True)
    assert np.array_equal(got['r'], again['r']) and np.array_equal(got['slope'], again['slope'])   # no atomics: identical bits
    r, slope = ppcc_oracle(t, lam)
    assert np.max(np.abs(got['r'] - r)) <= 1e-6
    top = np.sort(r)[-2:]
    if top[1] - top[0] >= 2e-6:
        assert got['index'] == int(np.argmax(r))
    assert np.max(np.abs(got['slope'] - slope) / np.abs(slope)) <= 1e-5
    if n >= 100000:
        assert abs(got['lam_hat'] - lam_true) <= STEP + 1e-12    # the shape the samples were drawn with is found (to one grid step)
    # unsorted input: the module sorts (torch.sort)
    perm = torch.from_numpy(rng.permutation(n)).cuda()
    assert np.array_equal(CAL.tukey_lambda_ppcc(td[perm])['r'], got['r'])


# ---- 3. closed loop on the project's sampler -------------------------------------------------------------------------------------
def synth_mosaics(params, flags, sample_ids, h, w, y=None, black=512.0, dn=1.0):
    """Sampler output times dn (its saturation / ratio: the sampler returns DN * ratio / saturation), unpacked to the Bayer mosaic,
    + black, rounded to uint16.  The bias frames run at saturation = ratio = 1: z is the sum of the terms in DN."""
    torch = _torch()
    N = len(params)
    if y is None:
        y = torch.zeros((N, 4, h, w), dtype=torch.float32, device='cuda')
    z = sample_noise(y, params, flags, 2018, sample_ids)
    mos = RawPacker('bayer').unpack_raw_bayer(z)
    return torch.clamp(torch.round(mos.double() * dn + black), 0, 65535).to(torch.int32).to(torch.uint16)


def _bias_params(lam, tl_scale, row_scale, cb, N):
    return [NoiseParams(1.0, 0.0, 1.0, 1.0, tl_lambda=lam, tl_scale=tl_scale, row_scale=row_scale, color_bias=cb) for _ in range(N)]


@pytest.mark.parametrize('lam_k', [-14, 0, 10])
def test_closed_loop_bias_recovers_the_sampler_parameters(eld_lib, lam_k):
    # Four Sony-size frames (2848 x 4256 mosaic, n = 12.1 M) per shape.  Standard errors at these sizes, per frame:
    #   colour bias: the row noise of the Hm/2 rows of a channel dominates: row_scale*sqrt(2/Hm) = 0.5*0.0265 = 0.013 DN, plus
    #     tl_scale*sd(TL)/sqrt(n/4) < 0.007 DN -> 0.015 DN; the mean of 4 frames 0.0075 DN: the 0.05 DN bound is 6.7 SE;
    #   R_scale: sd(rho^2 mean)/R^2 = sqrt(2/Hm)*(1 + s_t^2/(Wm R^2)) <= 0.03 -> 1.5 % on R; mean of 4 frames 0.75 %: 5 % is 6.7 SE;
    #   G_scale: the probplot slope over 12.1 M samples has SE < 0.1 %; rounding to DN adds variance 1/12 to tl_scale^2 var(TL) >= 36*1.6
    #     (< 0.1 % on the scale): 3 % is > 10 SE;
    #   lambda: the PPCC peak moves by far less than a grid step (0.0143) at this n (test_ppcc_matches_float64_oracle: found to one step
    #     from 1e5 samples).
    torch = _torch()
    lam = float(CAL.DEFAULT_LAMBDAS[70 + lam_k])
    tl_scale, row_scale, cb = 6.0, 0.5, (1.5, -1.0, 0.75, 0.25)
    F = 4
    u = synth_mosaics(_bias_params(lam, tl_scale, row_scale, cb, F), L.READ_TL | L.ROW | L.CBIAS, [100 * lam_k + 1000 + i for i in range(F)],
                      1424, 2128)
    assert tuple(u.shape) == (F, 2848, 4256)
    st = CAL.bias_frame_stats(u, SAMPLER_PATTERN, [512.0] * 4, residual=True)
    pp = CAL.tukey_lambda_ppcc(st.pop('t'))
    assert np.all(np.abs(pp['lam_hat'] - lam) <= STEP + 1e-12), pp['lam_hat']
    assert abs(np.mean(pp['scale']) / tl_scale - 1) < 0.03, pp['scale']
    assert abs(np.mean(st['R_scale']) / row_scale - 1) < 0.05, st['R_scale']
    assert np.max(np.abs(st['color_bias'].mean(axis=0) - np.asarray(cb))) < 0.05, st['color_bias']
    del u
    torch.cuda.empty_cache()


def test_closed_loop_flats_recover_K(eld_lib):
    # Six levels, one Sony-size pair each, K = 2.5, Gaussian read noise 3 DN.  var(a-b)/2 over n_c = 3.03 M pixels per channel has a
    # relative SE of sqrt(2/n_c) = 0.08 %; the OLS slope over 24 points spread over 400..8000 DN has SE ~0.05 %: the 1 % bound is > 3 SE
    # (20).  Rounding to DN adds a constant 1/12 to var(a-b)/2 (the intercept takes it).
    torch = _torch()
    K, S = 2.5, 16383.0 - 512.0
    levels = np.array([400.0, 1200, 2400, 4000, 6000, 8000])
    h, w = 1424, 2128
    y = torch.from_numpy(np.repeat(levels / S, 2).astype(np.float32)).cuda().view(-1, 1, 1, 1).expand(12, 4, h, w).contiguous()
    prm = [NoiseParams(K, 3.0, S, 1.0) for _ in range(12)]
    u = synth_mosaics(prm, L.SHOT_POISSON | L.READ_GAUSS, list(range(5000, 5012)), h, w, y=y, dn=S).view(6, 2, 2 * h, 2 * w)
    fl = CAL.flat_pair_stats(u, SAMPLER_PATTERN, [512.0] * 4, 16383, [0.0] * 4)
    assert fl['usable'].all()
    np.testing.assert_allclose(fl['mu'], levels[:, None].repeat(4, 1), rtol=2e-3)
    assert abs(CAL.ptc_gain(fl['mu'], fl['var'], fl['usable']) / K - 1) < 0.01


# ---- 4. end to end -----------------------------------------------------------------------------------------------------------
SONY = load_camera_params('SonyA7S2')['Profile-1']


def _law(name, K):
    return float(np.exp(SONY[name]['slope'] * np.log(K) + SONY[name]['bias']))


def make_sessions(h=128, w=192, F=2, P=6, seed=0):
    """Five sessions whose K, G_scale (Tukey-lambda scale) and R_scale follow the SonyA7S2 law exactly; 'g' read noise of the flats
    follows the g_scale law.  Mosaics (2h, 2w) uint16, black 512, white 16383."""
    torch = _torch()
    Ks = [0.5, 1.0, 2.0, 4.0, 8.0]
    sessions = []
    sid = 10000 * (seed + 1)
    for s, K in enumerate(Ks):
        lam = float(CAL.DEFAULT_LAMBDAS[70 + (4, 8, 10, 6, 9)[s]])
        cb = tuple(0.3 * np.sin(np.arange(4) + s))
        bias = synth_mosaics(_bias_params(lam, _law('G_scale', K), _law('R_scale', K), cb, F), L.READ_TL | L.ROW | L.CBIAS,
                             list(range(sid, sid + F)), h, w)
        sid += F
        S = 16383.0 - 512.0
        levels = np.linspace(300.0, 0.5 * S, P)
        y = torch.from_numpy(np.repeat(levels / S, 2).astype(np.float32)).cuda().view(-1, 1, 1, 1).expand(2 * P, 4, h, w).contiguous()
        flats = synth_mosaics([NoiseParams(K, _law('g_scale', K), S, 1.0) for _ in range(2 * P)], L.SHOT_POISSON | L.READ_GAUSS,
                              list(range(sid, sid + 2 * P)), h, w, y=y, dn=S).view(P, 2, 2 * h, 2 * w)
        sid += 2 * P
        sessions.append({'iso': int(100 * K), 'bias': bias.cpu().numpy(), 'flats': flats.cpu().numpy(), 'K': K, 'lambda': lam})
    return sessions


def cpu_calibration(sessions, pattern, black, white):
    """The CPU restatement (float64 NumPy from the pixels) of calibrate_camera."""
    frames, Ks = [], []
    for s in sessions:
        bs = [bias_ref(u, pattern, black) for u in s['bias']]
        cbm = np.mean([b[0] for b in bs], axis=0)
        pts = [flat_ref(p[0], p[1], pattern, black, white, cbm) for p in s['flats']]
        mu = np.concatenate([p[0][p[2]] for p in pts])
        var = np.concatenate([p[1][p[2]] for p in pts])
        K = np.polyfit(mu, var, 1)[0]
        Ks.append(K)
        for cb, rho, g, R, t in bs:
            r, slope = ppcc_ref(t, CAL.DEFAULT_LAMBDAS)
            k = int(np.argmax(r))
            frames.append({'K': K, 'lambda': CAL.DEFAULT_LAMBDAS[k], 'G_scale': slope[k], 'R_scale': R, 'g_scale': g, 'color_bias': cb})
    out = {'Kmin': min(Ks), 'Kmax': max(Ks), 'G_shape': np.array([f['lambda'] for f in frames]),
           'color_bias': np.array([f['color_bias'] for f in frames]), 'Profile-1': {}}
    x = np.log([f['K'] for f in frames])
    for k in CAL.SIGMA_KEYS:
        y = np.log([f[k] for f in frames])
        (a, b), ssr = np.polyfit(x, y, 1, full=True)[:2]
        out['Profile-1'][k] = {'slope': a, 'bias': b, 'sigma': np.sqrt(ssr[0] / (len(frames) - 2))}
    return out, frames


def test_end_to_end_law_cpu_restatement_and_sampler(eld_lib, tmp_path, monkeypatch, capsys):
    pattern, black, white = SAMPLER_PATTERN, [512.0] * 4, 16383
    sessions = make_sessions()
    params, diag = CAL.calibrate_camera([{k: s[k] for k in ('iso', 'bias', 'flats')} for s in sessions], pattern, black, white)
    # the GPU pipeline equals the CPU restatement on 256 x 384 mosaics
    ref, rframes = cpu_calibration(sessions, pattern, black, white)
    assert np.array_equal(params['G_shape'], ref['G_shape'])
    for s in sessions:
        cs, rs = sums_ref(s['bias'], pattern)
        st = CAL.bias_frame_stats(s['bias'], pattern, black)
        assert np.array_equal(st['chan_sums'], cs) and np.array_equal(st['row_sums'], rs)
        assert np.array_equal(CAL.flat_pair_stats(s['flats'], pattern, black, white, [0] * 4)['sums'], flat_sums_ref(s['flats'], pattern, white))
    for fr, rf in zip(diag['frames'], rframes):
        assert abs(fr['K'] - rf['K']) <= 1e-9 * rf['K']
        assert abs(fr['R_scale'] - rf['R_scale']) <= 1e-9 and abs(fr['g_scale'] - rf['g_scale']) <= 1e-9
        assert np.max(np.abs(fr['color_bias'] - rf['color_bias'])) <= 1e-9
        assert abs(fr['G_scale'] - rf['G_scale']) <= 1e-5 * rf['G_scale']
    assert abs(params['Kmin'] - ref['Kmin']) <= 1e-9 * ref['Kmin'] and abs(params['Kmax'] - ref['Kmax']) <= 1e-9 * ref['Kmax']
    np.testing.assert_allclose(params['color_bias'], ref['color_bias'].astype(np.float32), rtol=0, atol=1e-6)
    for k in CAL.SIGMA_KEYS:
        tol = 1e-5 if k == 'G_scale' else 1e-9     # G_scale samples agree to 1e-5 relative (fp32 quantiles), the others to 1e-9
        for f in ('slope', 'bias', 'sigma'):
            assert abs(params['Profile-1'][k][f] - ref['Profile-1'][k][f]) <= tol * (1 + abs(ref['Profile-1'][k][f])), (k, f)
    # the law comes back.  Per frame at 256 x 384: R_scale SE ~ sqrt(1/Hm) ~ 6 %, G_scale (probplot slope over 98 k samples) ~ 1 %,
    # over 10 frames spread over log K in [-0.7, 2.1] (sd 1.0): slope SE ~ 0.06 / (1.0 sqrt(10)) = 0.02 for R, < 0.01 for G;
    # bias SE about the same at the centre log K = 0.7, 0.7 x the slope's elsewhere.  Bounds: 0.08 (R) and 0.05 (G) on both, plus a
    # 3 % allowance on G_scale for the rounding to DN at the smallest scales (tl_scale 1.2 DN at K = 0.5).
    for k, tol in (('G_scale', 0.05), ('R_scale', 0.08)):
        assert abs(params['Profile-1'][k]['slope'] - SONY[k]['slope']) < tol, (k, params['Profile-1'][k])
        assert abs(params['Profile-1'][k]['bias'] - SONY[k]['bias']) < tol, (k, params['Profile-1'][k])
    for s, K in zip(sessions, diag['K']):                      # K within 1 %: the PTC slope over 24 points of 24.6 k pixels, SE ~0.3 %
        assert abs(K / s['K'] - 1) < 0.01, (K, s['K'])
    # the saved table drives the sampler
    monkeypatch.chdir(tmp_path)
    CAL.save_camera_params(params, 'Synth', 'camera_params/release')
    nm = NoiseModel(model='PGRUB', cameras=['Synth'])
    torch = _torch()
    np.random.seed(0)
    z = nm(torch.full((2, 4, 64, 96), 0.05, device='cuda'))
    assert bool(torch.isfinite(z).all())


def test_cli_writes_the_table(eld_lib, tmp_path, capsys):
    import json
    sessions = make_sessions(h=32, w=48, F=2, P=4, seed=1)
    man = {'raw_pattern': SAMPLER_PATTERN, 'black_level': [512] * 4, 'white_level': 16383, 'sessions': []}
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
    assert CAL.main([str(tmp_path / 'm.json'), '--camera', 'Cli', '--out', str(tmp_path / 'out')]) == 0
    p = load_camera_params('Cli', str(tmp_path / 'out'))
    assert p['G_shape'].shape == (10,) and p['color_bias'].shape == (10, 4)
    assert 'wrote' in capsys.readouterr().out


def test_saturated_session_and_flat_rows_raise(eld_lib):
    u = np.random.default_rng(1).integers(500, 524, (2, 8, 8)).astype(np.uint16)
    sat = np.full((3, 2, 8, 8), 16383, np.uint16)
    with pytest.raises(ValueError, match='usable flat'):
        CAL.calibrate_camera([{'bias': u, 'flats': sat}, {'bias': u, 'flats': sat}], SAMPLER_PATTERN, [512] * 4, 16383)
    flat = np.full((2, 8, 8), 512, np.uint16)                  # no row structure at all: R_scale sample 0
    rng = np.random.default_rng(0)
    fl = np.stack([np.stack([rng.poisson(lv, (8, 8)) + 512, rng.poisson(lv, (8, 8)) + 512]) for lv in (100, 400, 1600)]).astype(np.uint16)
    with pytest.raises(ValueError, match='row-noise sample is 0'):
        CAL.calibrate_camera([{'bias': flat, 'flats': fl}, {'bias': flat, 'flats': fl * 1}], SAMPLER_PATTERN, [512] * 4, 16383)
