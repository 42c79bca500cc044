"""CPU tests of the calibration (eld_amd/calibrate.py): the NumPy restatement of the estimators (also used by tests/test_calib_gpu.py)
against SciPy / NumPy, the host derivations from the exact sums, the release schema, the save -> NoiseModel round trip and every
argument error raised before device work."""
import os

import numpy as np
import pytest

from eld_amd import calibrate as CAL
from eld_amd.noise import NoiseModel, load_camera_params


# ---- NumPy restatement of DESIGN.md "Calibration" (float64) --------------------------------------------------------------------
def filliben(n):
    """Filliben's uniform order-statistic medians, as scipy.stats.probplot builds them."""
    m = np.empty(n)
    m[-1] = 0.5 ** (1.0 / n)
    m[0] = 1.0 - m[-1]
    i = np.arange(2, n)
    m[1:-1] = (i - 0.3175) / (n + 0.365)
    return m


def tukey_quantile(m, lam):
    if lam == 0:
        return np.log(m / (1.0 - m))
    return (m ** lam - (1.0 - m) ** lam) / lam


def ppcc_ref(t, lambdas):
    """(r, slope) over the grid: Pearson correlation and least-squares slope of the sorted samples on the quantiles."""
    x = np.sort(np.asarray(t, np.float64))
    m = filliben(x.size)
    r, slope = np.empty(len(lambdas)), np.empty(len(lambdas))
    xc = x - x.mean()
    for k, lam in enumerate(lambdas):
        M = tukey_quantile(m, lam)
        Mc = M - M.mean()
        r[k] = np.sum(Mc * xc) / np.sqrt(np.sum(Mc * Mc) * np.sum(xc * xc))
        slope[k] = np.sum(Mc * xc) / np.sum(Mc * Mc)
    return r, slope


def bias_ref(u, pattern, black):
    """One bias frame (Hm,Wm) -> (cb (4,), rho (Hm,), g_scale, R_scale, t float32 (Hm*Wm,)) straight from the pixels."""
    Hm, Wm = u.shape
    pattern = np.asarray(pattern).reshape(2, 2)
    ch = pattern[np.arange(Hm)[:, None] & 1, np.arange(Wm)[None, :] & 1]
    blk = np.asarray(black, np.float64)[ch]
    d = u.astype(np.float64) - blk
    cb = np.array([d[ch == c].mean() for c in range(4)])
    e = d - cb[ch]
    rho = e.mean(axis=1)
    t = e - rho[:, None]
    g = np.sqrt(np.mean(e * e))
    R = np.sqrt(max(0.0, np.mean(rho * rho) - np.mean(t * t) / Wm))
    t32 = (((u.astype(np.float64) - blk) - cb[ch]) - rho[:, None]).astype(np.float32).reshape(-1)
    return cb, rho, g, R, t32


def flat_ref(a, b, pattern, black, white, cbm):
    """One flat pair -> (mu (4,), var (4,), usable (4,))."""
    Hm, Wm = a.shape
    pattern = np.asarray(pattern).reshape(2, 2)
    ch = pattern[np.arange(Hm)[:, None] & 1, np.arange(Wm)[None, :] & 1]
    a64, b64 = a.astype(np.int64), b.astype(np.int64)
    mu, var, ok = np.empty(4), np.empty(4), np.empty(4, bool)
    for c in range(4):
        sa, sb = a64[ch == c], b64[ch == c]
        mu[c] = np.mean((sa + sb) / 2.0) - black[c] - cbm[c]
        var[c] = np.var(sa - sb) / 2.0
        ok[c] = not np.any((sa >= white) | (sb >= white)) and 0 < mu[c] <= 0.8 * (white - black[c])
    return mu, var, ok


def sums_ref(u, pattern):
    """The exact integer sums of eld_calib_bias_stats: (F,4,2) and (F,Hm,2)."""
    F, Hm, Wm = u.shape
    pattern = np.asarray(pattern).reshape(2, 2)
    ch = pattern[np.arange(Hm)[:, None] & 1, np.arange(Wm)[None, :] & 1]
    x = u.astype(np.int64)
    cs = np.stack([np.stack([np.stack([x[f][ch == c].sum(), (x[f][ch == c] ** 2).sum()]) for c in range(4)]) for f in range(F)])
    rs = np.stack([x[:, :, 0::2].sum(axis=2), x[:, :, 1::2].sum(axis=2)], axis=2)
    return cs, rs


def flat_sums_ref(ab, pattern, white):
    P, _, Hm, Wm = ab.shape
    pattern = np.asarray(pattern).reshape(2, 2)
    ch = pattern[np.arange(Hm)[:, None] & 1, np.arange(Wm)[None, :] & 1]
    x = ab.astype(np.int64)
    out = np.zeros((P, 4, 4), np.int64)
    for p in range(P):
        a, b = x[p, 0], x[p, 1]
        for c in range(4):
            sa, sb = a[ch == c], b[ch == c]
            out[p, c] = [(sa + sb).sum(), (sa - sb).sum(), ((sa - sb) ** 2).sum(), ((sa >= white) | (sb >= white)).sum()]
    return out


PATTERNS = ([[0, 1], [3, 2]], [[2, 3], [1, 0]], [[1, 0], [2, 3]], [[3, 2], [0, 1]])


# ---- tests -----------------------------------------------------------------------------------------------------------------------
def test_ppcc_restatement_equals_scipy_ppcc_plot():
    stats = pytest.importorskip('scipy.stats')
    rng = np.random.default_rng(7)
    u = rng.uniform(size=20000)
    x = 2.5 * tukey_quantile(u, 0.14) + 0.3
    svals, ppcc = stats.ppcc_plot(x, -1, 1, dist='tukeylambda', N=141)
    assert np.array_equal(svals, CAL.DEFAULT_LAMBDAS)                 # the default grid is ppcc_plot's
    r, slope = ppcc_ref(x, svals)
    np.testing.assert_allclose(r, ppcc, rtol=0, atol=1e-9)
    for k in (0, 60, 70, 79, 140):
        (_, _), (sl, _, _) = stats.probplot(x, svals[k], dist='tukeylambda', fit=True)
        assert abs(slope[k] - sl) <= 1e-9 * abs(sl)


def test_default_grid_holds_every_shipped_shape():
    from eld_amd.noise import ALL_CAMERAS
    for cam in ALL_CAMERAS:
        s = load_camera_params(cam)['G_shape']
        assert np.abs(s[:, None] - CAL.DEFAULT_LAMBDAS[None, :]).min(axis=1).max() < 1e-15, cam


def test_fit_log_linear_matches_polyfit():
    rng = np.random.default_rng(3)
    K = np.exp(rng.uniform(np.log(0.1), np.log(6), 16))
    sig = np.exp(0.46 * np.log(K) + 0.57 + 0.26 * rng.standard_normal(16))
    fit = CAL.fit_log_linear(K, sig)
    (slope, bias), ssr = np.polyfit(np.log(K), np.log(sig), 1, full=True)[:2]
    assert abs(fit['slope'] - slope) < 1e-12 and abs(fit['bias'] - bias) < 1e-12
    assert abs(fit['sigma'] - np.sqrt(ssr[0] / (16 - 2))) < 1e-12       # m - 2 degrees of freedom
    assert all(type(fit[k]) is np.float64 for k in ('slope', 'bias', 'sigma'))


@pytest.mark.parametrize('pattern', PATTERNS)
def test_host_derivations_from_sums_equal_the_pixel_restatement(pattern):
    rng = np.random.default_rng(11)
    F, Hm, Wm = 3, 34, 50
    black = np.array([512.0, 510.0, 514.0, 509.0])
    u = np.clip(np.round(rng.normal(512, 4, (F, Hm, Wm)) + rng.normal(0, 2, (F, Hm, 1))), 0, 65535).astype(np.uint16)
    cs, rs = sums_ref(u, pattern)
    d = CAL.bias_stats_from_sums(cs, rs, pattern, black, Hm, Wm)
    for f in range(F):
        cb, rho, g, R, _ = bias_ref(u[f], pattern, black)
        np.testing.assert_allclose(d['color_bias'][f], cb, rtol=0, atol=1e-9)
        np.testing.assert_allclose(d['row_offset'][f], rho, rtol=0, atol=1e-9)
        assert abs(d['g_scale'][f] - g) < 1e-9 and abs(d['R_scale'][f] - R) < 1e-9
    ab = rng.integers(500, 4000, (4, 2, Hm, Wm)).astype(np.uint16)
    ab[3, 1, 5, 7] = 4095
    white = 4095
    cbm = d['color_bias'].mean(axis=0)
    fl = CAL.flat_stats_from_sums(flat_sums_ref(ab, pattern, white), black, white, cbm, Hm, Wm)
    for p in range(4):
        mu, var, ok = flat_ref(ab[p, 0], ab[p, 1], pattern, black, white, cbm)
        np.testing.assert_allclose(fl['mu'][p], mu, rtol=0, atol=1e-9)
        np.testing.assert_allclose(fl['var'][p], var, rtol=1e-12)
        assert np.array_equal(fl['usable'][p], ok)
    assert not fl['usable'][3].all()                                  # the saturated pixel drops its channel


def synthetic_frames(seed=0):
    """Per-frame samples following the SonyA7S2 law (two frames per session, five sessions)."""
    ref = load_camera_params('SonyA7S2')['Profile-1']
    rng = np.random.default_rng(seed)
    Ks = list(np.exp(np.linspace(np.log(0.2), np.log(5), 5)))
    frames = []
    for K in Ks:
        for _ in range(2):
            fr = {'K': K, 'iso': int(100 * K), 'lambda': float(CAL.DEFAULT_LAMBDAS[70 + rng.integers(-10, 10)]),
                  'color_bias': rng.normal(0, 1, 4)}
            for k in CAL.SIGMA_KEYS:
                fr[k] = float(np.exp(ref[k]['slope'] * np.log(K) + ref[k]['bias'] + 0.05 * rng.standard_normal()))
            frames.append(fr)
    return frames, Ks


def _same_schema(a, b, path=''):
    assert type(a) is type(b), (path, type(a), type(b))
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), (path, sorted(a), sorted(b))
        for k in a:
            _same_schema(a[k], b[k], path + '/' + k)
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.ndim == b.ndim and a.shape[1:] == b.shape[1:], (path, a.dtype, a.shape, b.dtype, b.shape)


def test_schema_matches_the_release_table():
    frames, Ks = synthetic_frames()
    p = CAL.params_from_samples(frames, Ks)
    ref = load_camera_params('SonyA7S2')
    _same_schema(p, ref)
    assert p['G_shape'].shape == (10,) and p['color_bias'].shape == (10, 4) and p['color_bias'].dtype == np.float32
    assert p['Kmin'] == min(Ks) and p['Kmax'] == max(Ks)
    for k in CAL.SIGMA_KEYS:                                          # the law the samples follow comes back (noise 0.05 in log)
        assert abs(p['Profile-1'][k]['slope'] - ref['Profile-1'][k]['slope']) < 0.1


def test_save_load_and_sample_round_trip(tmp_path, monkeypatch, capsys):
    frames, Ks = synthetic_frames(1)
    p = CAL.params_from_samples(frames, Ks)
    rel = os.path.join('camera_params', 'release')
    path = CAL.save_camera_params(p, 'Synth', str(tmp_path / rel))
    assert path == str(tmp_path / rel / 'Synth_params.npy')
    back = np.load(path, allow_pickle=True).item()                    # the reference's own reader
    _same_schema(back, p)
    assert np.array_equal(back['G_shape'], p['G_shape']) and np.array_equal(back['color_bias'], p['color_bias'])
    monkeypatch.chdir(tmp_path)
    loaded = load_camera_params('Synth', rel)
    assert loaded['Profile-1']['R_scale']['bias'] == p['Profile-1']['R_scale']['bias']
    nm = NoiseModel(model='PGRUB', cameras=['Synth'])
    np.random.seed(0)
    for _ in range(5):
        q = nm._sample_params()
        assert np.isfinite([q[0], q[1], q.tl_lambda, q.tl_scale, q.row_scale]).all()
        assert q.tl_lambda in set(p['G_shape'].tolist())
        assert any(np.allclose(q.color_bias, row) for row in p['color_bias'])


def test_argument_errors_before_device_work():
    u = np.zeros((3, 8, 8), np.uint16)
    fl = np.zeros((2, 2, 8, 8), np.uint16)
    pat, blk = [[0, 1], [3, 2]], [0, 0, 0, 0]
    good = [{'iso': 100, 'bias': u, 'flats': fl}, {'iso': 200, 'bias': u, 'flats': fl}]
    with pytest.raises(ValueError, match='even'):
        CAL.bias_frame_stats(np.zeros((1, 7, 8), np.uint16), pat, blk)
    with pytest.raises(ValueError, match='even'):
        CAL.flat_pair_stats(np.zeros((1, 2, 8, 9), np.uint16), pat, blk, 1023, [0] * 4)
    for bad in ([[0, 1], [1, 2]], [[0, 1], [2, 4]], [0, 1, 2]):
        with pytest.raises(ValueError, match='permutation'):
            CAL.bias_frame_stats(u, bad, blk)
        with pytest.raises(ValueError, match='permutation'):
            CAL.calibrate_camera(good, bad, blk, 1023)
    with pytest.raises(ValueError, match='shapes differ'):
        CAL.calibrate_camera([{'bias': u, 'flats': np.zeros((2, 2, 8, 10), np.uint16)}] + good, pat, blk, 1023)
    with pytest.raises(ValueError, match='shapes differ'):
        CAL.calibrate_camera(good + [{'bias': np.zeros((1, 10, 8), np.uint16), 'flats': np.zeros((1, 2, 10, 8), np.uint16)}], pat, blk, 1023)
    with pytest.raises(ValueError, match=r'\(P, 2, Hm, Wm\)'):
        CAL.calibrate_camera([{'bias': u, 'flats': np.zeros((2, 3, 8, 8), np.uint16)}] + good, pat, blk, 1023)
    with pytest.raises(ValueError, match='n >= 3'):
        CAL.tukey_lambda_ppcc(np.zeros(2, np.float32))
    with pytest.raises(ValueError, match='3 bias frames'):
        CAL.calibrate_camera([{'bias': u[:1], 'flats': fl}, {'bias': u[:1], 'flats': fl}], pat, blk, 1023)
    with pytest.raises(ValueError, match='2 sessions'):
        CAL.calibrate_camera(good[:1], pat, blk, 1023)
    with pytest.raises(ValueError, match='uint16'):
        CAL.bias_frame_stats(u.astype(np.int32), pat, blk)
    # the checks that need the sums: their host halves
    frames, Ks = synthetic_frames()
    with pytest.raises(ValueError, match='2 distinct K'):
        CAL.params_from_samples([dict(f, K=1.0) for f in frames], [1.0] * 5)
    with pytest.raises(ValueError, match='3 bias frames'):
        CAL.params_from_samples(frames[:2], Ks)
    with pytest.raises(ValueError, match='row-noise sample is 0'):
        CAL.params_from_samples(frames[:3] + [dict(frames[3], R_scale=0.0)], Ks)
    mu, var = np.array([[10.0, 20, 30, 40]]), np.array([[1.0, 2, 3, 4]])
    with pytest.raises(ValueError, match='usable flat'):
        CAL.ptc_gain(mu, var, np.zeros((1, 4), bool))
    with pytest.raises(ValueError, match='usable flat'):
        CAL.ptc_gain(mu, var, np.array([[True, False, False, False]]))
    assert abs(CAL.ptc_gain(mu, var, np.ones((1, 4), bool)) - 0.1) < 1e-12
    with pytest.raises(ValueError, match='m >= 3'):
        CAL.fit_log_linear([1.0, 2.0], [1.0, 2.0])


def test_ppcc_refuses_a_host_tensor():
    """A CPU tensor's host pointer must never reach the kernel: ValueError before any device work."""
    torch = pytest.importorskip('torch')
    with pytest.raises(ValueError, match='CUDA'):
        CAL.tukey_lambda_ppcc(torch.from_numpy(np.arange(10, dtype=np.float32)))
    with pytest.raises(ValueError, match='CUDA'):
        CAL.bias_frame_stats(torch.zeros((1, 4, 4), dtype=torch.int16), [[0, 1], [3, 2]], [0] * 4)


def test_misaligned_mosaics_are_refused_by_the_abi(eld_lib):
    """The row kernels read 32-bit words: a mosaic pointer that is not 4-byte aligned is ELD_EINVAL, decided before any launch."""
    import ctypes
    pat = (ctypes.c_int * 4)(0, 1, 3, 2)
    blk = (ctypes.c_double * 4)(0, 0, 0, 0)
    ws, out = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000)
    for base, rc in ((0x30002, -1), (0x30001, -1)):
        p = ctypes.c_void_p(base)
        assert eld_lib.eld_calib_bias_stats(p, 1, 2, 4, pat, out, out, ws, 1 << 20, None) == rc
        assert eld_lib.eld_calib_flat_stats(p, 1, 2, 4, pat, 16383, out, ws, 1 << 20, None) == rc
        assert eld_lib.eld_calib_bias_residual(p, 1, 2, 4, pat, blk, out, out, out, None) == rc
    assert eld_lib.eld_calib_bias_residual(ctypes.c_void_p(0x30000), 1, 2, 4, pat, blk, out, out, ctypes.c_void_p(0x20004), None) == -1
    assert eld_lib.eld_calib_bias_stats(ctypes.c_void_p(0x30000), 1, 2, 4, pat, out, out, ws, 8, None) == -3   # aligned: on to ELD_EWS
    # a raw_pattern that is no permutation of 0..3 (a repeated code, a code out of range, none at all): refused, aligned or not, empty or not
    u = ctypes.c_void_p(0x30000)
    for bad in ((ctypes.c_int * 4)(0, 1, 1, 2), (ctypes.c_int * 4)(0, 1, 4, 2), (ctypes.c_int * 4)(0, -1, 3, 2), None):
        for F in (1, 0):
            assert eld_lib.eld_calib_bias_stats(u, F, 2, 4, bad, out, out, ws, 1 << 20, None) == -1
            assert eld_lib.eld_calib_flat_stats(u, F, 2, 4, bad, 16383, out, ws, 1 << 20, None) == -1
            assert eld_lib.eld_calib_bias_residual(u, F, 2, 4, bad, blk, out, out, out, None) == -1
    assert eld_lib.eld_calib_bias_stats(u, 0, 2, 4, pat, out, out, ws, 1 << 20, None) == 0
