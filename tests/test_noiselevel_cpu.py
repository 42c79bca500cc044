"""Noise level from a single frame, everything that needs no GPU: the argument checks of eld_tile_noise_sums_u16 (made before any
launch), the NumPy restatement against hand-made cases, the eligibility rules, the estimator's accuracy on the restatement's sums of a
synthetic scene, its errors, and the `--K auto` parser of eld_amd.classical.

Measured with tests/noiselevel_ref.py on tests/noiselevel_scene.py (cases (K, sigma, tex) of CASES, seeds 0..2), worst deviation from
the truth (sigma's truth is sqrt(sigma^2 + 1/12)):
    stride 2 (Bayer, 768 x 1024)            K +2.85 %   sigma 2.61 %     kept 55-92 % of the full tiles, 36-44 points
    stride 3 (green layout, 1536 x 2304)    K +2.68 %   sigma 5.66 %     kept 35-100 %,                  38-45 points
The tests assert 1.5 times these: the margin is for the scene's few realisations, not for the code."""
import ctypes

import numpy as np
import pytest

import noiselevel_ref as R
import noiselevel_scene as SC

BOUNDS = {2: (1.5 * 0.0285, 1.5 * 0.0261), 3: (1.5 * 0.0268, 1.5 * 0.0566)}       # stride -> (K, sigma): 1.5 x the measured worst case
RGGB = [0, 1, 3, 2]


# ---- argument errors (no device work) ---------------------------------------------------------------------------------------------------
def _args(**kw):
    """A valid call with F = 0 (which returns 0 after the value checks) and made-up, aligned device pointers."""
    a = dict(frames=16, F=0, Hm=40, Wm=48, Hc=40, Wc=48, p=2, stride=2, group=RGGB, G=4, black=[512] * 4, white=16383, bitmap=None, out=64,
             ws_bytes=0)
    a.update(kw)
    return a


def _call(lib, **kw):
    a = _args(**kw)
    n = a['p'] * a['p'] if a['p'] in (2, 6) else 4
    grp = None if a['group'] is None else (ctypes.c_int * n)(*a['group'])
    blk = None if a['black'] is None else (ctypes.c_int32 * n)(*a['black'])
    ptr = lambda v: None if v is None else ctypes.c_void_p(v)
    return lib.eld_tile_noise_sums_u16(ptr(a['frames']), a['F'], a['Hm'], a['Wm'], a['Hc'], a['Wc'], a['p'], a['stride'], grp, a['G'], blk, a['white'],
                                       ptr(a['bitmap']), ptr(a['out']), None, a['ws_bytes'], None)


@pytest.mark.parametrize('kw', [dict(p=3), dict(p=4), dict(stride=0), dict(stride=3), dict(stride=-2), dict(p=6, group=[0] * 36, black=[0] * 36, stride=4),
                                dict(p=6, group=[0] * 36, black=[0] * 36, stride=7), dict(G=0), dict(G=5), dict(F=-1), dict(F=65536), dict(Hm=-1, Hc=0),
                                dict(Wm=-1, Wc=0), dict(Hc=41), dict(Wc=49), dict(Hc=-1), dict(Wc=-1), dict(Hm=1 << 16, Wm=1 << 15, Hc=8, Wc=8),
                                dict(group=[0, 1, 4, 2]), dict(group=[0, -2, 3, 2]), dict(G=3), dict(black=[512, -1, 512, 512]),
                                dict(black=[512, 512, 65536, 512]), dict(white=0), dict(white=65537), dict(group=None), dict(black=None),
                                dict(F=1, frames=None), dict(F=1, out=None), dict(F=1, frames=17), dict(F=1, out=68), dict(F=1, bitmap=18)])
def test_argument_errors(eld_lib, kw):
    assert _call(eld_lib) == 0                                   # the base call is valid: each case is refused for its own fault
    assert _call(eld_lib, **kw) == -1, kw                        # ELD_EINVAL, before any launch: the "device pointers" are made-up numbers


def test_empty_calls_and_workspace(eld_lib):
    assert _call(eld_lib, F=0, frames=None, out=None) == 0
    assert _call(eld_lib, F=1, Hm=4, Hc=4, frames=None, out=None) == 0            # Hc <= 2 s: no tile rows
    assert _call(eld_lib, F=1, Wc=4, frames=None, out=None) == 0
    assert _call(eld_lib, F=1, Hm=0, Hc=0, Wm=0, Wc=0, frames=None, out=None) == 0
    need = eld_lib.eld_tile_noise_workspace_bytes(1, 40, 48)
    if need:                                                                      # a short workspace is refused (this build needs none)
        assert _call(eld_lib, ws_bytes=need - 1) == -3
    assert need == 0


# ---- the restatement against hand-made cases --------------------------------------------------------------------------------------------
def _full_count(Hc, Wc, s):
    return (Hc - 2 * s) * (Wc - 2 * s)


def test_constant_frame():
    Hm, Wm, c = 40, 70, 900
    black = [512, 520, 500, 505]
    out = R.tile_sums_ref(np.full((Hm, Wm), c, np.uint16), Hm, Wm, 2, 2, RGGB, 4, black, 16383)
    assert out.shape == (1, 2, 3, 4, 4)
    assert np.all(out[..., 2:] == 0)
    assert int(out[..., 0].sum()) == _full_count(Hm, Wm, 2)
    for cell, g in enumerate(RGGB):                                               # every position: S = 9 n (c - black)
        assert np.array_equal(out[..., g, 1], 9 * out[..., g, 0] * (c - black[cell]))
    assert np.array_equal(out[0, 0, 0, :, 0], [256] * 4) and np.array_equal(out[0, 1, 2, :, 0], [2 * 1] * 4)     # 4 x 2 sites in the last tile


@pytest.mark.parametrize('p,s,group,G', [(2, 2, RGGB, 4), (6, 3, list(SC.XT_GREEN), 3), (6, 6, list(SC.XT_COLOUR.reshape(-1)), 3)])
def test_integer_plane(p, s, group, G):
    a, b, c = 3, -2, 700
    Hm, Wm = 60, 66
    y, x = np.mgrid[:Hm, :Wm]
    out = R.tile_sums_ref((a * y + b * x + c).astype(np.uint16), Hm, Wm, p, s, group, G, [100] * (p * p), 16383)
    n = out[..., 0]
    assert n.sum() > 0 and np.all(out[..., 2] == 0)
    assert np.array_equal(out[..., 3], n * 4 * s * s * (a * a + b * b))


def test_one_neighbourhood_by_hand():
    v = np.array([[10, 20, 35], [50, 90, 40], [70, 25, 15]])
    fr = np.zeros((6, 6), np.uint16)
    fr[0::2, 0::2] = v                                                            # the one eligible site is (2, 2): every other one meets a 0
    out = R.tile_sums_ref(fr, 6, 6, 2, 2, [0, 1, 2, 3], 4, [3, 0, 0, 0], 16383)
    r = 10 - 2 * 20 + 35 - 2 * 50 + 4 * 90 - 2 * 40 + 70 - 2 * 25 + 15            # 220
    assert out.shape == (1, 1, 1, 4, 4)
    assert out[0, 0, 0, 0].tolist() == [1, int(v.sum()) - 27, r * r, (40 - 50) ** 2 + (25 - 20) ** 2]
    assert not out[0, 0, 0, 1:].any()


# ---- eligibility --------------------------------------------------------------------------------------------------------------------------
def _noise_frame(Hm=44, Wm=52, seed=3):
    return np.random.default_rng(seed).integers(600, 3000, size=(Hm, Wm)).astype(np.uint16)


@pytest.mark.parametrize('what', ['zero', 'white', 'flag'])
def test_one_bad_site_removes_its_nine(what):
    fr = _noise_frame()
    Hm, Wm = fr.shape
    base = R.tile_sums_ref(fr, Hm, Wm, 2, 2, RGGB, 4, [512] * 4, 16383)
    mask = None
    if what == 'flag':
        mask = np.zeros((Hm, Wm), bool)
        mask[20, 31] = True
    else:
        fr = fr.copy()
        fr[20, 31] = 0 if what == 'zero' else 16383
    out = R.tile_sums_ref(fr, Hm, Wm, 2, 2, RGGB, 4, [512] * 4, 16383, mask)
    g = RGGB[(20 % 2) * 2 + 31 % 2]
    d = base[..., 0] - out[..., 0]
    assert int(d.sum()) == 9 and int(d[..., g].sum()) == 9                        # the nine sites whose neighbourhood holds (20, 31)
    # ... and exactly those: removing them by hand from the clean frame's statistics gives the same sums
    lost = np.zeros_like(base)
    for dy in (-2, 0, 2):
        for dx in (-2, 0, 2):
            lost += R.tile_sums_ref(_noise_frame(), Hm, Wm, 2, 2, RGGB, 4, [512] * 4, 16383, _centre_only(Hm, Wm, 20 + dy, 31 + dx))
    assert np.array_equal(base - out, lost)


def _centre_only(Hm, Wm, y, x):
    """A mask that flags everything outside the 3 x 3 (stride 2) neighbourhood of (y, x): only that site stays eligible."""
    m = np.ones((Hm, Wm), bool)
    m[y - 2:y + 3:2, x - 2:x + 3:2] = False
    return m


def test_uncounted_group_and_wrong_stride():
    fr = _noise_frame()
    Hm, Wm = fr.shape
    base = R.tile_sums_ref(fr, Hm, Wm, 2, 2, RGGB, 4, [512] * 4, 16383)
    out = R.tile_sums_ref(fr, Hm, Wm, 2, 2, [0, -1, 3, 2], 4, [512] * 4, 16383)
    assert not out[..., 1, :].any() and np.array_equal(out[..., [0, 2, 3], :], base[..., [0, 2, 3], :])
    one = R.tile_sums_ref(fr, Hm, Wm, 2, 1, RGGB, 4, [512] * 4, 16383)            # Bayer at stride 1: the neighbours have other colours
    assert one.shape == (1, 3, 4, 4, 4) and not one.any()


# ---- the estimator ------------------------------------------------------------------------------------------------------------------------
def _estimate(u, p, s, group, G):
    from eld_amd.noiselevel import TileSums, estimate_noise
    Hm, Wm = u.shape
    sums = R.tile_sums_ref(u, Hm, Wm, p, s, group, G, [SC.BLACK] * (p * p), SC.WHITE)
    return estimate_noise(TileSums(sums, p, s, group, G, (Hm, Wm)))


@pytest.mark.parametrize('K,sigma,tex', SC.CASES)
@pytest.mark.parametrize('stride', [2, 3])
def test_accuracy_on_the_synthetic_scene(stride, K, sigma, tex):
    bK, bS = BOUNDS[stride]
    for seed in range(3):
        if stride == 2:
            est = _estimate(SC.synth_frame(K, sigma, tex, seed), 2, 2, RGGB, 4)
        else:
            est = _estimate(SC.synth_frame(K, sigma, tex, seed, 1536, 2304, colour=False), 6, 3, list(SC.XT_GREEN), 3)
        dK, dS = est.K / K - 1.0, est.sigma / np.sqrt(sigma * sigma + 1.0 / 12.0) - 1.0
        print('stride %d K %g sigma %g tex %g seed %d: K %+.2f %% sigma %+.2f %% kept %.2f (full tiles %.2f) points %d'
              % (stride, K, sigma, tex, seed, 100 * dK, 100 * dS, est.kept_share, est.full_kept_share, len(est.points['bin'])))
        assert abs(dK) <= bK and abs(dS) <= bS
        assert est.full_kept_share >= 0.30 and len(est.points['bin']) >= 30
        assert not est.negative_intercept and est.sigma0_sq == pytest.approx(est.sigma ** 2)
        if stride == 2:                                                           # every Bayer position carries its own line
            assert sorted(est.groups) == [0, 1, 2, 3]
            assert all(abs(d['K'] / K - 1.0) < 0.10 for d in est.groups.values())


def test_estimator_errors():
    from eld_amd.noiselevel import TileSums, estimate_noise
    rng = np.random.default_rng(0)
    flat = np.clip(np.rint(2.0 * rng.poisson(800.0, (768, 1024)) + 3.0 * rng.standard_normal((768, 1024)) + 512), 0, 16383).astype(np.uint16)
    with pytest.raises(ValueError, match='one level|one signal level'):           # a flat grey frame: all tiles in one or two bins
        _estimate(flat, 2, 2, RGGB, 4)
    with pytest.raises(ValueError, match='fewer than four usable points'):        # a tiny frame: no bin reaches min_sites
        _estimate(SC.synth_frame(2.0, 3.0, 0.0, 0, 64, 96), 2, 2, RGGB, 4)
    sums = R.tile_sums_ref(SC.synth_frame(2.0, 3.0, 0.0, 0, 128, 256), 128, 256, 2, 2, RGGB, 4, [512] * 4, 16383)
    for bad in (dict(ratio=(3, 0)), dict(ratio=(1.5, 1)), dict(ratio=3), dict(ratio=(2000, 1)), dict(min_fill=0.0), dict(min_fill=1.5), dict(min_sites=0)):
        with pytest.raises(ValueError):
            estimate_noise(TileSums(sums, 2, 2, RGGB, 4), **bad)
    with pytest.raises(ValueError):
        TileSums(sums, 2, 3, RGGB, 4)
    with pytest.raises(ValueError):
        TileSums(sums[..., :3], 2, 2, RGGB, 4)


def test_tile_sums_refuses_on_the_host(eld_lib):
    from eld_amd.noiselevel import tile_sums
    fr = np.zeros((40, 48), np.uint16)
    for kw in (dict(stride=3), dict(stride=0), dict(stride=True), dict(green_only=True), dict(cfa='foveon'), dict(white_level=0),
               dict(black_level=[1, 2, 3]), dict(cfa='xtrans', stride=4), dict(defects=3)):
        with pytest.raises(ValueError):
            tile_sums(fr, **kw)
    with pytest.raises(ValueError):
        tile_sums(fr.astype(np.int32))


def test_level_bins_follow_the_kernel_rule():
    from eld_amd.noiselevel import level_bins
    import pairstats_ref as P
    s = np.concatenate([np.arange(-5, 300), [1023, 1024, 4095, 4096, 20000, 65535]])
    assert np.array_equal(level_bins(s), [P.bin_loop(int(v), 0, 1 << 20) for v in s])


def test_burst_gain_is_unchanged_by_the_shared_line():
    """burst_gain through weighted_line against the arithmetic it had before, written out: equal to the bit."""
    from eld_amd.burst import NB, burst_gain
    rng = np.random.default_rng(5)
    ptc = np.zeros((4, NB, 4), np.int64)
    N = 8
    for g in range(4):
        for b in range(3, 50):
            n = int(rng.integers(100, 5000))
            mu = 3.0 * 2 ** (b / 4.0)
            V = int(n * N * (N - 1) * (1.7 * mu + 9.0) * rng.uniform(0.95, 1.05))
            ptc[g, b] = (n, int(n * N * (mu + 512)), V & 0xFFFFFFFF, V >> 32)
    st = {'ptc': ptc, 'N': N, 'group_black': [512.0] * 4}
    fit = burst_gain(st)
    n, mu, var = fit['n'].astype(np.float64), fit['mu'], fit['var']
    w = n / (var * var)
    sw = float(np.sum(w))
    mw, vw = float(np.sum(w * mu) / sw), float(np.sum(w * var) / sw)
    K = float(np.sum(w * (mu - mw) * (var - vw)) / float(np.sum(w * (mu - mw) ** 2)))
    assert fit['K'] == K and fit['sigma0_sq'] == vw - K * mw


# ---- python -m eld_amd.classical --K auto ---------------------------------------------------------------------------------------------------
def test_classical_parser_takes_auto():
    from eld_amd.classical import build_parser
    p = build_parser()
    base = ['a.npy', '-o', 'out']
    assert p.parse_args(base + ['--K', 'auto']).K == 'auto'
    k = p.parse_args(base + ['--K', '2.1']).K
    assert k == 2.1 and isinstance(k, float)
    with pytest.raises(SystemExit):
        p.parse_args(base + ['--K', 'abc'])
    with pytest.raises(SystemExit):
        p.parse_args(base)                                                        # --K is still required
