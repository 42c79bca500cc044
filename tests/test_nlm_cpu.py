"""CPU tests of the classical baseline: the two NumPy forms of the kernel's contract agree, the table builders have the
properties the contract relies on, the C entry refuses bad arguments before any device work, and the reference pipeline alone denoises."""
import ctypes
import math

import numpy as np
import pytest

import nlm_ref as R


def _noisy_x(N, C, h, w, seed, K=2.0, sigma=3.0, black=512):
    """codes / 65535 of a noisy synthetic scene: the distances then spread over the weight table"""
    clean = R.scene_planes(C, h, w)
    codes = np.stack([R.noisy_codes(clean, K, sigma, black, 16383, seed + n) for n in range(N)])
    return (codes.astype(np.float32) / np.float32(65535.0)).astype(np.float32)


@pytest.mark.parametrize('S', [0, 1, 3])
@pytest.mark.parametrize('P', [0, 1, 2])
def test_direct_and_cumulative_forms_agree(S, P):
    for (N, C, h, w), seed in (((1, 1, 1, 1), 1), ((2, 3, 3, 5), 2), ((1, 4, 7, 9), 3), ((1, 2, 1, 7), 4)):
        x = _noisy_x(N, C, h, w, seed)
        fwd = R.vst_tables(2.0, 3.0, [512] * C)
        sh, wtab = R.nlm_weight_table(C, P, 0.5)
        for frac in (0, 4):
            sa, sb = set(), set()
            a = R.nlm_direct(x, 65535.0, fwd, S, P, sh, wtab, frac, sa)
            b = R.nlm_cumsum(x, 65535.0, fwd, S, P, sh, wtab, frac, sb)
            assert a.dtype == b.dtype == np.int32 and np.array_equal(a, b), (S, P, N, C, h, w, frac)
            assert sa == sb
    # a coarse table with every weight different: a wrong bin shows
    x = _noisy_x(1, 3, 6, 7, 9)
    fwd = R.vst_tables(2.0, 3.0, [500, 512, 520])
    wtab = np.arange(255, -1, -1).astype(np.uint16)
    wtab[wtab == 0] = 1
    for sh in (0, 6, 9):
        assert np.array_equal(R.nlm_direct(x, 65535.0, fwd, S, P, sh, wtab, 8), R.nlm_cumsum(x, 65535.0, fwd, S, P, sh, wtab, 8))


def test_s0_returns_the_stabilised_code():
    x = _noisy_x(1, 4, 5, 6, 11)
    fwd = R.vst_tables(2.0, 3.0, [512] * 4)
    sh, wtab = R.nlm_weight_table(4, 2, 0.5)
    v = R.stabilised(x, 65535.0, fwd)
    assert np.array_equal(R.nlm_cumsum(x, 65535.0, fwd, 0, 2, sh, wtab, 4), (v << 4).astype(np.int32))      # (2 (255 v << 4) + 255) // 510


def test_codes_of_bad_inputs():
    x = np.array([np.nan, -1.0, -0.0, 0.5 / 65535, 1.5 / 65535, 2.5 / 65535, 1.0, 2.0, np.inf, -np.inf], np.float32)
    assert R.codes_of(x, 65535.0).tolist() == [0, 0, 0, 0, 2, 2, 65535, 65535, 65535, 0]               # ties to even; clamped; NaN -> 0


def test_weight_table_properties():
    from eld_amd import classical as Cl
    for C, P, strength in ((4, 2, 0.5), (9, 2, 0.5), (4, 0, 0.5), (1, 0, 0.25), (16, 3, 1.0), (4, 1, 2.0)):
        sh, wt = R.nlm_weight_table(C, P, strength)
        sh2, wt2 = Cl.nlm_weight_table(C, P, strength)
        assert sh == sh2 and np.array_equal(wt, wt2) and wt2.dtype == np.uint16 and wt2.shape == (256,)
        n = C * (2 * P + 1) ** 2
        top = 2 * 256 * n + strength ** 2 * 256 * n * math.log(510.0)
        assert (256 << sh) >= top and (sh == 0 or (256 << (sh - 1)) < top)                               # the least such shift
        assert 0 <= sh <= 24
        assert np.all(np.diff(wt.astype(np.int64)) <= 0)                                                 # non-increasing
        assert wt[0] == 255 and wt[255] == 0
        assert set(wt.tolist()) - {0, 255}                                                               # a real slope in between
    # hand-computed: C = 1, P = 0, strength = 1 -> n = 1, bias 512, h^2 = 256, top = 512 + 256 ln 510 = 2107.9 -> sh = 4 (4096 >= top > 2048)
    sh, wt = R.nlm_weight_table(1, 0, 1.0)
    assert sh == 4
    assert wt[31] == 255 and wt[32] == round(255 * math.exp(-(32.5 * 16 - 512) / 256.0)) == 247
    assert wt[100] == round(255 * math.exp(-(100.5 * 16 - 512) / 256.0)) == 4
    for bad in ((0, 1, 0.5), (17, 1, 0.5), (4, 4, 0.5), (4, -1, 0.5), (4, 1, 0.0), (4, 1, float('nan'))):
        with pytest.raises(ValueError):
            Cl.nlm_weight_table(*bad)


def test_forward_table_properties():
    from eld_amd import classical as Cl
    K, sigma, blk = 2.0, 3.0, [512, 500, 0, 1024]
    fwd = R.vst_tables(K, sigma, blk)
    got = Cl.vst_tables(K, sigma, blk)
    assert got.dtype == np.uint16 and got.shape == (4, 65536) and np.array_equal(fwd, got)
    assert np.all(np.diff(fwd.astype(np.int64), axis=1) >= 0)                                            # non-decreasing per plane
    for c, b in enumerate(blk):
        zero = b - (0.375 * K * K + sigma * sigma) / K                                                   # the zero of the root: black - 5.25
        below = np.arange(65536) <= math.floor(zero)
        assert np.all(fwd[c][below] == 0)
        first = int(math.floor(zero)) + 1
        if first >= 0:
            assert fwd[c][first] > 0
    # hand-computed: at the black level the argument is 3/8 K^2 + sigma^2 = 10.5: 16 * (2 / 2) * sqrt(10.5) = 51.85 -> 52
    assert fwd[0][512] == 52 and fwd[1][500] == 52 and fwd[2][0] == 52
    # one more DN of signal at the black level: sqrt(12.5) * 16 = 56.57 -> 57; far above it the slope is Q / sqrt(K s): one sigma = 16 codes
    assert fwd[0][513] == 57
    s = 10000.0
    step = math.sqrt(K * s + 10.5)
    assert abs((float(fwd[0][512 + int(s + step)]) - float(fwd[0][512 + int(s)])) - 16.0) <= 1.0
    # saturation of the table itself: a tiny gain
    assert R.vst_tables(0.01, 0.0, [0]).max() == 32767
    for bad in ((0.0, 1.0), (-1.0, 1.0), (2.0, -1.0), (float('inf'), 1.0)):
        with pytest.raises(ValueError):
            Cl.vst_tables(bad[0], bad[1], [512])


def test_unbiased_inverse_matches_the_restatement_and_inverts_the_mean():
    import torch
    from eld_amd import classical as Cl
    out = np.arange(0, 40000, 37, dtype=np.int32)
    for K, sigma in ((2.0, 3.0), (0.5, 8.0), (6.0, 1.5)):
        ref = R.unbiased_inverse(out, 4, K, sigma)
        got = Cl.unbiased_inverse(torch.from_numpy(out), 4, K, sigma)
        assert got.dtype == torch.float64
        np.testing.assert_allclose(got.numpy(), ref, rtol=1e-14, atol=1e-12)
        assert np.all(np.diff(ref) >= 0)
        # the algebraic inverse of D = 2 / K sqrt(K y + 3/8 K^2 + sigma^2) is K (D^2 / 4 - 3/8 - s^2); the unbiased one answers the MEAN of
        # the transformed samples, which lies below the transform of the mean: its constant is -1/8, so on D itself it returns y + K / 4
        y = 5000.0
        D = 2.0 / K * math.sqrt(K * y + 0.375 * K * K + sigma * sigma)
        assert abs(float(R.unbiased_inverse(np.array([D * 16 * 16]), 4, K, sigma)[0]) - (y + K / 4.0)) < 0.01 * K
        # and on the mean of transformed Poisson-Gaussian samples it returns the signal: 400000 samples put the mean of D within
        # 1 / sqrt(400000) = 0.0016 of a unit-variance quantity, about 0.0016 * sqrt(K y + sigma^2) DN after the inverse
        rng = np.random.default_rng(7)
        for y in (4.0, 40.0):
            x = K * rng.poisson(y / K, 400000) + sigma * rng.standard_normal(400000)
            Dbar = float(np.mean(2.0 / K * np.sqrt(np.maximum(K * x + 0.375 * K * K + sigma * sigma, 0.0))))
            z = float(R.unbiased_inverse(np.array([Dbar * 16 * 16]), 4, K, sigma)[0])
            assert abs(z - y) < 0.03 * y + 5 * 0.0016 * math.sqrt(K * y + sigma * sigma), (K, sigma, y, z)


def test_argument_errors_without_gpu(eld_lib):
    """Every range of the header, refused before any device work (a fake, non-null pointer is never dereferenced)."""
    wt = (ctypes.c_uint16 * 256)(*([255] * 256))
    p = ctypes.c_void_p(4096)
    ok = dict(N=1, C=4, h=8, w=8, S=7, P=2, sh=9, frac=4)

    def call(wtab=wt, x=p, fwd=p, out=p, **kw):
        a = dict(ok, **kw)
        return eld_lib.eld_nlm_vst_f32(x, a['N'], a['C'], a['h'], a['w'], 65535.0, fwd, a['S'], a['P'], a['sh'], wtab, a['frac'], out, None)

    for kw in (dict(N=0), dict(N=-1), dict(C=0), dict(C=17), dict(h=0), dict(w=0), dict(h=-3), dict(S=-1), dict(S=11), dict(P=-1), dict(P=4),
               dict(sh=-1), dict(sh=25), dict(frac=-1), dict(frac=9)):
        assert call(**kw) == -1, kw
    assert call(wtab=None) == -1 and call(x=None) == -1 and call(fwd=None) == -1 and call(out=None) == -1
    assert call(x=ctypes.c_void_p(4098)) == -1 and call(out=ctypes.c_void_p(4097)) == -1 and call(fwd=ctypes.c_void_p(4097)) == -1
    big = (ctypes.c_uint16 * 256)(*([255] * 255 + [256]))
    assert call(wtab=big) == -1                                                                          # a weight above 255
    zero = (ctypes.c_uint16 * 256)(*([0] + [255] * 255))
    assert call(wtab=zero) == -1                                                                         # d = 0 must count


def test_classical_denoiser_arguments():
    from eld_amd import classical as Cl
    d = Cl.ClassicalDenoiser('bayer', 2.0, sigma=3.0)
    assert (d.in_channels, d.out_channels, d.search, d.patch, d.strength) == (4, 4, 7, 2, 0.5)
    assert Cl.ClassicalDenoiser('xtrans', 2.0, sigma=3.0).in_channels == 9
    sh, wt = R.nlm_weight_table(4, 2, 0.5)
    assert d.sh == sh and np.array_equal(d.wtab, wt)
    from eld_amd.noise import load_camera_params
    line = load_camera_params('SonyA7S2')['Profile-1']['g_scale']
    want = math.exp(float(line['slope']) * math.log(2.0) + float(line['bias']))
    assert Cl.ClassicalDenoiser('bayer', 2.0, camera='SonyA7S2').sigma == want
    assert Cl.ClassicalDenoiser('bayer', 2.0, camera=load_camera_params('SonyA7S2')).sigma == want
    e = Cl.ClassicalDenoiser('bayer', 2.0, camera='SonyA7S2').with_gain(4.0)
    assert e.K == 4.0 and e.sigma == math.exp(float(line['slope']) * math.log(4.0) + float(line['bias']))
    assert d.with_gain(4.0).sigma == 3.0 and d.with_gain(2.0) is d
    for kw in (dict(K=0.0, sigma=1.0), dict(K=2.0), dict(K=2.0, sigma=-1.0), dict(K=2.0, sigma=1.0, search=11), dict(K=2.0, sigma=1.0, patch=4),
               dict(K=2.0, sigma=1.0, search=1.5), dict(K=2.0, sigma=1.0, strength=0.0), dict(K=2.0, camera='NoSuchCamera')):
        with pytest.raises(ValueError):
            Cl.ClassicalDenoiser('bayer', **kw)
    with pytest.raises(ValueError):
        Cl.ClassicalDenoiser('foveon', 2.0, sigma=1.0)


def test_command_lines_parse():
    from eld_amd import classical as Cl
    from eld_amd import evaluate as E
    a = Cl.build_parser().parse_args(['a.npy', 'b.npy', '-o', 'out', '--K', '2.5', '--camera', 'SonyA7S2', '--black', '512', '--ratio', '100'])
    assert a.K == 2.5 and a.sigma is None and a.camera == 'SonyA7S2' and (a.search, a.patch, a.strength) == (7, 2, 0.5) and a.ckpt is None
    with pytest.raises(SystemExit):
        Cl.build_parser().parse_args(['a.npy', '-o', 'out'])                                             # --K is required
    p = E.build_parser()
    a = p.parse_args(['pairs.json', '--ckpt', 'net.pt'])
    assert a.baseline_K is None
    a = p.parse_args(['pairs.json', '--ckpt', 'net.pt', '--baseline-K', '2', '--baseline-sigma', '3', '--baseline-search', '5'])
    assert (a.baseline_K, a.baseline_sigma, a.baseline_search, a.baseline_patch, a.baseline_strength) == (2.0, 3.0, 5, 2, 0.5)
    assert 'K' in E.PAIR_KEYS


def test_reference_pipeline_gains_6_db():
    """The NumPy pipeline alone on the synthetic scene: sinusoid + 16-pixel checkerboard + ramp at 0.05 to 7 DN, K = 2, sigma = 3, ratio 100,
    codes at black 512.  Measured here: +12.4 dB (4 planes); the bound leaves room for the seed."""
    K, sigma, black, white, ratio = 2.0, 3.0, 512, 16383, 100.0
    clean = R.scene_planes(4, 64, 64)
    assert clean.min() >= 0.05 and clean.max() <= 7.0
    codes = R.noisy_codes(clean, K, sigma, black, white, 5)[None]
    out = R.denoise_planes(codes, K, sigma, [black] * 4, white, ratio, search=7, patch=2, strength=0.5)
    target = clean * ratio / (white - black)
    clipped = np.clip((codes[0].astype(np.float64) - black) / (white - black) * ratio, 0.0, 1.0)
    gain = R.psnr(out[0], target) - R.psnr(clipped, target)
    print('PSNR in %.2f dB, out %.2f dB, gain %.2f dB' % (R.psnr(clipped, target), R.psnr(out[0], target), gain))
    assert gain >= 6.0
    # unbiased where the clip is not: the mean of the output is the mean of the scene to a few percent, the clipped input's is far above it
    assert abs(float(out[0].mean()) / float(target.mean()) - 1.0) < 0.05
    # (a Gaussian of mean m = 2.9 DN and deviation s = sqrt(K m + sigma^2) = 3.9 DN clipped at 0 has mean m Phi(m / s) + s phi(m / s) = 1.18 m)
    assert float(clipped.mean()) / float(target.mean()) > 1.1
