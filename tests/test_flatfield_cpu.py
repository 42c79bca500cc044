"""Flat-field maps without a GPU: exact properties and the recovery of planted gains on the NumPy restatement (tests/flatfield_ref.py), and the
host logic of eld_amd/flatfield.py -- the file format, the argument errors (all before any device work) and the command lines."""
import math
import types

import numpy as np
import pytest

import flatfield_ref as R
from eld_amd import flatfield as FF

PAT = [[0, 1], [3, 2]]
COL2 = R.CODE_COLOUR[np.asarray(PAT)]              # R G / G B
CEN2 = np.full((2, 2), 512)


def _pairs(frame, F):
    return np.repeat(frame[None], F, axis=0).astype(np.uint16)


def _ones(x):
    return np.array_equal(x.view(np.int32), np.full(x.shape, np.float32(1).view(np.int32)))


# ---- the restatement itself -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('p,shape,radius', [(2, (6, 10), 0), (2, (6, 10), 1), (2, (10, 12), 3), (6, (14, 20), 1), (6, (12, 18), 4)])
def test_box_by_prefix_sums_is_the_box_by_definition(p, shape, radius):
    rng = np.random.default_rng(radius + shape[0])
    S = rng.integers(0, 2 ** 32, size=shape, dtype=np.int64)
    bad = rng.random(shape) < 0.2
    a, b = R.box(S, bad, p, radius), R.box_brute(S, bad, p, radius)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_bitmap_layout_is_the_defect_bitmaps():
    from eld_amd.defects import pack_bitmap
    rng = np.random.default_rng(1)
    for shape in ((4, 8), (5, 34), (3, 64), (2, 70)):
        m = rng.random(shape) < 0.3
        assert np.array_equal(R.pack_bitmap(m), pack_bitmap(m))


# ---- exact properties -------------------------------------------------------------------------------------------------------------------------
def test_constant_flats_give_unit_maps():
    for cen, col, shape in ((CEN2, COL2, (12, 16)), (np.full((6, 6), 1024), np.arange(36).reshape(6, 6) % 3, (14, 20))):
        m = R.fit(_pairs(np.full(shape, 3000), 6), cen, col, radius=2)
        assert _ones(m['lens']) and _ones(m['prnu']) and m['invalid'] == 0


def test_doubling_one_colour_leaves_both_planes_at_one():
    """Every position plane is normalised by its own colour: a colour at twice the signal is not a gain."""
    frame = np.full((12, 16), 512 + 1000)
    frame[0::2, 0::2] = 512 + 2000                   # R
    m = R.fit(_pairs(frame, 4), CEN2, COL2, radius=3)
    assert _ones(m['lens']) and _ones(m['prnu'])
    assert m['report']['R']['falloff'] == 1.0 and m['report']['G']['prnu_sigma'] == 0.0


def test_one_site_at_five_quarters_of_its_neighbours():
    frame = np.full((20, 24), 512 + 1000)
    y, x = 8, 10                                     # an R site, its window whole at radius 2
    frame[y, x] = 512 + 1250
    F, rad = 4, 2
    m = R.fit(_pairs(frame, F), CEN2, COL2, radius=rad)
    n = (2 * rad + 1) ** 2
    V = np.float64(n * 1000 + 250) / np.float64(n)   # the window holds the site itself: nothing is excluded
    assert m['V'][y, x] == (n * F * 1000 + F * 250) / (n * F) and abs(m['V'][y, x] - V) < 1e-12
    assert m['prnu'][y, x] == np.float32(m['V'][y, x] / 1250.0) and m['r'][y, x] == 1250.0
    S, D, bad = R.sums(_pairs(frame, F), 16383)
    _, Bcnt = R.box(S, bad, 2, rad)
    assert Bcnt[y, x] == n and Bcnt[y, x + 2] == n and Bcnt[0, 0] == (rad + 1) ** 2
    assert m['V'][y, x + 2] == m['V'][y, x]           # the neighbour's window holds the hot site too
    assert m['prnu'][y, x + 2] == np.float32(m['V'][y, x] / 1000.0)
    assert m['V'][y, x + 1] == 1000.0 and m['prnu'][y, x + 1] == 1.0          # another position plane does not see it


def test_a_bad_site_stays_out_of_its_neighbours_windows_and_is_one():
    frame = np.full((20, 24), 512 + 1000)
    y, x = 8, 10
    frame[y, x] = 16383                              # saturated: bad by its code
    mask = np.zeros(frame.shape, bool)
    mask[9, 11] = True                               # bad by the defect map, a B site with an ordinary code
    frame[9, 11] = 512 + 4000
    m = R.fit(_pairs(frame, 4), CEN2, COL2, white=16383, radius=2, mask=mask)
    for (yy, xx) in ((y, x), (9, 11)):
        assert m['lens'][yy, xx] == 1.0 and m['prnu'][yy, xx] == 1.0 and not m['ok'][yy, xx]
    assert m['invalid'] == 2
    good = m['ok']
    assert np.all(m['V'][good] == 1000.0) and _ones(m['prnu']) and _ones(m['lens'])
    S, D, bad = R.sums(_pairs(frame, 4), 16383, mask)
    assert bad.sum() == 2 and R.box(S, bad, 2, 2)[1][y, x + 2] == 24


def test_a_window_wholly_on_bad_sites_gives_one_and_counts_as_invalid():
    frame = np.full((20, 24), 512 + 1000)
    mask = np.zeros(frame.shape, bool)
    mask[4:13:2, 6:15:2] = True                      # 5 x 5 sites of the R plane: the window of the middle one at radius 1 is all bad
    m = R.fit(_pairs(frame, 2), CEN2, COL2, radius=1, mask=mask)
    S, D, bad = R.sums(_pairs(frame, 2), 16383, mask)
    Bsum, Bcnt = R.box(S, bad, 2, 1)
    assert Bcnt[8, 10] == 0 and Bsum[8, 10] == 0 and Bcnt[4, 6] == 5
    assert m['lens'][8, 10] == 1.0 and m['prnu'][8, 10] == 1.0
    assert m['invalid'] == 25 and np.isfinite(m['lens']).all() and np.isfinite(m['prnu']).all()


# ---- recovery ---------------------------------------------------------------------------------------------------------------------------------
def test_a_planted_ramp_comes_back_to_the_quantisation_of_the_codes():
    """Per colour a ramp linear in (y, x), no noise.  Where the window is whole it is symmetric about the site, so the mean of the exact ramp
    over it is the ramp at the site; every code is off the ramp by at most 0.5 DN (rint), so V is off by at most 0.5 DN.  lens = float32(Vref /
    V) adds a relative 2^-24; Vref / lens gives V back within 0.5 DN + 2^-22 of the level (two roundings, with margin)."""
    Hm, Wm, rad = 48, 64, 3
    yy, xx = np.mgrid[0:Hm, 0:Wm].astype(np.float64)
    level = np.empty((Hm, Wm))
    slopes = {0: (3000.0, 9.5, 4.25), 1: (5000.0, -7.75, 6.5), 2: (2000.0, 5.25, -3.5)}
    cmap = R.cell_map(COL2, Hm, Wm)
    for k, (l0, sy, sx) in slopes.items():
        level[cmap == k] = (l0 + sy * yy + sx * xx)[cmap == k]
    m = R.fit(_pairs(np.rint(512 + level), 2), CEN2, COL2, radius=rad)
    inner = np.zeros((Hm, Wm), bool)
    inner[2 * rad:Hm - 2 * rad, 2 * rad:Wm - 2 * rad] = True
    assert np.all(np.abs(m['V'] - level)[inner] <= 0.5)
    back = m['vref'] / m['lens'].astype(np.float64)
    assert np.all(np.abs(back - level)[inner] <= 0.5 + 2.0 ** -22 * level[inner])
    assert m['lens'].min() >= 1.0 and m['invalid'] == 0
    for k, name in enumerate('RGB'):
        v = m['V'][cmap == k]
        assert m['report'][name]['falloff'] == v.min() / v.max()


MU, SIGMA_P, HM, WM = 2000.0, 0.01, 128, 128


def _poisson_flats(F, seed=5):
    rng = np.random.default_rng(seed)
    g = 1.0 + SIGMA_P * rng.standard_normal((HM, WM))
    return g, (512 + rng.poisson(MU * g, size=(F, HM, WM))).astype(np.uint16)


def test_planted_prnu_comes_back_within_five_standard_errors():
    """1 % PRNU under Poisson noise (gain 1 DN per electron, no read noise), F = 16 flats at 2000 DN.  Per colour over N sites:
    rho_var estimates s_p^2 + s_n^2 with the variance of a sample variance, 2 (s_p^2 + s_n^2)^2 / N; noise_var is the mean over N sites of
    D / (F V)^2, and D, a sum of P = F / 2 squared pair differences of variance 2 s^2 each, has relative variance 2 / P, so noise_var has
    variance 2 s_n^4 / (P N); pair sums and pair differences are independent.  x = rho_var - noise_var has the sum of the two variances, and
    sqrt(x) the standard error SE(x) / (2 s_p).  s_n^2 = 1 / (F MU).  The planted value is the standard deviation of the planted gains of
    the colour's own sites."""
    F = 16
    g, frames = _poisson_flats(F)
    m = R.fit(frames, CEN2, COL2, radius=16)
    cmap = R.cell_map(COL2, HM, WM)
    s_n2 = 1.0 / (F * MU)
    for k, name in enumerate('RGB'):
        rep = m['report'][name]
        N, P = rep['sites'], F // 2
        planted = float(np.std(g[cmap == k]))
        tot = planted ** 2 + s_n2
        se = math.sqrt(2 * tot ** 2 / N + 2 * s_n2 ** 2 / (P * N)) / (2 * planted)
        print('%s: prnu_sigma %.6f planted %.6f  se %.6f  noise_var %.4e (theory %.4e)  snr %.3f' % (name, rep['prnu_sigma'], planted, se,
                                                                                                    rep['noise_var'], s_n2, rep['snr']))
        assert N == (HM * WM // 4) * (2 if k == 1 else 1)
        assert abs(rep['prnu_sigma'] - planted) < 5 * se
        # a site's noise variance is g / (F MU): the mean over the colour is s_n^2 times the mean planted gain, 1 +- s_p / sqrt(N)
        assert abs(rep['noise_var'] - s_n2) < 5 * math.sqrt(2 * s_n2 ** 2 / (P * N)) + 5 * s_n2 * SIGMA_P / math.sqrt(N)
        assert rep['snr'] > 1


def test_snr_falls_below_one_where_theory_says_it_must():
    """snr = s_p / s_n with s_n^2 = 1 / (F MU): below 1 iff F < 1 / (MU s_p^2) = 5.  F = 2 gives sqrt(0.4) = 0.63, F = 16 gives 1.79."""
    assert 1.0 / (MU * SIGMA_P ** 2) == pytest.approx(5.0)
    lo = R.fit(_poisson_flats(2)[1], CEN2, COL2, radius=16)['report']
    hi = R.fit(_poisson_flats(16)[1], CEN2, COL2, radius=16)['report']
    for name in 'RGB':
        assert lo[name]['snr'] < 1 < hi[name]['snr']
    ff = FF.FlatField(np.ones((4, 8), np.float32), np.ones((4, 8), np.float32), report=lo)
    assert sum('snr < 1' in line for line in FF.report_lines(ff)) == 3
    assert not any('snr < 1' in line for line in FF.report_lines(FF.FlatField(np.ones((4, 8), np.float32), np.ones((4, 8), np.float32), report=hi)))


# ---- the float paths of the restatement -------------------------------------------------------------------------------------------------------
def test_apply_rounds_ties_to_even_and_passes_bad_sites_through():
    black = np.full((2, 2), 512, np.float32)
    u = np.array([[513, 514, 515, 516, 16383, 700, 65535, 512]], np.uint16).repeat(2, axis=0)
    g = np.array([[0.5, 1.25, 1.5, 1.0, 2.0, 400.0, 1.0, 3.0]], np.float32).repeat(2, axis=0)
    mask = np.zeros(u.shape, bool)
    mask[1, 1] = True
    out = R.apply(u, g, black, 16383, mask)
    # 512.5 -> 512, 514.5 -> 514, 516.5 -> 516 (ties to even), 516 unchanged, a saturated code passes, 188 * 400 clamps, 65535 >= white passes
    assert out[0].tolist() == [512, 514, 516, 516, 16383, 65535, 65535, 512]
    assert out[1, 1] == 514 and R.apply(u, g, black, 16383)[1, 1] == 514 and out[1, 0] == 512
    assert R.apply(np.array([[100, 100]], np.uint16), np.array([[3.0, 1.0]], np.float32), black, 16383)[0].tolist() == [0, 100]     # the lower clamp


# ---- host logic -------------------------------------------------------------------------------------------------------------------------------
def _ff(shape=(6, 8), cfa='bayer', pattern=PAT):
    rng = np.random.default_rng(2)
    rep = {c: {'rho_var': 1e-4, 'noise_var': 2e-5, 'prnu_sigma': 0.009, 'snr': 2.0, 'falloff': 0.7, 'sites': 12} for c in 'RGB'}
    return FF.FlatField(1 + rng.random(shape).astype(np.float32), (1 + 0.01 * rng.standard_normal(shape)).astype(np.float32), cfa, pattern,
                        radius=5, frames=12, white_level=16000, invalid=3, report=rep)


def test_save_load_round_trip(tmp_path):
    m = _ff()
    path = m.save(tmp_path / 'flat')
    assert path.endswith('flat.npz')
    k = FF.FlatField.load(path)
    assert np.array_equal(k.lens.view(np.int32), m.lens.view(np.int32)) and np.array_equal(k.prnu.view(np.int32), m.prnu.view(np.int32))
    assert (k.cfa, k.shape, k.radius, k.frames, k.white_level, k.invalid) == ('bayer', (6, 8), 5, 12, 16000, 3)
    assert np.array_equal(k.raw_pattern, np.asarray(PAT)) and k.report == m.report and k.period == 2
    assert np.array_equal(k.plane('both'), (m.lens * m.prnu).astype(np.float32)) and k.plane('lens') is k.lens
    np.savez(tmp_path / 'other.npz', lens=m.lens)
    with pytest.raises(ValueError, match='not a flat-field map'):
        FF.FlatField.load(tmp_path / 'other.npz')


def test_as_flat_field(tmp_path):
    m = _ff()
    assert FF.as_flat_field(m) is m
    assert FF.as_flat_field(m.save(tmp_path / 'f.npz')).shape == (6, 8)
    with pytest.raises(ValueError, match='no such'):
        FF.as_flat_field(str(tmp_path / 'missing.npz'))
    with pytest.raises(ValueError, match='FlatField'):
        FF.as_flat_field(3)


def test_constructor_refuses_planes_that_are_no_gains():
    one = np.ones((4, 8), np.float32)
    for lens, prnu in ((one, np.ones((4, 6), np.float32)), (np.ones((4, 7), np.float32),) * 2, (one, np.zeros((4, 8), np.float32)),
                       (np.full((4, 8), np.nan, np.float32), one), (one[0], one[0])):
        with pytest.raises(ValueError):
            FF.FlatField(lens, prnu)
    with pytest.raises(ValueError, match='radius'):
        FF.FlatField(one, one, radius=65)
    with pytest.raises(ValueError, match='cfa'):
        FF.FlatField(one, one, cfa='foveon')


def test_checks_of_frames_and_pattern():
    m = _ff()
    m.check_frames((3, 6, 8), 'bayer')
    with pytest.raises(ValueError, match='6 x 8'):
        m.check_frames((6, 10), 'bayer')
    with pytest.raises(ValueError, match='cfa'):
        m.check_frames((6, 8), 'xtrans')
    m.check_pattern(None)
    m.check_pattern(PAT)
    with pytest.raises(ValueError, match='raw_pattern'):
        m.check_pattern([[1, 0], [2, 3]])


def test_fit_refuses_bad_arguments_before_device_work(monkeypatch):
    from eld_amd import framepool
    monkeypatch.setattr(framepool, 'FramePool', lambda *a, **k: (_ for _ in ()).throw(AssertionError('an argument error must come before any upload')))
    flats = np.full((2, 2, 6, 8), 900, np.uint16)
    bias = np.full((3, 6, 8), 512, np.uint16)
    with pytest.raises(ValueError, match="'flats'"):
        FF.fit_flat_field([{'bias': bias}, {'bias': bias, 'iso': 100}])              # sessions without flats are skipped: none is left
    for sessions in ([], None, [3]):
        with pytest.raises(ValueError):
            FF.fit_flat_field(sessions)
    for radius in (-1, 65, 1.5, True, None):
        with pytest.raises(ValueError, match='radius'):
            FF.fit_flat_field([{'flats': flats}], radius=radius)
    with pytest.raises(ValueError, match='one shape'):
        FF.fit_flat_field([{'flats': flats}, {'flats': np.full((1, 2, 6, 10), 900, np.uint16)}])
    with pytest.raises(ValueError, match=r'\(P, 2, Hm, Wm\)'):
        FF.fit_flat_field([{'flats': np.full((2, 3, 6, 8), 900, np.uint16)}])
    with pytest.raises(ValueError, match='uint16'):
        FF.fit_flat_field([{'flats': flats.astype(np.float32)}])
    with pytest.raises(ValueError, match='cfa'):
        FF.fit_flat_field([{'flats': flats}], cfa='foveon')
    with pytest.raises(ValueError, match='raw_pattern'):
        FF.fit_flat_field([{'flats': flats}], raw_pattern=[[0, 1], [1, 2]])
    with pytest.raises(ValueError, match='black_level'):
        FF.fit_flat_field([{'flats': flats}], black_level=[512, 512])
    for white in (0, 70000, 100.5):
        with pytest.raises(ValueError, match='white_level'):
            FF.fit_flat_field([{'flats': flats}], white_level=white)
    from eld_amd.defects import DefectMap
    with pytest.raises(ValueError, match='defect map'):
        FF.fit_flat_field([{'flats': flats}], defects=DefectMap.from_sites([(1, 1)], (6, 10)))
    with pytest.raises(ValueError, match='X-Trans'):
        FF.fit_flat_field([{'flats': np.full((1, 2, 4, 8), 900, np.uint16)}], cfa='xtrans')
    # a session without flats beside one with: only the latter is read (the upload is the first thing after the checks)
    with pytest.raises(AssertionError, match='upload'):
        FF.fit_flat_field([{'bias': bias}, {'flats': flats}])


def test_apply_refuses_bad_arguments_before_device_work():
    m = _ff()
    u = np.full((6, 8), 600, np.uint16)
    for part in ('PRNU', 'all', None, 1):
        with pytest.raises(ValueError, match='part'):
            m.apply(u, part=part)
    with pytest.raises(ValueError, match='6 x 8'):
        m.apply(np.full((6, 10), 600, np.uint16))
    with pytest.raises(ValueError, match='uint16'):
        m.apply(u.astype(np.int32))
    with pytest.raises(ValueError, match='out='):
        m.apply(u, out=np.empty_like(u))
    with pytest.raises(ValueError, match='black_level'):
        m.apply(u, black_level=[1, 2, 3])
    with pytest.raises(ValueError, match='empty'):
        m.apply(np.zeros((0, 6, 8), np.uint16))
    from eld_amd.defects import DefectMap
    with pytest.raises(ValueError, match='defect map'):
        m.apply(u, defects=DefectMap.from_sites([(1, 1)], (6, 10)))


class FakeNet:
    def __init__(self, c):
        self.in_channels = self.out_channels = c

    def parameters(self):
        raise AssertionError('an argument error must come before any device work')


def test_denoise_raw_checks_the_map_before_device_work():
    from eld_amd.denoise import denoise_raw
    den = types.SimpleNamespace(cfa='bayer', in_channels=4, out_channels=4, net=FakeNet(4))
    raw = np.full((6, 8), 600, np.uint16)
    m = _ff()
    for lens in ('SRGB', 'on', None, 1):
        with pytest.raises(ValueError, match='lens'):
            denoise_raw(den, raw, 'bayer', flatfield=m, lens=lens)
    with pytest.raises(ValueError, match='lens'):
        denoise_raw(den, raw, 'bayer', lens='both')                                    # checked with or without a map
    with pytest.raises(ValueError, match='6 x 8'):
        denoise_raw(den, np.full((6, 10), 600, np.uint16), 'bayer', flatfield=m)
    with pytest.raises(ValueError, match='raw_pattern'):
        denoise_raw(den, raw, 'bayer', raw_pattern=[[1, 0], [2, 3]], flatfield=m)
    with pytest.raises(ValueError, match='cfa'):
        denoise_raw(types.SimpleNamespace(cfa='xtrans', in_channels=9, out_channels=9, net=FakeNet(9)), raw, 'xtrans', flatfield=m)
    with pytest.raises(ValueError, match='FlatField'):
        denoise_raw(den, raw, 'bayer', flatfield=3)
    with pytest.raises(AssertionError, match='device work'):
        denoise_raw(den, raw, 'bayer', flatfield=m, lens='all')                        # good arguments reach the device


def test_pool_and_evaluation_check_the_map_before_upload():
    from eld_amd.evaluate import evaluate_pairs
    from eld_amd.framepool import FramePool
    m = _ff()
    with pytest.raises(ValueError, match='6 x 8'):
        FramePool([np.full((6, 10), 600, np.uint16)], flatfield=m)
    with pytest.raises(ValueError, match='raw_pattern'):
        FramePool([np.full((6, 8), 600, np.uint16)], raw_pattern=[[1, 0], [2, 3]], flatfield=m)
    with pytest.raises(ValueError, match='FlatField'):
        FramePool([np.full((6, 8), 600, np.uint16)], flatfield=3)
    den = types.SimpleNamespace(cfa='bayer', in_channels=4, out_channels=4, net=FakeNet(4))
    pair = {'short': np.full((6, 10), 600, np.uint16), 'long': np.full((6, 10), 900, np.uint16), 'ratio': 100}
    with pytest.raises(ValueError, match='6 x 8'):
        evaluate_pairs(den, [pair], 'bayer', flatfield=m)


def test_command_lines(tmp_path):
    from eld_amd import denoise, evaluate, train_frames
    a = FF.build_parser().parse_args(['m.json', '-o', 'flat.npz'])
    assert (a.manifest, a.out, a.radius, a.defects) == ('m.json', 'flat.npz', 16, None)
    a = FF.build_parser().parse_args(['m.json', '-o', 'flat.npz', '--radius', '4', '--defects', 'd.npz'])
    assert (a.radius, a.defects) == (4, 'd.npz')
    with pytest.raises(SystemExit):
        FF.build_parser().parse_args(['m.json'])
    with pytest.raises(ValueError, match='radius'):
        FF.main(['m.json', '-o', 'flat.npz', '--radius', '65'])                          # before the manifest is opened
    base = ['in.npy', '-o', 'out', '--ckpt', 'm.pt']
    o = denoise.parse_args(base)[3]
    assert 'flatfield' not in o and 'lens' not in o
    o = denoise.parse_args(base + ['--flatfield', 'f.npz', '--lens', 'all'])[3]
    assert o['flatfield'] == 'f.npz' and o['lens'] == 'all'
    assert 'lens' not in denoise.parse_args(base + ['--flatfield', 'f.npz'])[3]         # main() then takes the default, 'srgb'
    with pytest.raises(ValueError, match='--flatfield'):
        denoise.parse_args(base + ['--lens', 'off'])
    with pytest.raises(SystemExit):
        denoise.parse_args(base + ['--flatfield', 'f.npz', '--lens', 'both'])
    (tmp_path / 'side.json').write_text('{"flatfield": "f.npz", "lens": "off"}')
    o = denoise.parse_args(base + ['--meta', str(tmp_path / 'side.json')])[3]
    assert o['flatfield'] == str(tmp_path / 'f.npz') and o['lens'] == 'off'
    (tmp_path / 'bad.json').write_text('{"flatfield": "f.npz", "lens": "both"}')
    with pytest.raises(ValueError, match='lens'):
        denoise.parse_args(base + ['--meta', str(tmp_path / 'bad.json')])
    a = train_frames.build_parser().parse_args(['f.npy', '-o', 'm.pt'])
    assert a.flatfield is None
    assert train_frames.build_parser().parse_args(['f.npy', '-o', 'm.pt', '--flatfield', 'f.npz']).flatfield == 'f.npz'
    assert evaluate.build_parser().parse_args(['p.json', '--ckpt', 'm.pt']).flatfield is None
    assert evaluate.build_parser().parse_args(['p.json', '--ckpt', 'm.pt', '--flatfield', 'f.npz']).flatfield == 'f.npz'
    assert 'flatfield' in evaluate.OPTION_KEYS
