"""Dark shading without a GPU: the host's coefficient formulas, the closed loop of DESIGN.md sec. 18 on the NumPy restatement
(tests/shading_ref.py), DarkShading's behaviour and the argument errors of the wiring."""
import math
import types

import numpy as np
import pytest

import shading_ref as R
from eld_amd import shading as SH

PAT = [[0, 1], [3, 2]]


# ---- coefficients ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('isos,w', [((800, 1600, 3200), (8, 8, 8)), ((100, 400, 1600, 6400, 12800), (2, 3, 8, 5, 2)),
                                    ((800, 3200), (1.5, 0.25)), ((800, 800, 3200), (2, 2, 4))])
def test_coefficients_reproduce_a_weighted_polyfit(isos, w):
    rng = np.random.default_rng(3)
    x0, alpha, beta = SH.fit_coefficients(isos, w)
    assert (x0, alpha, beta) == R.coefficients(isos, w)                       # the restatement repeats the host, operation for operation
    assert x0 == pytest.approx(np.dot(w, isos) / np.sum(w), rel=1e-15)
    for _ in range(5):
        y = rng.standard_normal(len(isos)) * 10
        slope, icpt = np.polyfit(np.asarray(isos, np.float64) - x0, y, 1, w=np.sqrt(np.asarray(w, np.float64)))
        scale = np.abs(y).max()
        assert abs(np.dot(alpha, y) - icpt) <= 1e-12 * scale
        assert abs(np.dot(beta, y) - slope) <= 1e-12 * scale / (max(isos) - min(isos))


@pytest.mark.parametrize('isos,w', [((1600,), (8,)), ((800, 800), (3, 5))])
def test_coefficients_without_two_distinct_isos(isos, w):
    x0, alpha, beta = SH.fit_coefficients(isos, w)
    assert x0 == isos[0] and beta == [0.0] * len(isos)
    assert alpha == [v / sum(w) for v in w]                                   # the weighted mean of the session means


def test_default_weights_are_the_frame_counts():
    assert SH._weights(None, [(0, 2), (2, 3)]) == [2.0, 3.0]
    assert SH._weights([1, 0.5], [(0, 2), (2, 3)]) == [1.0, 0.5]
    for bad in ([1], [1, 0], [1, -2], [1, float('nan')]):
        with pytest.raises(ValueError):
            SH._weights(bad, [(0, 2), (2, 3)])


# ---- the closed loop on the restatement -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def loop():
    d = R.closed_loop_inputs()
    c = R.LOOP
    x0, alpha, beta = R.coefficients(c['isos'], [c['frames']] * 3)
    a, b = R.fit(d['sessions'], alpha, beta, np.full((2, 2), c['black']))
    d.update(x0=x0, alpha=alpha, beta=beta, a=a, b=b)
    return d


def _predicted(loop, iso):
    c = R.LOOP
    t = iso - loop['x0']
    return sum((al + be * t) ** 2 * (sg ** 2 + 1.0 / 12.0) / c['frames'] for al, be, sg in zip(loop['alpha'], loop['beta'], c['sigmas']))


@pytest.mark.parametrize('iso', [800, 1600, 2400, 3200])
def test_closed_loop_error_of_the_map(loop, iso):
    N = loop['a'].size
    t = np.float32(iso - loop['x0'])
    err = R.step(loop['a'], loop['b'], t).astype(np.float64) - (loop['A'] + loop['B'] * iso)
    pred = _predicted(loop, iso)
    var = float(np.var(err))
    print('iso %d: variance of the map error %.5f, predicted %.5f (%.2f %%)' % (iso, var, pred, 100 * (var / pred - 1)))
    assert abs(var / pred - 1) < 5 * math.sqrt(2.0 / N)
    assert abs(float(err.mean())) < 5 * math.sqrt(pred / N)


def test_held_out_pair_loses_its_fixed_pattern(loop):
    c = R.LOOP
    N = loop['a'].size
    held = loop['held'].astype(np.float64) - c['black']
    before = float(np.mean((held[0] - held[0].mean()) * (held[1] - held[1].mean())))
    fixed = c['a_sigma'] ** 2 + (c['b_sigma'] * 1600 / 3200.0) ** 2
    assert abs(before - fixed) < 5 * (3.5 ** 2 + fixed) / math.sqrt(N)         # the plant: 4.5 DN^2
    cor = R.apply(loop['held'], loop['a'], loop['b'], np.float32(1600 - loop['x0'])).astype(np.float64) - c['black']
    after = float(np.mean((cor[0] - cor[0].mean()) * (cor[1] - cor[1].mean())))
    pred = _predicted(loop, 1600) + 1.0 / 12.0                                 # the map's own error and the remainder of rint(ds)
    print('fixed covariance of the held-out pair: %.3f before, %.3f after, predicted %.3f' % (before, after, pred))
    assert abs(after - pred) < 5 * (3.5 ** 2 + pred) / math.sqrt(N)


# ---- DarkShading ----------------------------------------------------------------------------------------------------------------------------
def _map(Hm=6, Wm=8, **kw):
    rng = np.random.default_rng(1)
    args = dict(x0=1866.5, iso_min=800, iso_max=3200, cfa='bayer', raw_pattern=PAT, centred=False, counts=[8, 8, 8], isos=[800, 1600, 3200])
    args.update(kw)
    return SH.DarkShading(rng.standard_normal((Hm, Wm)).astype(np.float32), rng.standard_normal((Hm, Wm)).astype(np.float32) / 1000, **args)


def test_save_load_round_trip_without_pickle(tmp_path):
    m = _map(centred=True)
    path = m.save(tmp_path / 'shading')
    assert path.endswith('shading.npz')
    with np.load(path, allow_pickle=False) as z:
        assert all(z[k].dtype != object for k in z.files)
    n = SH.DarkShading.load(path)
    assert np.array_equal(n.a.view(np.int32), m.a.view(np.int32)) and np.array_equal(n.b.view(np.int32), m.b.view(np.int32))
    assert (n.x0, n.iso_min, n.iso_max, n.cfa, n.shape, n.centred, n.counts, n.isos) == (m.x0, 800.0, 3200.0, 'bayer', (6, 8), True, [8, 8, 8],
                                                                                        [800.0, 1600.0, 3200.0])
    assert np.array_equal(n.raw_pattern, np.array(PAT))
    assert SH.as_dark_shading(path).shape == (6, 8) and SH.as_dark_shading(m) is m
    np.savez(tmp_path / 'other.npz', a=m.a)
    with pytest.raises(ValueError):
        SH.DarkShading.load(tmp_path / 'other.npz')
    for bad in (3, str(tmp_path / 'missing.npz')):
        with pytest.raises(ValueError):
            SH.as_dark_shading(bad)


def test_t_and_its_range():
    m = _map()
    assert m.t(1600) == np.float32(1600 - 1866.5) and isinstance(m.t(1600), np.float32)
    assert m.t(800) == np.float32(800 - 1866.5) and m.t(3200) == np.float32(3200 - 1866.5)
    for iso in (799, 3201, 100):
        with pytest.raises(ValueError):
            m.t(iso)
    assert m.t(6400, extrapolate=True) == np.float32(6400 - 1866.5)
    for bad in (None, 'x', float('nan'), True):
        with pytest.raises(ValueError):
            m.t(bad)
    one = _map(x0=1600, iso_min=1600, iso_max=1600, counts=[4], isos=[1600])
    assert one.t(1600) == np.float32(0)
    with pytest.raises(ValueError):
        one.t(1601)


def test_constructor_and_frame_checks():
    m = _map()
    m.check_frames((3, 6, 8), 'bayer')
    m.check_pattern(PAT)
    m.check_pattern(None)
    with pytest.raises(ValueError):
        m.check_frames((6, 10), 'bayer')
    with pytest.raises(ValueError):
        m.check_frames((6, 8), 'xtrans')
    with pytest.raises(ValueError):
        m.check_pattern([[1, 0], [2, 3]])
    z = np.zeros((4, 6), np.float32)
    for a, b in ((z, np.zeros((4, 8), np.float32)), (np.zeros((4, 5), np.float32),) * 2, (np.full((4, 6), np.nan, np.float32), z)):
        with pytest.raises(ValueError):
            SH.DarkShading(a, b, 100, 100, 100)
    with pytest.raises(ValueError):
        SH.DarkShading(z, z, 100, 200, 100)


@pytest.mark.parametrize('p,shape', [(2, (10, 14)), (6, (14, 20))])
def test_centred_planes_have_zero_mean_per_cell(p, shape):
    import torch
    rng = np.random.default_rng(2)
    a0 = (5 + 3 * rng.standard_normal(shape)).astype(np.float32)
    b0 = (1e-3 * (2 + rng.standard_normal(shape))).astype(np.float32)
    flagged = rng.random(shape) < 0.05
    a0[flagged] = 0
    b0[flagged] = 0
    for mask in (None, flagged):
        a, b = torch.from_numpy(a0.copy()), torch.from_numpy(b0.copy())
        SH.centre_planes(a, b, p, None if mask is None else torch.from_numpy(mask))
        for plane, src in ((a.numpy(), a0), (b.numpy(), b0)):
            for r in range(p):
                for c in range(p):
                    good = np.ones_like(flagged[r::p, c::p]) if mask is None else ~mask[r::p, c::p]
                    v = plane[r::p, c::p][good].astype(np.float64)
                    # float32 rounding: the mean as float32 and one subtraction per site, each half an ulp of the values' scale
                    assert abs(v.mean()) <= 2 * np.finfo(np.float32).eps * np.abs(src).max()
            if mask is not None:
                assert np.all(plane[mask] == 0)


def test_fit_argument_errors_come_before_any_device_work():
    f = np.full((2, 4, 8), 512, np.uint16)
    ok = [{'iso': 800, 'bias': f}, {'iso': 1600, 'bias': f}]
    bad = [
        dict(sessions=[]),
        dict(sessions=[{'bias': f}]),                                          # iso is required
        dict(sessions=[{'iso': 800}]),
        dict(sessions=[{'iso': -1, 'bias': f}]),
        dict(sessions=[{'iso': 800, 'bias': f}] * 17),
        dict(sessions=[{'iso': 800, 'bias': f}, {'iso': 1600, 'bias': np.zeros((2, 4, 10), np.uint16)}]),
        dict(sessions=[{'iso': 800, 'bias': f.astype(np.float32)}]),
        dict(sessions=ok, cfa='foveon'),
        dict(sessions=ok, raw_pattern=[[0, 1], [1, 2]]),
        dict(sessions=ok, black_level=[512, 512]),
        dict(sessions=ok, black_level=70000),
        dict(sessions=ok, weights=[1.0]),
        dict(sessions=ok, weights=[1.0, 0.0]),
        dict(sessions=ok, defects=3),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            SH.fit_dark_shading(**kw)
    from eld_amd.defects import DefectMap
    with pytest.raises(ValueError):
        SH.fit_dark_shading(ok, defects=DefectMap.from_sites([(0, 0)], (4, 10)))


# ---- wiring: errors raised without a device ---------------------------------------------------------------------------------------------------
class FakeNet:
    def __init__(self, c):
        self.in_channels = self.out_channels = c

    def parameters(self):
        raise AssertionError('an argument error must come before any device work')


def test_denoise_raw_checks_shading_before_device_work():
    from eld_amd.denoise import denoise_raw
    den = types.SimpleNamespace(cfa='bayer', in_channels=4, out_channels=4, net=FakeNet(4))
    raw = np.full((6, 8), 600, np.uint16)
    m = _map()
    with pytest.raises(ValueError, match='iso'):
        denoise_raw(den, raw, 'bayer', shading=m)
    with pytest.raises(ValueError, match='shading'):
        denoise_raw(den, raw, 'bayer', iso=1600)
    with pytest.raises(ValueError, match='6 x 8'):
        denoise_raw(den, np.full((6, 10), 600, np.uint16), 'bayer', shading=m, iso=1600)
    with pytest.raises(ValueError, match='range'):
        denoise_raw(den, raw, 'bayer', shading=m, iso=6400)
    with pytest.raises(ValueError, match='raw_pattern'):
        denoise_raw(den, raw, 'bayer', raw_pattern=[[1, 0], [2, 3]], shading=m, iso=1600)
    with pytest.raises(ValueError, match='cfa'):
        denoise_raw(types.SimpleNamespace(cfa='xtrans', in_channels=9, out_channels=9, net=FakeNet(9)), np.full((6, 8), 600, np.uint16), 'xtrans',
                    shading=m, iso=1600)
    with pytest.raises(ValueError):
        denoise_raw(den, raw, 'bayer', shading=3, iso=1600)


def test_dark_pool_checks_shading_before_upload():
    from eld_amd.darkpool import DarkPool
    f = np.full((2, 6, 8), 512, np.uint16)
    m = _map()
    with pytest.raises(ValueError, match='iso'):
        DarkPool([{'bias': f}], shading=m)
    with pytest.raises(ValueError, match='range'):
        DarkPool([{'bias': f, 'iso': 6400}], shading=m)
    with pytest.raises(ValueError, match='6 x 8'):
        DarkPool([{'bias': np.full((2, 6, 10), 512, np.uint16), 'iso': 800}], shading=m)


def test_parsers_take_the_new_flags_and_keep_their_defaults(tmp_path):
    from eld_amd import denoise, train_frames, validate
    base = ['in.npy', '-o', 'out', '--ckpt', 'm.pt']
    a = denoise.build_parser().parse_args(base)
    assert a.shading is None and a.iso is None
    o = denoise.parse_args(base)[3]
    assert 'shading' not in o and 'iso' not in o
    o = denoise.parse_args(base + ['--shading', 's.npz', '--iso', '1600'])[3]
    assert o['shading'] == 's.npz' and o['iso'] == 1600.0
    with pytest.raises(ValueError, match='--iso'):
        denoise.parse_args(base + ['--shading', 's.npz'])
    (tmp_path / 'side.json').write_text('{"shading": "s.npz", "iso": 800}')
    o = denoise.parse_args(base + ['--meta', str(tmp_path / 'side.json')])[3]
    assert o['shading'] == str(tmp_path / 's.npz') and o['iso'] == 800
    a = validate.parser().parse_args(['m.json'])
    assert a.shading is None and a.structure is False and a.lags == 8
    assert validate.parser().parse_args(['m.json', '--shading', 's.npz']).shading == 's.npz'
    a = train_frames.build_parser().parse_args(['f.npy', '-o', 'm.pt'])
    assert a.dark_shading is None and a.dark is None and a.noise == 'PGRU'
    assert train_frames.build_parser().parse_args(['f.npy', '-o', 'm.pt', '--dark-shading', 's.npz']).dark_shading == 's.npz'
    with pytest.raises(ValueError, match='--dark'):
        train_frames.dark_pool(None, 'SonyA7S2', 'PGRU', 64, shading='s.npz')
    a = SH.build_parser().parse_args(['m.json', '-o', 's.npz'])
    assert a.centred is False and a.defects is None


def test_validate_camera_checks_shading_before_device_work():
    from eld_amd.validate import validate_camera
    f = np.full((3, 6, 8), 512, np.uint16)
    fl = np.full((1, 2, 6, 8), 900, np.uint16)
    diag = {'frames': [{}] * 3}
    m = _map()
    with pytest.raises(ValueError, match='iso'):
        validate_camera([{'bias': f, 'flats': fl}], PAT, [512] * 4, 16383, diag=diag, shading=m)
    with pytest.raises(ValueError, match='range'):
        validate_camera([{'iso': 100, 'bias': f, 'flats': fl}], PAT, [512] * 4, 16383, diag=diag, shading=m)
    with pytest.raises(ValueError, match='raw_pattern'):
        validate_camera([{'iso': 800, 'bias': f, 'flats': fl}], [[1, 0], [2, 3]], [512] * 4, 16383, diag=diag, shading=m)


def test_entry_points_refuse_bad_arguments_without_a_device(eld_lib):
    """The checks run on the host before any launch, so they answer on a machine without a GPU; pointers are never dereferenced here."""
    import ctypes
    vp = ctypes.c_void_p
    ok, odd = vp(0x1000), vp(0x1002)
    ses, d1, cen = (ctypes.c_int32 * 2)(0, 3), (ctypes.c_double * 1)(1.0), (ctypes.c_int32 * 4)(512, 512, 512, 512)

    def fit(pool=ok, tab=ok, F=3, Hm=4, Wm=8, ses_=ses, S=1, al=d1, be=d1, cen_=cen, p=2, bm=None, a=ok, b=ok):
        return eld_lib.eld_shading_fit_u16(pool, 96, tab, F, Hm, Wm, ses_, S, al, be, cen_, p, bm, a, b, None)
    for kw in (dict(pool=None), dict(tab=None), dict(ses_=None), dict(al=None), dict(be=None), dict(cen_=None), dict(a=None), dict(b=None),
               dict(Wm=7), dict(p=3), dict(pool=odd), dict(bm=odd), dict(S=0), dict(S=17), dict(ses_=(ctypes.c_int32 * 2)(0, 0)),
               dict(ses_=(ctypes.c_int32 * 2)(0, 65537), F=70000), dict(ses_=(ctypes.c_int32 * 2)(1, 3)),
               dict(cen_=(ctypes.c_int32 * 4)(512, 65536, 512, 512))):
        assert fit(**kw) == -1, kw
    assert fit(Hm=0) == 0 and fit(Wm=0) == 0

    def app(i=ok, o=ok, N=2, Hm=4, Wm=8, a=ok, b=ok, bm=None):
        return eld_lib.eld_shading_apply_u16(i, o, N, Hm, Wm, a, b, 1.0, bm, None)
    for kw in (dict(i=None), dict(o=None), dict(a=None), dict(b=None), dict(Wm=7), dict(N=-1), dict(i=odd), dict(o=odd), dict(bm=odd)):
        assert app(**kw) == -1, kw
    assert app(N=0) == 0 and app(Hm=0) == 0
    pat, blk = (ctypes.c_int * 4)(0, 1, 3, 2), (ctypes.c_float * 4)(512, 512, 512, 512)
    lib = eld_lib
    assert lib.eld_pack_raw_bayer_u16_shaded(ok, ok, 1, 2, 4, pat, blk, 16383.0, ok, None, ok, 1.0, None) == -1
    assert lib.eld_pack_raw_bayer_u16_shaded(ok, ok, 1, 2, 4, pat, blk, 16383.0, None, ok, ok, 1.0, None) == -1
    assert lib.eld_pack_raw_bayer_u16_shaded(ok, ok, 1, 2, 4, (ctypes.c_int * 4)(0, 1, 1, 2), blk, 16383.0, ok, ok, ok, 1.0, None) == -1
    assert lib.eld_pack_raw_bayer_u16_shaded(None, None, 0, 2, 4, pat, blk, 16383.0, None, None, None, 1.0, None) == 0
    assert lib.eld_pack_raw_xtrans_u16_shaded(ok, ok, 1, 6, 6, 1024.0, 16383.0, ok, ok, None, 1.0, None) == -1
    assert lib.eld_pack_raw_xtrans_u16_shaded(ok, ok, 1, 6, 6, 1024.0, 1024.0, ok, ok, ok, 1.0, None) == -1
    assert lib.eld_pack_raw_xtrans_u16_shaded(None, None, 1, 5, 6, 1024.0, 16383.0, None, None, None, 1.0, None) == 0
    # the four Bayer entry points of the input stage share one pattern check: a repeated code, a code out of range and no pattern at all are
    # refused; the first two only where there is work (an empty call returns 0 before the pattern is read), the last always
    for bad in ((ctypes.c_int * 4)(0, 1, 1, 2), (ctypes.c_int * 4)(0, 1, 4, 2), (ctypes.c_int * 4)(0, -1, 3, 2), None):
        for N in (1, 0):
            want = 0 if (N == 0 and bad is not None) else -1
            assert lib.eld_pack_raw_bayer_u16(ok, ok, N, 2, 4, bad, blk, 16383.0, None) == want
            assert lib.eld_pack_raw_bayer_u16_gain(ok, ok, N, 2, 4, bad, blk, 16383.0, ok, None) == want
            assert lib.eld_pack_raw_bayer_u16_shaded(ok, ok, N, 2, 4, bad, blk, 16383.0, ok, ok, ok, 1.0, None) == want
            assert lib.eld_pack_raw_bayer_u16_flat(ok, ok, N, 2, 4, bad, blk, 16383.0, ok, ok, ok, 1.0, ok, None) == want
