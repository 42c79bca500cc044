"""CPU tests of the frame (eld_amd/isp.py Frame, csrc/frame_dev.h, eld_amd/dng.py, the command line): the tap tables against
the NumPy restatement (tests/frame_ref.py), the orientation table against Pillow, two quality yardsticks of the filters, the DNG tags read
and carried, every argument error, the entry point's rules with fake pointers, and the per-output arithmetic under AddressSanitizer
(tools/frame_hostcheck.cpp, a plain executable).  No device is touched."""
import hashlib
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import dng_ref as DR
import frame_ref as R
import jpeg_ref as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (Hs, Ws), crop, orientation, size
GEOMETRIES = (((37, 53), (2.5, 1.25, 30.5, 48.0), 1, (11, 17)), ((37, 53), (2.5, 1.25, 30.5, 48.0), 6, (11, 17)), ((70, 300), None, 7, (3, 5)),
              ((5, 7), None, 1, (23, 31)), ((4000, 6000), None, 1, 1024), ((4000, 6000), None, 8, 256), ((40, 60), (3, 4, 20, 30), 5, None),
              ((48, 64), (0.5, 0.25, 47.25, 63.5), 3, 20), ((9, 9), (4.25, 4.5, 0.4, 0.3), 1, (1, 1)))


def isp():
    from eld_amd import isp
    return isp


# ---- the tap tables -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('flt', ('area', 'lanczos'))
def test_tables_are_the_restatements(flt):
    for (Hs, Ws), crop, o, size in GEOMETRIES:
        t, out = isp().Frame(crop, o, size, flt).taps(Hs, Ws)
        r, rout = R.taps(Hs, Ws, crop, o, size, flt)
        assert out == rout, (crop, o, size)
        Hc, Wc = out if o <= 4 else out[::-1]
        assert t.ystart.shape == (Hc,) and t.xstart.shape == (Wc,) and t.yw.shape[0] == Hc and t.xw.shape[0] == Wc
        for a, b, name in zip(t, r, t._fields):
            assert a.dtype == b.dtype and a.shape == b.shape, name
            if a.dtype != np.float32:
                assert np.array_equal(a, b), (name, crop, o, size)
            elif flt == 'area':
                assert a.tobytes() == b.tobytes(), (name, crop, o, size)
            else:                                                    # the sin of two libraries may differ in the last bit
                ulp = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
                assert ulp.max() <= 1 and np.array_equal(a == 0, b == 0), (name, crop, o, size, int(ulp.max()))
        for start, count, w, S in ((t.ystart, t.ycount, t.yw, Hs), (t.xstart, t.xcount, t.xw, Ws)):
            assert count.min() >= 1 and count.max() == w.shape[1] and start.min() >= 0 and (start + count).max() <= S
            assert all(not w[i, count[i]:].any() for i in range(len(count)))
            assert np.abs(w.astype(np.float64).sum(axis=1) - 1).max() < 1e-6 * w.shape[1] ** 0.5 + 1e-6


def test_integer_crop_at_its_own_size_is_single_taps_of_weight_one():
    t, out = isp().Frame(crop=(3, 4, 20, 30)).taps(40, 60)
    assert out == (20, 30) and t.yw.shape == (20, 1) and t.xw.shape == (30, 1)
    assert (t.yw == 1).all() and (t.xw == 1).all() and (t.ycount == 1).all() and (t.xcount == 1).all()
    assert np.array_equal(t.ystart, np.arange(3, 23)) and np.array_equal(t.xstart, np.arange(4, 34))
    t, out = isp().Frame().taps(4000, 6000)                            # the identity frame of a 24 MP render
    assert out == (4000, 6000) and t.yw.shape == (4000, 1) and (t.yw == 1).all() and (t.xw == 1).all() and np.array_equal(t.xstart, np.arange(6000))


def test_area_weights_are_positive():
    for (Hs, Ws), size in (((4000, 6000), 1024), ((5, 7), (23, 31)), ((37, 53), (11, 17))):
        t, _ = isp().Frame(size=size).taps(Hs, Ws)
        for count, w in ((t.ycount, t.yw), (t.xcount, t.xw)):
            assert all((w[i, :count[i]] > 0).all() for i in range(len(count)))
    t, _ = isp().Frame(size=(23, 31)).taps(5, 7)                        # enlarging, 'area' is nearest-like: at most two taps per output
    assert t.yw.shape[1] <= 2 and t.xw.shape[1] <= 2


def test_sizes():
    F = isp().Frame
    assert F(size=None).out_size(48, 64) == (48, 64) and F(orientation=6).out_size(48, 64) == (64, 48)
    assert F(crop=(0, 0, 10.5, 20.49)).out_size(48, 64) == (11, 20) and F(crop=(0, 0, 0.2, 0.3)).out_size(48, 64) == (1, 1)
    assert F(size=20).out_size(48, 64) == (15, 20) and F(size=20, orientation=6).out_size(48, 64) == (20, 15)
    assert F(size=20, orientation=5, crop=(4, 6, 40, 50)).out_size(48, 64) == (20, 16)
    assert F(size=1000).out_size(4000, 3) == (1000, 1) and F(size=(7, 9), orientation=8).out_size(48, 64) == (7, 9)


def test_frame_argument_errors():
    F = isp().Frame
    bad = (dict(crop=(1, 2, 3)), dict(crop=(-1, 0, 4, 4)), dict(crop=(0, 0, 0, 4)), dict(crop=(0, 0, 4, float('nan'))), dict(crop='default'),
           dict(orientation=0), dict(orientation=9), dict(orientation=1.5), dict(orientation='6'), dict(size=0), dict(size=(4, 0)), dict(size=(1, 2, 3)),
           dict(size='big'), dict(filter='bicubic'), dict(filter=None))
    for kw in bad:
        with pytest.raises(ValueError):
            F(**kw)
    with pytest.raises(ValueError, match='inside'):
        F(crop=(0, 0, 41, 10)).taps(40, 60)
    with pytest.raises(ValueError, match='inside'):
        F(crop=(30, 55, 10, 5.5)).taps(40, 60)
    with pytest.raises(ValueError, match='4096'):
        F(size=(1, 1)).taps(4097, 8)                                 # 'area': 4097 taps for the one output row
    with pytest.raises(ValueError, match='4096'):
        F(size=(8, 4), filter='lanczos').taps(16, 6000)              # lanczos: 6 * 1500 taps, clipped to the 6000 source pixels
    F(size=(1, 1)).taps(4096, 8)
    with pytest.raises(ValueError, match='taps'):
        R.axis_taps(4097, 0, 4097, 1, 'area')


# ---- the orientation table ------------------------------------------------------------------------------------------------------------------
def test_orientation_table_is_pillows_exif_transpose():
    try:
        from PIL import Image, ImageOps
    except ImportError:
        pytest.skip('Pillow is not installed')
    a = np.arange(5 * 7, dtype=np.uint8).reshape(5, 7)
    for o in range(1, 9):
        img = Image.fromarray(a)
        img.getexif()[0x0112] = o
        up = np.asarray(ImageOps.exif_transpose(img))
        assert up.shape == ((5, 7) if o <= 4 else (7, 5)) and np.array_equal(up, R.orient(a, o)), o


# ---- quality yardsticks -----------------------------------------------------------------------------------------------------------------------
def test_area_is_the_block_mean_at_integer_factors():
    """With an integer crop and an integer factor k every output is the mean of a k x k block: k sums of k products p * wx, then k products
    with wy and their sum.  Values in [0, 1], weights 1/k rounded to float32: recursive summation of n terms is off by at most (n - 1) u of
    the sum of magnitudes, and each term carries up to two roundings more (the weight, the product): (k + 1) u per axis, (2 k + 2) u for
    both, u = 2^-24, plus u for the float64 mean's own conversion -- below (k^2 + 4) u, the rounding of a k^2-term sum, for every k >= 2."""
    rng = np.random.default_rng(21)
    worst = 0.0
    for k, (Hs, Ws), crop in ((2, (20, 26), (2, 4, 16, 20)), (3, (31, 40), (1, 1, 27, 36)), (4, (41, 50), (0, 2, 40, 48)), (7, (70, 77), (0, 0, 70, 77))):
        rgb = rng.uniform(0, 1, (1, 3, Hs, Ws)).astype(np.float32)
        y0, x0, ch, cw = crop
        t, out = isp().Frame(crop, 1, (ch // k, cw // k), 'area').taps(Hs, Ws)
        assert t.yw.shape[1] == k and t.xw.shape[1] == k and (t.ycount == k).all() and (t.xcount == k).all()
        got = R.resample(rgb, tuple(t)).astype(np.float64)
        mean = rgb[:, :, y0:y0 + ch, x0:x0 + cw].astype(np.float64).reshape(1, 3, ch // k, k, cw // k, k).mean(axis=(3, 5))
        err = float(np.abs(got - mean).max())
        worst = max(worst, err / ((k * k + 4) * 2.0 ** -24))
        assert err <= (k * k + 4) * 2.0 ** -24, (k, err)
    print('area against the block mean: at most %.2f of the bound' % worst)


LANCZOS_CASES = (((96, 128), (3.25, 5.5, 88.5, 117.0), (17, 23)), ((96, 128), (0.0, 0.0, 96.0, 128.0), (24, 32)), ((40, 30), (2.0, 1.5, 30.0, 25.25), (75, 61)),
                 ((61, 83), (0.0, 0.0, 61.0, 83.0), (7, 9)))
LANCZOS_MEASURED = 2.384e-7                      # the largest |difference| over LANCZOS_CASES when this test was written (Pillow 12.2): one float32 ulp below 1
LANCZOS_BOUND = 4 * LANCZOS_MEASURED


def test_lanczos_is_pillows():
    """Planes in [0, 1], mode F, against Image.resize(LANCZOS, box=...): the same support and the same normalised weights; Pillow keeps the
    weights and both accumulations in double precision and rounds each pass's result to float32, the frame rounds the weights and every
    product and sum to float32.  The negative control moves every centre by half a source pixel, the classic off-by-a-half of resamplers."""
    try:
        from PIL import Image
    except ImportError:
        pytest.skip('Pillow is not installed')
    worst = 0.0
    for seed, ((Hs, Ws), crop, (Ho, Wo)) in enumerate(LANCZOS_CASES):
        plane = np.random.default_rng(seed).uniform(0, 1, (Hs, Ws)).astype(np.float32)
        y0, x0, ch, cw = crop
        t, _ = isp().Frame(crop, 1, (Ho, Wo), 'lanczos').taps(Hs, Ws)
        got = R.resample(plane[None, None], tuple(t))[0, 0].astype(np.float64)
        pil = np.asarray(Image.fromarray(plane, mode='F').resize((Wo, Ho), Image.LANCZOS, box=(x0, y0, x0 + cw, y0 + ch)), np.float64)
        err = float(np.abs(got - pil).max())
        worst = max(worst, err)
        print('lanczos %s %s -> %s: max |frame - Pillow| = %.3e (bound %.3e)' % ((Hs, Ws), crop, (Ho, Wo), err, LANCZOS_BOUND))
        assert err <= LANCZOS_BOUND, (crop, err)
        shifted = R.axis_taps(Hs, y0, ch, Ho, 'lanczos', shift=0.5) + R.axis_taps(Ws, x0, cw, Wo, 'lanczos', shift=0.5)
        off = float(np.abs(R.resample(plane[None, None], shifted)[0, 0].astype(np.float64) - pil).max())
        assert off > 1000 * LANCZOS_BOUND, (crop, off)
    print('lanczos: worst %.3e' % worst)


# ---- the DNG tags -----------------------------------------------------------------------------------------------------------------------------
BASE_RAW = {50714: (DR.SHORT, (64,)), 50717: (DR.LONG, (4095,))}
BASE_0 = {50728: (DR.RATIONAL, ((1, 2), (1, 1), (2, 3))), 50778: (DR.SHORT, (21,))}
CROPS = {'short': ({50719: (DR.SHORT, (4, 2)), 50720: (DR.SHORT, (30, 20))}, [2, 4, 20, 30]),
         'long': ({50719: (DR.LONG, (4, 2)), 50720: (DR.LONG, (30, 20))}, [2, 4, 20, 30]),
         'rational': ({50719: (DR.RATIONAL, ((9, 2), (5, 4))), 50720: (DR.RATIONAL, ((61, 2), (20, 1)))}, [1.25, 4.5, 20, 30.5]),
         'size only': ({50720: (DR.SHORT, (30, 20))}, [0, 0, 20, 30])}


def source(tmp_path, name, raw_tags=None, tags0=None, **kw):
    img = DR.noisy_ramp(26, 40, 12, seed=3)
    path = str(tmp_path / name)
    DR.write_dng_file(path, img, bits=12, tags={**BASE_RAW, **(raw_tags or {})}, tags0={**BASE_0, **(tags0 or {})}, **kw)
    return path, img


@pytest.mark.parametrize('subifd', (False, True))
def test_meta_reads_the_crop_and_the_orientation(tmp_path, subifd):
    from eld_amd import dng as d
    plain, _ = source(tmp_path, 'plain.dng', subifd=subifd)
    base = d.dng_meta(plain)
    assert 'orientation' not in base and 'default_crop' not in base
    for name, (tags, want) in CROPS.items():
        for o in (None, 1, 6, 8):
            path, _ = source(tmp_path, 'c.dng', tags, None if o is None else {274: (DR.SHORT, (o,))}, subifd=subifd)
            m = d.dng_meta(path)
            assert m['default_crop'] == want and m.get('orientation') == o, (name, o)
            assert {k: v for k, v in m.items() if k not in ('default_crop', 'orientation')} == base
    path, _ = source(tmp_path, 'o.dng', None, {274: (DR.SHORT, (3,))}, subifd=subifd)
    assert d.dng_meta(path) == dict(base, orientation=3)
    # tags nobody can use give no key and no error: this is read_dng's path too, and such files read before the keys existed
    for tags, tags0 in (({50720: (DR.SHORT, (30, 0))}, None), ({50720: (DR.SHORT, (30,))}, None), ({50720: (DR.RATIONAL, ((30, 0), (20, 1)))}, None),
                        ({50719: (DR.SHORT, (4,)), 50720: (DR.SHORT, (30, 20))}, None), (None, {274: (DR.SHORT, (9,))}), (None, {274: (DR.SHORT, (0,))})):
        path, _ = source(tmp_path, 'bad.dng', tags, tags0, subifd=subifd)
        assert d.dng_meta(path) == base, (tags, tags0)


def test_write_dng_carries_the_crop_and_the_orientation(tmp_path):
    from eld_amd import dng as d
    jpg = J.encode(J.smooth(16, 24, 1), 90, '420')
    for subifd in (False, True):
        tags, want = CROPS['rational']
        src, img = source(tmp_path, 'src.dng', tags, {274: (DR.SHORT, (6,))}, subifd=subifd)
        for preview in (None, jpg):
            out = str(tmp_path / 'out.dng')
            d.write_dng(out, img, like=src, preview=preview)
            t, _ = d.parse_tiff(out)
            raw = d._raw_ifd(t)
            assert (raw is t.ifd0) == (preview is None)
            assert tuple(t.ifd0[274].values) == (6,) and t.ifd0[274].type == DR.SHORT and (preview is None or 274 not in raw)
            assert raw[50719].type == DR.RATIONAL and tuple(raw[50719].values) == ((9, 2), (5, 4))          # verbatim: the rationals they were
            assert raw[50720].type == DR.RATIONAL and tuple(raw[50720].values) == ((61, 2), (20, 1))
            assert preview is None or (50719 not in t.ifd0 and 50720 not in t.ifd0)
            m = d.dng_meta(out)
            assert m['default_crop'] == want and m['orientation'] == 6
        # meta= written from values (no like=) has neither tag
        d.write_dng(str(tmp_path / 'm.dng'), img, meta=dict(cfa='bayer', black_level=64, white_point=4095))
        m = d.dng_meta(str(tmp_path / 'm.dng'))
        assert 'orientation' not in m and 'default_crop' not in m


def test_a_source_without_the_tags_gives_the_bytes_of_before(tmp_path):
    """the two digests are of the files the parent of this change wrote from the same source"""
    from eld_amd import dng as d
    src, img = source(tmp_path, 'plain.dng')
    out = str(tmp_path / 'out.dng')
    d.write_dng(out, img, like=src)
    with open(out, 'rb') as fh:
        assert hashlib.sha256(fh.read()).hexdigest() == 'f8b717dc03662b48765465c28ca40f4c28fc924542a5c5add96db124c3bdb72f'
    d.write_dng(out, img, like=src, preview=J.encode(J.smooth(16, 24, 1), 90, '420'))
    with open(out, 'rb') as fh:
        assert hashlib.sha256(fh.read()).hexdigest() == '3b6181ce369124ffa0282abf4e43a657c3c9faf279e05474c09f1cf8a6ddad3b'


# ---- the command line's and denoise_raw's argument errors -----------------------------------------------------------------------------------------
def test_denoise_argument_errors(tmp_path, capsys):
    from eld_amd import denoise as D
    colour = ['--wb', '2', '1', '1.5', '--ccm', '1', '0', '0', '0', '1', '0', '0', '0', '1']
    npy = str(tmp_path / 'frame.npy')
    base = [npy, '-o', str(tmp_path / 'out'), '--ckpt', 'none.pt'] + colour
    full = base + ['--srgb-size', 'full']
    for opt in (['--crop', '2,4,20,30'], ['--crop', 'default'], ['--orient', '6'], ['--orient', 'auto'], ['--size', '256'], ['--size', '20x30'],
                ['--resample', 'lanczos'], ['--dng', '--dng-preview', '--dng-preview-size', '64']):
        with pytest.raises(ValueError, match='--srgb-size full'):
            D.parse_args(base + opt)
        with pytest.raises(ValueError, match='--srgb-size full'):
            D.parse_args(base + opt + ['--srgb-size', 'packed'])
    with pytest.raises(ValueError, match='frame.npy.*DefaultCrop'):
        D.parse_args(full + ['--crop', 'default'])
    with pytest.raises(ValueError, match='frame.npy.*Orientation'):
        D.parse_args(full + ['--orient', 'auto'])
    for opt in (['--crop', '1,2,3'], ['--crop', '0,0,0,5'], ['--crop', 'a,b,c,d'], ['--orient', '0'], ['--orient', '9'],
                ['--orient', 'up'], ['--size', '0'], ['--size', '20x'], ['--size', '4x0'], ['--size', '1x2x3']):
        with pytest.raises(ValueError, match=opt[0]):
            D.parse_args(full + opt)
    with pytest.raises(ValueError, match='--dng-preview'):
        D.parse_args(full + ['--dng', '--dng-preview-size', '64'])
    o = D.parse_args(full + ['--crop', '2.5,4,20,30.25', '--orient', '6', '--size', '20x30', '--resample', 'lanczos'])[3]
    assert o['crop'] == (2.5, 4.0, 20.0, 30.25) and o['orient'] == 6 and o['size'] == (20, 30) and o['resample'] == 'lanczos'
    assert D.parse_args(full + ['--size', '256'])[3]['size'] == 256
    plain = D.parse_args(full)[3]
    assert all(plain.get(k) is None for k in ('crop', 'orient', 'size', 'resample', 'dng_preview_size'))
    side = str(tmp_path / 'side.json')                                # the sidecar's keys
    with open(side, 'w') as fh:
        fh.write('{"crop": [2, 4, 20, 30], "orient": 8, "size": [20, 30], "resample": "area", "srgb_size": "full"}')
    o = D.parse_args(base + ['--meta', side])[3]
    assert o['crop'] == (2.0, 4.0, 20.0, 30.0) and o['orient'] == 8 and o['size'] == (20, 30) and o['resample'] == 'area'
    # one input: the crop against the render's rectangle
    raw = np.zeros((48, 64), np.uint16)
    o = D.parse_args(full + ['--crop', '40,60,20,30', '--orient', '6'])[3]
    frame, preview = D.frame_option(npy, raw, o)
    assert frame.crop == (40.0, 60.0, 8.0, 4.0) and frame.orientation == 6 and preview is None and 'clipped' in capsys.readouterr().out
    with pytest.raises(ValueError, match='frame.npy.*outside'):
        D.frame_option(npy, raw, D.parse_args(full + ['--crop', '48,0,10,10'])[3])
    assert D.frame_option(npy, raw, plain) == (None, None) and D.frame_option(npy, raw, D.parse_args(full + ['--orient', '1'])[3]) == (None, None)
    assert D.frame_option(npy, raw, D.parse_args(full + ['--resample', 'area'])[3]) == (None, None)
    frame, _ = D.frame_option(npy, raw, D.parse_args(full + ['--resample', 'lanczos'])[3])          # lanczos alone is no identity: it is kept and runs
    assert frame.filter == 'lanczos' and not frame.identity and frame.taps(48, 64)[0].yw.shape[1] > 1
    # DNG inputs: default and auto read the tags; the DNG preview keeps the crop and is not turned
    tags, want = CROPS['rational']
    dng, img = source(tmp_path, 'f.dng', tags, {274: (DR.SHORT, (6,))})
    args = [dng, '-o', str(tmp_path / 'out'), '--ckpt', 'none.pt', '--srgb-size', 'full'] + colour
    o = D.parse_args(args + ['--crop', 'default', '--orient', 'auto', '--size', '16', '--dng', '--dng-preview', '--dng-preview-size', '8'])[3]
    frame, preview = D.frame_option(dng, img, o)
    assert frame.crop == (1.25, 4.5, 20.0, 30.5) and frame.orientation == 6 and frame.size == 16 and frame.taps(26, 40)[1] == (16, 10)
    assert preview.crop == frame.crop and preview.orientation == 1 and preview.size == 8 and preview.taps(26, 40)[1] == (5, 8)
    o = D.parse_args(args + ['--orient', 'auto', '--dng', '--dng-preview'])[3]
    frame, preview = D.frame_option(dng, img, o)
    assert frame.crop is None and frame.orientation == 6 and preview.identity         # the preview: the whole picture, unturned, at its own size
    plain_dng, _ = source(tmp_path, 'g.dng')
    frame, preview = D.frame_option(plain_dng, img, D.parse_args([plain_dng] + args[1:] + ['--crop', 'default', '--orient', 'auto'])[3])
    assert frame is None and preview is None and 'no DefaultCropSize' in capsys.readouterr().out

    class Net:                                                       # denoise_raw's own checks come before it looks at the network or a device
        cfa, in_channels, out_channels = 'bayer', 4, 4
    F = isp().Frame
    kw = dict(wb=(2, 1, 1.5), ccm=np.eye(3))
    with pytest.raises(ValueError, match="srgb_size='full'"):
        D.denoise_raw(Net(), np.zeros((8, 8), np.uint16), 'bayer', frame=F(orientation=6), **kw)
    with pytest.raises(ValueError, match="srgb_size='full'"):
        D.denoise_raw(Net(), np.zeros((8, 8), np.uint16), 'bayer', preview_frame=F(size=4), jpeg={}, **kw)
    with pytest.raises(ValueError, match='Frame'):
        D.denoise_raw(Net(), np.zeros((8, 8), np.uint16), 'bayer', srgb_size='full', frame={'orientation': 6}, **kw)
    with pytest.raises(ValueError, match='jpeg'):
        D.denoise_raw(Net(), np.zeros((8, 8), np.uint16), 'bayer', srgb_size='full', preview_frame=F(size=4), **kw)
    with pytest.raises(ValueError, match='inside'):
        D.denoise_raw(Net(), np.zeros((8, 8), np.uint16), 'bayer', srgb_size='full', frame=F(crop=(0, 0, 9, 4)), **kw)


# ---- the entry point's argument rules ---------------------------------------------------------------------------------------------------------
def test_entry_point_refuses_bad_arguments_before_any_launch(eld_lib):
    import ctypes
    from eld_amd import _lib as L
    A, B, W, T = 0x10000000, 0x20000000, 0x30000000, 0x40000000      # fake device pointers: nothing is launched on a refusal or with N == 0

    def call(rgb=A, out=B, mode=L.RENDER_SRGB8, N=1, Hs=40, Ws=60, Ho=11, Wo=17, o=1, ys=T, yc=T + 256, yw=T + 512, Ty=4, xs=T + 4096, xc=T + 8192,
             xw=T + 12288, Tx=5, row0=2, rows=30, ws=W, ws_bytes=None, ccms=None, gamma=2.2, E=None, f=None, n=0):
        Wc = Ho if o >= 5 else Wo
        nbytes = max(N, 0) * 3 * rows * Wc * 4 if ws_bytes is None else ws_bytes
        return eld_lib.eld_frame_rgb_f32(rgb, out, mode, N, Hs, Ws, Ho, Wo, o, ys, yc, yw, Ty, xs, xc, xw, Tx, row0, rows, ws, nbytes, ccms, gamma, E, f, n,
                                         None)
    assert call(N=0) == 0 and call(N=0, mode=L.RENDER_LINEAR_F32, o=6) == 0 and call(N=0, Ty=4096, Tx=1, row0=0, rows=40) == 0
    bad = {'null rgb': dict(rgb=None), 'null out': dict(out=None), 'null workspace': dict(ws=None), 'null ystart': dict(ys=None),
           'null ycount': dict(yc=None), 'null yw': dict(yw=None), 'null xstart': dict(xs=None), 'null xcount': dict(xc=None), 'null xw': dict(xw=None),
           'rgb misaligned': dict(rgb=A + 2), 'float32 out misaligned': dict(out=B + 2, mode=L.RENDER_LINEAR_F32), 'workspace misaligned': dict(ws=W + 1),
           'table misaligned': dict(xc=T + 8193), 'N < 0': dict(N=-1), 'N > 21845': dict(N=21846), 'Hs 0': dict(Hs=0), 'Ws 0': dict(Ws=0),
           'Hs Ws = 2^31': dict(Hs=1 << 16, Ws=1 << 15), 'Ho 0': dict(Ho=0), 'Wo 0': dict(Wo=0), 'Ho Wo = 2^31': dict(Ho=1 << 16, Wo=1 << 15),
           'orientation 0': dict(o=0), 'orientation 9': dict(o=9), 'Ty 0': dict(Ty=0), 'Ty 4097': dict(Ty=4097), 'Tx 0': dict(Tx=0), 'Tx 4097': dict(Tx=4097),
           'row0 < 0': dict(row0=-1), 'rows 0': dict(rows=0), 'rows past the source': dict(row0=11, rows=30),
           'out_mode 2': dict(mode=2), 'gamma 0': dict(gamma=0.0), 'crf_n 1': dict(n=1, E=A, f=A), 'crf without tables': dict(n=4),
           'ccms misaligned': dict(ccms=A + 1)}
    for name, kw in bad.items():
        assert call(**kw) == -1, name
        if 'N' not in kw:
            assert call(**dict(kw, N=0)) == -1, name
    assert call(ws_bytes=3 * 30 * 17 * 4 - 4) == -3 and call(o=6, ws_bytes=3 * 30 * 11 * 4 - 4) == -3      # ELD_EWS
    for name, kw in {'out inside rgb': dict(out=A + 16), 'workspace inside rgb': dict(ws=A + 64), 'workspace inside out': dict(ws=B + 4),
                     'out ends inside the workspace': dict(out=W - 3 * 11 * 17 + 1)}.items():
        assert call(**kw) == -1, name
    th, tw, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert eld_lib.eld_frame_rgb_tile(ctypes.byref(th), ctypes.byref(tw), ctypes.byref(lds)) == 0
    assert th.value >= 1 and tw.value >= 1 and 0 < lds.value <= 65536
    assert eld_lib.eld_frame_rgb_tile(None, ctypes.byref(tw), None) == -1 and eld_lib.eld_frame_rgb_tile(ctypes.byref(th), None, None) == -1


# ---- the per-output arithmetic under AddressSanitizer -------------------------------------------------------------------------------------------
def hostcheck_case(Hs, Ws, crop, o, size, flt, seed):
    rng = np.random.default_rng(seed)
    rgb = rng.uniform(-0.1, 1.1, (1, 3, Hs, Ws)).astype(np.float32)
    t, (Ho, Wo) = isp().Frame(crop, o, size, flt).taps(Hs, Ws)
    want = R.frame_linear(rgb, tuple(t), o)
    assert want.shape == (1, 3, Ho, Wo)
    Hc, Wc = (Ho, Wo) if o <= 4 else (Wo, Ho)
    head = struct.pack('<7i', Hs, Ws, Hc, Wc, t.yw.shape[1], t.xw.shape[1], o)
    tables = list(t[:5]) + [t.xw.T]                                  # the x weights tap-major, as the entry point takes them
    return head + b''.join(np.ascontiguousarray(a).tobytes() for a in tables) + rgb.tobytes() + want.tobytes(), 3 * Ho * Wo


def test_arithmetic_under_address_sanitizer(tmp_path):
    cxx = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'frame_hostcheck')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
                           os.path.join(ROOT, 'tools', 'frame_hostcheck.cpp')])
    cases = [hostcheck_case(21, 30, (2.5, 1.25, 17.5, 26.0), 6, (9, 7), 'area', 1),
             hostcheck_case(24, 60, None, 7, (3, 5), 'lanczos', 2),
             hostcheck_case(5, 7, None, 4, (13, 17), 'lanczos', 3)]
    path = str(tmp_path / 'cases.bin')
    with open(path, 'wb') as fh:
        fh.write(struct.pack('<I', len(cases)) + b''.join(c for c, _ in cases))
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and 'hostcheck OK' in r.stdout, r.stdout
    assert '%d outputs of 3 cases' % sum(n for _, n in cases) in r.stdout and '6000 single-field corruptions' in r.stdout
