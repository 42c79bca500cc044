"""GPU tests of the frame (csrc/frame.hip through eld_amd.isp.frame_rgb) against the NumPy restatement tests/frame_ref.py,
bit for bit, and of the frame through the renders and denoise_raw.

Every direct call writes into a buffer between guard bands (tests/guarded.py) and gets a workspace that is NaN before the call (the guard's
fill), so a horizontal sum the row pass does not write, or a store outside the output, shows.  The pixel tests feed the PACKAGE's tap tables
to the restatement's sums: the tables themselves are compared on the CPU (tests/test_frame_cpu.py), where 'lanczos' may differ by an ulp
between two libraries' sin.

Shapes, the smallest at which the kernels can go wrong: 37 x 53 with a fractional crop to 11 x 17 (one column-pass tile, partly empty, all
eight orientations); 70 x 300 -> 3 x 5 (hundreds of taps per output, far more than a tile, clipped by the image on every side); 5 x 7 ->
23 x 31 (enlarging: neighbouring outputs share taps); 6 x 5000 -> 3 x 200 and 3 x 300 (wide tables, which the row pass stages in LDS: a span
of more than two chunks, a second workgroup); one output more than the column pass's tile in each direction (a second tile of one
row and one column, through the LDS transpose too)."""
import functools

import numpy as np
import pytest

import demosaic_ref as DM
import frame_ref as R
from guarded import Guards

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def isp(eld_lib):
    import torch
    if not torch.cuda.is_available():
        pytest.fail('these tests need a GPU')
    from eld_amd import isp
    return isp


@functools.lru_cache(maxsize=None)
def frames(N, Hs, Ws):
    """(camera RGB in [-0.1, 1.1], per-frame matrices that differ), computed once and left unchanged"""
    rng = np.random.default_rng(1000 * Hs + Ws)
    rgb = rng.uniform(-0.1, 1.1, (N, 3, Hs, Ws)).astype(np.float32)
    ccms = (np.eye(3)[None] * rng.uniform(1.2, 1.7, size=(N, 1, 1)) + rng.uniform(-0.35, 0.1, size=(N, 3, 3))).astype(np.float32)
    rgb.setflags(write=False)
    ccms.setflags(write=False)
    return rgb, ccms


def same_bits(t, want):
    a, b = t.cpu().numpy(), np.ascontiguousarray(want)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def run(isp, rgb, frame, ccms=None, linear=False, **kw):
    """frame_rgb on guarded buffers with a NaN workspace -> (the output tensor, the package's tables, (Ho, Wo))"""
    import torch
    N, _, Hs, Ws = rgb.shape
    t, (Ho, Wo) = frame.taps(Hs, Ws)
    Wc = Ho if frame.orientation >= 5 else Wo
    rows = int((t.ystart + t.ycount).max()) - int(t.ystart.min())
    g = Guards()
    x = g.ro(torch.from_numpy(np.array(rgb)).cuda(), 'rgb')
    m = None if ccms is None else g.ro(torch.from_numpy(np.array(ccms)).cuda().reshape(N, 9), 'ccms')
    out = g.new((N, 3, Ho, Wo), torch.float32 if linear else torch.uint8, 'out')
    ws = g.new((N * 3 * rows * Wc,), torch.float32, 'workspace')
    assert bool(torch.isnan(ws).all())
    got = isp.frame_rgb(x, frame, m, linear=linear, out=out, workspace=ws, **kw)
    torch.cuda.synchronize()
    g.check()
    assert got.data_ptr() == out.data_ptr()
    return got, tuple(t), (Ho, Wo)


def check(isp, rgb, frame, ccms, what, modes=(True, False)):
    for linear in modes:
        got, tables, (Ho, Wo) = run(isp, rgb, frame, ccms, linear)
        want = R.frame_linear(rgb, tables, frame.orientation, ccms) if linear else R.frame_srgb8(rgb, tables, frame.orientation, ccms)
        assert want.shape == (rgb.shape[0], 3, Ho, Wo)
        assert same_bits(got, want), (what, 'linear' if linear else 'srgb8')


# ---- the identity ties the frame to the renders -----------------------------------------------------------------------------------------------
def packed_inputs(N, planes, h, w, seed, gains):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.2, 1.3, size=(N, planes, h, w)).astype(np.float32)
    wbs = rng.uniform(0.7, 2.2, size=(N, gains)).astype(np.float32)
    ccms = (np.eye(3)[None] * rng.uniform(1.2, 1.7, size=(N, 1, 1)) + rng.uniform(-0.35, 0.1, size=(N, 3, 3))).astype(np.float32)
    return p, wbs, ccms


@pytest.mark.parametrize('cfa', ('bayer', 'xtrans'))
def test_identity_frame_gives_the_renders_own_output(isp, cfa):
    """the full rectangle at its own size, orientation 1, 'area': single taps of weight 1, so the three tails see the render's camera RGB"""
    import torch
    if cfa == 'bayer':
        p, wbs, ccms = packed_inputs(2, 4, 9, 14, 7, 4)
        render = lambda c, **kw: isp.render_bayer(x, [[2, 3], [1, 0]], wbs, c, **kw)
    else:
        p, wbs, ccms = packed_inputs(2, 9, 4, 6, 8, 3)
        render = lambda c, **kw: isp.render_xtrans(x, wbs, c, **kw)
    x = torch.from_numpy(p).cuda()
    cam = render(None, linear=True)
    ident = isp.Frame()
    assert ident.identity and not isp.Frame(orientation=3).identity
    for kw in (dict(), dict(gamma=2.0), dict(linear=True)):
        want = render(ccms, **kw).cpu().numpy()
        assert same_bits(render(ccms, frame=ident, **kw), want), (cfa, sorted(kw))
        got, _, _ = run(isp, cam.cpu().numpy(), ident, ccms, **kw)
        assert same_bits(got, want), (cfa, sorted(kw))
    got, _, _ = run(isp, cam.cpu().numpy(), ident, None, linear=True)
    assert same_bits(got, cam.cpu().numpy())
    with pytest.raises(ValueError, match='cam2rgbs'):
        render(None, frame=ident)
    with pytest.raises(ValueError, match='Frame'):
        isp.frame_rgb(cam, {'orientation': 1}, ccms)
    with pytest.raises(ValueError, match='CUDA'):
        isp.frame_rgb(cam.cpu(), ident, ccms)


# ---- every orientation ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('o', range(1, 9))
def test_every_orientation_in_both_output_modes(isp, o):
    rgb, ccms = frames(2, 37, 53)
    assert not np.array_equal(ccms[0], ccms[1])
    check(isp, rgb, isp.Frame(crop=(2.5, 1.25, 30.5, 48.0), orientation=o, size=(11, 17), filter='area'), ccms, o)


def test_orientations_differ_and_are_rearrangements(isp):
    """the eight outputs hold the same multiset of values, and no two of them are the same picture"""
    rgb, _ = frames(2, 37, 53)
    outs = [run(isp, rgb, isp.Frame(crop=(2.5, 1.25, 30.5, 48.0), orientation=o, size=(11, 17) if o <= 4 else (17, 11)), None, True)[0].cpu().numpy()
            for o in range(1, 9)]
    for o, a in enumerate(outs, 1):
        assert np.array_equal(np.sort(a.reshape(-1)), np.sort(outs[0].reshape(-1))), o
        assert a.shape[-2:] == ((11, 17) if o <= 4 else (17, 11))
        for b in outs[:o - 1]:
            assert a.shape != b.shape or not np.array_equal(a, b)


# ---- strong reduction, enlarging, the tile's edge ---------------------------------------------------------------------------------------------
def test_strong_reduction_clipped_by_the_image(isp):
    rgb, ccms = frames(1, 70, 300)
    f = isp.Frame(orientation=7, size=(3, 5), filter='lanczos')
    t, _ = f.taps(70, 300)
    th, tw = isp.frame_tile()
    assert t.xw.shape == (3, 300) and t.yw.shape[0] == 5 and t.yw.shape[1] > th and t.xw.shape[1] > tw        # the taps outrun any tile
    assert (t.xstart == 0).all() and (t.xcount == 300).all()          # ... and are clipped: every output column reads whole source rows,
    assert int(t.ystart.min()) == 0 and int((t.ystart + t.ycount).max()) == 70 and int(t.ycount.min()) < int(t.ycount.max())        # rows are cut at both ends
    check(isp, rgb, f, ccms, 'reduction')


@pytest.mark.parametrize('flt', ('area', 'lanczos'))
def test_rows_wider_than_a_staged_chunk(isp, flt):
    """5000 columns to 200: 25 and 150 taps, so the row pass stages its span in LDS, and one workgroup's span, the whole row, is more than two
    of its chunks of 2048 elements; a second workgroup takes the last 44 outputs of 300"""
    rgb, ccms = frames(1, 6, 5000)
    check(isp, rgb, isp.Frame(size=(3, 200), filter=flt), ccms, flt, modes=(True,))
    check(isp, rgb, isp.Frame(crop=(0, 100.5, 6, 4800.25), size=(3, 300), filter=flt), ccms, flt, modes=(True,))


@pytest.mark.parametrize('flt', ('area', 'lanczos'))
def test_enlarging(isp, flt):
    rgb, ccms = frames(1, 5, 7)
    check(isp, rgb, isp.Frame(size=(23, 31), filter=flt), ccms, flt)


@pytest.mark.parametrize('o', (1, 6))
def test_one_output_past_the_tile_in_each_direction(isp, o):
    th, tw = isp.frame_tile()
    rgb, ccms = frames(1, th + 9, tw + 14)
    f = isp.Frame(crop=(1.5, 2.0, th + 6.25, tw + 11.0), orientation=o, size=(th + 1, tw + 1) if o <= 4 else (tw + 1, th + 1), filter='area')
    t, _ = f.taps(th + 9, tw + 14)
    assert len(t.ystart) == th + 1 and len(t.xstart) == tw + 1
    check(isp, rgb, f, ccms, o)


# ---- NaN and -0.0 -----------------------------------------------------------------------------------------------------------------------------
def test_nan_and_negative_zero_land_where_the_restatement_puts_them(isp):
    rgb = np.array(frames(1, 37, 53)[0])
    rgb[0, 1, 20, 31] = np.nan
    rgb[0, 2, 5, 7] = -0.0
    # resampled: the NaN reaches exactly the outputs whose tap ranges hold (20, 31), in its plane only
    for o in (1, 6):
        f = isp.Frame(crop=(2.5, 1.25, 30.5, 48.0), orientation=o, size=(11, 17), filter='area')
        got, tables, (Ho, Wo) = run(isp, rgb, f, None, True)
        want = R.frame_linear(rgb, tables, o)
        assert same_bits(got, want), o
        Hc, Wc = (Ho, Wo) if o <= 4 else (Wo, Ho)
        hit = np.zeros((Ho, Wo), bool)
        for Y in range(Ho):
            for X in range(Wo):
                rows, cols = R.footprint(tables, o, Y, X, Hc, Wc)
                hit[Y, X] = 20 in rows and 31 in cols
        g = got.cpu().numpy()
        assert np.array_equal(np.isnan(g[0, 1]), hit) and 1 <= hit.sum() <= 4 and not np.isnan(g[0, 0]).any() and not np.isnan(g[0, 2]).any()
    # an integer crop at its own size, turned by 180 degrees: single taps of weight 1, so both values pass through with their bits
    f = isp.Frame(crop=(2, 3, 30, 40), orientation=3)
    got, tables, _ = run(isp, rgb, f, None, True)
    assert same_bits(got, R.frame_linear(rgb, tables, 3))
    g = got.cpu().numpy()
    assert same_bits(got, rgb[:, :, 2:32, 3:43][:, :, ::-1, ::-1])
    assert np.isnan(g[0, 1, 29 - 18, 39 - 28]) and np.isnan(g).sum() == 1
    assert g[0, 2, 29 - 3, 39 - 4] == 0 and np.signbit(g[0, 2, 29 - 3, 39 - 4])


# ---- denoise_raw end to end -------------------------------------------------------------------------------------------------------------------
class Stub:
    """a denoiser that returns a fixed packed frame (the classical denoisers' interface: no network)"""
    is_classical, cfa, in_channels, out_channels = True, 'bayer', 4, 4

    def __init__(self, packed):
        self.packed = packed

    def denoise_codes(self, *args):
        return self.packed


def test_denoise_raw_frames_the_render_and_the_jpegs(isp):
    import io
    import torch
    from eld_amd import denoise
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:24, 0:32]
    base = 0.45 + 0.35 * np.sin(xx / 4.0) * np.cos(yy / 5.0)
    packed = torch.from_numpy((base[None, None] + rng.uniform(-0.01, 0.01, (1, 4, 24, 32))).astype(np.float32)).cuda()
    mosaic = rng.integers(512, 4000, (48, 64)).astype(np.uint16)
    ccm = np.eye(3) * 1.4 - 0.1
    kw = dict(raw_pattern=[[0, 1], [3, 2]], black_level=512, white_point=4095, wb=(2.0, 1.0, 1.5), ccm=ccm, srgb_size='full')
    frame = isp.Frame(crop=(4, 6, 40, 50), orientation=6, size=20)
    assert frame.taps(48, 64)[1] == (20, 16)                          # upright: the 50 columns become the long, vertical edge
    plain = denoise.denoise_raw(Stub(packed), mosaic, 'bayer', **kw)
    res = denoise.denoise_raw(Stub(packed), mosaic, 'bayer', frame=frame, jpeg={}, **kw)
    assert res['srgb'].shape == (1, 3, 20, 16) and plain['srgb'].shape == (1, 3, 48, 64)
    assert np.array_equal(res['mosaic'], plain['mosaic']) and np.array_equal(res['packed'], plain['packed']) and 'preview' not in res
    wbs, ccms = denoise.colour_args('bayer', kw['wb'], ccm, 1)
    cam = isp.render_bayer(packed, [0, 1, 3, 2], wbs, None, linear=True)
    assert np.array_equal(res['srgb'], isp.frame_rgb(cam, frame, ccms).cpu().numpy())
    assert np.array_equal(res['srgb'], R.frame_srgb8(cam.cpu().numpy(), tuple(frame.taps(48, 64)[0]), 6, ccms))
    lin = denoise.denoise_raw(Stub(packed), mosaic, 'bayer', frame=frame, linear=True, **kw)
    assert same_bits(torch.from_numpy(lin['linear']), R.frame_linear(cam.cpu().numpy(), tuple(frame.taps(48, 64)[0]), 6, ccms))
    assert np.array_equal(lin['srgb'], res['srgb'])
    unturned = isp.Frame(crop=(4, 6, 40, 50), orientation=1, size=(16, 20))
    both = denoise.denoise_raw(Stub(packed), mosaic, 'bayer', frame=frame, preview_frame=unturned, jpeg={'quality': 85, 'subsampling': '444'}, **kw)
    assert np.array_equal(both['srgb'], res['srgb']) and len(both['jpeg']) == 1 and len(both['preview']) == 1
    only = denoise.denoise_raw(Stub(packed), mosaic, 'bayer', preview_frame=unturned, jpeg={'quality': 85, 'subsampling': '444'}, **kw)
    assert np.array_equal(only['srgb'], plain['srgb']) and only['preview'] == both['preview']
    try:
        from PIL import Image
    except ImportError:
        return
    assert Image.open(io.BytesIO(res['jpeg'][0])).size == (16, 20)    # PIL: (width, height)
    assert Image.open(io.BytesIO(both['jpeg'][0])).size == (16, 20)
    pv = Image.open(io.BytesIO(both['preview'][0]))
    assert pv.size == (20, 16)
    # the preview is the picture's own content, unturned: turning it as orientation 6 says (a quarter turn clockwise) gives the upright JPEG's
    # pixels up to two quality-85 encodes of a smooth picture, a few codes each; any other turn of this sine pattern (amplitude 0.35 of
    # full scale) is tens of codes away on average
    a = np.asarray(pv.convert('RGB'), np.float64)
    b = np.asarray(Image.open(io.BytesIO(both['jpeg'][0])).convert('RGB'), np.float64)
    assert np.abs(np.rot90(a, -1) - b).mean() < 8.0


def test_command_line_frames_the_picture_and_carries_the_tags(isp, tmp_path):
    """classical.main (no checkpoint) on a DNG with Orientation 6 and a rational default crop: --crop default --orient auto against frame_rgb
    on the unframed run's camera RGB; the written DNG keeps both tags and its preview is cropped, small and not turned"""
    import torch
    import dng_ref as DR
    import eld_amd.dng as D
    from eld_amd import classical, denoise
    rng = np.random.default_rng(4)
    yy, xx = np.mgrid[0:48, 0:64]
    img = np.clip(900 + 600 * np.sin(xx / 5.0) * np.cos(yy / 7.0) + rng.normal(0, 20, (48, 64)), 512, 4095).astype(np.uint16)
    CM = ((8000, 10000), (-2000, 10000), (-500, 10000), (-3000, 10000), (11000, 10000), (2000, 10000), (-500, 10000), (1500, 10000), (6000, 10000))
    path = str(tmp_path / 'f.dng')
    DR.write_dng_file(path, img, bits=12, tags={50714: (DR.SHORT, (512,)), 50717: (DR.LONG, (4095,)), 50719: (DR.RATIONAL, ((9, 2), (3, 1))),
                                                50720: (DR.RATIONAL, ((111, 2), (40, 1)))},
                      tags0={50728: (DR.RATIONAL, ((1, 2), (1, 1), (2, 3))), 50721: (DR.SRATIONAL, CM), 50778: (DR.SHORT, (21,)), 274: (DR.SHORT, (6,))})
    args = ['--method', 'nlm', '--K', '2.0', '--sigma', '3.0', '--srgb-size', 'full']
    plain, framed = str(tmp_path / 'plain'), str(tmp_path / 'framed')
    assert classical.main([path, '-o', plain] + args) == 0
    assert classical.main([path, '-o', framed, '--crop', 'default', '--orient', 'auto', '--size', '20', '--dng', '--dng-preview',
                           '--dng-preview-size', '16', '--jpeg', '85'] + args) == 0
    den = {d: np.load('%s/f_denoised.npy' % d) for d in (plain, framed)}
    assert np.array_equal(den[plain], den[framed]) and den[plain].shape == (48, 64)          # the mosaic is not framed
    srgb = np.load(framed + '/f_srgb.npy')
    frame = isp.Frame(crop=(3.0, 4.5, 40.0, 55.5), orientation=6, size=20)
    assert srgb.shape == (20, 14, 3) and frame.taps(48, 64)[1] == (20, 14)
    # the prediction: the same denoiser through denoise_raw without a frame -> its packed output -> camera RGB -> frame_rgb
    a = classical.parse_method_args(classical.build_parser(), [path, '-o', str(tmp_path / 'unused')] + args)
    o = denoise.options_from(a)[3]
    dn = classical.ClassicalDenoiser('bayer', 2.0, sigma=3.0, camera=None, search=a.search, patch=a.patch, strength=a.strength, method='nlm', step=a.step,
                                     group=a.group, mix=None)
    kw = {k: o.get(k) for k in ('raw_pattern', 'black_level', 'white_point', 'ratio', 'wb', 'ccm', 'chop', 'rounding', 'srgb_size')}
    res = denoise.denoise_raw(dn, img, 'bayer', **kw)
    wbs, ccms = denoise.colour_args('bayer', o['wb'], o['ccm'], 1)
    cam = isp.render_bayer(torch.from_numpy(res['packed']).cuda(), np.asarray(o['raw_pattern']).reshape(-1).tolist(), wbs, None, linear=True)
    want = R.frame_srgb8(cam.cpu().numpy(), tuple(frame.taps(48, 64)[0]), 6, ccms)
    assert np.array_equal(np.moveaxis(want, 1, -1)[0], srgb)
    m = D.dng_meta(framed + '/f_denoised.dng')
    assert m['orientation'] == 6 and m['default_crop'] == [3, 4.5, 40, 55.5]
    back, _ = D.read_dng(framed + '/f_denoised.dng')
    assert np.array_equal(back, den[framed])
    t, buf = D.parse_tiff(framed + '/f_denoised.dng')
    assert (D._get1(t.ifd0, D.T_LENGTH), D._get1(t.ifd0, D.T_WIDTH)) == (12, 16)               # the crop's 40 x 55.5 at a long edge of 16, unturned
    try:
        from PIL import Image
    except ImportError:
        return
    assert Image.open(framed + '/f_srgb.jpg').size == (14, 20)
