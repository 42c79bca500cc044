"""CPU tests of the full-resolution renders: the NumPy restatement (tests/demosaic_ref.py) has the properties a demosaic must have
(sampled values pass through, constant colours come back exact, it beats binning + replication on a synthetic scene), the compile-time
X-Trans tables of csrc/demosaic.hip equal a brute-force scan of the cell, and denoise_raw refuses bad srgb_size arguments before any
device work.  The kernels themselves are compared with the restatement in tests/test_demosaic_gpu.py."""
import ctypes
import types

import numpy as np
import pytest

import demosaic_ref as D

F32 = np.float32
PATTERNS = [[[0, 1], [3, 2]], [[2, 3], [1, 0]], [[1, 0], [2, 3]], [[3, 2], [0, 1]]]      # RGGB, BGGR, GRBG, GBRG


# ---- 1. sampled values pass through ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pat', PATTERNS)
def test_bayer_sampled_values_pass_through(pat):
    rng = np.random.default_rng(1)
    p = rng.uniform(0, 1, size=(2, 4, 9, 13)).astype(F32)
    rgb = D.linear_bayer(p, pat, np.ones((2, 4), F32))
    m = D.mosaic_bayer(p, pat, np.ones((2, 4), F32))
    col = D.bayer_colour_map(pat, 18, 26)
    assert rgb.dtype == F32 and rgb.shape == (2, 3, 18, 26)
    for k in range(3):
        assert np.array_equal(rgb[:, k][:, col == k], m[:, col == k])
    for k in range(4):                                      # ... and every plane sits where raw_pattern puts it
        (oy,), (ox,) = np.where(np.asarray(pat) == k)
        assert np.array_equal(rgb[:, D.CODE_COLOUR[k], oy::2, ox::2], p[:, k])


def test_xtrans_sampled_values_pass_through():
    rng = np.random.default_rng(2)
    p = rng.uniform(0, 1, size=(2, 9, 4, 6)).astype(F32)
    rgb = D.linear_xtrans(p, np.ones((2, 3), F32))
    m = D.mosaic_xtrans(p, np.ones((2, 3), F32))
    col = D.xtrans_colour_map(12, 18)
    assert rgb.dtype == F32 and rgb.shape == (2, 3, 12, 18)
    for k in range(3):
        assert np.array_equal(rgb[:, k][:, col == k], m[:, col == k])


# ---- 2. constant colours come back exact, borders included ----------------------------------------------------------------------------------
CONST = [(37 / 256, 201 / 256, 90 / 256), (1.0, 0.0, 3 / 256), (128 / 256, 129 / 256, 255 / 256)]


@pytest.mark.parametrize('pat', PATTERNS)
@pytest.mark.parametrize('hw', [(2, 2), (5, 7)])
def test_bayer_constant_colour_is_exact(pat, hw):
    h, w = hw
    p = np.zeros((len(CONST), 4, h, w), F32)
    for i, rgb in enumerate(CONST):
        for k in range(4):
            p[i, k] = rgb[D.CODE_COLOUR[k]]
    out = D.linear_bayer(p, pat, np.ones((len(CONST), 4), F32))
    for i, rgb in enumerate(CONST):
        for k in range(3):
            assert np.all(out[i, k] == F32(rgb[k])), (i, k)


@pytest.mark.parametrize('hw', [(2, 2), (2, 6), (4, 4), (6, 8)])
def test_xtrans_constant_colour_is_exact(hw):
    h, w = hw
    p = np.zeros((len(CONST), 9, h, w), F32)
    for i, rgb in enumerate(CONST):
        for k in range(9):
            p[i, k] = rgb[D.PLANE_COLOUR[k]]
    out = D.linear_xtrans(p, np.ones((len(CONST), 3), F32))
    for i, rgb in enumerate(CONST):
        for k in range(3):
            assert np.all(out[i, k] == F32(rgb[k])), (i, k)


# ---- 3. the kernel's compile-time tables -----------------------------------------------------------------------------------------------
def test_xtrans_phase_tables_equal_a_brute_force_scan(eld_lib):
    buf = (ctypes.c_int * 288)()
    assert eld_lib.eld_debug_xtrans_demosaic_tables(buf, 288) == 0
    got = np.frombuffer(buf, dtype=np.int32).reshape(36, 8).astype(np.int64)
    assert np.array_equal(got, D.xtrans_phase_tables())
    assert eld_lib.eld_debug_xtrans_demosaic_tables(buf, 287) == -1 and eld_lib.eld_debug_xtrans_demosaic_tables(None, 288) == -1
    cell = D.xtrans_cell_colours()
    assert [int((cell == k).sum()) for k in range(3)] == [8, 20, 8]


def test_xtrans_window_coverage():
    """Every frame of whole cells from 6 x 6 to 18 x 24: every clipped 3x3 window holds a G site, every clipped 5x5 window an R and a B
    site -- the corner of the GG/GG block included, where a 3x3 window holds no R or B."""
    for Hm in (6, 12, 18):
        for Wm in (6, 12, 18, 24):
            col = D.xtrans_colour_map(Hm, Wm)
            for y in range(Hm):
                for x in range(Wm):
                    w3 = col[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2]
                    w5 = col[max(y - 2, 0):y + 3, max(x - 2, 0):x + 3]
                    assert (w3 == 1).any() and (w5 == 0).any() and (w5 == 2).any(), (Hm, Wm, y, x)
    col = D.xtrans_colour_map(12, 12)
    assert (col[10:, :2] == 1).all()                        # the clipped 3x3 window of the bottom-left corner: the GG/GG block, no R, no B


# ---- 4. quality against the parent's only render -----------------------------------------------------------------------------------------
def scene(H=384, W=480, seed=7):
    """a smooth RGB scene with step edges: low-frequency sinusoids per channel, a few rectangles and a diagonal half-plane of other colours"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.stack([0.45 + 0.25 * np.sin(yy / rng.uniform(30, 60) + rng.uniform(0, 6)) * np.cos(xx / rng.uniform(30, 60) + rng.uniform(0, 6))
                    + 0.1 * np.sin((xx + yy) / rng.uniform(15, 25)) for _ in range(3)])
    for _ in range(12):
        y0, x0 = int(rng.integers(0, H - 40)), int(rng.integers(0, W - 40))
        hh, ww = int(rng.integers(17, 90)), int(rng.integers(17, 90))
        img[:, y0:y0 + hh, x0:x0 + ww] = rng.uniform(0.1, 0.9, size=(3, 1, 1))
    half = (xx * 0.6 + yy) > 0.9 * H
    img = np.where(half[None], 0.6 * img + 0.4 * rng.uniform(0.1, 0.9, size=(3, 1, 1)), img)
    return np.clip(img, 0.0, 1.0)


def psnr(a, b):
    return float(10 * np.log10(1.0 / np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def test_bayer_quality_beats_binning():
    img = scene()
    _, H, W = img.shape
    for pat in (PATTERNS[0], PATTERNS[2]):
        p = np.zeros((1, 4, H // 2, W // 2))
        for k in range(4):
            (oy,), (ox,) = np.where(np.asarray(pat) == k)
            p[0, k] = img[D.CODE_COLOUR[k], oy::2, ox::2]
        ones = np.ones((1, 4))
        base = psnr(D.binning_replicated_bayer(p, ones)[0], img)
        full64 = psnr(D.linear_bayer(p, pat, ones, dtype=np.float64)[0], img)
        full32 = psnr(D.linear_bayer(p.astype(F32), pat, ones)[0], img)
        print('bayer PSNR: binning + replication %.2f dB, Malvar float64 %.2f dB, float32 %.2f dB' % (base, full64, full32))
        assert full64 > base
        assert full32 >= base + 0.5 * (full64 - base)


def test_xtrans_quality_beats_binning():
    img = scene()
    _, H, W = img.shape
    h, w = H // 3, W // 3
    rows, cols = D.O.xtrans_source_index(h, w)
    p = np.stack([img[D.PLANE_COLOUR[k], rows[k], cols[k]] for k in range(9)])[None]
    ones = np.ones((1, 3))
    base = psnr(D.binning_replicated_xtrans(p, ones)[0], img)
    full64 = psnr(D.linear_xtrans(p, ones, dtype=np.float64)[0], img)
    full32 = psnr(D.linear_xtrans(p.astype(F32), ones)[0], img)
    print('xtrans PSNR: binning + replication %.2f dB, normalised convolution float64 %.2f dB, float32 %.2f dB' % (base, full64, full32))
    assert full64 > base
    assert full32 >= base + 0.5 * (full64 - base)


# ---- 5. denoise_raw argument handling -----------------------------------------------------------------------------------------------------
class FakeNet:
    def parameters(self):
        raise AssertionError('device work before the argument checks')


def fake(cfa):
    from eld_amd.denoise import PLANES
    return types.SimpleNamespace(cfa=cfa, in_channels=PLANES[cfa], out_channels=PLANES[cfa], net=FakeNet())


@pytest.mark.parametrize('cfa', ['bayer', 'xtrans'])
@pytest.mark.parametrize('kw,msg', [
    (dict(srgb_size='mosaic'), 'srgb_size'),
    (dict(srgb_size=None), 'srgb_size'),
    (dict(srgb_size='full'), 'wb and ccm'),
    (dict(srgb_size='full', wb=[2.0, 1.0, 1.5]), 'wb and ccm'),
    (dict(srgb_size='full', ccm=np.eye(3)), 'wb and ccm'),
    (dict(linear=True, wb=[2.0, 1.0, 1.5], ccm=np.eye(3)), 'linear'),
])
def test_denoise_raw_srgb_size_errors(cfa, kw, msg):
    from eld_amd.denoise import denoise_raw
    with pytest.raises(ValueError, match=msg):
        denoise_raw(fake(cfa), np.full((12, 24), 1100, np.uint16), cfa, **kw)


def test_denoise_raw_full_needs_a_bayer_pattern_with_diagonal_greens():
    from eld_amd.denoise import denoise_raw
    with pytest.raises(ValueError, match='diagonal'):
        denoise_raw(fake('bayer'), np.full((12, 24), 1100, np.uint16), 'bayer', raw_pattern=[[0, 2], [1, 3]], wb=[2.0, 1.0, 1.5], ccm=np.eye(3),
                    srgb_size='full')


def test_cli_srgb_size():
    from eld_amd.denoise import parse_args
    base = ['--ckpt', 'm.pt', 'a.npy', '-o', 'x']
    assert parse_args(base)[3]['srgb_size'] == 'packed'
    colour = ['--wb', '2', '1', '1.5', '--ccm', '1', '0', '0', '0', '1', '0', '0', '0', '1']
    assert parse_args(base + colour + ['--srgb-size', 'full'])[3]['srgb_size'] == 'full'
    with pytest.raises(ValueError, match='srgb-size full'):
        parse_args(base + ['--srgb-size', 'full'])
    with pytest.raises(SystemExit):
        parse_args(base + colour + ['--srgb-size', 'huge'])
