"""GPU tests of the directional X-Trans render (csrc/demosaic_xdir.hip eld_render_xtrans_dir, eld_amd.isp.render_xtrans(demosaic='directional'),
denoise_raw(demosaic='directional')): the linear output bit for bit against the NumPy float32 restatement
(tests/demosaic_xdir_ref.py), the 8-bit codes, guarded buffers, agreement with the default render on frames of constant colour, the identity
warp, determinism, the refusals, and denoise_raw / the command line / jpeg= end to end.

Packed shapes, the smallest at which the kernel can go wrong: 2 x 2 (one cell: every site is border and the extension folds twice), 2 x 4,
4 x 2, 6 x 10 (every border inside one tile), and tile + 2 x tile + 6 from the kernel's own constants (two tiles down, two across, ragged last
tiles both ways).  Two frames everywhere (the batch stride)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import demosaic_ref as D              # noqa: E402
import demosaic_xdir_ref as X         # noqa: E402
import jpeg_ref as R                  # noqa: E402
import warp_ref as W                  # noqa: E402
from guarded import Guards            # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SMALL = [(2, 2), (2, 4), (4, 2), (6, 10)]
CRF_E = np.linspace(0, 1, 1024, dtype=F32)
CRF = (CRF_E, (CRF_E ** 0.45).astype(F32))


@pytest.fixture(scope='module')
def lib(eld_lib):
    assert torch.cuda.is_available()
    return eld_lib


def tile_shape():
    from eld_amd.isp import xdir_tile
    th, tw = xdir_tile()
    assert th >= 2 and tw >= 2 and th % 2 == 0 and tw % 2 == 0
    return th + 2, tw + 6                                   # one cell below the first tile, three cells right of it


def inputs(h, w, seed, N=2):
    """packed values in [-0.1, 1.3] with both ends present, per-frame gains that differ and drive sites to both clamps, per-frame matrices"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.1, 1.3, size=(N, 9, h, w)).astype(F32)
    p[:, 0, 0, 0], p[:, 1, 0, 0] = -0.1, 1.3
    wbs = rng.uniform(0.8, 2.2, size=(N, 3)).astype(F32)
    assert N < 2 or not np.array_equal(wbs[0], wbs[1])
    ccms = (np.eye(3)[None] * rng.uniform(1.2, 1.7, size=(N, 1, 1)) + rng.uniform(-0.35, 0.1, size=(N, 3, 3))).astype(F32)
    return p, wbs, ccms


def dev(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()           # a copy: the shared references are read-only


def bits_equal(got, want):
    return got.shape == want.shape and got.dtype == want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


_REF = {}


def reference(h, w):
    """(inputs, restatement with the matrix, restatement without) of one shape: computed once, shared, never written to"""
    if (h, w) not in _REF:
        p, wbs, ccms = inputs(h, w, 200 + 3 * h + w)
        m = D.mosaic_xtrans(p, wbs)
        for n in range(p.shape[0]):
            assert m[n].min() == 0.0 and m[n].max() == 1.0           # both clamps, in every frame
        cam = X.linear_xtrans_dir(p, wbs)
        lin = D.apply_ccm(cam, ccms)
        for a in (p, cam, lin):
            a.setflags(write=False)
        _REF[(h, w)] = (p, wbs, ccms, lin, cam)
    return _REF[(h, w)]


# ---- 1. linear output, bit for bit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', SMALL + ['tile'])
def test_linear_equals_the_restatement(lib, hw):
    from eld_amd.isp import render_xtrans
    h, w = tile_shape() if hw == 'tile' else hw
    p, wbs, ccms, lin, cam = reference(h, w)
    x = dev(p)
    got = render_xtrans(x, wbs, ccms, linear=True, demosaic='directional')
    assert got.dtype == torch.float32 and got.shape == (2, 3, 3 * h, 3 * w) and got.is_cuda
    assert bits_equal(got.cpu().numpy(), lin)
    assert bits_equal(render_xtrans(x, wbs, None, linear=True, demosaic='directional').cpu().numpy(), cam)       # camera RGB
    assert not np.array_equal(cam, D.linear_xtrans(p, wbs))                                                          # ... not the default render's


# ---- 2. the 8-bit codes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', SMALL + ['tile'])
def test_srgb8_codes_at_gamma_22(lib, hw):
    """gamma 2.2 (the threshold table): every code equal"""
    from eld_amd.isp import render_xtrans
    h, w = tile_shape() if hw == 'tile' else hw
    p, wbs, ccms, lin, _ = reference(h, w)
    got = render_xtrans(dev(p), wbs, ccms, demosaic='directional').cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == lin.shape
    assert np.array_equal(got, D.srgb8(lin))


def test_srgb8_codes_other_gamma_and_crf(lib):
    """another gamma and a CRF at the existing X-Trans test's 88 x 134: the rule and the cap of tests/test_demosaic_gpu.py check_codes (at most
    one code off on at most ISP_CAP of the values: the tail is shared code)"""
    from test_demosaic_gpu import check_codes
    from eld_amd.isp import render_xtrans
    p, wbs, ccms, lin, _ = reference(88, 134)
    x = dev(p)
    check_codes(lambda **kw: render_xtrans(x, wbs, ccms, demosaic='directional', **kw), lin)


# ---- 3. guarded, poisoned buffers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', [(2, 2), (6, 10), 'tile'])
def test_guarded_buffers(lib, hw):
    """every operand between guard bands of NaN, the outputs poisoned with 0xFF (NaN): nothing outside is written, every element inside is, and
    no NaN (a read outside an input) reaches the result"""
    from eld_amd import _lib as L
    h, w = tile_shape() if hw == 'tile' else hw
    p, wbs, ccms, lin, _ = reference(h, w)
    g = Guards()
    x, wb, cm = g.ro(dev(p), 'packed'), g.ro(dev(wbs), 'wbs'), g.ro(dev(ccms.reshape(2, 9)), 'ccms')
    o32 = g.new((2, 3, 3 * h, 3 * w), torch.float32, 'linear out')
    o8 = g.new((2, 3, 3 * h, 3 * w), torch.uint8, 'srgb out')
    for out, mode in ((o32, L.RENDER_LINEAR_F32), (o8, L.RENDER_SRGB8)):
        L.check(lib.eld_render_xtrans_dir(L.dptr(x), L.dptr(wb), L.dptr(cm), L.dptr(out), mode, 2, h, w, 2.2, None, None, 0, L.cur_stream()),
                'eld_render_xtrans_dir')
    torch.cuda.synchronize()
    g.check()
    got = o32.cpu().numpy()
    assert not np.isnan(got).any()
    assert bits_equal(got, lin) and np.array_equal(o8.cpu().numpy(), D.srgb8(lin))


# ---- 4. agreement with the default render where both are exact ---------------------------------------------------------------------------------
def test_constant_colour_gives_the_codes_of_the_default_render(lib):
    """frames of one colour on the 2^-8 grid with gains from GAINS: both demosaics return the colour exactly, so both renders write one code --
    which pins the gain-by-colour mapping and the tail"""
    from test_demosaic_gpu import constant_frames
    from eld_amd.isp import render_xtrans
    for h, w in ((2, 2), (4, 6), tile_shape()):
        p, wbs, ccms = constant_frames(9, D.PLANE_COLOUR, h, w, 3, 70 + h)
        x = dev(p)
        for kw in (dict(), dict(CRF=CRF), dict(gamma=2.7), dict(linear=True)):
            xdir = render_xtrans(x, wbs, ccms, demosaic='directional', **kw)
            assert torch.equal(xdir, render_xtrans(x, wbs, ccms, **kw)), (h, w, sorted(kw))
            for n in range(p.shape[0]):
                for c in range(3):
                    assert float(xdir[n, c].min()) == float(xdir[n, c].max()), (h, w, n, c)


# ---- 5. behind the warp, determinism, refusals --------------------------------------------------------------------------------------------------
def test_identity_warp_returns_the_unwarped_bits(lib):
    from eld_amd.dng_opcodes import Warp
    from eld_amd.isp import render_xtrans
    h, w = tile_shape()
    p, wbs, ccms, lin, _ = reference(h, w)
    x = dev(p)
    ident = Warp(W.IDENTITY, 0.4871, 0.5123)
    for kw in (dict(), dict(CRF=CRF), dict(linear=True)):
        want = render_xtrans(x, wbs, ccms, demosaic='directional', **kw)
        got = render_xtrans(x, wbs, ccms, demosaic='directional', warp=ident, **kw)
        assert got.dtype == want.dtype and torch.equal(got.view(torch.uint8), want.view(torch.uint8)), sorted(kw)
    assert bits_equal(render_xtrans(x, wbs, ccms, demosaic='directional', warp=ident, linear=True).cpu().numpy(), lin)


def test_two_calls_return_identical_bytes(lib):
    from eld_amd.isp import render_xtrans
    h, w = tile_shape()
    p, wbs, ccms, _, _ = reference(h, w)
    x = dev(p)
    for kw in (dict(), dict(linear=True)):
        a = render_xtrans(x, wbs, ccms, demosaic='directional', **kw)
        b = render_xtrans(x, wbs, ccms, demosaic='directional', **kw)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_refusals_leave_the_output_untouched(lib):
    from eld_amd import _lib as L
    N, h, w = 1, 4, 4
    xx = torch.rand(N, 9, h, w, device='cuda')
    wb = torch.ones(N, 3, device='cuda')
    ccm = torch.eye(3, device='cuda').reshape(1, 9).contiguous()
    E = torch.linspace(0, 1, 8, device='cuda')
    out = torch.full((N * 3 * 3 * h * 3 * w * 4 + 64,), 0x5A, dtype=torch.uint8, device='cuda')
    st = L.cur_stream()
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off) if t is not None else None      # noqa: E731

    def xdir(packed=xx, wbs=wb, ccms=ccm, o=out, ooff=0, poff=0, mode=L.RENDER_SRGB8, n=N, hh=h, ww=w, gamma=2.2, e=None, f=None, cn=0):
        return lib.eld_render_xtrans_dir(P(packed, poff), P(wbs), P(ccms), P(o, ooff), mode, n, hh, ww, gamma, P(e), P(f), cn, st)

    bad = [xdir(packed=None), xdir(wbs=None), xdir(o=None), xdir(poff=4), xdir(ooff=4), xdir(ooff=8), xdir(n=0), xdir(n=-1), xdir(hh=0), xdir(ww=-2),
           xdir(hh=1), xdir(ww=1), xdir(hh=3), xdir(ww=5), xdir(mode=2), xdir(mode=-1), xdir(cn=1, e=E, f=E), xdir(cn=-1), xdir(cn=8), xdir(cn=8, e=E),
           xdir(gamma=0.0)]
    assert bad == [-1] * len(bad), bad
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all())                                          # nothing was launched
    assert xdir() == 0 and xdir(cn=8, e=E, f=E) == 0 and xdir(ccms=None, mode=L.RENDER_LINEAR_F32) == 0
    torch.cuda.synchronize()
    assert not bool((out[:N * 3 * 9 * h * w * 4] == 0x5A).all()) and bool((out[N * 3 * 9 * h * w * 4:] == 0x5A).all())
    with pytest.raises(ValueError):
        from eld_amd.isp import render_xtrans
        render_xtrans(xx, wb, None, demosaic='directional')                   # the sRGB render needs a matrix


# ---- 6. denoise_raw, the command line and jpeg= end to end -----------------------------------------------------------------------------------------
def test_denoise_raw_end_to_end(lib, tmp_path):
    """denoise_raw(srgb_size='full', demosaic='directional') returns the directional render of its own written-back network output, the command
    line writes the same picture, jpeg= encodes it; the default is untouched"""
    from test_demosaic_gpu import CCM, make_opt, noisy_frame
    from eld_amd.denoise import denoise_raw, load_denoiser
    from eld_amd.isp import render_xtrans
    from eld_amd.model import ELDModel
    torch.manual_seed(2027)
    m = ELDModel()
    m.initialize(make_opt(tmp_path, 9))
    m.save('latest')
    ckpt = os.path.join(m.save_dir, 'model_latest.pt')
    den = load_denoiser(ckpt, cfa='xtrans')
    del m
    u = noisy_frame((96, 134), 1024, 2)                       # 134 columns: two beyond the last whole cell
    kw = dict(black_level=1024, white_point=16383, ratio=20.0, wb=[2.1, 1.0, 1.6], ccm=CCM, srgb_size='full')
    res = denoise_raw(den, u, 'xtrans', linear=True, demosaic='directional', **kw)
    base = denoise_raw(den, u, 'xtrans', linear=True, **kw)
    assert np.array_equal(res['mosaic'], base['mosaic']) and np.array_equal(res['packed'], base['packed'])
    assert res['srgb'].dtype == np.uint8 and res['srgb'].shape == (1, 3, 96, 132) and res['linear'].dtype == np.float32
    wbs, ccms = np.float32([[2.1, 1.0, 1.6]]), CCM[None]
    x = dev(res['packed'])
    assert np.array_equal(res['srgb'], render_xtrans(x, wbs, ccms, demosaic='directional').cpu().numpy())
    assert bits_equal(res['linear'], render_xtrans(x, wbs, ccms, linear=True, demosaic='directional').cpu().numpy())
    assert bits_equal(res['linear'], X.linear_xtrans_dir(res['packed'], wbs, ccms))
    assert np.array_equal(base['srgb'], render_xtrans(x, wbs, ccms).cpu().numpy())                          # the default: as before
    assert np.array_equal(denoise_raw(den, u, 'xtrans', demosaic='mhc', **kw)['srgb'], base['srgb'])
    assert not np.array_equal(res['linear'], base['linear'])
    with_jpeg = denoise_raw(den, u, 'xtrans', demosaic='directional', jpeg=dict(quality=85, subsampling='444'), **kw)
    assert np.array_equal(with_jpeg['srgb'], res['srgb'])
    assert with_jpeg['jpeg'] == [R.encode(np.ascontiguousarray(np.moveaxis(res['srgb'][0], 0, -1)), 85, '444')]
    src = tmp_path / 'frame.npy'
    np.save(str(src), u)
    out = tmp_path / 'out'
    r = subprocess.run([sys.executable, '-m', 'eld_amd.denoise', '--ckpt', ckpt, '--cfa', 'xtrans', '--black', '1024', '--white', '16383',
                        '--ratio', '20', '--wb', '2.1', '1', '1.6', '--ccm'] + [str(float(v)) for v in CCM.reshape(-1)]
                       + ['--srgb-size', 'full', '--demosaic', 'directional', str(src), '-o', str(out)], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    srgb = np.load(str(out / 'frame_srgb.npy'))
    assert srgb.dtype == np.uint8 and srgb.shape == (96, 132, 3) and np.array_equal(srgb, np.moveaxis(res['srgb'][0], 0, -1))
