"""GPU tests of the full-resolution renders (csrc/demosaic.hip eld_render_bayer / eld_render_xtrans, eld_amd.isp.render_*, denoise_raw's
srgb_size='full'): the linear output bit for bit against the NumPy float32 restatement (tests/demosaic_ref.py), the 8-bit codes, guarded
buffers, agreement with the packed-resolution ISP kernels on frames of constant colour, denoise_raw end to end, and the argument refusals."""
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import demosaic_ref as D              # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
PATTERNS = [[[0, 1], [3, 2]], [[2, 3], [1, 0]], [[1, 0], [2, 3]], [[3, 2], [0, 1]]]      # RGGB, BGGR, GRBG, GBRG
ISP_CAP = 2e-4      # tests/test_isp.py: the share of pixels eld_isp_process may have one code off for non-2.2 gammas and the CRF


@pytest.fixture(scope='module')
def lib(eld_lib):
    assert torch.cuda.is_available()
    return eld_lib


def inputs(N, planes, h, w, seed, gains):
    """random packed values reaching below 0 and above 1, per-frame gains and matrices"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.2, 1.3, size=(N, planes, h, w)).astype(F32)
    wbs = rng.uniform(0.7, 2.2, size=(N, gains)).astype(F32)
    ccms = (np.eye(3)[None] * rng.uniform(1.2, 1.7, size=(N, 1, 1)) + rng.uniform(-0.35, 0.1, size=(N, 3, 3))).astype(F32)
    return p, wbs, ccms


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 6. linear output, bit for bit --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,h,w', [(1, 2, 2), (1, 89, 133), (1, 512, 512), (2, 736, 1088)])
def test_bayer_linear_equals_the_restatement(lib, N, h, w):
    from eld_amd.isp import render_bayer
    for i, pat in enumerate(PATTERNS if h < 700 else PATTERNS[1:3]):
        p, wbs, ccms = inputs(N, 4, h, w, 10 + i, 4)
        x = dev(p)
        got = render_bayer(x, pat, wbs, ccms, linear=True)
        assert got.dtype == torch.float32 and got.shape == (N, 3, 2 * h, 2 * w) and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), D.linear_bayer(p, pat, wbs, ccms)), pat
        assert np.array_equal(render_bayer(x, pat, wbs, None, linear=True).cpu().numpy(), D.linear_bayer(p, pat, wbs)), pat


@pytest.mark.parametrize('N,h,w', [(1, 2, 2), (2, 88, 134), (1, 512, 512), (1, 1344, 2010)])
def test_xtrans_linear_equals_the_restatement(lib, N, h, w):
    from eld_amd.isp import render_xtrans
    p, wbs, ccms = inputs(N, 9, h, w, 20, 3)
    x = dev(p)
    got = render_xtrans(x, wbs, ccms, linear=True)
    assert got.dtype == torch.float32 and got.shape == (N, 3, 3 * h, 3 * w) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), D.linear_xtrans(p, wbs, ccms))
    assert np.array_equal(render_xtrans(x, wbs, None, linear=True).cpu().numpy(), D.linear_xtrans(p, wbs))


# ---- 7. the 8-bit codes --------------------------------------------------------------------------------------------------------------------
def check_codes(render, linear):
    """gamma 2.2: every code equal (the threshold table is exact); another gamma and a CRF: the rule tests/test_isp.py applies to
    eld_isp_process -- at most one code off, on at most ISP_CAP of the pixels."""
    got = render().cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == linear.shape
    assert np.array_equal(got, D.srgb8(linear))
    E = np.linspace(0, 1, 1024, dtype=F32)
    fs = (E ** 0.45).astype(F32)
    for kw in (dict(gamma=2.7), dict(CRF=(E, fs))):
        diff = np.abs(render(**kw).cpu().numpy().astype(int) - D.srgb8(linear, **kw).astype(int))
        print('codes off by one: %d of %d (%s)' % (int((diff > 0).sum()), diff.size, sorted(kw)))
        assert diff.max() <= 1 and (diff > 0).mean() <= ISP_CAP


@pytest.mark.parametrize('h,w', [(89, 133), (256, 384)])
def test_bayer_srgb8(lib, h, w):
    from eld_amd.isp import render_bayer
    for i, pat in enumerate(PATTERNS[:2] if w % 4 else PATTERNS[2:]):
        p, wbs, ccms = inputs(2, 4, h, w, 30 + i, 4)
        x = dev(p)
        check_codes(lambda **kw: render_bayer(x, pat, wbs, ccms, **kw), D.linear_bayer(p, pat, wbs, ccms))


@pytest.mark.parametrize('h,w', [(88, 134), (256, 384)])
def test_xtrans_srgb8(lib, h, w):
    from eld_amd.isp import render_xtrans
    p, wbs, ccms = inputs(2, 9, h, w, 40, 3)
    x = dev(p)
    check_codes(lambda **kw: render_xtrans(x, wbs, ccms, **kw), D.linear_xtrans(p, wbs, ccms))


# ---- 7b. guarded, poisoned buffers -----------------------------------------------------------------------------------------------------------
# Packed shapes, the smallest at which each store path and its edge can go wrong.  Bayer: 2 x 2 (one run of two columns), 3 x 5 (the non-vector
# path, the last run holds one column), 5 x 8 (the vector path, every lane at a border: the mirrored gather), 9 x 12 (the vector path with
# interior lanes).  X-Trans: 2 x 2 (one cell), 6 x 10, 10 x 66 (5 x 33 cells: two tiles of 4 x 32 cells down and two across, ragged both ways).
GUARDED = [('bayer', 2, 2), ('bayer', 3, 5), ('bayer', 5, 8), ('bayer', 9, 12), ('xtrans', 2, 2), ('xtrans', 6, 10), ('xtrans', 10, 66)]


@pytest.mark.parametrize('cfa,h,w', GUARDED)
def test_guarded_buffers(lib, cfa, h, w):
    """every operand between guard bands of NaN, the outputs poisoned with 0xFF (NaN), two frames (the batch stride): nothing outside is written,
    every element inside is, no NaN (a read outside an input) reaches the result, and the linear output has the restatement's bits"""
    from eld_amd import _lib as L
    from guarded import Guards
    bayer = cfa == 'bayer'
    pat = PATTERNS[(h + w) % 4]
    p, wbs, ccms = inputs(2, 4 if bayer else 9, h, w, 90 + 3 * h + w, 4 if bayer else 3)
    lin = D.linear_bayer(p, pat, wbs, ccms) if bayer else D.linear_xtrans(p, wbs, ccms)
    s = 2 if bayer else 3
    g = Guards()
    x, wb, cm = g.ro(dev(p), 'packed'), g.ro(dev(wbs), 'wbs'), g.ro(dev(ccms.reshape(2, 9)), 'ccms')
    o32 = g.new((2, 3, s * h, s * w), torch.float32, 'linear out')
    o8 = g.new((2, 3, s * h, s * w), torch.uint8, 'srgb out')
    cpat = (ctypes.c_int * 4)(*np.asarray(pat).reshape(-1).tolist())
    for out, mode in ((o32, L.RENDER_LINEAR_F32), (o8, L.RENDER_SRGB8)):
        tail = (L.dptr(wb), L.dptr(cm), L.dptr(out), mode, 2, h, w, 2.2, None, None, 0, L.cur_stream())
        if bayer:
            L.check(lib.eld_render_bayer(L.dptr(x), cpat, *tail), 'eld_render_bayer')
        else:
            L.check(lib.eld_render_xtrans(L.dptr(x), *tail), 'eld_render_xtrans')
    torch.cuda.synchronize()
    g.check()
    got = o32.cpu().numpy()
    assert not np.isnan(got).any()
    assert got.shape == lin.shape and got.dtype == lin.dtype == np.float32 and np.array_equal(got.view(np.uint32), lin.view(np.uint32))
    assert np.array_equal(o8.cpu().numpy(), D.srgb8(lin))


# ---- 8. consistency with the packed-resolution render ----------------------------------------------------------------------------------------
GAINS = np.array([0.75, 1.0, 1.5, 2.0], F32)


def constant_frames(planes, colour_of_plane, h, w, gains, seed):
    """N frames, each colour constant over the frame (values on the 2^-8 grid, so with gains from GAINS every sum of the demosaic formulas is
    exact), per-frame gains from GAINS and a CCM per frame"""
    rng = np.random.default_rng(seed)
    N = 5
    rgb = rng.integers(0, 257, size=(N, 3)).astype(F32) / F32(256)
    rgb[0] = (1.0, 0.0, 0.5)
    p = np.ascontiguousarray(np.broadcast_to(rgb[:, colour_of_plane, None, None], (N, planes, h, w)))
    wbs = GAINS[rng.integers(0, 4, size=(N, gains))]
    ccms = (np.eye(3)[None] * rng.uniform(1.2, 1.7, size=(N, 1, 1)) + rng.uniform(-0.35, 0.1, size=(N, 3, 3))).astype(F32)
    return p, wbs, ccms


def check_consistent(full, packed_rgb, tag):
    """every pixel of the full render carries the code the packed-resolution kernel writes for that frame"""
    ref = torch.round(packed_rgb * 255).to(torch.uint8)
    assert ref.shape[2] * ref.shape[3] > 0
    for n in range(ref.shape[0]):
        for c in range(3):
            assert int(ref[n, c].min()) == int(ref[n, c].max())           # the packed render is constant over a frame of constant colour
    diff = (full.to(torch.int32) - ref[:, :, :1, :1].to(torch.int32)).abs().cpu().numpy()
    return diff


@pytest.mark.parametrize('pat', PATTERNS)
def test_bayer_matches_isp_process_on_constant_frames(lib, pat):
    from eld_amd.isp import process, render_bayer
    E = np.linspace(0, 1, 1024, dtype=F32)
    fs = (E ** 0.45).astype(F32)
    for h, w in ((2, 2), (37, 53), (64, 96)):
        # the packed planes are R, G1, B, G2 for both kernels: plane k holds colour CODE_COLOUR[k]; G1 and G2 get the same gain here, as a
        # frame of constant colour needs (binning averages them)
        p, wbs, ccms = constant_frames(4, list(D.CODE_COLOUR), h, w, 4, 50 + h)
        wbs[:, 3] = wbs[:, 1]
        x = dev(p)
        diff = check_consistent(render_bayer(x, pat, wbs, ccms), process(x, wbs, ccms), pat)
        assert diff.max() == 0
        for kw in (dict(gamma=2.7), dict(CRF=(E, fs))):
            diff = check_consistent(render_bayer(x, pat, wbs, ccms, **kw), process(x, wbs, ccms, **kw), pat)
            assert diff.max() <= 1 and (diff > 0).mean() <= ISP_CAP


def test_xtrans_matches_isp_process_xtrans_on_constant_frames(lib):
    from eld_amd.isp import process_xtrans, render_xtrans
    E = np.linspace(0, 1, 1024, dtype=F32)
    fs = (E ** 0.45).astype(F32)
    for h, w in ((2, 2), (4, 66), (36, 54)):
        p, wbs, ccms = constant_frames(9, D.PLANE_COLOUR, h, w, 3, 60 + h)
        x = dev(p)
        # the packed render divides sums of 2 or 5 equal values by 2 or 5: exact on this grid, so both renders see the same camera RGB
        diff = check_consistent(render_xtrans(x, wbs, ccms), process_xtrans(x, wbs, ccms), 'xtrans')
        assert diff.max() == 0
        for kw in (dict(gamma=2.7), dict(CRF=(E, fs))):
            diff = check_consistent(render_xtrans(x, wbs, ccms, **kw), process_xtrans(x, wbs, ccms, **kw), 'xtrans')
            assert diff.max() <= 1 and (diff > 0).mean() <= ISP_CAP


# ---- 9. denoise_raw end to end ---------------------------------------------------------------------------------------------------------------
def make_opt(tmp, channels):
    return types.SimpleNamespace(gpu_ids=[0], isTrain=True, checkpoints_dir=str(tmp), name='t', netG='unet', channels=channels, stage_in='raw',
                                 stage_out='raw', lr=1e-4, beta1=0.9, wd=0.0, loss='l1', resume=False, chop=False, precision='fp32')


@pytest.fixture(scope='module')
def checkpoints(tmp_path_factory, lib):
    from eld_amd.model import ELDModel
    tmp = tmp_path_factory.mktemp('ckpt')
    out = {}
    for ch in (4, 9):
        torch.manual_seed(2018 + ch)
        m = ELDModel()
        m.initialize(make_opt(tmp / str(ch), ch))
        m.save('latest')
        out[ch] = os.path.join(m.save_dir, 'model_latest.pt')
        del m
    torch.cuda.empty_cache()
    return out


def noisy_frame(shape, black, seed):
    """(Hm, Wm) or (N, Hm, Wm): a smooth scene (the same in every frame) with independent noise"""
    rng = np.random.default_rng(seed)
    H, W = shape[-2:]
    yy, xx = np.mgrid[0:H, 0:W].astype(F32)
    scene = np.broadcast_to(60 + 40 * np.sin(yy / 23.0) * np.cos(xx / 31.0), shape)
    return np.clip(np.rint(black + rng.poisson(np.maximum(scene, 0)) + rng.normal(0, 3, size=shape)), 0, 16383).astype(np.uint16)


WB4 = [2100.0, 1024.0, 1500.0, 1024.0]
CCM = np.float32([[1.6, -0.4, -0.2], [-0.2, 1.5, -0.3], [0.0, -0.5, 1.5]])


def test_denoise_raw_full_bayer(lib, checkpoints):
    from eld_amd.denoise import denoise_raw, load_denoiser
    from eld_amd.isp import render_bayer
    pat = [[2, 3], [1, 0]]
    u = noisy_frame((2, 96, 160), 512, 1)
    den = load_denoiser(checkpoints[4], cfa='bayer')
    kw = dict(raw_pattern=pat, black_level=512, ratio=40.0, wb=WB4, ccm=CCM)
    base = denoise_raw(den, u, 'bayer', **kw)
    res = denoise_raw(den, u, 'bayer', srgb_size='full', linear=True, **kw)
    assert 'linear' not in base and base['srgb'].shape == (2, 3, 48, 80)
    assert np.array_equal(res['mosaic'], base['mosaic']) and np.array_equal(res['packed'], base['packed'])
    assert np.array_equal(denoise_raw(den, u, 'bayer', srgb_size='packed', **kw)['srgb'], base['srgb'])
    assert res['srgb'].dtype == np.uint8 and res['srgb'].shape == (2, 3, 96, 160)
    assert res['linear'].dtype == np.float32 and res['linear'].shape == (2, 3, 96, 160)
    wbs = np.tile(np.asarray(WB4, np.float64) / WB4[1], (2, 1)).astype(F32)
    ccms = np.tile(CCM, (2, 1, 1))
    x = dev(res['packed'])
    assert np.array_equal(res['srgb'], render_bayer(x, pat, wbs, ccms).cpu().numpy())
    assert np.array_equal(res['linear'], render_bayer(x, pat, wbs, ccms, linear=True).cpu().numpy())
    t = torch.from_numpy(u.view(np.int16)).cuda()            # CUDA in -> CUDA out
    rt = denoise_raw(den, t, 'bayer', srgb_size='full', **kw)
    assert rt['srgb'].is_cuda and rt['srgb'].dtype == torch.uint8 and rt['srgb'].device == t.device and 'linear' not in rt
    assert np.array_equal(rt['srgb'].cpu().numpy(), res['srgb'])


def test_denoise_raw_full_xtrans_and_cli(lib, checkpoints, tmp_path):
    from eld_amd.denoise import denoise_raw, load_denoiser
    from eld_amd.isp import render_xtrans
    u = noisy_frame((96, 134), 1024, 2)                       # 134 columns: two beyond the last whole cell
    den = load_denoiser(checkpoints[9], cfa='xtrans')
    kw = dict(black_level=1024, white_point=16383, ratio=20.0, wb=[2.1, 1.0, 1.6], ccm=CCM)
    base = denoise_raw(den, u, 'xtrans', **kw)
    res = denoise_raw(den, u, 'xtrans', srgb_size='full', **kw)
    assert np.array_equal(res['mosaic'], base['mosaic']) and np.array_equal(res['packed'], base['packed']) and 'linear' not in res
    assert base['srgb'].shape == (1, 3, 32, 44)
    assert res['srgb'].dtype == np.uint8 and res['srgb'].shape == (1, 3, 96, 132)
    assert np.array_equal(res['srgb'], render_xtrans(dev(res['packed']), np.float32([[2.1, 1.0, 1.6]]), CCM[None]).cpu().numpy())
    src = tmp_path / 'frame.npy'
    np.save(str(src), u)
    out = tmp_path / 'out'
    r = subprocess.run([sys.executable, '-m', 'eld_amd.denoise', '--ckpt', checkpoints[9], '--cfa', 'xtrans', '--black', '1024', '--white', '16383',
                        '--ratio', '20', '--wb', '2.1', '1', '1.6', '--ccm'] + [str(float(v)) for v in CCM.reshape(-1)]
                       + ['--srgb-size', 'full', str(src), '-o', str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    srgb = np.load(str(out / 'frame_srgb.npy'))
    assert srgb.dtype == np.uint8 and srgb.shape == (96, 132, 3) and np.array_equal(srgb, np.moveaxis(res['srgb'][0], 0, -1))
    assert np.array_equal(np.load(str(out / 'frame_denoised.npy')), res['mosaic'])


# ---- 10. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched(lib):
    from eld_amd import _lib as L
    N, h, w = 1, 4, 4
    xb = torch.rand(N, 4, h, w, device='cuda')
    xx = torch.rand(N, 9, h, w, device='cuda')
    wb = torch.ones(N, 4, device='cuda')
    ccm = torch.eye(3, device='cuda').reshape(1, 9).contiguous()
    E = torch.linspace(0, 1, 8, device='cuda')
    out = torch.full((N * 3 * 3 * h * 3 * w * 4 + 64,), 0x5A, dtype=torch.uint8, device='cuda')
    st = L.cur_stream()
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off) if t is not None else None      # noqa: E731
    pat = (ctypes.c_int * 4)(0, 1, 3, 2)

    def bayer(packed=xb, pattern=pat, wbs=wb, ccms=ccm, o=out, ooff=0, poff=0, mode=L.RENDER_SRGB8, n=N, hh=h, ww=w, gamma=2.2, e=None, f=None, cn=0):
        return lib.eld_render_bayer(P(packed, poff), pattern, P(wbs), P(ccms), P(o, ooff), mode, n, hh, ww, gamma, P(e), P(f), cn, st)

    def xtrans(packed=xx, wbs=wb, ccms=ccm, o=out, ooff=0, poff=0, mode=L.RENDER_SRGB8, n=N, hh=h, ww=w, gamma=2.2, e=None, f=None, cn=0):
        return lib.eld_render_xtrans(P(packed, poff), P(wbs), P(ccms), P(o, ooff), mode, n, hh, ww, gamma, P(e), P(f), cn, st)

    for fn in (bayer, xtrans):
        bad = [fn(packed=None), fn(wbs=None), fn(o=None), fn(poff=4), fn(ooff=4), fn(ooff=8), fn(n=0), fn(n=-1), fn(hh=0), fn(ww=-2), fn(hh=1),
               fn(ww=1), fn(mode=2), fn(mode=-1), fn(cn=1, e=E, f=E), fn(cn=-1), fn(cn=8), fn(cn=8, e=E), fn(gamma=0.0)]
        assert bad == [-1] * len(bad), (fn.__name__, bad)
    assert xtrans(hh=3) == -1 and xtrans(ww=5) == -1                          # odd X-Trans sides
    for bad_pat in ((0, 1, 2, 2), (0, 1, 2, 4), (-1, 0, 1, 2), (0, 0, 0, 0), (0, 2, 1, 3)):
        assert bayer(pattern=(ctypes.c_int * 4)(*bad_pat)) == -1, bad_pat
    assert bayer(pattern=None) == -1
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all())                                          # nothing was launched
    assert bayer() == 0 and xtrans() == 0 and bayer(cn=8, e=E, f=E) == 0 and xtrans(ccms=None, mode=L.RENDER_LINEAR_F32) == 0
    torch.cuda.synchronize()
    assert not bool((out[:N * 3 * 9 * h * w * 4] == 0x5A).all()) and bool((out[N * 3 * 9 * h * w * 4:] == 0x5A).all())
    with pytest.raises(ValueError):
        from eld_amd.isp import render_bayer
        render_bayer(xb, [[0, 1], [3, 2]], wb, None)                          # the sRGB render needs a matrix
