"""GPU tests of eld_amd.denoise and its kernels: the write-back (eld_unpack_raw_*_u16) bit for bit against the NumPy restatement of the
reference's expression, round trips, X-Trans borders, the fused evaluation input stage (eld_pack_raw_*_u16_gain), the X-Trans ISP
(eld_isp_process_xtrans), denoise_raw end to end against the manual composition of its stages, against the torch-CPU oracle network,
and the command line.  Checkers: tests/denoise_ref.py, oracle/unet_ref.py."""
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import denoise_ref as R              # noqa: E402
from oracle import unet_ref as U     # noqa: E402  (checker only)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERNS = [[[0, 1], [3, 2]], [[2, 3], [1, 0]], [[1, 0], [2, 3]], [[3, 2], [0, 1]]]      # RGGB, BGGR, GRBG, GBRG
BLACKS = [512, 600, 1024, 2047]


@pytest.fixture(scope='module')
def lib(eld_lib):
    assert torch.cuda.is_available()
    return eld_lib


def dev_u16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).cuda()


def host_u16(t):
    return t.cpu().numpy().view(np.uint16)


MODE = {'trunc': 0, 'nearest': 1, 'trunc_f32': 2}


def unpack_bayer(p, pat, blk, white, rounding):
    from eld_amd import _lib as L
    p = torch.from_numpy(np.ascontiguousarray(p, np.float32)).cuda()
    N, _, h, w = p.shape
    out = torch.zeros((N, 2 * h, 2 * w), dtype=torch.int16, device='cuda')
    L.check(L.lib().eld_unpack_raw_bayer_u16(L.dptr(p), L.dptr(out), N, h, w, (ctypes.c_int * 4)(*np.ravel(pat).tolist()),
                                             (ctypes.c_float * 4)(*blk), float(white), MODE[rounding], L.cur_stream()))
    return host_u16(out)


def unpack_xtrans(p, mosaic, blk, white, rounding):
    from eld_amd import _lib as L
    p = torch.from_numpy(np.ascontiguousarray(p, np.float32)).cuda()
    m = dev_u16(mosaic)
    L.check(L.lib().eld_unpack_raw_xtrans_u16(L.dptr(p), L.dptr(m), m.shape[0], m.shape[1], m.shape[2], float(blk), float(white), MODE[rounding],
                                              L.cur_stream()))
    return host_u16(m)


def boundary_values(black, white):
    """the float32 nearest to (k - black) / (white - black) for every code k in [black, white], its two float32 neighbours, and values
    outside [0, 1]"""
    k = np.arange(black, white + 1, dtype=np.float64)
    x = ((k - black) / (white - black)).astype(np.float32)
    v = np.concatenate([x, np.nextafter(x, np.float32(-1)), np.nextafter(x, np.float32(2)),
                        np.float32([-1.0, -1e-30, -0.0, 1.0000001, 2.0, 1e30, -1e30])])
    return v


@pytest.mark.parametrize('rounding', ['trunc', 'nearest', 'trunc_f32'])
def test_bayer_write_back_bit_exact(lib, rounding):
    """Every raw_pattern, unequal per-channel black levels, packed values at and next to every integer boundary of every channel; and
    (0, 65535).  The vector path (w % 4 == 0) and the scalar path (w odd)."""
    for blk, white in ((BLACKS, 16383), ([0, 0, 0, 0], 65535)):
        vals = np.concatenate([boundary_values(b, white) for b in sorted(set(blk))])
        for w in (256, 37):
            h = -(-vals.size // w)
            p = np.resize(vals, (1, 4, h, w)).astype(np.float32)
            p[0, 1] = np.roll(p[0, 1], 7)                                  # each channel sees other values at a position
            p[0, 2] = p[0, 2, ::-1]
            for pat in PATTERNS:
                got = unpack_bayer(p, pat, blk, white, rounding)
                assert np.array_equal(got, R.unpack_bayer(p, pat, blk, white, rounding)), (pat, blk, w)


@pytest.mark.parametrize('rounding', ['trunc', 'nearest', 'trunc_f32'])
def test_xtrans_write_back_bit_exact(lib, rounding):
    for black, white in ((1024, 16383), (0, 65535)):
        vals = boundary_values(black, white)
        ca, cb = 40, -(-vals.size // (9 * 4 * 40))
        p = np.resize(vals, (1, 9, 2 * ca, 2 * cb)).astype(np.float32)
        for Hm, Wm in ((6 * ca, 6 * cb), (6 * ca + 4, 6 * cb + 3)):                # even width (paired stores) and odd width
            m = np.random.default_rng(Hm).integers(0, 65536, size=(1, Hm, Wm), dtype=np.uint16)
            got = unpack_xtrans(p, m, black, white, rounding)
            assert np.array_equal(got, R.unpack_xtrans(p, m, black, white, rounding)), (Hm, Wm)


def every_code(h, w, seed=0):
    u = (np.arange(h * w) % 65536).astype(np.uint16)
    return np.random.default_rng(seed).permutation(u).reshape(1, h, w)


def test_round_trip_nearest(lib):
    """unpack(pack(u)) == clip(u, black, white) for every code 0..65535, Bayer (4 patterns, unequal blacks) and X-Trans; with the
    reference's truncation the Bayer trip loses one DN on the stated share of the codes."""
    from eld_amd.noise import pack_raw_bayer, pack_raw_xtrans
    u = every_code(256, 256)
    for pat in PATTERNS:
        for blk, white in ((BLACKS, 16383), ([0] * 4, 65535)):
            p = pack_raw_bayer(dev_u16(u), pat, blk, white)
            back = unpack_bayer(p.cpu().numpy(), pat, blk, white, 'nearest')
            exp = np.empty_like(u)
            for k, (oy, ox) in enumerate(R.bayer_offsets(pat)):
                exp[:, oy::2, ox::2] = np.clip(u[:, oy::2, ox::2], blk[k], white)
            assert np.array_equal(back, exp), (pat, blk)
    p = pack_raw_bayer(dev_u16(u), PATTERNS[0], [512] * 4, 16383).cpu().numpy()
    back = unpack_bayer(p, PATTERNS[0], [512] * 4, 16383, 'trunc')
    inside = (u >= 512) & (u <= 16383)
    assert np.array_equal(back, R.unpack_bayer(p, PATTERNS[0], [512] * 4, 16383, 'trunc'))
    assert int((back != u)[inside].sum()) == 7893                   # every code of [512, 16383] appears once in u
    ux = every_code(252, 264, seed=1)
    for black, white in ((1024, 16383), (0, 65535)):
        px = pack_raw_xtrans(dev_u16(ux), black, white).cpu().numpy()
        back = unpack_xtrans(px, np.zeros_like(ux), black, white, 'nearest')
        assert np.array_equal(back, np.clip(ux, black, white)), black


@pytest.mark.parametrize('Hm,Wm', [(4158, 6240), (4040, 6034)])
def test_xtrans_borders_keep_the_input(lib, Hm, Wm):
    from eld_amd.noise import pack_raw_xtrans
    u = np.random.default_rng(Hm).integers(0, 16384, size=(1, Hm, Wm), dtype=np.uint16)
    px = pack_raw_xtrans(dev_u16(u), 1024, 16383)
    p = (px * 0.5 + 0.25).cpu().numpy()                               # anything but the input: every whole-cell pixel changes
    got = unpack_xtrans(p, u, 1024, 16383, 'nearest')
    H6, W6 = 6 * (Hm // 6), 6 * (Wm // 6)
    assert np.array_equal(got[:, H6:, :], u[:, H6:, :]) and np.array_equal(got[:, :, W6:], u[:, :, W6:])
    assert np.array_equal(got, R.unpack_xtrans(p, u, 1024, 16383, 'nearest'))


def test_gain_stage_bit_exact(lib):
    """pack -> x ratio -> clip in one kernel == NumPy's expression on the existing pack, three ratios in one batch."""
    from eld_amd.denoise import pack_input
    from eld_amd.noise import pack_raw_bayer, pack_raw_xtrans
    ratios = [1.0, 100.0, 287.3]
    rng = np.random.default_rng(5)
    u = rng.integers(0, 16384, size=(3, 96, 130), dtype=np.uint16)
    for pat in PATTERNS[:2]:
        got = pack_input(dev_u16(u), 'bayer', np.ravel(pat).tolist(), [float(b) for b in BLACKS], 16383.0, ratios).cpu().numpy()
        base = pack_raw_bayer(dev_u16(u), pat, BLACKS, 16383).cpu().numpy()
        assert np.array_equal(got, R.gain(base, ratios))
        assert np.array_equal(base, R.pack_bayer(u, pat, BLACKS, 16383))
    ux = rng.integers(0, 16384, size=(3, 100, 134), dtype=np.uint16)
    got = pack_input(dev_u16(ux), 'xtrans', None, [1024.0], 16383.0, ratios).cpu().numpy()
    base = pack_raw_xtrans(dev_u16(ux), 1024, 16383).cpu().numpy()
    assert np.array_equal(got, R.gain(base, ratios))


def crf_table():
    E = np.linspace(0, 1, 1024, dtype=np.float32)
    return E, (E ** np.float32(0.6)).astype(np.float32)


@pytest.mark.parametrize('shape', [(1, 9, 16, 24), (2, 9, 50, 66), (1, 9, 1344, 2010)])
@pytest.mark.parametrize('crf', [False, True], ids=['gamma', 'crf'])
def test_xtrans_isp_bit_exact(lib, shape, crf):
    from eld_amd.isp import process_xtrans
    rng = np.random.default_rng(shape[2])
    x = (rng.random(shape, dtype=np.float32) * np.float32(1.2) - np.float32(0.05)).astype(np.float32)
    N = shape[0]
    wbs = np.float32([[2.1, 1.0, 1.6], [1.5, 1.0, 2.2]])[:N]
    ccms = np.float32([[[1.6, -0.4, -0.2], [-0.2, 1.5, -0.3], [0.0, -0.5, 1.5]], [[1.2, -0.1, -0.1], [-0.3, 1.4, -0.1], [0.1, -0.2, 1.1]]])[:N]
    CRF = crf_table() if crf else None
    got = process_xtrans(torch.from_numpy(x).cuda(), wbs, ccms, CRF=CRF).cpu().numpy()
    assert np.array_equal(got, R.isp_xtrans(x, wbs, ccms, CRF=CRF))


# ---- denoise_raw end to end ---------------------------------------------------------------------------------------------------------
def make_opt(tmp, channels, precision='fp32'):
    return types.SimpleNamespace(gpu_ids=[0], isTrain=True, checkpoints_dir=str(tmp), name='t', netG='unet', channels=channels, stage_in='raw',
                                 stage_out='raw', lr=1e-4, beta1=0.9, wd=0.0, loss='l1', resume=False, chop=False, precision=precision)


@pytest.fixture(scope='module')
def checkpoints(tmp_path_factory, lib):
    """seeded random-init checkpoints written by ELDModel.save (the reference's dict): Bayer 4 -> 4 and X-Trans 9 -> 9"""
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


def fresh_net(path, precision):
    from eld_amd.unet import UNetSeeInDark
    sd = torch.load(path, map_location='cpu')['netG']
    net = UNetSeeInDark(sd['conv1_1.weight'].shape[1], sd['conv10_1.weight'].shape[0])
    net.load_state_dict(sd)
    net = net.cuda()
    net.requires_grad_(False)
    net.inference_precision = precision
    return net


def synthetic_frame(shape, black, seed):
    """a noisy dark frame: a smooth scene, Poisson-like noise, black level, a few saturated pixels"""
    rng = np.random.default_rng(seed)
    H, W = shape
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    scene = 40 + 30 * np.sin(yy / 97.0) * np.cos(xx / 131.0)
    u = black + rng.poisson(np.maximum(scene, 0)).astype(np.float64) + rng.normal(0, 3, size=shape)
    u = np.clip(np.rint(u), 0, 16383).astype(np.uint16)
    u[::997, ::1009] = 16383
    return u


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_end_to_end_bayer_frame(lib, checkpoints, precision):
    """2848 x 4256 Bayer frame (whole-frame U-Net): denoise_raw == pack -> x ratio -> clip -> netG -> write-back, bit for bit, and its sRGB
    output == eld_amd.isp.process on the same packed output."""
    from eld_amd.denoise import denoise_raw, load_denoiser
    from eld_amd.isp import process
    from eld_amd.noise import pack_raw_bayer
    pat, blk, ratio = [[0, 1], [3, 2]], [512, 510, 512, 514], 100.0
    u = synthetic_frame((2848, 4256), 512, 1)
    wb = [2100.0, 1024.0, 1500.0, 1024.0]
    ccm = np.float32([[1.6, -0.4, -0.2], [-0.2, 1.5, -0.3], [0.0, -0.5, 1.5]])
    den = load_denoiser(checkpoints[4], cfa='bayer', precision=precision)
    res = denoise_raw(den, u, 'bayer', raw_pattern=pat, black_level=blk, white_point=16383, ratio=ratio, wb=wb, ccm=ccm)
    net = fresh_net(checkpoints[4], precision)
    p = pack_raw_bayer(dev_u16(u), pat, blk, 16383)
    x = torch.clamp(p * np.float32(ratio), 0, 1).unsqueeze(0)
    with torch.no_grad():
        out = net(x)
    assert np.array_equal(res['packed'], out.cpu().numpy())
    exp = R.unpack_bayer(out.cpu().numpy(), pat, blk, 16383, 'nearest')[0]
    assert res['mosaic'].dtype == np.uint16 and res['mosaic'].shape == u.shape
    assert np.array_equal(res['mosaic'], exp)
    wb4 = np.asarray(wb, np.float64) / wb[1]
    rgb = process(out, torch.from_numpy(wb4.astype(np.float32)).reshape(1, 4).cuda(), torch.from_numpy(ccm).reshape(1, 3, 3).cuda())
    assert res['srgb'].dtype == np.uint8 and res['srgb'].shape == (1, 3, 1424, 2128)
    assert np.array_equal(res['srgb'], torch.round(rgb * 255).to(torch.uint8).cpu().numpy())
    # the same frame as a CUDA tensor: the result stays on the device, same bits
    t = dev_u16(u)
    rt = denoise_raw(den, t, 'bayer', raw_pattern=pat, black_level=blk, white_point=16383, ratio=ratio)
    assert rt['mosaic'].is_cuda and rt['mosaic'].dtype == torch.int16 and rt['srgb'] is None
    assert np.array_equal(host_u16(rt['mosaic']), exp)


def test_end_to_end_xtrans_chop(lib, checkpoints):
    """4032 x 6032 X-Trans frame: packs to 9 x 1344 x 2010, which the U-Net cannot take whole -- denoise_raw chops and equals the manual
    forward_chop composition bit for bit; the two columns beyond the last whole cell keep the input; the sRGB is the X-Trans ISP's."""
    from eld_amd.denoise import denoise_raw, load_denoiser
    from eld_amd.isp import process_xtrans
    from eld_amd.model import forward_chop
    from eld_amd.noise import pack_raw_xtrans
    u = synthetic_frame((4032, 6032), 1024, 2)
    wb, ccm = [2.1, 1.0, 1.6], np.float32([[1.6, -0.4, -0.2], [-0.2, 1.5, -0.3], [0.0, -0.5, 1.5]])
    den = load_denoiser(checkpoints[9], cfa='xtrans')
    res = denoise_raw(den, u, 'xtrans', black_level=1024, white_point=16383, ratio=50.0, wb=wb, ccm=ccm)
    net = fresh_net(checkpoints[9], 'fp32')
    p = pack_raw_xtrans(dev_u16(u), 1024, 16383)
    x = torch.clamp(p * np.float32(50.0), 0, 1).unsqueeze(0)
    out = forward_chop(net, x)
    assert out.shape == (1, 9, 1344, 2010)
    assert np.array_equal(res['packed'], out.cpu().numpy())
    exp = R.unpack_xtrans(out.cpu().numpy(), u[None], 1024, 16383, 'nearest')[0]
    assert np.array_equal(res['mosaic'], exp)
    assert np.array_equal(res['mosaic'][:, 6030:], u[:, 6030:])
    rgb = process_xtrans(out, np.float32([wb]), ccm[None])
    assert np.array_equal(res['srgb'], torch.round(rgb * 255).to(torch.uint8).cpu().numpy())
    with pytest.raises(RuntimeError, match='multiples of 16'):
        denoise_raw(den, u, 'xtrans', chop=False)


def test_against_the_oracle_network(lib, checkpoints):
    """A small Bayer frame, fp32: the packed output against the torch-CPU oracle U-Net on the same input, within the fp32 parity bound of
    tests/test_parity_full_gpu.py (|ours - cpu32| <= 1e-5 (1 + max|ref|))."""
    from eld_amd.denoise import denoise_raw, load_denoiser
    u = synthetic_frame((256, 384), 512, 3)
    res = denoise_raw(load_denoiser(checkpoints[4]), u, 'bayer', black_level=512, ratio=30.0)
    x = R.gain(R.pack_bayer(u[None], [[0, 1], [3, 2]], [512] * 4, 16383), [30.0])
    sd = torch.load(checkpoints[4], map_location='cpu')['netG']
    with torch.no_grad():
        ref = U.unet_forward(sd, torch.from_numpy(x)).numpy()
    err = float(np.abs(res['packed'] - ref).max())
    assert err <= 1e-5 * (1 + float(np.abs(ref).max())), err


def test_cli_writes_what_the_api_returns(lib, checkpoints, tmp_path):
    from eld_amd.denoise import denoise_raw, load_denoiser
    u = synthetic_frame((96, 132), 1024, 4)
    src = tmp_path / 'frame.npy'
    np.save(str(src), u)
    meta = tmp_path / 'frame.json'
    meta.write_text('{"camera_whitebalance": [2100.0, 1024.0, 1500.0, 0.0], "rgb_camera_matrix": '
                    '[[1.6, -0.4, -0.2, 0], [-0.2, 1.5, -0.3, 0], [0.0, -0.5, 1.5, 0]]}')
    out = tmp_path / 'out'
    r = subprocess.run([sys.executable, '-m', 'eld_amd.denoise', '--ckpt', checkpoints[9], '--cfa', 'xtrans', '--black', '1024', '--white', '16383',
                        '--ratio', '20', '--meta', str(meta), str(src), '-o', str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    res = denoise_raw(load_denoiser(checkpoints[9], cfa='xtrans'), u, 'xtrans', black_level=1024, white_point=16383, ratio=20.0,
                      wb=[2100.0, 1024.0, 1500.0, 0.0], ccm=[[1.6, -0.4, -0.2], [-0.2, 1.5, -0.3], [0.0, -0.5, 1.5]])
    assert np.array_equal(np.load(str(out / 'frame_denoised.npy')), res['mosaic'])
    srgb = np.load(str(out / 'frame_srgb.npy'))
    assert srgb.dtype == np.uint8 and np.array_equal(srgb, np.moveaxis(res['srgb'][0], 0, -1))
