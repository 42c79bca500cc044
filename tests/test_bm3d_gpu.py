"""BM3D on the device: eld_bm3d_vst_f32 against tests/bm3d_ref.py bit for bit -- no tolerance -- in both steps, over the
shapes that reach each path of the kernel, then the closed loop: ClassicalDenoiser(method='bm3d') through denoise_raw and evaluate_pairs."""
import contextlib
import ctypes
import io
import json

import numpy as np
import pytest

import bm3d_ref as R
import nlm_ref as NR

pytestmark = pytest.mark.gpu

PAT = [[0, 1], [3, 2]]
BLK, WHITE, RATIO, K, SIGMA = 512, 16383, 100.0, 2.0, 3.0
HALF = (np.arange(65536) >> 1).astype(np.uint16)
TAU_MAX = (1 << 30) - 1


@pytest.fixture(scope='module')
def dev(eld_lib):
    import torch
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def _scene_x(N, C, h, w, seed, black=BLK):
    """codes / 65535 of the noisy synthetic scene, one realisation per frame"""
    clean = NR.scene_planes(C, h, w)
    codes = np.stack([NR.noisy_codes(clean, K, SIGMA, black, WHITE, seed + n) for n in range(N)])
    return (codes.astype(np.float32) / np.float32(65535.0)).astype(np.float32)


def _equal(got, ref, what):
    g = got.cpu().numpy()
    assert g.dtype == np.int32 and g.shape == ref.shape
    bad = np.argwhere(g != ref)
    assert bad.size == 0, '%s: first of %d differences at %s: %d != %d' % (what, len(bad), bad[0].tolist(), g[tuple(bad[0])], ref[tuple(bad[0])])


def _both(dev, x, fwd, S, step, Gmax, mix, tables, frac, x_dev=None, stats=None, wide=None):
    """step 1, then step 2 guided by the REFERENCE's step 1: kernel and restatement on the same inputs -> the kernel's two outputs"""
    import torch
    from eld_amd.classical import bm3d_vst
    tau1, thr, tau2, s2, win = tables
    st = {} if stats is None else stats
    ref1 = R.bm3d_fast(x, 65535.0, fwd, None, S, step, Gmax, mix, tau1, thr, win, frac, st.setdefault(1, {}), wide)
    ref2 = R.bm3d_fast(x, 65535.0, fwd, ref1, S, step, Gmax, mix, tau2, s2, win, frac, st.setdefault(2, {}), wide)
    xd = torch.from_numpy(x).to(dev) if x_dev is None else x_dev
    fd = torch.from_numpy(np.ascontiguousarray(fwd).view(np.int16)).to(dev)
    got1 = bm3d_vst(xd, 65535.0, fd, None, S, step, Gmax, mix, tau1, thr, win, frac)
    got2 = bm3d_vst(xd, 65535.0, fd, torch.from_numpy(ref1).to(dev), S, step, Gmax, mix, tau2, s2, win, frac)
    torch.cuda.synchronize()
    _equal(got1, ref1, 'step 1')
    _equal(got2, ref2, 'step 2')
    return got1, got2


@pytest.mark.parametrize('h,w', [(8, 8), (8, 9), (9, 8), (15, 17), (24, 27), (19, 33), (37, 70)])
def test_plane_sizes(dev, h, w):
    """one block; the extra last grid row or column alone; grids that end ragged"""
    x = _scene_x(1, 4, h, w, 10 + h)
    _both(dev, x, NR.vst_tables(K, SIGMA, [BLK] * 4), 6, 3, 16, 1, R.bm3d_tables(4, 1), R.FRAC)


@pytest.mark.parametrize('C,mix', [(1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (4, 0), (4, 1), (9, 0), (16, 0), (16, 1)])
def test_planes_mix_and_batch(dev, C, mix):
    x = _scene_x(2, C, 15, 17, 30 + C)
    assert not np.array_equal(x[0], x[1])
    fwd = NR.vst_tables(K, SIGMA, [BLK + 3 * c for c in range(C)])             # a table per plane
    _both(dev, x, fwd, 6, 3, 16, mix, R.bm3d_tables(C, mix), R.FRAC)


@pytest.mark.parametrize('S', [0, 1, 6, 16])
def test_search_radius_on_a_plane_narrower_than_the_window(dev, S):
    x = _scene_x(1, 4, 12, 21, 40 + S)
    _both(dev, x, NR.vst_tables(K, SIGMA, [BLK] * 4), S, 3, 16, 1, R.bm3d_tables(4, 1), R.FRAC)


@pytest.mark.parametrize('step', [1, 3, 8])
@pytest.mark.parametrize('Gmax', [1, 2, 4, 8, 16])
def test_step_group_and_fraction(dev, step, Gmax):
    frac = 0 if (step + Gmax) % 2 else 4                                       # both fractions under every step and every Gmax
    x = _scene_x(1, 2, 15, 18, 50 + step + Gmax)
    _both(dev, x, NR.vst_tables(K, SIGMA, [BLK] * 2), 5, step, Gmax, 1, R.bm3d_tables(2, 1), frac)
    _both(dev, x[:, :1], NR.vst_tables(K, SIGMA, [BLK]), 5, step, Gmax, 0, R.bm3d_tables(1, 0), 4 - frac)


@pytest.mark.parametrize('name', sorted(R.GROUP_SIZE_CASES))
def test_every_group_size(dev, name):
    x, fwd, S, step, Gmax, mix, tables = R.group_size_case(name)
    stats = {}
    _both(dev, x, fwd, S, step, Gmax, mix, tables, R.FRAC, stats=stats)
    assert set(stats[1]) == set(stats[2]) == {0, 1, 2, 3, 4}, stats


def test_saturated_codes_largest_coefficient_and_numerator(dev):
    """every code 32767 (the table holds 65535: the min applies), 16 planes in one set, groups of 16: the DC term is 32767 * 2^14, and with
    step 1 and S = 16 the sites in the middle collect the most contributions the shape allows"""
    x = np.full((1, 16, 24, 24), 2.0, np.float32)
    fwd = np.full((16, 65536), 65535, np.uint16)
    stats = {}
    a, b = _both(dev, x, fwd, 16, 1, 16, 1, R.bm3d_tables(16, 1), 4, stats=stats)
    assert stats[1] == stats[2] == {4: 17 * 17}
    assert int(a.min()) == int(a.max()) == 32767 << 4
    assert int(b.min()) == int(b.max()) == (((32767 << 14) * 4095 + 2048 >> 12) + 512) >> 10       # R = 4095 on the DC term, the only one


def test_checkerboard_reaches_the_clamp_and_the_largest_distance(dev):
    yy, xx = np.mgrid[0:17, 0:19]
    x = np.broadcast_to((((yy + xx) & 1) * 1.0).astype(np.float32), (1, 16, 17, 19)).copy()
    fwd = np.zeros((16, 65536), np.uint16)
    fwd[:, 32768:] = 40000                                                     # codes 0 and 32767: the difference clamps at 1023
    assert set(np.unique(NR.stabilised(x, 65535.0, fwd)).tolist()) == {0, 32767}
    assert 1023 * 1023 * 16 * 64 <= TAU_MAX
    tau1, thr, tau2, s2, win = R.bm3d_tables(16, 1)
    stats = {}
    _both(dev, x, fwd, 3, 3, 16, 1, (TAU_MAX, thr, TAU_MAX, s2, win), 4, stats=stats)      # every candidate counts, at D = 0 or 1023^2 * 1024
    assert set(stats[1]) == {4}
    _both(dev, x, fwd, 3, 3, 16, 1, (1023 * 1023 * 16 * 64 - 1, thr, 0, s2, win), 0)                    # one below: only the even offsets


def test_inverse_beyond_32_bits(dev):
    """full-range random codes, 16 planes x 16 blocks and a threshold of 0: sum |T'| is about 2^34, where the partial sums of the inverse leave
    32 bits; the contract's I is the exact integer, and the estimate is the input again"""
    rng = np.random.default_rng(90)
    x = (rng.integers(0, 65536, size=(1, 16, 11, 11)).astype(np.float32) / np.float32(65535.0)).astype(np.float32)
    fwd = np.stack([HALF] * 16)
    win = R.WIN.reshape(-1)
    wide = []
    a, b = _both(dev, x, fwd, 3, 8, 16, 1, (TAU_MAX, np.zeros(5, np.uint32), TAU_MAX, np.ones(5, np.uint32), win), 4, wide=wide)
    assert len(wide) == 8 and all(wide)
    assert np.array_equal(a.cpu().numpy(), (NR.stabilised(x, 65535.0, fwd) << 4).astype(np.int32))


def test_bad_inputs(dev):
    x = _scene_x(1, 4, 21, 35, 60)
    rng = np.random.default_rng(61)
    flat = x.reshape(-1)
    idx = rng.permutation(flat.size)[:400]
    flat[idx[:100]] = np.nan
    flat[idx[100:200]] = -rng.random(100).astype(np.float32)
    flat[idx[200:300]] = 1.0 + 3.0 * rng.random(100).astype(np.float32)
    flat[idx[300:350]] = np.inf
    flat[idx[350:]] = -np.inf
    _both(dev, x, NR.vst_tables(K, SIGMA, [BLK] * 4), 5, 3, 16, 1, R.bm3d_tables(4, 1), R.FRAC)


@pytest.mark.parametrize('h,w', [(9, 33), (12, 11)])
def test_unaligned_base_and_odd_widths(dev, h, w):
    import torch
    x = _scene_x(1, 4, h, w, 70 + w)
    buf = torch.zeros(x.size + 64, dtype=torch.float32, device=dev)
    off = (-(buf.data_ptr() // 4)) % 4 + 1                                     # one float past a 16-byte boundary
    view = buf[off:off + x.size].view(x.shape)
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    _both(dev, x, NR.vst_tables(K, SIGMA, [BLK] * 4), 7, 3, 16, 1, R.bm3d_tables(4, 1), R.FRAC, x_dev=view)


def _entry(dev, xd, fd, guide, S, step, Gmax, mix, tau, par, win, frac, out, ws, ws_bytes):
    import torch
    from eld_amd import _lib as L
    N, C, h, w = (int(v) for v in xd.shape)
    pr = np.ascontiguousarray(par, dtype=np.uint32)
    wn = np.ascontiguousarray(win, dtype=np.uint8)
    with torch.cuda.device(dev):
        rc = L.lib().eld_bm3d_vst_f32(L.dptr(xd), N, C, h, w, 65535.0, L.dptr(fd), L.dptr(guide), S, step, Gmax, mix, tau,
                                      pr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), wn.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), frac,
                                      L.dptr(out), L.dptr(ws), ws_bytes, L.cur_stream())
    torch.cuda.synchronize()
    return rc


def test_repeat_call_sentinel_output_dirty_workspace_and_short_workspace(dev):
    import torch
    from eld_amd import _lib as L
    x = _scene_x(2, 4, 19, 23, 80)
    fwd = NR.vst_tables(K, SIGMA, [BLK] * 4)
    tau1, thr, tau2, s2, win = R.bm3d_tables(4, 1)
    ref1 = R.bm3d_fast(x, 65535.0, fwd, None, 6, 3, 16, 1, tau1, thr, win, R.FRAC)
    ref2 = R.bm3d_fast(x, 65535.0, fwd, ref1, 6, 3, 16, 1, tau2, s2, win, R.FRAC)
    xd = torch.from_numpy(x).to(dev)
    fd = torch.from_numpy(fwd.view(np.int16)).to(dev)
    gd = torch.from_numpy(ref1).to(dev)
    need = int(L.lib().eld_bm3d_vst_workspace_bytes(2, 4, 19, 23))
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=dev)               # never cleared by the caller
    out = torch.full((2, 4, 19, 23), -123456789, dtype=torch.int32, device=dev)
    for guide, tau, par, ref in ((None, tau1, thr, ref1), (gd, tau2, s2, ref2), (None, tau1, thr, ref1), (gd, tau2, s2, ref2)):
        assert _entry(dev, xd, fd, guide, 6, 3, 16, 1, tau, par, win, R.FRAC, out, ws, need) == 0
        _equal(out, ref, 'into a used workspace')
        out.fill_(0x5A5A5A5A)
    assert _entry(dev, xd, fd, None, 6, 3, 16, 1, tau1, thr, win, R.FRAC, out, ws, need - 1) == -3          # ELD_EWS: nothing ran
    assert int(out.min()) == int(out.max()) == 0x5A5A5A5A


# ---- the closed loop ------------------------------------------------------------------------------------------------------------------------
def _mosaic(planes, cfa):
    """(C,h,w) codes of the packed planes -> the uint16 mosaic that packs to them (X-Trans: whole cells only)"""
    C, h, w = planes.shape
    if cfa == 'bayer':
        m = np.zeros((2 * h, 2 * w), np.uint16)
        for k in range(4):
            oy, ox = [int(v[0]) for v in np.where(np.asarray(PAT) == k)]
            m[oy::2, ox::2] = planes[k]
        return m
    from oracle import noise_ref as O
    rows, cols = O.xtrans_source_index(h, w)
    m = np.zeros((3 * h, 3 * w), np.uint16)
    m[rows, cols] = planes
    return m


@pytest.fixture(scope='module')
def scenes():
    """cfa -> (clean DN (C,h,w), noisy codes (C,h,w), mosaic, black, the NumPy pipeline's output (C,h,w)): computed once, left unchanged"""
    out = {}
    for cfa, C, black in (('bayer', 4, BLK), ('xtrans', 9, 1024)):
        clean = NR.scene_planes(C, 64, 64)
        codes = NR.noisy_codes(clean, K, SIGMA, black, WHITE, 5)
        ref = R.denoise_planes_bm3d(codes[None], K, SIGMA, [black] * C, WHITE, RATIO)[0]
        for a in (clean, codes, ref):
            a.setflags(write=False)
        out[cfa] = (clean, codes, _mosaic(codes, cfa), black, ref)
    return out


@pytest.mark.parametrize('cfa', ['bayer', 'xtrans'])
def test_denoise_raw_equals_the_numpy_pipeline(dev, scenes, cfa):
    """Only the float64 elementwise inverse can differ between the device and NumPy: a final float32 rounding, 1e-6 = 16 float32 ulps."""
    from eld_amd.classical import ClassicalDenoiser
    from eld_amd.denoise import denoise_raw
    clean, codes, mosaic, black, ref = scenes[cfa]
    den = ClassicalDenoiser(cfa, K, sigma=SIGMA, method='bm3d')
    assert den.mix is (cfa == 'bayer')
    res = denoise_raw(den, mosaic, cfa, raw_pattern=PAT if cfa == 'bayer' else None, black_level=black, white_point=WHITE, ratio=RATIO)
    got = res['packed']
    assert got.dtype == np.float32 and got.shape == (1,) + ref.shape
    np.testing.assert_allclose(got[0], ref, rtol=1e-6, atol=0)
    target = clean * RATIO / (WHITE - black)
    clipped = np.clip((codes.astype(np.float64) - black) / (WHITE - black) * RATIO, 0.0, 1.0)
    gain = NR.psnr(got[0], target) - NR.psnr(clipped, target)
    print('%s: PSNR in %.2f dB, out %.2f dB, gain %.2f dB' % (cfa, NR.psnr(clipped, target), NR.psnr(got[0], target), gain))
    assert gain >= 6.0
    import denoise_ref as DR
    if cfa == 'bayer':
        want = DR.unpack_bayer(got, PAT, [black] * 4, WHITE, 'nearest')
    else:
        want = DR.unpack_xtrans(got, mosaic[None], black, WHITE, 'nearest')
    assert res['mosaic'].dtype == np.uint16 and np.array_equal(res['mosaic'], want[0])


def test_outputs_have_the_shapes_and_types_of_the_network_path(dev, scenes):
    import torch
    from eld_amd.classical import ClassicalDenoiser
    from eld_amd.denoise import denoise_raw, load_denoiser
    from eld_amd.unet import UNetSeeInDark
    _, _, mosaic, black, _ = scenes['bayer']
    torch.manual_seed(7)
    net = load_denoiser(UNetSeeInDark(4, 4), cfa='bayer')
    kw = dict(raw_pattern=PAT, black_level=black, white_point=WHITE, ratio=RATIO, wb=[2.0, 1.0, 1.5], ccm=np.eye(3))
    base = ClassicalDenoiser('bayer', K, sigma=SIGMA, method='bm3d')
    for extra in ({}, {'srgb_size': 'full', 'linear': True}):
        a, b = denoise_raw(net, mosaic, 'bayer', **kw, **extra), denoise_raw(base, mosaic, 'bayer', **kw, **extra)
        assert set(a) == set(b)
        for k in a:
            assert type(a[k]) is type(b[k]) and a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
    t = torch.from_numpy(np.stack([mosaic, mosaic]).view(np.int16)).to(dev)
    res = denoise_raw(base, t, 'bayer', raw_pattern=PAT, black_level=black, white_point=WHITE, ratio=[RATIO, 50.0])
    assert res['packed'].is_cuda and res['packed'].shape == (2, 4, 64, 64) and res['mosaic'].shape == t.shape and res['mosaic'].dtype == t.dtype
    np.testing.assert_allclose(res['packed'][1].cpu().numpy() * 2.0, res['packed'][0].cpu().numpy(), rtol=1e-6)           # the ratio is per frame
    with pytest.raises(ValueError, match='6 x 7'):
        denoise_raw(base, np.full((12, 14), 600, np.uint16), 'bayer', raw_pattern=PAT, black_level=black, white_point=WHITE, ratio=RATIO)


def test_evaluate_pairs_with_either_baseline(dev, scenes):
    import torch
    from eld_amd.classical import ClassicalDenoiser
    from eld_amd.denoise import load_denoiser
    from eld_amd.evaluate import curve_lines, evaluate_pairs, table_lines
    from eld_amd.unet import UNetSeeInDark
    clean, codes, mosaic, black, _ = scenes['bayer']
    long_ = _mosaic(np.clip(np.rint(clean * RATIO + black), 0, WHITE).astype(np.uint16), 'bayer')
    pairs = [{'short': mosaic, 'long': long_, 'ratio': RATIO, 'iso': 800, 'name': 'a'},
             {'short': mosaic, 'long': long_, 'ratio': RATIO, 'iso': 800, 'name': 'b', 'K': 3.0}]
    torch.manual_seed(7)
    net = load_denoiser(UNetSeeInDark(4, 4), cfa='bayer')
    plain = evaluate_pairs(net, pairs, 'bayer', PAT, black, WHITE)
    rep = evaluate_pairs(net, pairs, 'bayer', PAT, black, WHITE, baseline=ClassicalDenoiser('bayer', K, sigma=SIGMA, method='bm3d'))
    old = evaluate_pairs(net, pairs, 'bayer', PAT, black, WHITE, baseline=ClassicalDenoiser('bayer', K, sigma=SIGMA))
    for row, prow, orow in zip(rep['pairs'], plain['pairs'], old['pairs']):
        print('%s: PSNR bm3d %.2f, nlm %.2f, in %.2f' % (row['name'], row['psnr_bm3d'], orow['psnr_nlm'], row['psnr_in']))
        assert set(row) - set(prow) == {'psnr_bm3d', 'ssim_bm3d'} and set(orow) - set(prow) == {'psnr_nlm', 'ssim_nlm'}
        assert row['psnr_bm3d'] > row['psnr_in'] and 0.0 < row['ssim_bm3d'] <= 1.0
        assert set(row['sums']) == set(row['curves']) == set(orow['sums']) == {'output', 'input', 'baseline'}
        assert row['psnr'] == prow['psnr'] == orow['psnr']
    assert rep['pairs'][0]['psnr_bm3d'] > old['pairs'][0]['psnr_nlm']          # the gain of sec. 25 at the scene's own K
    assert rep['pairs'][0]['psnr_bm3d'] != rep['pairs'][1]['psnr_bm3d']         # the pair's own K reached with_gain
    assert set(rep['pooled']) == set(old['pooled']) == {'output', 'input', 'baseline'}
    assert set(rep['mean']) - set(plain['mean']) == {'psnr_bm3d', 'ssim_bm3d'} and set(old['mean']) - set(plain['mean']) == {'psnr_nlm', 'ssim_nlm'}
    assert rep['mean']['psnr_bm3d'] == float(np.mean([r['psnr_bm3d'] for r in rep['pairs']]))
    assert rep['table'][0]['psnr_bm3d'] == rep['mean']['psnr_bm3d'] and set(old['table'][0]) - set(plain['table'][0]) == {'psnr_nlm', 'ssim_nlm'}
    # the printed report: NLM's lines are what they were, BM3D's carry its label
    r = old['table'][0]
    assert table_lines(old['table'])[0] == table_lines(plain['table'])[0] + ' %9s %8s' % ('PSNR nlm', 'SSIM nlm')
    assert table_lines(old['table'])[1] == table_lines(plain['table'])[1] + ' %9.3f %8.4f' % (r['psnr_nlm'], r['ssim_nlm'])
    assert table_lines(rep['table'])[0] == table_lines(plain['table'])[0] + ' %9s %8s' % ('PSNR bm3d', 'SSIM bm3d')
    head = curve_lines(plain['pooled'], plain['groups'])[0]
    assert curve_lines(old['pooled'], old['groups'])[0] == head + ' | %10s %10s' % ('bias nlm', 'rmse nlm')
    assert curve_lines(rep['pooled'], rep['groups'], 'bm3d')[0] == head + ' | %10s %10s' % ('bias bm3d', 'rmse bm3d')


def test_command_lines(dev, scenes, tmp_path):
    import torch
    from eld_amd import classical as Cl
    from eld_amd import evaluate as E
    from eld_amd.denoise import denoise_raw, load_denoiser
    from eld_amd.unet import UNetSeeInDark
    clean, codes, mosaic, black, _ = scenes['bayer']
    np.save(str(tmp_path / 'f.npy'), mosaic)
    meta = {'cfa': 'bayer', 'raw_pattern': PAT, 'black_level_per_channel': [black] * 4, 'white_level': WHITE, 'ratio': RATIO,
            'camera_whitebalance': [2.0, 1.0, 1.5, 1.0], 'rgb_camera_matrix': np.eye(3).tolist()}
    (tmp_path / 'sensor.json').write_text(json.dumps(meta))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = Cl.main([str(tmp_path / 'f.npy'), '-o', str(tmp_path / 'out'), '--meta', str(tmp_path / 'sensor.json'), '--K', str(K), '--sigma', str(SIGMA),
                      '--method', 'bm3d', '--step', '4', '--no-mix'])
    assert rc == 0 and 'f_denoised.npy' in buf.getvalue()
    want = denoise_raw(Cl.ClassicalDenoiser('bayer', K, sigma=SIGMA, method='bm3d', step=4, mix=False), mosaic, 'bayer', raw_pattern=PAT,
                       black_level=[black] * 4, white_point=WHITE, ratio=RATIO, wb=[2.0, 1.0, 1.5, 1.0], ccm=np.eye(3))
    assert np.array_equal(np.load(str(tmp_path / 'out' / 'f_denoised.npy')), want['mosaic'])
    long_ = _mosaic(np.clip(np.rint(clean * RATIO + black), 0, WHITE).astype(np.uint16), 'bayer')
    np.save(str(tmp_path / 'l.npy'), long_)
    man = dict({k: meta[k] for k in ('cfa', 'raw_pattern', 'black_level_per_channel', 'white_level')},
               pairs=[{'short': 'f.npy', 'long': 'l.npy', 'ratio': RATIO, 'iso': 800}])
    (tmp_path / 'pairs.json').write_text(json.dumps(man))
    torch.manual_seed(7)
    net = load_denoiser(UNetSeeInDark(4, 4), cfa='bayer')
    torch.save({'netG': net.net.state_dict()}, str(tmp_path / 'net.pt'))
    args = [str(tmp_path / 'pairs.json'), '--ckpt', str(tmp_path / 'net.pt'), '--baseline-K', str(K), '--baseline-sigma', str(SIGMA)]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = E.main(args + ['--json', str(tmp_path / 'rep.json'), '--baseline-method', 'bm3d'])
    text = buf.getvalue()
    assert rc == 0 and 'PSNR bm3d' in text and 'bias bm3d' in text and 'nlm' not in text
    assert 'classical baseline bm3d (search 12, step 3, group 16, across the planes, strength 1)' in text
    got = json.loads((tmp_path / 'rep.json').read_text())
    rep = E.evaluate_pairs(net, [{'short': mosaic, 'long': long_, 'ratio': RATIO, 'iso': 800, 'name': 'f'}], 'bayer', PAT, [black] * 4, WHITE,
                           baseline=Cl.ClassicalDenoiser('bayer', K, sigma=SIGMA, method='bm3d'))
    assert got['pairs'][0]['psnr_bm3d'] == rep['pairs'][0]['psnr_bm3d'] and 'psnr_nlm' not in got['pairs'][0]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = E.main(args)                                                      # the default method: every printed line is what it was
    text = buf.getvalue()
    assert rc == 0 and 'PSNR nlm' in text and 'bias nlm' in text and 'bm3d' not in text
    assert 'classical baseline (search 7, patch 2, strength 0.5): PSNR' in text
