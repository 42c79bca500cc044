"""The classical baseline on the device: eld_nlm_vst_f32 against tests/nlm_ref.py bit for bit -- no tolerance -- over
the shapes that reach each path of the kernel, then the closed loop: ClassicalDenoiser through denoise_raw and evaluate_pairs."""
import contextlib
import io
import json

import numpy as np
import pytest

import nlm_ref as R

pytestmark = pytest.mark.gpu

PAT = [[0, 1], [3, 2]]
BLK, WHITE, RATIO, K, SIGMA = 512, 16383, 100.0, 2.0, 3.0
LINEAR = np.maximum(255 - np.arange(256), 1).astype(np.uint16)            # every bin its own weight, none 0: a wrong bin or a lost candidate shows


@pytest.fixture(scope='module')
def dev(eld_lib):
    import torch
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def _scene_x(N, C, h, w, seed, black=BLK):
    """codes / 65535 of the noisy synthetic scene, one realisation per frame"""
    clean = R.scene_planes(C, h, w)
    codes = np.stack([R.noisy_codes(clean, K, SIGMA, black, WHITE, seed + n) for n in range(N)])
    return (codes.astype(np.float32) / np.float32(65535.0)).astype(np.float32)


def _mixed_x(N, C, h, w, seed):
    """full-range random codes in the left half (differences reach the clamp), a smooth ramp with +-3 codes of noise in the right half (small
    distances): with the table i -> i >> 1 every shift from 0 to 24 meets distances on both sides of its bins"""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 65536, size=(N, C, h, w))
    smooth = 2000 + 40 * np.arange(w)[None, None, None, :] + rng.integers(-3, 4, size=(N, C, h, w)) * 2
    codes[..., w // 2:] = smooth[..., w // 2:]
    return (codes.astype(np.float32) / np.float32(65535.0)).astype(np.float32)


HALF = (np.arange(65536) >> 1).astype(np.uint16)


def _run(dev, x, fwd, S, P, sh, wtab, frac, real=True, out=None, x_dev=None):
    """reference and kernel on the same inputs -> the kernel's output (asserted equal); real: some counted weight is neither 0 nor 255"""
    import torch
    from eld_amd.classical import nlm_vst
    seen = set()
    ref = R.nlm_cumsum(x, 65535.0, fwd, S, P, sh, wtab, frac, seen)
    if real:
        assert seen - {0, 255}, 'the case exercises no weight of the table: %r' % sorted(seen)
    xd = torch.from_numpy(x).to(dev) if x_dev is None else x_dev
    fd = torch.from_numpy(np.ascontiguousarray(fwd).view(np.int16)).to(dev)
    got = nlm_vst(xd, 65535.0, fd, S, P, sh, wtab, frac, out=out)
    torch.cuda.synchronize()
    g = got.cpu().numpy()
    assert g.dtype == np.int32 and g.shape == ref.shape
    bad = np.argwhere(g != ref)
    assert bad.size == 0, 'first of %d differences at %s: %d != %d' % (len(bad), bad[0].tolist(), g[tuple(bad[0])], ref[tuple(bad[0])])
    return got


@pytest.mark.parametrize('h,w', [(1, 1), (1, 7), (3, 5), (8, 8), (33, 70), (64, 64), (37, 129)])
def test_plane_sizes(dev, h, w):
    """planes smaller than the search radius and the halo; one tile and several with ragged edges"""
    x = _scene_x(1, 4, h, w, 10 + h)
    fwd = R.vst_tables(K, SIGMA, [BLK] * 4)
    sh, wtab = R.nlm_weight_table(4, 2, 0.5)
    _run(dev, x, fwd, 7, 2, sh, wtab, R.FRAC, real=(h, w) != (1, 1))
    if h * w <= 64:                                                          # the largest radii on the smallest planes
        _run(dev, _scene_x(1, 3, h, w, 20 + w), R.vst_tables(K, SIGMA, [BLK] * 3), 10, 3, 9, LINEAR, 8, real=(h, w) != (1, 1))


@pytest.mark.parametrize('C', [1, 3, 4, 9, 16])
def test_planes_and_batch(dev, C):
    x = _scene_x(2, C, 33, 40, 30 + C)
    assert not np.array_equal(x[0], x[1])
    fwd = R.vst_tables(K, SIGMA, [BLK + 3 * c for c in range(C)])             # a table per plane
    sh, wtab = R.nlm_weight_table(C, 1, 0.5)
    _run(dev, x, fwd, 5, 1, sh, wtab, R.FRAC)


@pytest.mark.parametrize('S', [0, 1, 5, 7, 10])
@pytest.mark.parametrize('P', [0, 1, 2, 3])
def test_radii(dev, S, P):
    x = _scene_x(1, 4, 20, 37, 40 + 4 * S + P)
    fwd = R.vst_tables(K, SIGMA, [BLK] * 4)
    sh, wtab = R.nlm_weight_table(4, P, 0.5)
    _run(dev, x, fwd, S, P, sh, wtab, R.FRAC, real=S > 0)


@pytest.mark.parametrize('frac', [0, 4, 8])
@pytest.mark.parametrize('sh', [0, 9, 24])
def test_fixed_point(dev, frac, sh):
    _run(dev, _mixed_x(1, 3, 17, 34, 50 + sh), np.stack([HALF] * 3), 3, 1, sh, LINEAR, frac)


def test_saturated_codes_largest_numerator(dev):
    """every code 32767 (the table holds 65535: the min applies), every weight 255, 441 candidates: num = 255 * 32767 * 441 > 2^31"""
    x = np.full((1, 16, 40, 45), 2.0, np.float32)
    fwd = np.full((16, 65536), 65535, np.uint16)
    got = _run(dev, x, fwd, 10, 3, 0, np.full(256, 255, np.uint16), 8, real=False)
    assert int(got.min()) == int(got.max()) == 32767 << 8
    assert 255 * 32767 * 441 > 2 ** 31


def test_checkerboard_reaches_the_clamp_and_the_largest_distance(dev):
    yy, xx = np.mgrid[0:35, 0:33]
    x = np.broadcast_to((((yy + xx) & 1) * 1.0).astype(np.float32), (1, 16, 35, 33)).copy()
    fwd = np.zeros((16, 65536), np.uint16)
    fwd[:, 32768:] = 40000                                                   # codes 0 and 32767: the difference clamps at 1023
    v = R.stabilised(x, 65535.0, fwd)
    assert set(np.unique(v).tolist()) == {0, 32767}
    _run(dev, x, fwd, 4, 3, 24, LINEAR, 4)                                    # D = 1023^2 * 16 * 49 at odd offsets inside the plane: bin 48
    assert (1023 * 1023 * 16 * 49) >> 24 == 48 and 1023 * 1023 * 16 * 49 < 2 ** 31
    _run(dev, x, fwd, 2, 3, 22, LINEAR, 0)


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
    fwd = R.vst_tables(K, SIGMA, [BLK] * 4)
    sh, wtab = R.nlm_weight_table(4, 2, 0.5)
    _run(dev, x, fwd, 5, 2, sh, wtab, R.FRAC)


@pytest.mark.parametrize('h,w', [(9, 33), (12, 7)])
def test_unaligned_base_and_odd_widths(dev, h, w):
    import torch
    x = _scene_x(1, 4, h, w, 70 + w)
    buf = torch.zeros(x.size + 64, dtype=torch.float32, device=dev)
    off = (-(buf.data_ptr() // 4)) % 4 + 1                                   # one float past a 16-byte boundary
    view = buf[off:off + x.size].view(x.shape)
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    fwd = R.vst_tables(K, SIGMA, [BLK] * 4)
    sh, wtab = R.nlm_weight_table(4, 2, 0.5)
    _run(dev, x, fwd, 7, 2, sh, wtab, R.FRAC, x_dev=view)


def test_repeat_call_into_a_sentinel_filled_output(dev):
    import torch
    x = _scene_x(2, 4, 33, 37, 80)
    fwd = R.vst_tables(K, SIGMA, [BLK] * 4)
    sh, wtab = R.nlm_weight_table(4, 2, 0.5)
    out = torch.full((2, 4, 33, 37), -123456789, dtype=torch.int32, device=dev)
    a = _run(dev, x, fwd, 7, 2, sh, wtab, R.FRAC, out=out).clone()
    out.fill_(0x5A5A5A5A)
    b = _run(dev, x, fwd, 7, 2, sh, wtab, R.FRAC, out=out)
    assert b.data_ptr() == out.data_ptr() and torch.equal(a, b)


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
        clean = R.scene_planes(C, 64, 64)
        codes = R.noisy_codes(clean, K, SIGMA, black, WHITE, 5)
        ref = R.denoise_planes(codes[None], K, SIGMA, [black] * C, WHITE, RATIO)[0]
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
    den = ClassicalDenoiser(cfa, K, sigma=SIGMA)
    res = denoise_raw(den, mosaic, cfa, raw_pattern=PAT if cfa == 'bayer' else None, black_level=black, white_point=WHITE, ratio=RATIO)
    got = res['packed']
    assert got.dtype == np.float32 and got.shape == (1,) + ref.shape
    np.testing.assert_allclose(got[0], ref, rtol=1e-6, atol=0)
    target = clean * RATIO / (WHITE - black)
    clipped = np.clip((codes.astype(np.float64) - black) / (WHITE - black) * RATIO, 0.0, 1.0)
    gain = R.psnr(got[0], target) - R.psnr(clipped, target)
    print('%s: PSNR in %.2f dB, out %.2f dB, gain %.2f dB' % (cfa, R.psnr(clipped, target), R.psnr(got[0], target), gain))
    assert gain >= 6.0
    # the mosaic written back is the packed output's codes
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
    wb, ccm = [2.0, 1.0, 1.5], np.eye(3)
    kw = dict(raw_pattern=PAT, black_level=black, white_point=WHITE, ratio=RATIO, wb=wb, ccm=ccm)
    base = ClassicalDenoiser('bayer', K, sigma=SIGMA)
    for extra in ({}, {'srgb_size': 'full', 'linear': True}):
        a, b = denoise_raw(net, mosaic, 'bayer', **kw, **extra), denoise_raw(base, mosaic, 'bayer', **kw, **extra)
        assert set(a) == set(b)
        for k in a:
            assert type(a[k]) is type(b[k]) and a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
    t = torch.from_numpy(np.stack([mosaic, mosaic]).view(np.int16)).to(dev)
    res = denoise_raw(base, t, 'bayer', raw_pattern=PAT, black_level=black, white_point=WHITE, ratio=[RATIO, 50.0], chop=True)      # chop: ignored
    assert res['packed'].is_cuda and res['packed'].shape == (2, 4, 64, 64) and res['mosaic'].shape == t.shape and res['mosaic'].dtype == t.dtype
    assert res['srgb'] is None
    np.testing.assert_allclose(res['packed'][1].cpu().numpy() * 2.0, res['packed'][0].cpu().numpy(), rtol=1e-6)           # the ratio is per frame
    with pytest.raises(ValueError):
        denoise_raw(ClassicalDenoiser('xtrans', K, sigma=SIGMA), mosaic, 'bayer', black_level=black)


def _same(a, b, path=''):
    if isinstance(a, dict):
        assert isinstance(b, dict) and set(a) == set(b), path
        for k in a:
            _same(a[k], b[k], path + '/' + str(k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (u, v) in enumerate(zip(a, b)):
            _same(u, v, path + '/%d' % i)
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == 'f'), path
    else:
        assert a == b or (a != a and b != b), path


def test_evaluate_pairs_with_a_baseline(dev, scenes):
    import torch
    from eld_amd.classical import ClassicalDenoiser
    from eld_amd.denoise import load_denoiser
    from eld_amd.evaluate import curve_lines, evaluate_pairs, table_lines
    from eld_amd.unet import UNetSeeInDark
    clean, codes, mosaic, black, _ = scenes['bayer']
    long_ = _mosaic(np.clip(np.rint(clean * RATIO + black), 0, WHITE).astype(np.uint16), 'bayer')
    short2 = _mosaic(R.noisy_codes(clean, K, SIGMA, black, WHITE, 6), 'bayer')
    pairs = [{'short': mosaic, 'long': long_, 'ratio': RATIO, 'iso': 800, 'name': 'a'},
             {'short': short2, 'long': long_, 'ratio': RATIO, 'iso': 800, 'name': 'b', 'K': K}]
    torch.manual_seed(7)
    net = load_denoiser(UNetSeeInDark(4, 4), cfa='bayer')
    base = ClassicalDenoiser('bayer', K, sigma=SIGMA)
    plain = evaluate_pairs(net, pairs, 'bayer', PAT, black, WHITE)
    rep = evaluate_pairs(net, pairs, 'bayer', PAT, black, WHITE, baseline=base)
    for row, prow in zip(rep['pairs'], plain['pairs']):
        print('%s: PSNR nlm %.2f, in %.2f, net %.2f' % (row['name'], row['psnr_nlm'], row['psnr_in'], row['psnr']))
        assert row['psnr_nlm'] > row['psnr_in'] and 0.0 < row['ssim_nlm'] <= 1.0
        assert set(row) - set(prow) == {'psnr_nlm', 'ssim_nlm'}
        assert set(row['sums']) == set(row['curves']) == {'output', 'input', 'baseline'}
        for k in ('sums', 'curves'):
            prow = dict(prow, **{k: dict(prow[k], baseline=row[k]['baseline'])})
        _same({k: v for k, v in row.items() if k not in ('psnr_nlm', 'ssim_nlm')}, prow)
    assert set(rep['pooled']) == {'output', 'input', 'baseline'} and set(plain['pooled']) == {'output', 'input'}
    _same({k: rep['pooled'][k] for k in plain['pooled']}, plain['pooled'])
    _same({k: rep['mean'][k] for k in plain['mean']}, plain['mean'])
    assert rep['mean']['psnr_nlm'] == float(np.mean([r['psnr_nlm'] for r in rep['pairs']]))
    assert len(rep['table']) == 1 and rep['table'][0]['psnr_nlm'] == rep['mean']['psnr_nlm']
    _same({k: v for k, v in rep['table'][0].items() if not k.endswith('_nlm')}, plain['table'][0])
    _same({k: rep[k] for k in ('groups', 'bin_lower_edges')}, {k: plain[k] for k in ('groups', 'bin_lower_edges')})
    # the baseline's level sums count every site once, and its shadows carry less bias than the clipped input's
    n = rep['pooled']['baseline']['n']
    assert int(n.sum()) == 2 * mosaic.size == int(rep['pooled']['input']['n'].sum())
    # the printed report: the old lines are a prefix of the new ones
    for old, new in zip(table_lines(plain['table']) + curve_lines(plain['pooled'], plain['groups']),
                        table_lines(rep['table']) + curve_lines(rep['pooled'], rep['groups'])):
        assert new.startswith(old) and len(new) > len(old)
    with pytest.raises(ValueError):
        evaluate_pairs(net, pairs, 'bayer', PAT, black, WHITE, baseline=net)


def test_command_lines(dev, scenes, tmp_path):
    """python -m eld_amd.classical writes what denoise_raw returns; python -m eld_amd.evaluate --baseline-K reports what the API does, and
    a pair's own 'K' replaces the command line's."""
    import torch
    from eld_amd import classical as Cl
    from eld_amd import evaluate as E
    from eld_amd.denoise import denoise_raw, load_denoiser
    from eld_amd.unet import UNetSeeInDark
    from eld_amd.validate import to_jsonable
    clean, codes, mosaic, black, _ = scenes['bayer']
    np.save(str(tmp_path / 'f.npy'), mosaic)
    meta = {'cfa': 'bayer', 'raw_pattern': PAT, 'black_level_per_channel': [black] * 4, 'white_level': WHITE, 'ratio': RATIO,
            'camera_whitebalance': [2.0, 1.0, 1.5, 1.0], 'rgb_camera_matrix': np.eye(3).tolist()}
    (tmp_path / 'sensor.json').write_text(json.dumps(meta))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = Cl.main([str(tmp_path / 'f.npy'), '-o', str(tmp_path / 'out'), '--meta', str(tmp_path / 'sensor.json'), '--K', str(K), '--sigma', str(SIGMA)])
    assert rc == 0 and 'f_denoised.npy' in buf.getvalue() and 'f_srgb.npy' in buf.getvalue()
    want = denoise_raw(Cl.ClassicalDenoiser('bayer', K, sigma=SIGMA), mosaic, 'bayer', raw_pattern=PAT, black_level=[black] * 4, white_point=WHITE,
                       ratio=RATIO, wb=[2.0, 1.0, 1.5, 1.0], ccm=np.eye(3))
    assert np.array_equal(np.load(str(tmp_path / 'out' / 'f_denoised.npy')), want['mosaic'])
    assert np.array_equal(np.load(str(tmp_path / 'out' / 'f_srgb.npy')), np.moveaxis(want['srgb'], 1, -1)[0])
    with pytest.raises(ValueError):
        Cl.main([str(tmp_path / 'f.npy'), '-o', str(tmp_path / 'out'), '--meta', str(tmp_path / 'sensor.json'), '--K', str(K)])      # no read noise
    # evaluate: the second pair names its own gain
    long_ = _mosaic(np.clip(np.rint(clean * RATIO + black), 0, WHITE).astype(np.uint16), 'bayer')
    np.save(str(tmp_path / 'l.npy'), long_)
    man = dict({k: meta[k] for k in ('cfa', 'raw_pattern', 'black_level_per_channel', 'white_level')},
               pairs=[{'short': 'f.npy', 'long': 'l.npy', 'ratio': RATIO, 'iso': 800}, {'short': 'f.npy', 'long': 'l.npy', 'ratio': RATIO, 'iso': 1600, 'K': 3.0}])
    (tmp_path / 'pairs.json').write_text(json.dumps(man))
    torch.manual_seed(7)
    net = load_denoiser(UNetSeeInDark(4, 4), cfa='bayer')
    torch.save({'netG': net.net.state_dict()}, str(tmp_path / 'net.pt'))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = E.main([str(tmp_path / 'pairs.json'), '--ckpt', str(tmp_path / 'net.pt'), '--json', str(tmp_path / 'rep.json'), '--baseline-K', str(K),
                     '--baseline-camera', 'SonyA7S2', '--baseline-search', '5'])
    text = buf.getvalue()
    assert rc == 0 and 'PSNR nlm' in text and 'bias nlm' in text and 'classical baseline (search 5, patch 2, strength 0.5)' in text
    base = Cl.ClassicalDenoiser('bayer', K, camera='SonyA7S2', search=5)
    pairs = [{'short': mosaic, 'long': long_, 'ratio': RATIO, 'iso': 800, 'name': 'f'}, {'short': mosaic, 'long': long_, 'ratio': RATIO, 'iso': 1600, 'name': 'f', 'K': 3.0}]
    want = json.loads(json.dumps(to_jsonable(E.evaluate_pairs(net, pairs, 'bayer', PAT, [black] * 4, WHITE, baseline=base))))
    got = json.loads((tmp_path / 'rep.json').read_text())
    assert json.dumps(got) == json.dumps(want)
    assert got['pairs'][0]['psnr_nlm'] != got['pairs'][1]['psnr_nlm'] and got['pairs'][0]['psnr'] == got['pairs'][1]['psnr']      # only K differs
    with pytest.raises(ValueError):
        E.main([str(tmp_path / 'pairs.json'), '--ckpt', str(tmp_path / 'net.pt'), '--baseline-K', str(K)])                       # no read noise
    with pytest.raises(ValueError):
        E.main([str(tmp_path / 'pairs.json'), '--ckpt', str(tmp_path / 'net.pt'), '--baseline-sigma', '3'])                      # no gain


@pytest.mark.parametrize('cfa', ['bayer', 'xtrans'])
def test_shading_and_flat_field_maps_apply_to_the_codes(dev, cfa):
    """With both maps the result equals the reference fed with the same corrected codes, and those codes are
    ((u - black) - (a + b t)) * g + black: the gain multiplies the signal above black, not the pedestal."""
    import torch
    from eld_amd.classical import FRAC, ClassicalDenoiser
    from eld_amd.denoise import denoise_raw
    from eld_amd.flatfield import FlatField
    from eld_amd.shading import DarkShading
    C, black = (4, BLK) if cfa == 'bayer' else (9, 1024)
    h, w = 24, 26
    clean = R.scene_planes(C, h, w)
    planes = R.noisy_codes(clean, K, SIGMA, black, WHITE, 8)
    mosaic = _mosaic(planes, cfa)
    rng = np.random.default_rng(9)
    a = rng.normal(0, 1.5, mosaic.shape).astype(np.float32)
    b = rng.normal(0, 0.002, mosaic.shape).astype(np.float32)
    g = (1.0 + rng.normal(0, 0.01, mosaic.shape)).astype(np.float32)
    pat = PAT if cfa == 'bayer' else None
    sh_map = DarkShading(a, b, 800.0, 100.0, 3200.0, cfa=cfa, raw_pattern=pat)
    ff = FlatField(np.ones_like(g), g, cfa=cfa, raw_pattern=pat)
    den = ClassicalDenoiser(cfa, K, sigma=SIGMA, search=5, patch=1)
    res = denoise_raw(den, mosaic, cfa, raw_pattern=pat, black_level=black, white_point=WHITE, ratio=RATIO, shading=sh_map, iso=1600, flatfield=ff)
    # the corrected codes the filter saw
    t3 = torch.from_numpy(mosaic.view(np.int16)).to(dev)[None]
    blk = [float(black)] * (4 if cfa == 'bayer' else 1)
    x = den.pack_codes(t3, [0, 1, 3, 2] if cfa == 'bayer' else None, blk, sh_map, sh_map.t(1600), ff).cpu().numpy()
    u = mosaic.astype(np.float64)
    want_m = ((u - black) - (a.astype(np.float64) + b.astype(np.float64) * 800.0)) * g.astype(np.float64) + black
    if cfa == 'bayer':
        want = np.stack([want_m[oy::2, ox::2] for oy, ox in ([int(v[0]) for v in np.where(np.asarray(PAT) == k)] for k in range(4))])
    else:
        from oracle import noise_ref as O
        rows, cols = O.xtrans_source_index(h, w)
        want = want_m[rows, cols]
    # float32: a relative 6e-8 per operation on values of about 600 codes, a handful of operations
    assert np.max(np.abs(x[0].astype(np.float64) * 65535.0 - want)) < 1e-3
    assert np.max(np.abs(want - planes)) > 3.0                                # the maps moved the codes
    fwd = R.vst_tables(K, SIGMA, [black] * C)
    sh, wtab = R.nlm_weight_table(C, 1, 0.5)
    out = R.nlm_cumsum(x, 65535.0, fwd, 5, 1, sh, wtab, FRAC)
    z = R.unbiased_inverse(out, FRAC, K, SIGMA)
    ref = (z * RATIO / (WHITE - black)).astype(np.float32)
    np.testing.assert_allclose(res['packed'], ref, rtol=1e-6, atol=0)
