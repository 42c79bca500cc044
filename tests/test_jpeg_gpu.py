"""GPU tests of the baseline-JPEG writer (eld_amd/jpeg.py, csrc/jpeg.hip): encode_jpeg byte for byte against the yardstick
tests/jpeg_ref.py (which test_jpeg_cpu.py pins to libjpeg-turbo) for every case, at both ends of the segment, chunk and LDS-image lengths and
from every input layout; the coefficient and histogram buffers between guard bands; denoise_raw(jpeg=...) and the DNG preview end to end."""
import io
import os
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import jpeg_ref as R                 # noqa: E402
from guarded import Guards           # noqa: E402

CASES = R.cases()
_want = {}


def want(case):
    if case.name not in _want:
        _want[case.name] = case.encode()
    return _want[case.name]


@pytest.fixture(scope='module')
def lib(eld_lib):
    assert torch.cuda.is_available()
    return eld_lib


def J():
    import eld_amd.jpeg as j
    return j


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_encode_equals_the_reference_byte_for_byte(lib, case, monkeypatch):
    j = J()
    data, _ = want(case)
    kw = dict(quality=case.quality, subsampling=case.subsampling)
    dev = torch.from_numpy(case.rgb).cuda()
    assert j.encode_jpeg(case.rgb, **kw) == data                                     # NumPy, the defaults
    assert j.encode_jpeg(dev, **kw) == data                                          # (H, W, 3) on the device
    planar = dev.permute(2, 0, 1).contiguous()
    assert j.encode_jpeg(planar, segment=R.MIN_SEGMENT, chunk=16, **kw) == data      # (3, H, W), the shortest segments and chunks
    assert j.encode_jpeg(planar, segment=2048, chunk=4096, **kw) == data
    monkeypatch.setattr(j, '_LDS_BYTES', 0)                                          # every segment by global atomic ORs
    assert j.encode_jpeg(planar, segment=R.MIN_SEGMENT, **kw) == data
    monkeypatch.setattr(j, '_LDS_BYTES', 64)                                         # some segments fit the image, some do not
    assert j.encode_jpeg(planar, segment=R.MIN_SEGMENT, **kw) == data


def test_batch_and_strided_inputs(lib):
    j = J()
    a, b = R.smooth(37, 53, 11), R.noise(37, 53, 12)
    batch = torch.from_numpy(np.stack([a, b]).transpose(0, 3, 1, 2).copy()).cuda()
    files = j.encode_jpeg(batch, quality=75, subsampling='420')
    assert isinstance(files, list) and files == [R.encode(a, 75, '420'), R.encode(b, 75, '420')]
    wide = torch.from_numpy(np.concatenate([a, b], axis=1)).cuda()
    assert j.encode_jpeg(wide[:, 53:], quality=75, subsampling='444') == R.encode(b, 75, '444')      # a view that is not contiguous
    assert j.encode_jpeg(batch.cpu().numpy(), quality=75) == files


def test_write_jpeg_and_the_command_line(lib, tmp_path):
    j = J()
    rgb = R.smooth(24, 40, 3)
    np.save(str(tmp_path / 'in.npy'), rgb)
    assert j.main([str(tmp_path / 'in.npy'), '-o', str(tmp_path / 'out.jpg'), '--quality', '80', '--subsampling', '444']) == 0
    assert open(str(tmp_path / 'out.jpg'), 'rb').read() == R.encode(rgb, 80, '444')
    assert j.write_jpeg(str(tmp_path / 'b.jpg'), rgb.transpose(2, 0, 1)) == len(R.encode(rgb, 90, '420'))
    Image = pytest.importorskip('PIL.Image')
    assert Image.open(str(tmp_path / 'b.jpg')).size == (40, 24)


EDGE = [c for c in CASES if c.name in ('one_pixel_420', 'smooth_37x53_420', 'noise_9x70_420', 'noise_9x70_444', 'dc_size_11', 'noise_q100_444')]


@pytest.mark.parametrize('case', EDGE, ids=repr)
def test_coefficients_and_histograms_between_guards(lib, case):
    from eld_amd import _lib as L
    _, info = want(case)
    H, W = case.rgb.shape[:2]
    sub = R.SUBSAMPLING[case.subsampling]
    nb = info['blocks']
    g = Guards()
    rgb = g.ro(torch.from_numpy(np.ascontiguousarray(case.rgb.transpose(2, 0, 1))).cuda(), 'rgb')
    coef = g.new((nb * 64,), torch.int16, 'coef')
    q = np.array(sum(R.quant_tables(case.quality), []), dtype=np.uint16)
    L.check(lib.eld_jpeg_coef_u8(L.dptr(rgb), H, W, sub, q.ctypes.data, L.dptr(coef), nb * 64, L.cur_stream()), 'eld_jpeg_coef_u8')
    torch.cuda.synchronize()
    g.check()
    assert np.array_equal(coef.cpu().numpy().reshape(nb, 64), info['coef'])
    ro = g.ro(coef, 'coef (read)')
    nseg = -(-nb // R.MIN_SEGMENT)
    hist = g.new((nseg * 536,), torch.int32, 'hist')
    L.check(lib.eld_jpeg_hist_i16(L.dptr(ro), nb * 64, H, W, sub, R.MIN_SEGMENT, L.dptr(hist), nseg * 536, L.cur_stream()), 'eld_jpeg_hist_i16')
    torch.cuda.synchronize()
    g.check()
    dc0, ac0, dc1, ac1 = info['hist']
    assert np.array_equal(hist.cpu().numpy().reshape(nseg, 536).sum(axis=0), np.array(dc0 + dc1 + ac0 + ac1))


def test_a_plan_that_disagrees_writes_nothing(lib):
    """seg_bit off by one bit in the second segment: that segment leaves its zeroed dwords alone, no band is touched"""
    from eld_amd import _lib as L
    j = J()
    case = [c for c in CASES if c.name == 'noise_q100_444'][0]
    planes = torch.from_numpy(np.ascontiguousarray(case.rgb.transpose(2, 0, 1))).cuda()
    e = j.Encoder(planes, case.quality, case.subsampling, segment=R.MIN_SEGMENT)
    e.coef(), e.hist(), e.plan()
    e.pack()
    good = e.d_raw.cpu().numpy().copy()
    seg = e.d_seg_bit.cpu().numpy().view(np.uint64).copy()
    bad = seg.copy()
    bad[2:] += 1
    g = Guards()
    raw = g.new((e.raw_bytes // 4 + 1,), torch.int32, 'raw')
    d_bad = torch.from_numpy(bad.view(np.uint8)).cuda()
    L.check(lib.eld_jpeg_pack_i16(L.dptr(e.d_coef), e.nblocks * 64, e.H, e.W, R.SUBSAMPLING[e.sub], e.segment, L.dptr(e.d_tables), L.dptr(d_bad),
                                  L.dptr(raw), e.raw_bytes // 4 + 1, -1, L.cur_stream()), 'eld_jpeg_pack_i16')
    torch.cuda.synchronize()
    g.check()
    got = raw.cpu().numpy()
    first_end = int(seg[1]) // 32                                    # dwords wholly inside segment 0 are as in the good run
    assert np.array_equal(got[:first_end], good[:first_end])
    lo, hi = -(-int(bad[1]) // 32), int(bad[2]) // 32                # dwords wholly inside the refused segment stay zero
    assert hi > lo and not got[lo:hi].any()


# ---- denoise_raw and the DNG preview ---------------------------------------------------------------------------------------------------------
def make_opt(tmp, channels):
    return types.SimpleNamespace(gpu_ids=[0], isTrain=True, checkpoints_dir=str(tmp), name='t', netG='unet', channels=channels, stage_in='raw',
                                 stage_out='raw', lr=1e-4, beta1=0.9, wd=0.0, loss='l1', resume=False, chop=False, precision='fp32')


@pytest.fixture(scope='module')
def checkpoints(tmp_path_factory, lib):
    """seeded random-init checkpoints, as tests/test_denoise_gpu.py writes them"""
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


def frame(shape, black, seed):
    if len(shape) == 3:
        return np.stack([frame(shape[1:], black, seed + i) for i in range(shape[0])])
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float32)
    u = black + rng.poisson(60 + 40 * np.sin(yy / 9.0 + seed) * np.cos(xx / 13.0)) + rng.normal(0, 3, size=shape)
    return np.clip(np.rint(u), 0, 16383).astype(np.uint16)


COLOUR = dict(wb=[2.1, 1.0, 1.6], ccm=[[1.6, -0.4, -0.2], [-0.2, 1.5, -0.3], [0.0, -0.5, 1.5]])


def same_result(a, b):
    assert set(a) == set(b) | {'jpeg'}
    for k in b:
        assert (a[k] is None and b[k] is None) or np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.mark.parametrize('cfa,shape,black,extra', [('bayer', (2, 64, 96), 512, {}), ('xtrans', (96, 132), 1024, {}),
                                                   ('bayer', (64, 96), 512, {'srgb_size': 'full', 'warp': True})],
                         ids=['bayer-stack', 'xtrans', 'bayer-full-warp'])
def test_denoise_raw_with_jpeg(lib, checkpoints, cfa, shape, black, extra):
    from eld_amd.denoise import denoise_raw, load_denoiser
    from eld_amd.dng_opcodes import Warp
    u = frame(shape, black, 5)
    kw = dict(COLOUR, black_level=black, ratio=40.0, **extra)
    if kw.get('warp'):
        kw['warp'] = Warp([[1.0, 0.02, -0.01, 0.0, 0.001, -0.001]], 0.48, 0.53)
    den = load_denoiser(checkpoints[4 if cfa == 'bayer' else 9], cfa=cfa)
    plain = denoise_raw(den, u, cfa, **kw)
    res = denoise_raw(den, u, cfa, jpeg=dict(quality=85, subsampling='444'), **kw)
    same_result(res, plain)
    n = 1 if u.ndim == 2 else u.shape[0]
    assert isinstance(res['jpeg'], list) and len(res['jpeg']) == n and res['srgb'].std() > 0
    for i in range(n):
        assert res['jpeg'][i] == R.encode(np.ascontiguousarray(np.moveaxis(res['srgb'][i], 0, -1)), 85, '444')
    if cfa == 'xtrans':                                              # the defaults; a device tensor in, device tensors and host bytes out
        t = torch.from_numpy(u.view(np.int16)).cuda()
        rt = denoise_raw(den, t, cfa, jpeg={}, **kw)
        assert rt['srgb'].is_cuda and rt['jpeg'][0] == R.encode(np.ascontiguousarray(np.moveaxis(res['srgb'][0], 0, -1)), 90, '420')
        with pytest.raises(ValueError, match='jpeg'):
            denoise_raw(den, u, cfa, black_level=black, jpeg={})    # no sRGB output to encode
        with pytest.raises(ValueError, match='quality'):
            denoise_raw(den, u, cfa, jpeg=dict(quality=0), **kw)
    if extra:
        with pytest.raises(ValueError, match='linear'):
            denoise_raw(den, u, cfa, jpeg={}, linear=True, **kw)


def test_run_frames_writes_jpeg_and_a_dng_with_a_preview(lib, checkpoints, tmp_path):
    from eld_amd import dng as d
    from eld_amd.denoise import load_denoiser, parse_args, run_frames
    u = frame((64, 96), 512, 6)
    src = tmp_path / 'frame.npy'
    np.save(str(src), u)
    argv = ['--ckpt', checkpoints[4], '--raw-pattern', '0', '1', '3', '2', '--black', '512', '--ratio', '40', '--wb', '2.1', '1.0', '1.6', '--ccm'] + [str(v) for r in COLOUR['ccm'] for v in r]
    argv += ['--dng', '--dng-preview', '--dng-compression', 'ljpeg', '--jpeg', '80', '--jpeg-subsampling', '444', str(src), '-o', str(tmp_path / 'out')]
    inputs, outdir, ckpt, o = parse_args(argv)
    assert run_frames(load_denoiser(ckpt, cfa='bayer'), inputs, outdir, o) == 0
    out = tmp_path / 'out'
    srgb = np.load(str(out / 'frame_srgb.npy'))
    jpg = open(str(out / 'frame_srgb.jpg'), 'rb').read()
    assert jpg == R.encode(srgb, 80, '444')
    path = str(out / 'frame_denoised.dng')
    mosaic, meta = d.read_dng(path)
    assert np.array_equal(mosaic, np.load(str(out / 'frame_denoised.npy'))) and meta['compression'] == 7
    t, buf = d.parse_tiff(path)
    off, n = d._get1(t.ifd0, d.T_STRIPOFFSETS), d._get1(t.ifd0, d.T_STRIPBYTECOUNTS)
    assert bytes(buf[off:off + n]) == jpg and d._get1(t.ifd0, d.T_NEWSUBFILETYPE) == 1 and len(t.subifds) == 1
    Image = pytest.importorskip('PIL.Image')
    shown = np.asarray(Image.open(io.BytesIO(bytes(buf[off:off + n]))).convert('RGB'))
    assert shown.shape == srgb.shape
    # quality 80 at 4:4:4 on a smooth render: the decoded preview is the render to within the quantisation's few grey levels
    print('preview against the render: mean |d| %.3f, max %d' % (np.abs(shown.astype(int) - srgb).mean(), np.abs(shown.astype(int) - srgb).max()))
    assert np.array_equal(shown, np.asarray(Image.open(io.BytesIO(R.encode(srgb, 80, '444'))).convert('RGB')))
    # the converter's --preview: the same mosaic and tags re-written around another JPEG
    other = tmp_path / 'other.jpg'
    other.write_bytes(R.encode(srgb, 60, '420'))
    assert d.main([path, '-o', str(tmp_path / 'again.dng'), '--compression', 'ljpeg', '--preview', str(other)]) == 0
    t2, buf2 = d.parse_tiff(str(tmp_path / 'again.dng'))
    off2, n2 = d._get1(t2.ifd0, d.T_STRIPOFFSETS), d._get1(t2.ifd0, d.T_STRIPBYTECOUNTS)
    assert bytes(buf2[off2:off2 + n2]) == other.read_bytes() and tuple(t2.ifd0[d.T_YCBCRSUBSAMPLING].values) == (2, 2)
    assert np.array_equal(d.read_dng(str(tmp_path / 'again.dng'))[0], mosaic) and d.dng_meta(str(tmp_path / 'again.dng'))['wb'] == meta['wb']
    # without the new options the outputs are the files of before
    inputs, outdir, ckpt, o = parse_args(argv[:argv.index('--dng-preview')] + ['--dng-compression', 'ljpeg', str(src), '-o', str(tmp_path / 'old')])
    assert run_frames(load_denoiser(ckpt, cfa='bayer'), inputs, outdir, o) == 0
    assert sorted(os.listdir(str(tmp_path / 'old'))) == [f for f in sorted(os.listdir(str(out))) if f != 'frame_srgb.jpg']
    assert len(d.parse_tiff(str(tmp_path / 'old' / 'frame_denoised.dng'))[0].subifds) == 0
    assert np.array_equal(np.load(str(tmp_path / 'old' / 'frame_srgb.npy')), srgb)
