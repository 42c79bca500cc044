"""GPU tests of the lossless-JPEG DNG writer (csrc/dng_enc.hip behind eld_amd.dng.encode_ljpeg / write_dng(compression=7)): every stream
byte for byte against tests/dng_ref.py (write_dng_file with geometry 'nf2', predictor 1, the table of Annex K.2), at the smallest segment
and chunk lengths the kernels take (64 samples, 16 bytes: every 16 x 16 tile spans four segments) and at the defaults; round trips through
the reference's bit-serial decoder and through read_dng; the range check; the two command lines.  The reference streams are encoded once."""
import json
import os
import types

import numpy as np
import pytest

import dng_enc_cases as C
import dng_ref as R

pytestmark = pytest.mark.gpu

CM = ((8000, 10000), (-2000, 10000), (-500, 10000), (-3000, 10000), (11000, 10000), (2000, 10000), (-500, 10000), (1500, 10000), (6000, 10000))
XTRANS = [0, 2, 1, 2, 0, 1, 1, 1, 0, 1, 1, 2, 1, 1, 2, 1, 1, 0, 2, 0, 1, 0, 2, 1, 1, 1, 2, 1, 1, 0, 1, 1, 0, 1, 1, 2]
SMALLEST = (64, 16)                                                  # segment (samples), chunk (bytes)
CASES = C.gpu_cases()


@pytest.fixture(scope='module')
def dng(eld_lib):
    import torch
    if not torch.cuda.is_available():
        pytest.fail('these tests need a GPU')
    import eld_amd.dng as d
    return d


@pytest.fixture(scope='module')
def reference(tmp_path_factory):
    """name -> the info of dng_ref.write_dng_file: its streams are what encode_ljpeg must return"""
    tmp = tmp_path_factory.mktemp('ref')
    return {name: R.write_dng_file(str(tmp / (name + '.dng')), img, bits=bits, compression=7, tile=tile, ljpeg=dict(P=bits, geometry='nf2', pred=1))
            for name, (img, tile, bits, _) in CASES.items()}


def test_reference_holds_what_the_cases_are_for(reference):
    """the figures the cases were chosen for, from the reference alone"""
    stuffed = {k: sum(n['stuffed'] for n in v['notes']) for k, v in reference.items()}
    entropy = {k: [len(s) - n['header_len'] - 2 for s, n in zip(v['streams'], v['notes'])] for k, v in reference.items()}
    assert len(reference['ramp_edges']['streams']) == 12 and stuffed['ramp_edges'] == 15
    assert len(reference['ramp_large']['streams']) == 9 and stuffed['ramp_large'] == 350
    assert max(n['max_code_len'] for n in reference['ramp_large']['notes']) == 13
    from eld_amd import _lib as L
    assert 64 * 128 >= 2 * L.DNG_ENC_SEGMENT                         # at least two segments a stream at the default
    assert entropy['flat'] == [32] and reference['flat']['notes'][0]['tables'][0] == ([1] + [0] * 15, [0])
    assert 16 in reference['columns']['notes'][0]['tables'][0][1]
    assert stuffed['ramp255'] == 32
    assert stuffed['walk'] == 933 and 4000 < entropy['walk'][0] < 4200
    assert reference['walk']['streams'][0].count(b'\xff\x00\xff\x00') == 43
    for name, (_, _, _, need) in CASES.items():
        assert stuffed[name] >= need, name


@pytest.mark.parametrize('cut', [SMALLEST, (0, 0)], ids=['smallest', 'default'])
@pytest.mark.parametrize('name', list(CASES))
def test_streams_equal_the_reference(dng, reference, name, cut):
    img, tile, bits, need = CASES[name]
    ref = reference[name]
    assert sum(n['stuffed'] for n in ref['notes']) >= need
    assert tile[0] * tile[1] >= 3 * SMALLEST[0]                      # at least three segments a stream at the smallest setting
    got = dng.encode_ljpeg(img, tile=tile, bits=bits, segment=cut[0], chunk=cut[1])
    assert len(got) == len(ref['streams'])
    for i, (a, b) in enumerate(zip(got, ref['streams'])):
        assert isinstance(a, bytes) and a == b, (name, cut, i)


def test_device_tensor_is_used_in_place(dng, reference):
    import torch
    img, tile, bits, _ = CASES['ramp_edges']
    t = torch.from_numpy(img.view(np.int16)).cuda()
    keep = t.clone()
    assert dng.encode_ljpeg(t, tile=tile, bits=bits) == reference['ramp_edges']['streams']
    assert torch.equal(t, keep)
    with pytest.raises(ValueError, match='CUDA'):
        dng.encode_ljpeg(t.cpu(), tile=tile, bits=bits)


def source(path, img, cfa):
    """a source DNG whose tags must survive like=: levels, neutral, colour matrix, make, ISO"""
    kw = dict(cfa=XTRANS, cfa_dim=(6, 6), tags={50713: (R.SHORT, (1, 1)), 50714: (R.SHORT, (1024,)), 50717: (R.LONG, (16000,))}) if cfa == 'xtrans' else \
        dict(cfa=(2, 1, 1, 0), tags={50714: (R.RATIONAL, ((1024, 2),)), 50717: (R.LONG, (16000,))})
    return R.write_dng_file(str(path), img, bits=14, compression=1,
                            tags0={50728: (R.RATIONAL, ((473, 1000), (1, 1), (640001, 1000000))), 50721: (R.SRATIONAL, CM), 50778: (R.SHORT, (21,)),
                                   271: (R.ASCII, 'Acme'), 272: (R.ASCII, 'Cam 1')}, exif={34855: (R.SHORT, (1600,)), 33434: (R.RATIONAL, ((10, 300),))}, **kw)


@pytest.mark.parametrize('cfa', ['bayer', 'xtrans'])
def test_round_trips(dng, tmp_path, cfa):
    """our streams through the reference's bit-serial decoder (no code shared with any encoder); our file through read_dng; the tags of the
    source survive"""
    import torch
    img = R.noisy_ramp(40, 56, 14, seed=3) if cfa == 'bayer' else R.noisy_ramp(36, 42, 14, seed=6)
    src = source(tmp_path / 'src.dng', img, cfa)['path']
    streams = dng.encode_ljpeg(img, tile=(16, 16), bits=14)
    for s, t in zip(streams, C.tiles_of(img, (16, 16))):
        seq, hdr = R.ljpeg_decode(s)
        assert hdr == {'P': 14, 'X': 8, 'Y': 16, 'Nf': 2, 'pred': 1} and np.array_equal(seq.reshape(16, 16), t)
    out = str(tmp_path / 'out.dng')
    dng.write_dng(out, torch.from_numpy(img.view(np.int16)).cuda(), like=src, compression=7, tile=(16, 16), bits=14)
    back, m = dng.read_dng(out)
    assert np.array_equal(back, img) and m['compression'] == 7 and m['bits'] == 14
    a = dng.dng_meta(src)
    for k in ('cfa', 'raw_pattern', 'black_level', 'white_point', 'wb', 'ccm', 'iso', 'exposure_time', 'make', 'model'):
        assert a[k] == m[k], k
    t, buf = dng.parse_tiff(out)
    assert tuple(t.ifd0[50721].values) == CM                         # the source's rationals
    assert cfa == 'xtrans' or tuple(t.ifd0[50714].values) == ((1024, 2),)
    assert 273 not in t.ifd0 and 278 not in t.ifd0 and 279 not in t.ifd0                # no strip tags
    assert tuple(t.ifd0[322].values) == (16,) and tuple(t.ifd0[323].values) == (16,)
    offs, cnts = [int(v) for v in t.ifd0[324].values], [int(v) for v in t.ifd0[325].values]
    assert cnts == [len(s) for s in streams] and [bytes(buf[o:o + c]) for o, c in zip(offs, cnts)] == streams
    assert np.array_equal(R.ref_read({'H': img.shape[0], 'W': img.shape[1], 'compression': 7, 'streams': streams,
                                      'geo': [(x0, y0, 16, 16) for y0 in range(0, img.shape[0], 16) for x0 in range(0, img.shape[1], 16)]}), img)
    # the defaults: one 256 x 256 tile at 16 bits, a NumPy mosaic
    dng.write_dng(out, img, like=src, compression=7)
    back, m = dng.read_dng(out)
    assert np.array_equal(back, img) and m['compression'] == 7 and m['bits'] == 16
    t, _ = dng.parse_tiff(out)
    assert tuple(t.ifd0[322].values) == (256,) and tuple(t.ifd0[323].values) == (256,) and len(t.ifd0[324].values) == 1


def test_code_beyond_bits_is_refused(dng, reference, tmp_path):
    img = R.noisy_ramp(40, 56, 12, seed=9)
    img[21, 37] = 4096                                               # tile 1 * 4 + 2 = 6 of the 16 x 16 cut
    p = str(tmp_path / 'x.dng')
    with pytest.raises(ValueError, match=r'4096 in tile 6\b'):
        dng.write_dng(p, img, meta={'cfa': 'bayer'}, compression=7, tile=(16, 16), bits=12)
    assert not os.path.exists(p)
    with pytest.raises(ValueError, match=r'4096 in tile 6\b'):
        dng.encode_ljpeg(img, tile=(16, 16), bits=12)
    assert len(dng.encode_ljpeg(img, tile=(16, 16), bits=13)) == 12
    name = 'ramp_edges'                                              # the next encode is still exact
    assert dng.encode_ljpeg(CASES[name][0], tile=CASES[name][1], bits=CASES[name][2]) == reference[name]['streams']


def test_converter_rewrites_a_dng(dng, tmp_path):
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:48, 0:64]
    img = np.clip(np.rint(600 + 20 * xx + 9 * yy + rng.normal(0, 5, (48, 64))), 0, 16383).astype(np.uint16)   # about 6 bits a sample
    src = source(tmp_path / 'in.dng', img, 'bayer')['path']
    plain, packed = str(tmp_path / 'plain.dng'), str(tmp_path / 'packed.dng')
    assert dng.main([src, '-o', plain]) == 0
    assert dng.main([src, '-o', packed, '--compression', 'ljpeg', '--tile', '16', '32', '--bits', '14']) == 0
    a, ma = dng.read_dng(plain)
    b, mb = dng.read_dng(packed)
    assert np.array_equal(a, img) and np.array_equal(b, img)
    assert (ma['compression'], ma['bits'], mb['compression'], mb['bits']) == (1, 16, 7, 14)
    assert ma['black_level'] == mb['black_level'] == dng.dng_meta(src)['black_level'] and ma['make'] == mb['make'] == 'Acme'
    assert os.path.getsize(packed) < os.path.getsize(plain)
    with pytest.raises(SystemExit):
        dng.main([src, '-o', str(tmp_path / 'f.npy'), '--compression', 'ljpeg'])


def test_denoise_command_line_writes_ljpeg(dng, tmp_path):
    """denoise --dng --dng-compression ljpeg on one 256 x 256 frame (one tile of the default cut): the file reads back as the .npy of the same
    call, carries the source's tags and is smaller than the uncompressed file of the same mosaic"""
    import torch
    from eld_amd import denoise
    from eld_amd.model import ELDModel
    torch.manual_seed(2018)
    m = ELDModel()
    m.initialize(types.SimpleNamespace(gpu_ids=[0], isTrain=True, checkpoints_dir=str(tmp_path / 'ck'), name='t', netG='unet', channels=4, stage_in='raw',
                                       stage_out='raw', lr=1e-4, beta1=0.9, wd=0.0, loss='l1', resume=False, chop=False, precision='fp32'))
    m.save('latest')
    ckpt = os.path.join(m.save_dir, 'model_latest.pt')
    del m
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:256, 0:256]
    img = np.clip(np.rint(512 + 300 * (xx + yy) / 512.0 + rng.normal(0, 6, (256, 256))), 0, 16383).astype(np.uint16)
    src = source(tmp_path / 'f.dng', img, 'bayer')['path']
    out = str(tmp_path / 'out')
    assert denoise.main([src, '--ckpt', ckpt, '-o', out, '--dng', '--dng-compression', 'ljpeg']) == 0
    want = np.load(os.path.join(out, 'f_denoised.npy'))
    back, meta = dng.read_dng(os.path.join(out, 'f_denoised.dng'))
    assert np.array_equal(back, want) and meta['compression'] == 7 and meta['bits'] == 16
    assert meta['black_level'] == dng.dng_meta(src)['black_level'] and meta['make'] == 'Acme'
    plain = str(tmp_path / 'plain.dng')
    dng.write_dng(plain, want, like=src)
    assert os.path.getsize(os.path.join(out, 'f_denoised.dng')) < os.path.getsize(plain)
    with pytest.raises(ValueError, match='--dng'):
        denoise.main([src, '--ckpt', ckpt, '-o', out, '--dng-compression', 'ljpeg'])


def test_burst_command_line_writes_ljpeg(dng, tmp_path):
    """burst -o clean.dng: the stack leaves the device as lossless-JPEG tiles, with the tags of the first .dng input, or of the sidecar"""
    import burst_ref as B
    from eld_amd.burst import main
    fr = B.scene_burst(2, N=4, Hm=256, Wm=256)
    names = []
    for i, f in enumerate(fr):
        names.append(R.write_dng_file(str(tmp_path / ('f%d.dng' % i)), f, bits=14, compression=1, tags={50714: (R.SHORT, (512,)), 50717: (R.LONG, (16383,))},
                                      tags0={271: (R.ASCII, 'Acme')})['path'])
        np.save(str(tmp_path / ('g%d.npy' % i)), f)
    (tmp_path / 'sensor.json').write_text(json.dumps({'raw_pattern': [[0, 1], [3, 2]], 'black_level_per_channel': [512] * 4, 'white_level': 16383}))
    npy = str(tmp_path / 'clean.npy')
    assert main(names + ['-o', npy]) == 0
    want = np.load(npy)
    for tag, argv in (('like', names), ('meta', [str(tmp_path / 'g*.npy'), '--meta', str(tmp_path / 'sensor.json')])):
        out = str(tmp_path / (tag + '.dng'))
        assert main(argv + ['-o', out]) == 0
        back, meta = dng.read_dng(out)
        assert np.array_equal(back, want) and meta['compression'] == 7 and meta['black_level'] == [512] * 4 and meta['white_point'] == 16383
        assert meta.get('make') == ('Acme' if tag == 'like' else None)
        assert os.path.getsize(out) < 2 * want.size
