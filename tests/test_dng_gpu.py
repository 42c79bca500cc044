"""GPU tests of the DNG reader: every decode of eld_amd.dng.read_dng (csrc/dng.hip) against tests/dng_ref.py, bit for bit, on the
device='cuda' path and on the device=None path.  Shapes are the smallest that reach every branch: clipped edge tiles in both directions,
strips, more streams than one wave's lanes, rows that end inside a byte."""
import json
import os

import numpy as np
import pytest

import dng_ref as R

pytestmark = pytest.mark.gpu

CM = ((8000, 10000), (-2000, 10000), (-500, 10000), (-3000, 10000), (11000, 10000), (2000, 10000), (-500, 10000), (1500, 10000), (6000, 10000))


@pytest.fixture(scope='module')
def dng(eld_lib):
    import torch
    if not torch.cuda.is_available():
        pytest.fail('these tests need a GPU')
    import eld_amd.dng as d
    return d


def check(d, info, want=None, lanes=(0,), **ref_kw):
    """read_dng on both paths against the reference decode of the same streams"""
    if want is None:
        want = R.ref_read(info, **ref_kw)
    for n in lanes:
        d._LANES = n
        try:
            t, meta = d.read_dng(info['path'], device='cuda')
            a, _ = d.read_dng(info['path'])
        finally:
            d._LANES = 0
        assert t.is_cuda and t.is_contiguous() and str(t.dtype) == 'torch.int16' and tuple(t.shape) == want.shape
        assert isinstance(a, np.ndarray) and a.dtype == np.uint16
        assert np.array_equal(t.cpu().numpy().view(np.uint16), want), n
        assert np.array_equal(a, want), n
    return meta


def content(kind, P):
    if kind == 'ramp':
        return R.noisy_ramp(37, 50, P, seed=P)
    return R.alternating(37, 50, 0, 32768 if kind == 'ssss16' else 65535)


@pytest.mark.parametrize('P', [8, 12, 14, 16])
@pytest.mark.parametrize('geometry', ['nf1', 'nf2', 'rowdouble'])
def test_ljpeg_tiles(dng, tmp_path, P, geometry):
    """37 x 50 in 16 x 16 tiles: 3 x 4 streams, the last row and column of tiles clipped; all seven predictors; shared and per-component tables"""
    img = content('ramp', P)
    stuffed = deep16 = 0
    for pred in range(1, 8):
        per_component = geometry != 'nf1' and pred % 2 == 0          # two tables for two components
        info = R.write_dng_file(str(tmp_path / ('p%d.dng' % pred)), img, bits=P, compression=7, tile=(16, 16),
                                ljpeg=dict(P=P, geometry=geometry, pred=pred, per_component=per_component, deep=(pred == 3)))
        stuffed += sum(n['stuffed'] for n in info['notes'])
        deep16 += sum(n['max_code_len'] == 16 for n in info['notes'])
        if per_component:
            assert any(n['tables'][0] != n['tables'][1] for n in info['notes'])
        meta = check(dng, info, lanes=(0, 64) if pred in (1, 7) else (0,))
        assert meta['compression'] == 7 and meta['bits'] == P
        assert np.array_equal(R.ref_read(info), img)
    assert stuffed >= 1 and deep16 >= 1                              # a stuffed FF byte and a 16-bit code were in what the device decoded


@pytest.mark.parametrize('kind', ['ssss16', 'wrap'])
def test_ljpeg_extreme_differences(dng, tmp_path, kind):
    img = content(kind, 16)
    for geometry, pred in (('nf1', 1), ('nf2', 1), ('rowdouble', 4), ('nf1', 7), ('nf2', 6)):
        info = R.write_dng_file(str(tmp_path / 'e.dng'), img, bits=16, compression=7, tile=(16, 16), ljpeg=dict(P=16, geometry=geometry, pred=pred))
        if kind == 'ssss16' and geometry == 'nf1' and pred == 1:
            assert all(16 in n['tables'][0][1] for n in info['notes'])
        check(dng, info, want=img)


def test_more_streams_than_a_wave(dng, tmp_path):
    """144 x 128 in 16 x 16 tiles: 72 streams, each with a table of its own; every lane count from one stream per wave to a full wave"""
    img = R.noisy_ramp(144, 128, 14, seed=5)
    img[::16] = np.roll(img[::16], 7, axis=1)
    info = R.write_dng_file(str(tmp_path / 'w.dng'), img, bits=14, compression=7, tile=(16, 16), ljpeg=dict(P=14, geometry='nf2', pred=1, per_component=True))
    assert len(info['streams']) == 72
    plan = dng._plan(info['path'])
    assert len(plan[6]) > 64                                         # distinct tables after the deduplication
    check(dng, info, want=img, lanes=(0, 1, 7, 64))
    info = R.write_dng_file(str(tmp_path / 'w5.dng'), img, bits=14, compression=7, tile=(16, 16), ljpeg=dict(P=14, geometry='nf2', pred=5))
    check(dng, info, want=img, lanes=(0, 64))                        # 72 row buffers in the workspace


def test_ljpeg_strips(dng, tmp_path):
    img = R.noisy_ramp(23, 50, 12, seed=2)
    for geometry, pred in (('nf1', 1), ('nf2', 4)):
        info = R.write_dng_file(str(tmp_path / 's.dng'), img, bits=12, compression=7, rows_per_strip=5, ljpeg=dict(P=12, geometry=geometry, pred=pred))
        assert len(info['streams']) == 5 and info['geo'][-1][3] == 3
        check(dng, info, want=img)


def test_container_features(dng, tmp_path):
    img = content('ramp', 12)
    lin = (np.arange(3000, dtype=np.uint32) * 5 % 65536).astype(np.uint16)      # shorter than 2^12: the codes above 2999 take the last entry
    assert int(img.max()) > lin.size
    for compression, extra in ((7, dict(tile=(16, 16), ljpeg=dict(P=12, geometry='nf2', pred=1))), (1, dict(tile=(16, 16))), (1, dict(rows_per_strip=5))):
        info = R.write_dng_file(str(tmp_path / 'c.dng'), img, order='>', bits=12, compression=compression, subifd=True, cfa=(1, 0, 2, 1),
                                tags={50829: (R.LONG, (3, 5, 35, 45)), 50712: (R.SHORT, tuple(int(v) for v in lin))},
                                tags0={50721: (R.SRATIONAL, CM)}, **extra)
        meta = check(dng, info, active_area=(3, 5, 35, 45), lin=lin)
        assert meta['active_area'] == [3, 5, 35, 45] and meta['raw_pattern'] == [[1, 0], [2, 3]]
        want = lin[np.minimum(img, lin.size - 1)][3:35, 5:45]
        assert np.array_equal(R.ref_read(info, active_area=(3, 5, 35, 45), lin=lin), want)


@pytest.mark.parametrize('bits', [8, 10, 12, 14, 16])
def test_uncompressed(dng, tmp_path, bits):
    """width 13: 10- and 12-bit rows end inside a byte; strips and tiles; both byte orders"""
    img = R.noisy_ramp(23, 13, bits, seed=bits)
    for order in '<>':
        for extra in (dict(rows_per_strip=5), dict(), dict(tile=(16, 16)), dict(tile=(8, 5))):
            info = R.write_dng_file(str(tmp_path / 'u.dng'), img, order=order, bits=bits, compression=1, **extra)
            check(dng, info, want=img)
    big = R.noisy_ramp(70, 1030, bits, seed=1)                       # more quads than one workgroup's lanes, a grid-stride tail
    check(dng, R.write_dng_file(str(tmp_path / 'b.dng'), big, bits=bits, compression=1), want=big)


def test_corrupt_streams(dng, tmp_path):
    """the cases tools/dng_hostcheck.cpp runs on the host: a stream cut short, bits that are no code, more samples than the tile.  The error
    names the stream, and the next decode in the process is still exact."""
    img = R.noisy_ramp(32, 48, 12, seed=9)
    kw = dict(bits=12, compression=7, tile=(16, 16), ljpeg=dict(P=12, geometry='nf2', pred=1))
    good = R.write_dng_file(str(tmp_path / 'good.dng'), img, **kw)

    def cut(streams):
        n = good['notes'][4]['header_len']
        streams[4] = streams[4][:n + (len(streams[4]) - n) // 2]
        return streams
    R.write_dng_file(str(tmp_path / 'cut.dng'), img, mutate=cut, **kw)
    with pytest.raises(ValueError, match='stream 4: truncated'):
        dng.read_dng(str(tmp_path / 'cut.dng'), device='cuda')
    check(dng, good, want=img)

    def nocode(streams):
        # every table leaves the all-ones code point free (T.81 Annex C); entropy data of all-one bits (stuffed FF bytes) is no code
        n = good['notes'][2]['header_len']
        streams[2] = streams[2][:n] + b'\xff\x00' * 40 + streams[2][-2:]
        return streams
    R.write_dng_file(str(tmp_path / 'nocode.dng'), img, mutate=nocode, **kw)
    with pytest.raises(ValueError, match='stream 2: invalid code'):
        dng.read_dng(str(tmp_path / 'nocode.dng'))
    check(dng, good, want=img)

    def toomany(streams):
        t = R.noisy_ramp(18, 16, 12, seed=9)
        streams[5] = R.ljpeg_encode(t.reshape(-1), 12, 8, 18, 2)[0]
        return streams
    R.write_dng_file(str(tmp_path / 'many.dng'), img, mutate=toomany, **kw)
    with pytest.raises(ValueError, match='stream 5'):
        dng.read_dng(str(tmp_path / 'many.dng'), device='cuda')
    check(dng, good, want=img)

    def short_rows(streams):
        streams[1] = streams[1][:-3]
        return streams
    R.write_dng_file(str(tmp_path / 'rows.dng'), img, bits=12, compression=1, tile=(16, 16), mutate=short_rows)
    with pytest.raises(ValueError, match='stream 1'):
        dng.read_dng(str(tmp_path / 'rows.dng'))


def test_converter_command_line(dng, tmp_path, capsys):
    img = R.noisy_ramp(24, 36, 14, seed=3)
    info = R.write_dng_file(str(tmp_path / 'in.dng'), img, bits=14, compression=7, tile=(16, 16), ljpeg=dict(P=14, geometry='nf2'),
                            tags={50714: (R.SHORT, (512,)), 50717: (R.LONG, (16383,)), 51009: (R.UNDEFINED, bytes(8))},
                            tags0={50728: (R.RATIONAL, ((1, 2), (1, 1), (2, 3))), 50721: (R.SRATIONAL, CM)})
    assert dng.main([info['path'], '-o', str(tmp_path / 'frame.npy'), '--meta-out', str(tmp_path / 'sensor.json')]) == 0
    assert np.array_equal(np.load(str(tmp_path / 'frame.npy')), img)
    from eld_amd.denoise import read_sidecar
    side = read_sidecar(str(tmp_path / 'sensor.json'))
    assert side['raw_pattern'] == [[0, 1], [3, 2]] and side['black_level'] == [512] * 4 and side['white_point'] == 16383 and side['wb'] == [2.0, 1.0, 1.5]
    assert 'OpcodeList2 present and not applied' in capsys.readouterr().out


def test_denoise_end_to_end(dng, tmp_path):
    """run_frames with the classical baseline (no checkpoint) on a 48 x 64 Bayer DNG and on the same mosaic as .npy + sidecar: the same
    arrays; --dng writes a file that reads back as the denoised mosaic, with the source's tags"""
    from eld_amd import classical, denoise
    rng = np.random.default_rng(4)
    img = np.clip(rng.normal(900, 40, (48, 64)), 512, 4095).astype(np.uint16)
    info = R.write_dng_file(str(tmp_path / 'f.dng'), img, bits=12, compression=7, tile=(16, 32), ljpeg=dict(P=12, geometry='nf2'),
                            tags={50714: (R.SHORT, (512,)), 50717: (R.LONG, (4095,))},
                            tags0={50728: (R.RATIONAL, ((1, 2), (1, 1), (2, 3))), 50721: (R.SRATIONAL, CM), 50778: (R.SHORT, (21,))})
    meta = dng.dng_meta(info['path'])
    np.save(str(tmp_path / 'g.npy'), img)
    with open(str(tmp_path / 'g.json'), 'w') as fh:
        json.dump({k: meta[k] for k in ('cfa', 'raw_pattern', 'black_level', 'white_point', 'wb', 'ccm')}, fh)
    args = ['--method', 'nlm', '--K', '2.0', '--sigma', '3.0']
    outs = {}
    for name, argv in (('f', [info['path'], '--dng']), ('g', [str(tmp_path / 'g.npy'), '--meta', str(tmp_path / 'g.json'), '--dng'])):
        out = str(tmp_path / ('out_' + name))
        assert classical.main(argv + ['-o', out] + args) == 0
        outs[name] = {k: np.load(os.path.join(out, '%s_%s.npy' % (name, k))) for k in ('denoised', 'srgb')}
        back, m = dng.read_dng(os.path.join(out, name + '_denoised.dng'))
        assert np.array_equal(back, outs[name]['denoised'])
        assert m['raw_pattern'] == meta['raw_pattern'] and m['black_level'] == meta['black_level'] and m['white_point'] == meta['white_point']
        assert m['wb'] == meta['wb']
    assert np.array_equal(outs['f']['denoised'], outs['g']['denoised']) and np.array_equal(outs['f']['srgb'], outs['g']['srgb'])
    assert not np.array_equal(outs['f']['denoised'], img)
    t, _ = dng.parse_tiff(os.path.join(str(tmp_path / 'out_f'), 'f_denoised.dng'))
    assert tuple(t.ifd0[50721].values) == CM                         # like=: the source's rationals
