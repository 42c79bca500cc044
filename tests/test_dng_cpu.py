"""CPU tests of the DNG reader (eld_amd/dng.py, csrc/dng_dev.h): the yardstick tests/dng_ref.py against decoders that are not ours, the
container and metadata rules on written files, every rejection, the argument checks of the two entry points, the per-stream decoder under
AddressSanitizer (tools/dng_hostcheck.cpp, a plain executable), and the command-line precedence.  No device is touched."""
import io
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import dng_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CM = ((8000, 10000), (-2000, 10000), (-500, 10000), (-3000, 10000), (11000, 10000), (2000, 10000), (-500, 10000), (1500, 10000), (6000, 10000))
CM2 = ((7000, 10000), (-1000, 10000), (-400, 10000), (-2500, 10000), (10000, 10000), (2500, 10000), (-300, 10000), (1200, 10000), (5000, 10000))


def D():
    import eld_amd.dng as d
    return d


def small(path, **kw):
    """a 6 x 8 uncompressed 16-bit RGGB file with the given switches of dng_ref.write_dng_file"""
    img = (np.arange(48, dtype=np.uint16) * 97 % 4096).reshape(6, 8)
    return img, R.write_dng_file(str(path), img, **kw)


# ---- the yardstick against decoders that are not ours --------------------------------------------------------------------------------
@pytest.mark.parametrize('nf', [1, 3])
@pytest.mark.parametrize('pred', range(1, 8))
def test_encoder_against_pillow(nf, pred):
    Image = pytest.importorskip('PIL.Image')
    for seed in range(200):                                          # the first noise image whose stream holds an FF byte
        rng = np.random.default_rng(seed)
        img = rng.integers(0, 256, (13, 21, nf)).astype(np.uint8)
        img[0, 0], img[1, 1], img[5:7] = 0, 255, 255
        data, info = R.ljpeg_encode(img.reshape(-1), 8, 21, 13, nf, pred=pred, per_component=(nf == 3))
        if info['stuffed']:
            break
    ent = data[info['header_len']:-2]
    assert b'\xff\x00' in ent and info['stuffed'] >= 1               # the stream holds a stuffed FF
    got = np.asarray(Image.open(io.BytesIO(data))).reshape(13, 21, nf)
    assert np.array_equal(got, img)
    seq, hdr = R.ljpeg_decode(data)
    assert np.array_equal(seq.reshape(13, 21, nf), img) and hdr == {'P': 8, 'X': 21, 'Y': 13, 'Nf': nf, 'pred': pred}


def test_container_parser_reads_a_pillow_tiff(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    from PIL import TiffImagePlugin
    rng = np.random.default_rng(3)
    img = rng.integers(0, 65536, (11, 17)).astype(np.uint16)
    ifd = TiffImagePlugin.ImageFileDirectory_v2()
    ifd[50717] = 16383
    ifd.tagtype[50717] = 4
    ifd[33422] = bytes([0, 1, 1, 2])
    ifd.tagtype[33422] = 1
    ifd[50714] = (TiffImagePlugin.IFDRational(1025, 2),)
    ifd.tagtype[50714] = 5
    p = str(tmp_path / 'pil.tif')
    Image.fromarray(img).save(p, tiffinfo=ifd)
    d = D()
    t, buf = d.parse_tiff(p)
    assert t.ifd0[50717].type == 4 and tuple(t.ifd0[50717].values) == (16383,)
    assert t.ifd0[33422].type == 1 and tuple(t.ifd0[33422].values) == (0, 1, 1, 2)
    assert t.ifd0[50714].type == 5 and tuple(t.ifd0[50714].values) == ((1025, 2),)
    lay = d.image_layout(t, t.ifd0)
    assert (lay.H, lay.W, lay.bits, lay.compression) == (11, 17, 16, 1)
    got = np.zeros((11, 17), dtype=np.uint16)
    for off, n, x0, y0, tw, th in lay.streams:
        got[y0:y0 + th, x0:x0 + tw] = np.frombuffer(buf, dtype=t.order + 'u2', count=tw * th, offset=off).reshape(th, tw)
    assert np.array_equal(got, img)
    with pytest.raises(ValueError, match='PhotometricInterpretation = 32803'):
        d.dng_meta(p)                                               # a grey TIFF is no raw file


@pytest.mark.parametrize('P', [12, 14, 16])
@pytest.mark.parametrize('geometry', ['nf2', 'rowdouble'])
def test_round_trip(P, geometry):
    t = R.noisy_ramp(16, 22, P, seed=P)
    X, Y, Nf = R.tile_sequences(t, geometry)
    assert Nf == 2
    for pred in range(1, 8):
        for per_component, deep in ((False, False), (True, False), (False, True)):
            data, info = R.ljpeg_encode(t.reshape(-1), P, X, Y, Nf, pred=pred, per_component=per_component, deep=deep)
            assert info['max_code_len'] == 16 if deep else info['max_code_len'] <= 16
            seq, _ = R.ljpeg_decode(data)
            assert np.array_equal(seq.reshape(t.shape), t), (P, geometry, pred, per_component, deep)


def test_round_trip_wrap_and_ssss16():
    for a, b in ((0, 32768), (0, 65535)):
        t = R.alternating(6, 10, a, b)
        data, info = R.ljpeg_encode(t.reshape(-1), 16, 10, 6, 1)
        # the first sample 0 against 2^15 is SSSS = 16 in both; 0 <-> 65535 are the differences -1 and +1 modulo 65536 (SSSS = 1)
        assert sorted(info['tables'][0][1]) == ([0, 16] if b == 32768 else [0, 1, 16])      # 0: a row's first sample under its equal
        assert np.array_equal(R.ljpeg_decode(data)[0].reshape(6, 10), t)


@pytest.mark.parametrize('bits', [8, 10, 12, 14, 16])
def test_packed_rows_round_trip(bits):
    t = R.noisy_ramp(5, 13, bits, seed=bits)
    for order in '<>':
        data = R.pack_rows(t, bits, order)
        assert len(data) == 5 * ((13 * bits + 7) // 8)
        assert np.array_equal(R.unpack_rows(data, 5, 13, bits, order), t)
    assert R.pack_rows(np.array([[0x123, 0x3FF]], np.uint16), 10) == bytes([0x48, 0xFF, 0xF0])      # 0100100011 1111111111 0000


# ---- metadata -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cfa,want', [((0, 1, 1, 2), [[0, 1], [3, 2]]), ((1, 0, 2, 1), [[1, 0], [2, 3]]), ((1, 2, 0, 1), [[1, 2], [0, 3]]),
                                      ((2, 1, 1, 0), [[2, 1], [3, 0]])])
def test_bayer_phases(tmp_path, cfa, want):
    small(tmp_path / 'a.dng', cfa=cfa)
    m = D().dng_meta(str(tmp_path / 'a.dng'))
    assert m['cfa'] == 'bayer' and m['raw_pattern'] == want


def test_metadata_mapping(tmp_path):
    d = D()
    p = str(tmp_path / 'a.dng')
    img, _ = small(p, bits=12, order='>', cfa=(1, 0, 2, 1), subifd=True,
                   tags={50713: (R.SHORT, (2, 2)), 50714: (R.RATIONAL, ((512, 1), (1026, 2), (514, 1), (515, 1))), 50717: (R.LONG, (4000,)),
                         50829: (R.LONG, (1, 3, 5, 7)), 51009: (R.UNDEFINED, bytes(8))},
                   tags0={50728: (R.RATIONAL, ((1, 2), (1, 1), (2, 3))), 50721: (R.SRATIONAL, CM2), 50722: (R.SRATIONAL, CM), 50778: (R.SHORT, (17,)),
                          50779: (R.SHORT, (21,)), 271: (R.ASCII, 'Acme'), 272: (R.ASCII, 'Cam 1'), 50727: (R.RATIONAL, ((3, 1), (1, 1), (1, 1)))},
                   exif={34855: (R.SHORT, (800,)), 33434: (R.RATIONAL, ((1, 30),))})
    m = d.dng_meta(p)
    # the pattern is the one of the mosaic returned (relative to the ActiveArea's corner): an odd origin leaves the tag's pattern as it is, and
    # so shifts it against the full frame -- the site (0, 0) of the mosaic is the full frame's (1, 3)
    assert m['raw_pattern'] == [[1, 0], [2, 3]] and m['active_area'] == [1, 3, 5, 7]
    assert m['black_level'] == [513, 512, 514, 515]                 # by rawpy code: R (code 0) sits at (0, 1) of the cell
    assert m['white_point'] == 4000 and m['bits'] == 12 and m['compression'] == 1
    assert m['wb'] == [2.0, 1.0, 1.5]
    want = R.ccm_formula([a / b for a, b in CM])                    # ColorMatrix2: its illuminant is 21
    assert np.allclose(np.asarray(m['ccm']), want, rtol=1e-12, atol=0)
    assert m['iso'] == 800 and m['exposure_time'] == 1 / 30 and m['make'] == 'Acme' and m['model'] == 'Cam 1'
    assert m['opcodes'] == ['OpcodeList2']
    from eld_amd.denoise import SIDECAR_KEYS
    assert all(k in SIDECAR_KEYS for k in ('cfa', 'raw_pattern', 'black_level', 'white_point', 'wb', 'ccm', 'iso'))
    # without illuminant 21: ColorMatrix1; ISO and exposure in IFD0; no neutral -> no wb; defaults
    q = str(tmp_path / 'b.dng')
    small(q, bits=14, compression=1, tags0={50721: (R.SRATIONAL, CM2), 50722: (R.SRATIONAL, CM), 50778: (R.SHORT, (17,)), 50779: (R.SHORT, (23,)),
                                           34855: (R.SHORT, (200,)), 33434: (R.RATIONAL, ((2, 1),))})
    m = d.dng_meta(q)
    assert np.allclose(np.asarray(m['ccm']), R.ccm_formula([a / b for a, b in CM2]), rtol=1e-12, atol=0)
    assert 'wb' not in m and m['iso'] == 200 and m['exposure_time'] == 2.0
    assert m['black_level'] == [0, 0, 0, 0] and m['white_point'] == 16383 and m['active_area'] == [0, 0, 6, 8] and m['opcodes'] == []


def test_xtrans_metadata(tmp_path):
    d = D()
    pat = [0, 2, 1, 2, 0, 1, 1, 1, 0, 1, 1, 2, 1, 1, 2, 1, 1, 0, 2, 0, 1, 0, 2, 1, 1, 1, 2, 1, 1, 0, 1, 1, 0, 1, 1, 2]
    img = np.arange(144, dtype=np.uint16).reshape(12, 12)
    p = str(tmp_path / 'x.dng')
    R.write_dng_file(p, img, cfa=pat, cfa_dim=(6, 6), tags={50713: (R.SHORT, (1, 1)), 50714: (R.SHORT, (1024,))})
    m = d.dng_meta(p)
    assert m['cfa'] == 'xtrans' and m['black_level'] == 1024 and np.asarray(m['raw_pattern']).reshape(-1).tolist() == pat
    R.write_dng_file(p, img, cfa=pat, cfa_dim=(6, 6), tags={50713: (R.SHORT, (1, 2)), 50714: (R.SHORT, (1024, 1023))})
    with pytest.raises(ValueError, match='BlackLevel'):
        d.dng_meta(p)


def test_write_dng_like_and_meta(tmp_path):
    d = D()
    src = str(tmp_path / 'src.dng')
    neutral = ((473, 1000), (1, 1), (640001, 1000000))
    img, _ = small(src, bits=14, cfa=(2, 1, 1, 0), tags={50714: (R.RATIONAL, ((2049, 4),)), 50717: (R.LONG, (16000,))},
                   tags0={50728: (R.RATIONAL, neutral), 50721: (R.SRATIONAL, CM), 50778: (R.SHORT, (21,)), 271: (R.ASCII, 'Acme'), 272: (R.ASCII, 'Cam 1')},
                   exif={34855: (R.SHORT, (1600,)), 33434: (R.RATIONAL, ((10, 300),))})
    out = str(tmp_path / 'like.dng')
    d.write_dng(out, img, like=src)
    t, buf = d.parse_tiff(out)
    assert buf[:2] == b'II' and not t.subifds
    assert tuple(t.ifd0[50728].values) == neutral and tuple(t.ifd0[50721].values) == CM      # the source's rationals, not re-derived ones
    assert tuple(t.ifd0[33434].values) == ((10, 300),) and tuple(t.ifd0[50714].values) == ((2049, 4),)
    a, b = d.dng_meta(src), d.dng_meta(out)
    for k in ('cfa', 'raw_pattern', 'black_level', 'white_point', 'wb', 'ccm', 'iso', 'exposure_time', 'make', 'model'):
        assert a[k] == b[k], k
    assert b['bits'] == 16 and b['compression'] == 1
    lay = d.image_layout(t, t.ifd0)
    got = np.concatenate([np.frombuffer(buf, '<u2', tw * th, off).reshape(th, tw) for off, n, x0, y0, tw, th in lay.streams])
    assert np.array_equal(got, img)
    # from sidecar keys
    meta = {'cfa': 'bayer', 'raw_pattern': [[1, 0], [2, 3]], 'black_level': [512, 513, 514, 515], 'white_point': 4095, 'wb': [2.0, 1.0, 1.5],
            'ccm': [[1.7, -0.5, -0.2], [-0.3, 1.6, -0.3], [0.0, -0.6, 1.6]], 'iso': 100}
    out = str(tmp_path / 'meta.dng')
    d.write_dng(out, img, meta=meta, rows_per_strip=4)
    m = d.dng_meta(out)
    for k in ('raw_pattern', 'black_level', 'white_point', 'wb', 'iso'):
        assert m[k] == meta[k], k
    t, _ = d.parse_tiff(out)
    assert tuple(t.ifd0[50721].values) == tuple(d.color_matrix_from_ccm(meta['ccm'])) and tuple(t.ifd0[50778].values) == (21,)
    assert len(t.ifd0[273].values) == 2
    assert np.allclose(np.asarray(m['ccm']), meta['ccm'], atol=2e-3)       # the rows of this ccm sum to 1; ColorMatrix1 is rounded to 1e-4


# ---- rejections -------------------------------------------------------------------------------------------------------------------
def lj_file(path, **lj):
    img = R.noisy_ramp(8, 8, 12)
    kw = dict(geometry='nf2', P=12)
    kw.update(lj)
    return R.write_dng_file(str(path), img, bits=12, compression=7, tile=(8, 8), ljpeg=kw)


def test_container_rejections(tmp_path):
    d = D()
    p = str(tmp_path / 'r.dng')
    for kw, pat in ((dict(photometric=34892), 'PhotometricInterpretation = 34892'),
                    (dict(tags={259: (R.SHORT, (34892,))}), 'Compression = 34892'),
                    (dict(tags={259: (R.SHORT, (52546,))}), 'Compression = 52546'),
                    (dict(tags={259: (R.SHORT, (8,))}), 'Compression = 8'),
                    (dict(magic=43), 'BigTIFF'),
                    (dict(tags={266: (R.SHORT, (2,))}), 'FillOrder = 2'),
                    (dict(tags={339: (R.SHORT, (3,))}), 'SampleFormat = 3'),
                    (dict(tags={277: (R.SHORT, (3,))}), 'SamplesPerPixel = 3'),
                    (dict(bits=9), 'BitsPerSample = 9'),
                    (dict(cfa_dim=(4, 4), cfa=(0,) * 16), 'CFARepeatPatternDim'),
                    (dict(cfa=(0, 0, 1, 2)), 'CFAPattern'),
                    (dict(tags={50715: (R.RATIONAL, ((0, 1),) * 7 + ((1, 2),))}), 'BlackLevelDeltaH'),
                    (dict(tags={50716: (R.RATIONAL, ((1, 1),) * 6)}), 'BlackLevelDeltaV'),
                    (dict(tags={50829: (R.LONG, (0, 0, 7, 8))}), 'ActiveArea'),
                    (dict(tags={279: (R.LONG, (40,))}), 'stream 0'),
                    (dict(tags={273: (R.LONG, (1 << 20,))}), r'StripOffsets\[0\]')):
        small(p, **kw)
        with pytest.raises(ValueError, match=pat):
            d._plan(p)
    small(p, tags={50715: (R.RATIONAL, ((0, 1),) * 8)})             # an all-zero delta is accepted
    d._plan(p)


def test_ljpeg_prelaunch_rejections(tmp_path):
    d = D()
    p = str(tmp_path / 'j.dng')
    lj_file(p)
    d._plan(p)
    for lj, pat in ((dict(restart_interval=8), r'restart interval \(DRI\)'), (dict(point_transform=1), 'point transform 1'),
                    (dict(scans=1), 'more than one scan')):
        lj_file(p, **lj)
        with pytest.raises(ValueError, match='stream 0.*' + pat):
            d._plan(p)

    def other_geometry(streams):                                    # a JPEG of 8 x 10 samples in an 8 x 8 tile
        t = R.noisy_ramp(10, 8, 12)
        return [R.ljpeg_encode(t.reshape(-1), 12, 4, 10, 2)[0]]
    R.write_dng_file(p, R.noisy_ramp(8, 8, 12), bits=12, compression=7, tile=(8, 8), ljpeg=dict(geometry='nf2', P=12), mutate=other_geometry)
    with pytest.raises(ValueError, match='stream 0.*10 x 4 x 2 samples'):
        d._plan(p)

    def lossy(streams):
        return [streams[0].replace(b'\xff\xc3', b'\xff\xc0', 1)]
    R.write_dng_file(p, R.noisy_ramp(8, 8, 12), bits=12, compression=7, tile=(8, 8), ljpeg=dict(geometry='nf2', P=12), mutate=lossy)
    with pytest.raises(ValueError, match='FFC0'):
        d._plan(p)


# ---- the two entry points ----------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_without_a_device(eld_lib):
    one = 16                                                        # any non-null address: nothing is dereferenced before the checks
    u = eld_lib.eld_dng_unpack_u16
    good = [one, 64, one, 1, 12, 0, 8, 8, 0, 0, 8, 8, None, 0, one, one, None]

    def bad(fn, args, **ch):
        a = list(args)
        for i, v in ch.items():
            a[int(i[1:])] = v
        return fn(*a)
    assert bad(u, good, _3=0) == 0                                  # no streams: a no-op
    for ch in (dict(_0=None), dict(_2=None), dict(_14=None), dict(_15=None), dict(_3=-1), dict(_4=9), dict(_4=0), dict(_6=0), dict(_7=-1),
               dict(_8=-1), dict(_9=-1), dict(_10=9), dict(_11=9), dict(_8=1), dict(_9=1), dict(_13=5), dict(_13=-1), dict(_13=65537),
               dict(_14=17), dict(_2=18), dict(_15=18), dict(_6=1 << 16, _7=1 << 16)):
        assert bad(u, good, **ch) == -1, ch
    j = eld_lib.eld_dng_ljpeg_u16
    good = [one, 64, one, 1, one, 1, 8, 8, 0, 0, 8, 8, None, 0, None, 0, 0, one, one, None]
    assert bad(j, good, _3=0) == 0
    for ch in (dict(_0=None), dict(_2=None), dict(_4=None), dict(_5=0), dict(_5=-1), dict(_17=None), dict(_18=None), dict(_16=65), dict(_16=-1),
               dict(_15=4), dict(_14=17), dict(_10=9), dict(_9=1), dict(_13=3), dict(_4=18), dict(_3=-1)):
        assert bad(j, good, **ch) == -1, ch


# ---- the per-stream decoder under AddressSanitizer ---------------------------------------------------------------------------------
def hostcheck_cases():
    """(record, tables, entropy bytes, expected tile) of a handful of streams, through the package's own host-side parser"""
    d = D()
    from eld_amd import _lib as L
    cases = []
    for P, geometry, pred, per_component, deep, content in ((12, 'nf2', 1, False, False, 'ramp'), (16, 'nf1', 7, False, True, 'ramp'),
                                                            (14, 'rowdouble', 4, True, False, 'ramp'), (16, 'nf2', 6, True, False, 'ramp'),
                                                            (16, 'nf1', 1, False, False, 'ssss16'), (16, 'nf2', 5, False, False, 'wrap'),
                                                            (8, 'nf1', 2, False, False, 'ramp'), (12, 'nf2', 3, False, False, 'ramp')):
        t = {'ramp': R.noisy_ramp(12, 14, P, seed=pred), 'ssss16': R.alternating(12, 14, 0, 32768), 'wrap': R.alternating(12, 14, 0, 65535)}[content]
        X, Y, Nf = R.tile_sequences(t, geometry)
        data, _ = R.ljpeg_encode(t.reshape(-1), P, X, Y, Nf, pred=pred, per_component=per_component, deep=deep)
        j = d.parse_ljpeg(data, 0, len(data), 'case')
        rec = np.zeros((), dtype=L.DNG_STREAM_DTYPE)
        rec['tw'], rec['th'], rec['P'], rec['X'], rec['Y'], rec['Nf'], rec['pred'] = 14, 12, j['P'], j['X'], j['Y'], j['Nf'], j['pred']
        tabs = []
        for k, (counts, syms) in enumerate(j['tables']):
            rec['table'][k] = len(tabs)
            tabs.append(d.huff_record(counts, syms, 'case'))
        ent = data[j['data'][0]:j['data'][0] + j['data'][1]]
        cases.append((rec, tabs, ent, t))
    return cases


def test_stream_decoder_under_address_sanitizer(tmp_path):
    cxx = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'dng_hostcheck')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
                           os.path.join(ROOT, 'tools', 'dng_hostcheck.cpp')])
    cases = hostcheck_cases()
    blob = struct.pack('<I', len(cases))
    for rec, tabs, ent, t in cases:
        blob += rec.tobytes() + struct.pack('<I', len(tabs)) + b''.join(x.tobytes() for x in tabs) + struct.pack('<I', len(ent)) + ent
        blob += struct.pack('<I', t.size) + t.astype('<u2').tobytes()
    path = str(tmp_path / 'cases.bin')
    with open(path, 'wb') as fh:
        fh.write(blob)
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and 'hostcheck OK' in r.stdout, r.stdout


# ---- command line -------------------------------------------------------------------------------------------------------------------
def test_denoise_options_precedence(tmp_path):
    from eld_amd import denoise
    p = str(tmp_path / 'in.DNG')
    small(p, cfa=(1, 0, 2, 1), tags={50714: (R.SHORT, (256,)), 50717: (R.LONG, (4000,))},
          tags0={50728: (R.RATIONAL, ((1, 2), (1, 1), (2, 3))), 50721: (R.SRATIONAL, CM), 34855: (R.SHORT, (800,))})
    inputs, out, ckpt, o = denoise.parse_args([p, '-o', str(tmp_path), '--ckpt', 'x.pt'])
    assert inputs == [p] and o['cfa'] == 'bayer' and o['raw_pattern'] == [[1, 0], [2, 3]] and o['black_level'] == [256.0] * 4 and o['white_point'] == 4000
    assert o['wb'] == [2.0, 1.0, 1.5] and np.allclose(o['ccm'], R.ccm_formula([a / b for a, b in CM]), rtol=1e-12) and 'iso' not in o and 'dng' not in o
    side = str(tmp_path / 's.json')
    with open(side, 'w') as fh:
        json.dump({'white_point': 3000, 'black_level': 300, 'shading': 'map.npz'}, fh)
    o = denoise.parse_args([p, '-o', str(tmp_path), '--ckpt', 'x.pt', '--meta', side, '--black', '200', '--dng'])[3]
    assert o['black_level'] == 200.0 and o['white_point'] == 3000 and o['raw_pattern'] == [[1, 0], [2, 3]]      # command line > sidecar > tags
    assert o['iso'] == 800 and o['dng'] is True                     # the tags' ISO fills --iso for --shading
    o = denoise.parse_args([p, '-o', str(tmp_path), '--ckpt', 'x.pt', '--meta', side, '--iso', '400'])[3]
    assert o['iso'] == 400
    q = str(tmp_path / 'other.dng')
    small(q, cfa=(1, 0, 2, 1), tags={50714: (R.SHORT, (256,)), 50717: (R.LONG, (4001,))})
    with pytest.raises(ValueError, match='other.dng.*white_point'):
        denoise.parse_args([p, q, '-o', str(tmp_path), '--ckpt', 'x.pt'])
    o = denoise.parse_args([str(tmp_path / 'a.npy'), '-o', str(tmp_path), '--ckpt', 'x.pt'])[3]      # .npy inputs: today's defaults
    assert o.get('raw_pattern') is None and o['white_point'] == 16383 and o.get('wb') is None


def test_manifest_takes_its_levels_from_the_first_dng(tmp_path, monkeypatch):
    d = D()
    from eld_amd import calibrate
    img, _ = small(tmp_path / 'b0.dng', cfa=(1, 0, 2, 1), tags={50714: (R.SHORT, (256,)), 50717: (R.LONG, (4000,))})
    monkeypatch.setattr(d, 'read_dng', lambda path, device=None: (img.copy(), d.dng_meta(path)))      # the pixels are the GPU tests' business
    np.save(str(tmp_path / 'f0.npy'), img)
    man = {'sessions': [{'iso': 100, 'bias': ['b0.dng', 'b0.dng'], 'flats': [['f0.npy', 'b0.dng']]}]}
    with open(str(tmp_path / 'm.json'), 'w') as fh:
        json.dump(man, fh)
    sessions, pat, black, white, cfa = calibrate.load_manifest(str(tmp_path / 'm.json'), with_cfa=True)
    assert (pat, black, white, cfa) == ([[1, 0], [2, 3]], [256] * 4, 4000, 'bayer') and sessions[0]['bias'].shape == (2, 6, 8)
    with open(str(tmp_path / 'm.json'), 'w') as fh:
        json.dump(dict(man, raw_pattern=[[0, 1], [3, 2]], black_level=512, white_level=16383), fh)
    assert calibrate.load_manifest(str(tmp_path / 'm.json'))[1:] == ([[0, 1], [3, 2]], 512, 16383)       # a manifest that names them: as before
    assert d.load_frame(str(tmp_path / 'f0.npy')).dtype == np.uint16
