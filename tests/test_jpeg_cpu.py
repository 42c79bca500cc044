"""CPU tests of the baseline-JPEG writer (eld_amd/jpeg.py, csrc/jpeg_dev.h): the yardstick tests/jpeg_ref.py against the
coefficients of Pillow-written files (every block, dummy ones included) and against Pillow's decode; the yardstick's own decoder; the
per-block routines of the kernels under AddressSanitizer and UBSan (tools/jpeg_hostcheck.cpp, a plain executable) against the yardstick;
write_dng's preview IFD on the host path; the argument checks of encode_jpeg and of the three entry points.  No device is touched."""
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.cases()
QUALITIES = {'noise_37x53_420': (50, 100), 'smooth_9x70_444': (50, 100)}      # beside the case's own quality


def J():
    import eld_amd.jpeg as j
    return j


def pil():
    return pytest.importorskip('PIL.Image')


def pillow_file(rgb, quality, sub):
    buf = io.BytesIO()
    pil().fromarray(rgb).save(buf, 'JPEG', quality=quality, subsampling=R.SUBSAMPLING[sub])
    return buf.getvalue()


_encoded = {}


def encoded(case):
    """the yardstick's file and what it recorded, computed once per case"""
    if case.name not in _encoded:
        _encoded[case.name] = case.encode()
    return _encoded[case.name]


def settings():
    for c in CASES:
        for q in (c.quality,) + QUALITIES.get(c.name, ()):
            yield pytest.param(c, q, id='%s-q%d' % (c.name, q))


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_case_keeps_its_point(case):
    case.check(encoded(case)[1])


@pytest.mark.parametrize('case,quality', list(settings()))
def test_reference_coefficients_equal_pillows(case, quality):
    d = R.decode(pillow_file(case.rgb, quality, case.subsampling))
    want = R.coefficients(case.rgb, quality, case.subsampling)
    assert (d['H'], d['W'], d['subsampling']) == (case.rgb.shape[0], case.rgb.shape[1], case.subsampling)
    assert d['coef'].shape == want.shape and np.array_equal(d['coef'], want)


@pytest.mark.parametrize('case,quality', list(settings()))
def test_pillow_decodes_the_reference_file_like_its_own(case, quality):
    Image = pil()
    mine = R.encode(case.rgb, quality, case.subsampling)
    theirs = pillow_file(case.rgb, quality, case.subsampling)
    a, b = Image.open(io.BytesIO(mine)), Image.open(io.BytesIO(theirs))
    assert a.quantization == b.quantization
    ql, qc = R.quant_tables(quality)
    assert {k: list(v) for k, v in R.decode(theirs)['qtables'].items()} == {0: ql, 1: qc} == {0: J().quant_tables(quality)[0], 1: J().quant_tables(quality)[1]}
    assert a.size == b.size and np.array_equal(np.asarray(a.convert('RGB')), np.asarray(b.convert('RGB')))


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_reference_decoder_reads_the_reference_file(case):
    data, info = encoded(case)
    d = R.decode(data)
    assert np.array_equal(d['coef'], info['coef']) and d['pad_ok'] and d['end'] == len(data)
    assert d['markers'] == ['SOI', 'APP0', 'DQT', 'DQT', 'SOF0', 'DHT', 'DHT', 'DHT', 'DHT', 'SOS', 'EOI']
    assert [c[0] for c in d['comps']] == [1, 2, 3] and sorted(d['tables']) == [0x00, 0x01, 0x10, 0x11]
    assert J().jpeg_info(data) == dict(width=case.rgb.shape[1], height=case.rgb.shape[0], subsampling=(2, 2) if case.subsampling == '420' else (1, 1))


def test_package_tables_and_header_equal_the_references():
    """the host half of encode_jpeg without a device: K.2 tables from the reference's histograms, the markers from those"""
    from eld_amd import dng
    j = J()
    for case in CASES:
        data, info = encoded(case)
        dht = [dng.huffman_lengths(h, len(h)) for h in info['hist']]
        assert [(list(c), list(s)) for c, s in dht] == [(list(c), list(s)) for c, s in info['tables']]
        for (c, s), h in zip(dht, info['hist']):
            tab = dng.encoder_table(c, s, len(h))
            assert {k: (int(tab[k]) & 0xFFFF, int(tab[k]) >> 16) for k in range(len(h)) if tab[k]} == R.canonical(c, s)
        hd = j.header(case.rgb.shape[0], case.rgb.shape[1], case.subsampling, j.quant_tables(case.quality), dht)
        assert data.startswith(hd) and data[len(hd) - 14:len(hd) - 12] == b'\xff\xda'


# ---- the per-block routines under AddressSanitizer and UBSan --------------------------------------------------------------------------------
def table_words(info):
    """ELD_JPEG_TABLE uint32 in the library's layout, from the reference's four tables (DC0, AC0, DC1, AC1)"""
    tab = np.zeros(546, dtype='<u4')
    for (bits, vals), base in zip(info['tables'], (0, 34, 17, 290)):
        for s, (code, length) in R.canonical(bits, vals).items():
            tab[base + s] = (length << 16) | code
    return tab


def hist_words(info):
    dc0, ac0, dc1, ac1 = info['hist']
    return np.array(dc0 + dc1 + ac0 + ac1, dtype=np.uint32)


def scan_bytes(data):
    """the entropy-coded bytes of a file, stuffing removed"""
    sos = data.index(b'\xff\xda')
    n, = struct.unpack_from('>H', data, sos + 2)
    return data[sos + 2 + n:-2].replace(b'\xff\x00', b'\xff')


def test_block_routines_under_sanitizers(tmp_path):
    cxx = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'jpeg_hostcheck')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
                           os.path.join(ROOT, 'tools', 'jpeg_hostcheck.cpp')])
    blob, want = b'', []
    for case in CASES:
        data, info = encoded(case)
        ql, qc = R.quant_tables(case.quality)
        for segment in (R.MIN_SEGMENT, 256):                         # a lane per block with many boundaries; the default
            H, W = case.rgb.shape[:2]
            blob += struct.pack('<4I', H, W, R.SUBSAMPLING[case.subsampling], segment) + np.array(ql + qc, dtype='<u2').tobytes()
            blob += table_words(info).tobytes() + np.ascontiguousarray(case.rgb.transpose(2, 0, 1)).tobytes()
            want.append((case.name, segment, info['coef'], hist_words(info), scan_bytes(data)))
    for case in CASES:                                               # once more with 16-bit codes: a DC word of 27 bits, an AC word of 26
        if case.name in ('dc_size_11', 'ac_size_10'):
            info = {}
            data = R.encode(case.rgb, case.quality, case.subsampling, info, deep=True)
            assert R.decode(data)['coef'].tobytes() == info['coef'].tobytes()
            ql, qc = R.quant_tables(case.quality)
            blob += struct.pack('<4I', case.rgb.shape[0], case.rgb.shape[1], R.SUBSAMPLING[case.subsampling], R.MIN_SEGMENT)
            blob += np.array(ql + qc, dtype='<u2').tobytes() + table_words(info).tobytes() + np.ascontiguousarray(case.rgb.transpose(2, 0, 1)).tobytes()
            want.append((case.name + '_deep', R.MIN_SEGMENT, info['coef'], hist_words(info), scan_bytes(data)))
    cases, out = str(tmp_path / 'cases.bin'), str(tmp_path / 'out.bin')
    with open(cases, 'wb') as fh:
        fh.write(struct.pack('<I', len(want)) + blob)
    r = subprocess.run([exe, cases, out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and 'hostcheck OK' in r.stdout, r.stdout
    assert 'coverage: longest DC word 27 bits, longest AC word 26 bits, 32 of 32 start phases' in r.stdout, r.stdout
    got = open(out, 'rb').read()
    pos = 0
    for name, segment, coef, hist, ent in want:
        nb, = struct.unpack_from('<I', got, pos)
        assert nb == coef.shape[0], (name, segment)
        c = np.frombuffer(got, dtype='<i2', count=nb * 64, offset=pos + 4).reshape(nb, 64)
        assert np.array_equal(c, coef), (name, segment, np.flatnonzero((c != coef).any(axis=1))[:8])
        pos += 4 + nb * 128
        assert np.array_equal(np.frombuffer(got, dtype='<u4', count=536, offset=pos), hist), (name, segment)
        pos += 536 * 4
        n, = struct.unpack_from('<I', got, pos)
        assert got[pos + 4:pos + 4 + n] == ent, (name, segment)
        pos += 4 + n
    assert pos == len(got)


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------
def no_device(monkeypatch):
    """any use of the library from here on is an error"""
    from eld_amd import _lib as L

    def boom(*a, **k):
        raise AssertionError('device work before the arguments were checked')
    monkeypatch.setattr(L, 'lib', boom)


@pytest.mark.parametrize('kw,word', [(dict(quality=0), 'quality'), (dict(quality=101), 'quality'), (dict(quality=90.5), 'quality'),
                                     (dict(subsampling='422'), 'subsampling'), (dict(subsampling=1), 'subsampling'), (dict(segment=4), 'segment'),
                                     (dict(segment=12), 'segment'), (dict(segment=4096), 'segment'), (dict(chunk=8), 'chunk'), (dict(chunk=8192), 'chunk')])
def test_encode_jpeg_names_a_bad_argument_before_device_work(monkeypatch, kw, word):
    no_device(monkeypatch)
    with pytest.raises(ValueError, match=word) as e:
        J().encode_jpeg(R.smooth(8, 8), **kw)
    assert repr(list(kw.values())[0]) in str(e.value) or str(list(kw.values())[0]) in str(e.value)


@pytest.mark.parametrize('rgb', [np.zeros((8, 8, 3), np.float32), np.zeros((8, 8, 3), np.uint16), np.zeros((8, 8), np.uint8), np.zeros((8, 8, 4), np.uint8),
                                 np.zeros((0, 8, 3), np.uint8), np.zeros((2, 4, 8, 8), np.uint8), [[1, 2, 3]]], ids=lambda a: str(getattr(a, 'shape', 'list')))
def test_encode_jpeg_refuses_other_pictures_before_device_work(monkeypatch, rgb):
    no_device(monkeypatch)
    with pytest.raises(ValueError, match='rgb'):
        J().encode_jpeg(rgb)


def test_jpeg_info_refuses_what_is_no_baseline_jpeg():
    Image = pil()
    j = J()
    buf = io.BytesIO()
    Image.fromarray(R.smooth(16, 16)).save(buf, 'JPEG', progressive=True)
    grey = io.BytesIO()
    Image.fromarray(R.smooth(16, 16)[..., 0]).save(grey, 'JPEG')
    for bad in (b'', b'II*\0', buf.getvalue(), grey.getvalue(), b'\xff\xd8\xff\xd9', 'text'):
        with pytest.raises(ValueError, match='JPEG'):
            j.jpeg_info(bad)


def test_entry_points_refuse_bad_arguments(eld_lib):
    """status -1 before any launch: no device is needed to be told so"""
    buf = np.zeros(1 << 16, dtype=np.uint64)
    p = buf.ctypes.data
    p += -p % 16
    q = np.array(sum(R.quant_tables(90), []), dtype=np.uint16)
    good = dict(H=16, W=16, sub=2, segment=0)

    def coef(**ch):
        a = dict(good, **ch)
        nb = a.get('elems', 6 * 64 * (-(-a['H'] // 16)) * (-(-a['W'] // 16)))
        return eld_lib.eld_jpeg_coef_u8(a.get('rgb', p), a['H'], a['W'], a['sub'], a.get('q', q).ctypes.data if a.get('q', q) is not None else None,
                                        a.get('coef', p), nb, None)

    def hist(**ch):
        a = dict(good, **ch)
        return eld_lib.eld_jpeg_hist_i16(a.get('coef', p), a.get('elems', 384), a['H'], a['W'], a['sub'], a['segment'], a.get('hist', p),
                                         a.get('hist_elems', 536), None)

    def pack(**ch):
        a = dict(good, **ch)
        return eld_lib.eld_jpeg_pack_i16(a.get('coef', p), a.get('elems', 384), a['H'], a['W'], a['sub'], a['segment'], a.get('tables', p),
                                         a.get('seg_bit', p), a.get('raw', p), a.get('raw_dwords', 16), a.get('lds', -1), None)
    for ch in (dict(H=0), dict(W=0), dict(H=65536), dict(W=65536), dict(H=65535, W=65535), dict(sub=1), dict(sub=3), dict(sub=-1), dict(elems=383),
               dict(elems=385), dict(coef=None), dict(coef=p + 2), dict(coef=p + 8)):
        assert coef(**ch) == -1, ch
        assert hist(**ch) == -1, ch
        assert pack(**ch) == -1, ch
    for seg in (4, 12, 2056, 4096, -8):
        assert hist(segment=seg) == -1 and pack(segment=seg) == -1, seg
    zero, big = q.copy(), q.copy()
    zero[70], big[3] = 0, 256
    assert coef(rgb=None) == -1 and coef(q=None) == -1 and coef(q=zero) == -1 and coef(q=big) == -1
    assert hist(hist=None) == -1 and hist(hist=p + 2) == -1 and hist(hist_elems=535) == -1 and hist(hist_elems=1072) == -1
    assert pack(tables=None) == -1 and pack(seg_bit=None) == -1 and pack(raw=None) == -1 and pack(raw_dwords=0) == -1
    assert pack(tables=p + 2) == -1 and pack(seg_bit=p + 4) == -1 and pack(raw=p + 1) == -1 and pack(lds=61441) == -1


# ---- the preview IFD of write_dng ------------------------------------------------------------------------------------------------------------
def test_write_dng_preview_on_the_host_path(tmp_path):
    Image = pil()
    from eld_amd import dng as d
    from eld_amd import dng_opcodes as O
    import dng_ref
    img = dng_ref.noisy_ramp(37, 50, 14, seed=2)
    meta = dict(cfa='bayer', raw_pattern=[[0, 1], [3, 2]], black_level=[512, 512, 512, 512], white_point=16383, wb=[2.0, 1.0, 1.5], iso=800,
                make='Maker', model='Model X')
    ops = {'OpcodeList2': struct.pack('>I', 0), 'OpcodeList3': struct.pack('>I', 0)}
    plain, with_preview, again = (str(tmp_path / n) for n in ('a.dng', 'b.dng', 'c.dng'))
    d.write_dng(plain, img, meta=meta, opcodes=ops)
    d.write_dng(again, img, meta=meta, opcodes=ops, preview=None)
    assert open(plain, 'rb').read() == open(again, 'rb').read()     # preview=None: the bytes of before
    for sub, factors in (('420', (2, 2)), ('444', (1, 1))):
        rgb = R.smooth(19, 25, 5)
        jpg = R.encode(rgb, 90, sub)
        d.write_dng(with_preview, img, meta=meta, opcodes=ops, preview=jpg)
        t, buf = d.parse_tiff(with_preview)
        i0 = t.ifd0
        one = lambda ifd, tag: d._get1(ifd, tag)
        assert one(i0, d.T_NEWSUBFILETYPE) == 1 and one(i0, d.T_COMPRESSION) == 7 and one(i0, d.T_PHOTOMETRIC) == 6 and one(i0, d.T_SPP) == 3
        assert tuple(i0[d.T_BITS].values) == (8, 8, 8) and (one(i0, d.T_WIDTH), one(i0, d.T_LENGTH)) == (25, 19)
        assert tuple(i0[d.T_YCBCRSUBSAMPLING].values) == factors and one(i0, d.T_ROWSPERSTRIP) == 19
        off, n = one(i0, d.T_STRIPOFFSETS), one(i0, d.T_STRIPBYTECOUNTS)
        assert n == len(jpg) and buf[off:off + n] == jpg
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(bytes(buf[off:off + n]))).convert('RGB')), np.asarray(Image.open(io.BytesIO(jpg)).convert('RGB')))
        for tag in (d.T_DNGVERSION, d.T_DNGBACKWARD, d.T_UNIQUEMODEL, d.T_MAKE, d.T_MODEL, d.T_ASSHOTNEUTRAL, d.T_ISO, d.T_SUBIFDS):
            assert tag in i0, tag
        assert len(t.subifds) == 1
        raw = t.subifds[0]
        assert raw is d._raw_ifd(t) and one(raw, d.T_NEWSUBFILETYPE) == 0 and one(raw, d.T_PHOTOMETRIC) == d.CFA_PHOTOMETRIC
        for tag in (d.T_CFADIM, d.T_CFAPATTERN, d.T_BLACK, d.T_WHITE) + tuple(tg for tg, _ in d.OPCODE_TAGS if tg != d.OPCODE_TAGS[0][0]):
            assert tag in raw and tag not in i0, tag
        lay = d.image_layout(t, raw)                                 # the strips read_dng would upload (it decodes on the device)
        assert (lay.H, lay.W, lay.compression, lay.bits) == (37, 50, 1, 16)
        assert b''.join(bytes(buf[o:o + n]) for o, n, *_ in lay.streams) == img.astype('<u2').tobytes()
        assert d.dng_meta(with_preview) == d.dng_meta(plain)
        assert O.read_opcodes(with_preview).raw == O.read_opcodes(plain).raw == ops
    for bad in (b'', b'not a jpeg', 12):
        with pytest.raises(ValueError, match='preview'):
            d.write_dng(with_preview, img, meta=meta, preview=bad)
