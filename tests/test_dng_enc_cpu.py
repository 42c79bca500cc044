"""CPU tests of the lossless-JPEG DNG writer (eld_amd/dng.py, csrc/dng_enc_dev.h): the package's Huffman table builder against the
yardstick's (tests/dng_ref.py code_lengths), the argument checks of write_dng / encode_ljpeg and of the four entry points, the unchanged
compression-1 bytes, and the per-lane routines of the kernels under AddressSanitizer and UBSan (tools/dng_enc_hostcheck.cpp, a plain
executable) against dng_ref.ljpeg_encode, byte for byte.  No device is touched."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import dng_enc_cases as C
import dng_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def D():
    import eld_amd.dng as d
    return d


def fibonacci(n=17):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f


# ---- the table builder --------------------------------------------------------------------------------------------------------------------
def same_table(hist):
    bits, vals = D().huffman_lengths(hist)
    rbits, rvals = R.code_lengths(hist)
    assert list(bits) == list(rbits) and list(vals) == list(rvals), (list(hist), bits, vals, rbits, rvals)
    return rbits


def test_table_single_bins():
    for s in range(17):
        for n in (1, 7, 65536):
            h = [0] * 17
            h[s] = n
            assert same_table(h)[0] == 1                             # one symbol: the 1-bit code 0, the all-ones code stays free


def test_table_random_histograms():
    rng = np.random.default_rng(2018)
    for i in range(200):
        h = rng.integers(1, [10, 1000, 1 << 20][i % 3], size=17) * (rng.random(17) < rng.uniform(0.2, 1.0))
        if not h.any():
            h[int(rng.integers(0, 17))] = 1
        same_table(h)


def test_table_of_the_gpu_cases():
    n = 0
    for name, (img, tile, bits, _) in C.gpu_cases().items():
        for t in C.tiles_of(img, tile):
            same_table(C.ssss_hist(t, bits))
            n += 1
    assert n == 12 + 9 + 4


def test_table_fibonacci_runs_the_length_limit():
    """Fibonacci counts with the largest on symbol 0: the unlimited code is 17 deep, so Figure K.3 runs.  (With the counts rising over the
    symbols the tie rule -- the larger index wins -- pairs equal sums and the code is 10 deep at most: that order is compared too, but it
    does not reach the limiting step.)"""
    fall = fibonacci()[::-1]
    assert R.code_lengths(fall)[0][15] >= 1                          # the reference's table has a 16-bit code
    assert same_table(fall)[15] >= 1
    same_table(fibonacci())
    tab = D().encoder_table(*D().huffman_lengths(fall))
    want = R.canonical_codes(*R.code_lengths(fall))
    assert {s: (int(tab[s]) & 0xFFFF, int(tab[s]) >> 16) for s in range(17)} == want


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------
def no_device(monkeypatch):
    """any use of the library or of a CUDA device from here on is an error"""
    from eld_amd import _lib as L

    def boom(*a, **k):
        raise AssertionError('device work before the arguments were checked')
    monkeypatch.setattr(L, 'lib', boom)


@pytest.mark.parametrize('kw', [dict(tile=(24, 16)), dict(tile=(16, 24)), dict(tile=(16, 15)), dict(tile=(16, 17)), dict(tile=(0, 16)), dict(bits=7),
                                dict(bits=17)])
def test_bad_tile_and_bits_raise_before_device_work(tmp_path, monkeypatch, kw):
    d = D()
    no_device(monkeypatch)
    img = R.noisy_ramp(16, 32, 12)
    with pytest.raises(ValueError):
        d.encode_ljpeg(img, **kw)
    with pytest.raises(ValueError):
        d.write_dng(str(tmp_path / 'x.dng'), img, compression=7, **kw)
    assert not (tmp_path / 'x.dng').exists()


def test_bad_compression_segment_and_chunk(tmp_path, monkeypatch):
    d = D()
    no_device(monkeypatch)
    img = R.noisy_ramp(16, 32, 12)
    p = str(tmp_path / 'x.dng')
    with pytest.raises(ValueError, match='compression'):
        d.write_dng(p, img, compression=8)
    with pytest.raises(ValueError, match='rows_per_strip'):
        d.write_dng(p, img, compression=7, rows_per_strip=4)
    with pytest.raises(ValueError):
        d.write_dng(p, img, tile=(16, 16))                           # tile and bits belong to compression 7
    with pytest.raises(ValueError):
        d.write_dng(p, img.astype(np.float32), compression=7)
    for kw in (dict(segment=32), dict(segment=100), dict(segment=8256), dict(chunk=8), dict(chunk=24), dict(chunk=8192)):
        with pytest.raises(ValueError):
            d.encode_ljpeg(img, **kw)
    assert not os.path.exists(p)


def test_entry_points_refuse_bad_arguments(eld_lib):
    """status -1 before any launch: no device is needed to be told so"""
    buf = np.zeros(4096, dtype=np.uint32)
    p = buf.ctypes.data
    good = dict(H=32, W=32, th=16, tw=16, bits=14, segment=0)

    def hist(**ch):
        a = dict(good, **ch)
        return eld_lib.eld_dng_enc_hist_u16(a.get('mos', p), a['H'], a['W'], a['th'], a['tw'], a['bits'], a['segment'], a.get('hist', p), p, None)

    def pack(**ch):
        a = dict(good, **ch)
        return eld_lib.eld_dng_enc_pack_u16(p, a['H'], a['W'], a['th'], a['tw'], a['bits'], a['segment'], a.get('tables', p), p, p, p, a.get('raw_dwords', 16), None)
    for ch in (dict(tw=15), dict(tw=17), dict(tw=24), dict(th=24), dict(th=0), dict(bits=7), dict(bits=17), dict(segment=32), dict(segment=100),
               dict(segment=8256), dict(segment=-64), dict(H=0), dict(W=0), dict(H=65536, W=65536), dict(th=8192, tw=4096)):
        assert hist(**ch) == -1, ch
        assert pack(**ch) == -1, ch
    assert hist(mos=None) == -1 and hist(hist=None) == -1 and hist(mos=p + 1) == -1 and hist(hist=p + 2) == -1
    assert pack(tables=None) == -1 and pack(raw_dwords=0) == -1
    assert hist(H=16 * 300, W=16 * 300) == -1                        # more than 65535 tiles
    for chunk in (8, 24, 8192, -16):
        assert eld_lib.eld_dng_enc_ffcount_u8(p, 64, p, 1, chunk, p, None) == -1
        assert eld_lib.eld_dng_enc_stuff_u8(p, 64, p, 1, chunk, p, p, 64, None) == -1
    assert eld_lib.eld_dng_enc_ffcount_u8(None, 64, p, 1, 0, p, None) == -1
    assert eld_lib.eld_dng_enc_ffcount_u8(p, 64, p, -1, 0, p, None) == -1
    assert eld_lib.eld_dng_enc_ffcount_u8(p, 64, p, 1, 0, None, None) == -1
    assert eld_lib.eld_dng_enc_stuff_u8(p, 64, p, 1, 0, p, None, 64, None) == -1
    assert eld_lib.eld_dng_enc_stuff_u8(p, 64, p, 1, 0, p, p + 1, 64, None) == -1
    assert eld_lib.eld_dng_enc_ffcount_u8(None, 0, None, 0, 0, None, None) == 0         # no chunks: a no-op
    assert eld_lib.eld_dng_enc_stuff_u8(None, 0, None, 0, 0, None, None, 0, None) == 0


def test_compression_1_is_unchanged(tmp_path):
    """the bytes of an uncompressed file do not depend on the new arguments being named"""
    d = D()
    img = R.noisy_ramp(37, 50, 14, seed=2)
    meta = dict(cfa='bayer', raw_pattern=[[0, 1], [3, 2]], black_level=[512, 512, 512, 512], white_point=16383, wb=[2.0, 1.0, 1.5], iso=800)
    a, b, c = (str(tmp_path / n) for n in ('a.dng', 'b.dng', 'c.dng'))
    d.write_dng(a, img, meta=meta)
    d.write_dng(b, img, meta=meta, compression=1, tile=None, bits=None)
    d.write_dng(c, img, meta, None, 5)                               # the positional order of before
    d.write_dng(str(tmp_path / 'e.dng'), img, meta=meta, rows_per_strip=5, compression=1)
    assert open(a, 'rb').read() == open(b, 'rb').read()
    assert open(c, 'rb').read() == open(str(tmp_path / 'e.dng'), 'rb').read()
    t, buf = d.parse_tiff(a)
    lay = d.image_layout(t, d._raw_ifd(t))
    assert lay.compression == 1 and lay.bits == 16 and d.T_TILEOFFSETS not in t.ifd0
    o, n = lay.streams[0][0], sum(s[1] for s in lay.streams)
    assert buf[o:o + n] == img.astype('<u2').tobytes() and o + n == len(buf)


# ---- the per-lane routines under AddressSanitizer and UBSan --------------------------------------------------------------------------------
def table_words(bits, vals):
    tab = np.zeros(17, dtype='<u4')
    for s, (code, length) in R.canonical_codes(bits, vals).items():
        tab[s] = (length << 16) | code
    return tab


def hostcheck_cases():
    """(tile, P, deep): the five tiles of the issue with the table of Annex K.2, and the walk once more with the reference's deep table, in
    which category 15 has a 16-bit code: a sample of 31 bits"""
    return [('flat', C.flat(16, 16), 16, False), ('walk', C.walk(16, 16), 16, False), ('ramp255', C.ramp255(16, 16), 16, False),
            ('columns', C.columns(16, 16), 16, False), ('noisy_ramp', R.noisy_ramp(16, 16, 14), 14, False), ('walk_deep', C.walk(16, 16), 16, True)]


def test_lane_routines_under_sanitizers(tmp_path):
    cxx = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'dng_enc_hostcheck')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
                           os.path.join(ROOT, 'tools', 'dng_enc_hostcheck.cpp')])
    blob, want = b'', []
    for name, t, P, deep in hostcheck_cases():
        data, info = R.ljpeg_encode(t.reshape(-1), P, t.shape[1] // 2, t.shape[0], 2, pred=1, deep=deep)
        bits, vals = info['tables'][0]
        if name == 'walk_deep':
            assert R.canonical_codes(bits, vals)[15][1] == 16 and C.ssss_hist(t, P)[15] > 0
        for segment, chunk in ((64, 16), (192, 48), (4096, 4096)):   # one sample a run; a last segment cut short; 16 samples a run
            blob += struct.pack('<5I', t.shape[0], t.shape[1], P, segment, chunk) + table_words(bits, vals).tobytes() + t.astype('<u2').tobytes()
            want.append((name, segment, data[info['header_len']:-2]))
    cases, out = str(tmp_path / 'cases.bin'), str(tmp_path / 'out.bin')
    with open(cases, 'wb') as fh:
        fh.write(struct.pack('<I', len(want)) + blob)
    r = subprocess.run([exe, cases, out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and 'hostcheck OK' in r.stdout, r.stdout
    assert 'coverage: 1-bit sample yes, 31-bit sample yes, 32 of 32 start phases' in r.stdout, r.stdout
    got = open(out, 'rb').read()
    pos = 0
    for name, segment, ent in want:
        n, = struct.unpack_from('<I', got, pos)
        assert got[pos + 4:pos + 4 + n] == ent, (name, segment)
        pos += 4 + n
    assert pos == len(got)
