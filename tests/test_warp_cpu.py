"""CPU tests of DNG WarpRectilinear (eld_amd/dng_opcodes.py Warp, csrc/warp_dev.h): the opcode's bytes and every rejection,
the entry point's argument rules with fake pointers, the per-pixel arithmetic under AddressSanitizer (tools/warp_hostcheck.cpp, a plain
executable), the command line's argument errors, and the NumPy restatement (tests/warp_ref.py) against properties it must have.  No device
is touched."""
import ctypes
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import dng_opcodes_ref as R
import warp_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIXED = (0.96, 0.06, -0.01, 0.002, 0.001, -0.001)
THREE = ((1.002, 0.01, 0.0, 0.0, 0.0, 0.0), (1.0, 0.01, 0.0, 0.0, 0.0, 0.0), (0.998, 0.01, 0.0, 0.0, 0.0, 0.0))


def O():
    from eld_amd import dng_opcodes
    return dng_opcodes


# ---- the opcode's bytes -------------------------------------------------------------------------------------------------------------------
def test_warp_round_trips_through_the_list():
    o = O()
    for sets, cx, cy in ((MIXED, 0.47, 0.53), (THREE, 0.5, 0.5)):
        op = o.pack_warp(sets, cx, cy, flags=1)
        assert op.id == 1 and op.optional and op.f is None and op.data == W.pack_params(sets, cx, cy)       # the restatement's bytes
        data = o.pack_opcode_list([op])
        assert data == R.pack_list([W.spec(sets, cx, cy, flags=1)])
        back = o.parse_opcode_list(data, 'OpcodeList3')
        assert back == [op] and o.pack_opcode_list(back) == data
        f = o.warp_params(back[0])
        assert f['sets'].dtype == np.float64 and f['sets'].shape == (len(np.reshape(sets, (-1, 6))), 6)
        assert np.array_equal(f['sets'], np.reshape(sets, (-1, 6))) and f['cx'] == cx and f['cy'] == cy
        w = o.warp_from_opcodes(back, 40, 60)
        assert np.array_equal(w.sets, f['sets']) and (w.cx, w.cy) == (cx, cy) and not w.identity
    assert o.Warp(W.IDENTITY, 0.3, 0.9).identity and o.Warp([W.IDENTITY] * 3).identity and not o.Warp(MIXED).identity
    assert o.warp_from_opcodes([], 8, 8) is None and o.warp_from_opcodes(None, 8, 8) is None


def test_unchanged_behaviour_of_the_lists():
    """a list 3 with a warp still parses to raw bytes and is still reported as never applied"""
    o = O()
    ops = o.parse_opcode_list(R.pack_list([W.spec(MIXED, 0.5, 0.5), {'id': 3, 'flags': 0, 'k': (0.1, 0, 0, 0, 0), 'cx': 0.5, 'cy': 0.5}]), 'OpcodeList3')
    assert ops[0].f is None and ops[0].data == W.pack_params(MIXED, 0.5, 0.5) and ops[0].name == 'WarpRectilinear'
    assert o.disposition(ops[0], 3) == 'never' and o.disposition(ops[0], 2) == 'never' and o.NEVER_APPLIED == (1, 2, 6)
    assert len(o.gain_program([], ops, 8, 8)) == 1                   # the vignette is compiled, the warp passed over


def _op(params, flags=0, id_=1):
    return O().Opcode(id_, None, params, flags)


BAD_PARAMS = {
    'no bytes': (b'', 'N'),
    'N = 2': (struct.pack('>I', 2) + bytes(8 * 14), 'N '),
    'N = 0': (struct.pack('>I', 0) + bytes(16), 'N '),
    'one byte short': (W.pack_params(MIXED, 0.5, 0.5)[:-1], 'byte count'),
    'one set announced, three stored': (struct.pack('>I', 1) + W.pack_params(THREE, 0.5, 0.5)[4:], 'byte count'),
    'trailing bytes': (W.pack_params(THREE, 0.5, 0.5) + b'\0' * 8, 'byte count'),
    'NaN kr1': (W.pack_params((1, float('nan'), 0, 0, 0, 0), 0.5, 0.5), 'kr1'),
    'inf kt0 of set 2': (W.pack_params((W.IDENTITY, W.IDENTITY, (1, 0, 0, 0, float('inf'), 0)), 0.5, 0.5), 'set 2 kt0'),
    'NaN cy': (W.pack_params(MIXED, 0.5, float('nan')), 'cy'),
}


@pytest.mark.parametrize('case', sorted(BAD_PARAMS))
def test_malformed_warps_name_list_opcode_and_field(case):
    params, word = BAD_PARAMS[case]
    o = O()
    ops = o.parse_opcode_list(R.pack_list([{'id': 9999, 'flags': 1, 'data': b'x'}, {'id': 1, 'flags': 0, 'data': params}]), 'OpcodeList3')
    assert ops[1].data == params                                     # parsing keeps whatever the bytes are
    with pytest.raises(ValueError) as e:
        o.warp_from_opcodes(ops, 40, 60, 'f.dng: OpcodeList3')
    text = str(e.value)
    assert 'f.dng: OpcodeList3' in text and 'opcode 1' in text and 'WarpRectilinear' in text and word in text, text
    with pytest.raises(ValueError, match='WarpRectilinear'):
        o.warp_params(ops[1])


def test_two_warps_and_fisheyes():
    o = O()
    one = o.pack_warp(MIXED, 0.5, 0.5)
    with pytest.raises(ValueError, match='second WarpRectilinear'):
        o.warp_from_opcodes([one, _op(b'abc', 1, 99), one], 8, 8)
    with pytest.raises(ValueError, match='WarpFisheye'):
        o.warp_from_opcodes([one, _op(bytes(56), 0, 2)], 8, 8)
    with pytest.raises(ValueError, match='WarpFisheye'):
        o.warp_from_opcodes([_op(bytes(56), 0, 2)], 8, 8)
    w = o.warp_from_opcodes([_op(bytes(56), 1, 2), one], 8, 8)        # optional: skipped
    assert np.array_equal(w.sets, np.reshape(MIXED, (1, 6)))
    assert o.warp_from_opcodes([_op(bytes(56), 1, 2)], 8, 8) is None
    with pytest.raises(ValueError, match='1 or 3'):
        o.Warp([W.IDENTITY] * 2)
    with pytest.raises(ValueError, match='finite'):
        o.Warp((1, 0, float('nan'), 0, 0, 0))
    with pytest.raises(ValueError, match='no WarpRectilinear'):
        o.warp_params(_op(bytes(56), 0, 2))


def test_record_is_the_restatements():
    """Warp.record against warp_ref.record, field by field and bit for bit, and the layout of EldWarp"""
    from eld_amd import _lib as L
    o = O()
    assert L.WARP_DTYPE.itemsize == 184 and L.WARP_DTYPE.fields['k'][1] == 8 and L.WARP_DTYPE.fields['cxp'][1] == 152
    for sets, cx, cy, Hm, Wm in ((MIXED, 0.47, 0.53, 33, 70), (THREE, 0.4871, 0.5123, 4000, 6000), (W.IDENTITY, -3.0, 7.5, 5, 7)):
        r = o.Warp(sets, cx, cy).record(Hm, Wm)
        want = W.record(sets, cx, cy, Hm, Wm)
        n = len(want['k'])
        assert int(r['nsets'][0]) == n and int(r['reserved'][0]) == 0
        assert r['k'][0, :n].tobytes() == want['k'].tobytes() and not r['k'][0, n:].any()
        for k in ('cxp', 'cyp', 'm', 'm2'):
            assert np.float64(r[k][0]).tobytes() == np.float64(want[k]).tobytes(), k
    with pytest.raises(ValueError):
        o.Warp(MIXED).record(0, 8)
    with pytest.raises(ValueError):
        o.Warp(MIXED).record(1 << 16, 1 << 15)


# ---- the entry point's argument rules ---------------------------------------------------------------------------------------------------------
def test_entry_point_refuses_bad_arguments_before_any_launch(eld_lib):
    from eld_amd import _lib as L
    o = O()
    A, B = 0x10000000, 0x20000000                                    # fake device pointers: nothing is launched on a refusal or with N == 0
    rec = o.Warp(MIXED, 0.47, 0.53).record(40, 60)

    def call(rgb=A, out=B, mode=L.RENDER_SRGB8, N=1, Hm=40, Wm=60, warp=rec, ccms=None, gamma=2.2, E=None, f=None, n=0, lds=-1):
        w = None if warp is None else ctypes.c_void_p(warp.ctypes.data)
        return eld_lib.eld_warp_rgb_f32(rgb, out, mode, N, Hm, Wm, w, ccms, gamma, E, f, n, lds, None)

    def with_field(name, value, index=None):
        r = rec.copy()
        if index is None:
            r[name][0] = value
        else:
            r[name][0][index] = value
        return r
    assert call(N=0) == 0                                            # the successful no-op, every other argument being valid
    assert call(N=0, mode=L.RENDER_LINEAR_F32, lds=0) == 0 and call(N=0, lds=65536) == 0
    assert call(N=0, warp=with_field('nsets', 3)) == 0               # three sets (two of them zero: the identity for G and B)
    bad = {'null rgb': dict(rgb=None), 'null out': dict(out=None), 'null warp': dict(warp=None),
           'rgb 8-byte aligned': dict(rgb=A + 8), 'float32 out 2-byte aligned': dict(out=B + 2, mode=L.RENDER_LINEAR_F32),
           'N < 0': dict(N=-1), 'N > 65535': dict(N=65536), 'Hm 0': dict(Hm=0), 'Wm 0': dict(Wm=0), 'Hm Wm = 2^31': dict(Hm=1 << 16, Wm=1 << 15),
           'nsets 2': dict(warp=with_field('nsets', 2)), 'nsets 0': dict(warp=with_field('nsets', 0)),
           'NaN kr1': dict(warp=with_field('k', np.nan, (0, 1))), 'inf kt1': dict(warp=with_field('k', np.inf, (0, 5))),
           'NaN cxp': dict(warp=with_field('cxp', np.nan)), '-inf cyp': dict(warp=with_field('cyp', -np.inf)),
           'inf m': dict(warp=with_field('m', np.inf)), 'NaN m2': dict(warp=with_field('m2', np.nan)),
           'm2 0': dict(warp=with_field('m2', 0.0)), 'm2 < 0': dict(warp=with_field('m2', -1.0)),
           'out_mode 2': dict(mode=2), 'out_mode -1': dict(mode=-1),
           'gamma 0': dict(gamma=0.0), 'gamma NaN': dict(gamma=float('nan')), 'crf_n 1': dict(n=1, E=A, f=A), 'crf_n < 0': dict(n=-2),
           'crf without tables': dict(n=4), 'crf_E misaligned': dict(n=4, E=A + 2, f=A), 'ccms misaligned': dict(ccms=A + 1),
           'lds_bytes 65537': dict(lds=65537),
           'out inside rgb': dict(out=A + 16), 'rgb inside a float32 out': dict(rgb=B + 4 * 40 * 60, mode=L.RENDER_LINEAR_F32),
           'out ends inside rgb': dict(out=A - 3 * 40 * 60 + 1)}
    for name, kw in bad.items():
        assert call(**kw) == -1, name                                # before any launch: the pointers are fake
        if 'N' not in kw and 'inside' not in name:                   # the rules come before the N == 0 return (an empty batch overlaps nothing)
            assert call(**dict(kw, N=0)) == -1, name
    assert call(N=0, warp=with_field('k', np.nan, (1, 0))) == 0      # a set that nsets = 1 does not read


# ---- the per-pixel arithmetic under AddressSanitizer ----------------------------------------------------------------------------------------
def hostcheck_case(Hm, Wm, sets, cx, cy, seed):
    from eld_amd import _lib as L
    rng = np.random.default_rng(seed)
    rgb = rng.uniform(-0.1, 1.1, (1, 3, Hm, Wm)).astype(np.float32)
    want = W.warp(rgb, sets, cx, cy)
    rec = O().Warp(sets, cx, cy).record(Hm, Wm)
    assert rec.dtype == L.WARP_DTYPE
    return struct.pack('<2I', Hm, Wm) + rec.tobytes() + rgb.tobytes() + want.tobytes()


def test_arithmetic_under_address_sanitizer(tmp_path):
    cxx = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'warp_hostcheck')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
                           os.path.join(ROOT, 'tools', 'warp_hostcheck.cpp')])
    cases = [hostcheck_case(5, 7, (3.0, 0, 0, 0, 0, 0), 0.5, 0.5, 1),
             hostcheck_case(12, 18, MIXED, 0.47, 0.53, 2),
             hostcheck_case(33, 20, THREE, 0.52, 0.46, 3)]
    path = str(tmp_path / 'cases.bin')
    with open(path, 'wb') as fh:
        fh.write(struct.pack('<I', len(cases)) + b''.join(cases))
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and 'hostcheck OK' in r.stdout, r.stdout
    assert '%d pixels of 3 cases' % (3 * (5 * 7 + 12 * 18 + 33 * 20)) in r.stdout and '4000 single-field corruptions' in r.stdout


# ---- the command line's argument errors ---------------------------------------------------------------------------------------------------------
def test_denoise_argument_errors(tmp_path):
    from eld_amd import denoise as D
    colour = ['--wb', '2', '1', '1.5', '--ccm', '1', '0', '0', '0', '1', '0', '0', '0', '1']
    base = [str(tmp_path / 'frame.npy'), '-o', str(tmp_path / 'out'), '--ckpt', 'none.pt'] + colour
    wfile = str(tmp_path / 'warp.json')
    with open(wfile, 'w') as fh:
        json.dump({'sets': [list(MIXED)], 'cx': 0.47, 'cy': 0.53}, fh)
    with pytest.raises(ValueError, match='--srgb-size full'):
        D.parse_args(base + ['--warp', wfile])
    with pytest.raises(ValueError, match='--srgb-size full'):
        D.parse_args(base + ['--warp', 'opcodes', '--srgb-size', 'packed'])
    with pytest.raises(ValueError, match='.dng inputs'):
        D.parse_args(base + ['--warp', 'opcodes', '--srgb-size', 'full'])
    o = D.parse_args(base + ['--warp', wfile, '--srgb-size', 'full'])[3]
    assert o['warp'] == wfile and o.get('opcodes') is None
    w = D.read_warp(wfile)
    assert np.array_equal(w.sets, np.reshape(MIXED, (1, 6))) and (w.cx, w.cy) == (0.47, 0.53)
    assert 'warp' not in D.parse_args(base)[3] or D.parse_args(base)[3]['warp'] is None
    side = str(tmp_path / 'side.json')                                # the sidecar key, relative to the sidecar
    with open(side, 'w') as fh:
        json.dump({'warp': 'warp.json', 'srgb_size': 'full'}, fh)
    assert D.parse_args(base + ['--meta', side])[3]['warp'] == wfile
    with open(wfile, 'w') as fh:
        json.dump({'sets': [list(MIXED)] * 2, 'cx': 0.47, 'cy': 0.53}, fh)
    with pytest.raises(ValueError, match='1 or 3'):
        D.read_warp(wfile)
    with open(wfile, 'w') as fh:
        json.dump({'sets': [list(MIXED)], 'cx': 0.47}, fh)
    with pytest.raises(ValueError, match='sets, cx, cy'):
        D.read_warp(wfile)

    class Net:                                                       # denoise_raw's own check comes before it looks at the network or a device
        cfa, in_channels, out_channels = 'bayer', 4, 4
    with pytest.raises(ValueError, match="srgb_size='full'"):
        D.denoise_raw(Net(), np.zeros((8, 8), np.uint16), 'bayer', wb=(2, 1, 1.5), ccm=np.eye(3), warp=O().Warp(MIXED))
    with pytest.raises(ValueError, match='Warp'):
        D.denoise_raw(Net(), np.zeros((8, 8), np.uint16), 'bayer', wb=(2, 1, 1.5), ccm=np.eye(3), srgb_size='full', warp={'sets': MIXED})


# ---- the restatement itself -------------------------------------------------------------------------------------------------------------------
def test_identity_returns_its_input_bit_for_bit():
    rng = np.random.default_rng(11)
    for (Hm, Wm), (cx, cy) in (((5, 7), (0.5, 0.5)), ((33, 70), (0.4871, 0.5123)), ((40, 61), (-2.0, 9.0))):
        rgb = rng.uniform(-0.1, 1.1, (2, 3, Hm, Wm)).astype(np.float32)
        rec = W.record(W.IDENTITY, cx, cy, Hm, Wm)
        u, v = W.coords(rec['k'][0], rec, Hm, Wm)
        assert np.array_equal(u, np.arange(Wm, dtype=np.float64)[None, :] + np.zeros((Hm, 1)))          # the displacement form: exact for any centre
        assert np.array_equal(v, np.arange(Hm, dtype=np.float64)[:, None] + np.zeros((1, Wm)))
        for sets in (W.IDENTITY, [W.IDENTITY] * 3):
            out = W.warp(rgb, sets, cx, cy)
            assert np.array_equal(out.view(np.uint32), rgb.view(np.uint32))


def test_affine_ramp_is_reproduced():
    """Catmull-Rom reproduces polynomials of degree 1 (sum w = 1, sum w q = t + 1 over the taps q = 0 .. 3), so on a ramp a x + b y + c the exact
    16-tap sum at (u, v) is a u + b v + c wherever no tap is clamped.  The float32 evaluation differs from it by: the sum itself, sum |w| <=
    1.25^2 = 1.5625 and about 24 float32 roundings of terms <= 1, 24 * 1.5625 * 2^-24 = 2.3e-6; t's rounding to float32, at most 2^-25 of a
    pixel times the ramp's slope (< 0.02 per pixel here), 6e-10; the ramp's own rounding to float32 in the input, 2^-25 per tap, 4.7e-8 after
    the weights.  Together below the cap of 1e-5."""
    Hm, Wm = 48, 64
    a, b, c = 0.009, 0.011, 0.1                                      # scaled below so that the ramp's largest value is 1
    yy, xx = np.mgrid[0:Hm, 0:Wm].astype(np.float64)
    scale = 1.0 / (a * (Wm - 1) + b * (Hm - 1) + c)
    a, b, c = a * scale, b * scale, c * scale
    ramp = (a * xx + b * yy + c)
    assert ramp.min() >= 0.0 and ramp.max() <= 1.0
    rgb = np.broadcast_to(ramp.astype(np.float32), (1, 3, Hm, Wm)).copy()
    worst = 0.0
    for sets, cx, cy in ((MIXED, 0.47, 0.53), ((1, 0.05, 0, 0, 0, 0), 0.5, 0.5), (THREE, 0.5, 0.5), ((1.0005, 0, 0, 0, 0, 0), 0.5, 0.5)):
        out = W.warp(rgb, sets, cx, cy)
        rec = W.record(sets, cx, cy, Hm, Wm)
        for ch in range(3):
            u, v = W.coords(rec['k'][ch if len(rec['k']) == 3 else 0], rec, Hm, Wm)
            inside = (u >= 1) & (u < Wm - 2) & (v >= 1) & (v < Hm - 2)          # no tap clamped: j0 - 1 >= 0 and j0 + 2 <= Wm - 1
            assert inside.sum() > Hm * Wm // 2
            err = np.abs(out[0, ch].astype(np.float64) - (a * u + b * v + c))[inside].max()
            worst = max(worst, float(err))
            assert err <= 1e-5, (sets, ch, err)
    print('max |restatement - ramp at (u, v)| over the interior: %.3e (cap 1e-5)' % worst)


def test_edge_is_replicated_and_nan_coordinates_go_to_the_corner():
    """kr0 = 3 sends most coordinates outside: a pixel whose clamped footprint lies in one corner returns that corner's value"""
    Hm, Wm = 5, 7
    rng = np.random.default_rng(3)
    rgb = rng.uniform(0.1, 1.0, (1, 3, Hm, Wm)).astype(np.float32)
    out = W.warp(rgb, (3.0, 0, 0, 0, 0, 0), 0.5, 0.5)
    for ch in range(3):
        assert out[0, ch, 0, 0] == rgb[0, ch, 0, 0] and out[0, ch, -1, -1] == rgb[0, ch, -1, -1]
        assert out[0, ch, 0, -1] == rgb[0, ch, 0, -1] and out[0, ch, -1, 0] == rgb[0, ch, -1, 0]
    i0, t = W.cell(np.array([np.nan, -5.0, -1.0, -0.25, 6.5, 7.0, 1e300, np.inf, -np.inf]), 7)
    assert i0.tolist() == [-1, -1, -1, -1, 6, 7, 7, 7, -1] and t.tolist() == [0, 0, 0, 0.75, 0.5, 0, 0, 0, 0]
    w = W.weights(np.float32(0.5))
    assert [float(x) for x in w] == [-0.0625, 0.5625, 0.5625, -0.0625]
