"""CPU tests of the directional X-Trans demosaic: the NumPy restatement (tests/demosaic_xdir_ref.py) has the properties a
demosaic must have (sampled values pass through, constant colours come back exact at every small size, finite output), the pattern facts its
stage C and its extension stand on hold, and it beats the normalised convolution where a directional method must (fine oriented gratings)
without losing on the existing scenes; the per-site functions of csrc/demosaic_xdir_dev.h give the restatement's bits under AddressSanitizer
(tools/demosaic_xdir_hostcheck.cpp, a plain executable); the entry point refuses what eld_render_xtrans refuses; render_xtrans, render_bayer,
denoise_raw and the command line refuse bad `demosaic` arguments before any device work.  The kernel is compared with the restatement in
tests/test_demosaic_xdir_gpu.py."""
import ctypes
import json
import os
import shutil
import struct
import subprocess
import types

import numpy as np
import pytest

import demosaic_edge_ref as E
import demosaic_ref as D
import demosaic_xdir_ref as X
from test_demosaic_cpu import CONST, psnr, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SMALL = [(2, 2), (2, 4), (4, 2), (6, 10)]


# ---- 1. sampled values pass through -------------------------------------------------------------------------------------------------------
def test_sampled_values_pass_through():
    rng = np.random.default_rng(2)
    p = rng.uniform(0, 1, size=(2, 9, 4, 6)).astype(F32)
    ones = np.ones((2, 3), F32)
    rgb = X.linear_xtrans_dir(p, ones)
    m = D.mosaic_xtrans(p, ones)
    col = D.xtrans_colour_map(12, 18)
    assert rgb.dtype == F32 and rgb.shape == (2, 3, 12, 18) and np.isfinite(rgb).all()
    for k in range(3):
        assert np.array_equal(rgb[:, k][:, col == k], m[:, col == k])
    rows, cols = D.O.xtrans_source_index(4, 6)
    for k in range(9):                                      # ... and every plane sits where the pack puts it
        assert np.array_equal(rgb[:, D.PLANE_COLOUR[k], rows[k], cols[k]], p[:, k])


# ---- 2. constant colours come back exact, down to one cell ------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', SMALL)
def test_constant_colour_is_exact(hw):
    h, w = hw
    p = np.zeros((len(CONST), 9, h, w), F32)
    for i, rgb in enumerate(CONST):
        for k in range(9):
            p[i, k] = rgb[D.PLANE_COLOUR[k]]
    out = X.linear_xtrans_dir(p, np.ones((len(CONST), 3), F32))
    for i, rgb in enumerate(CONST):
        for k in range(3):
            assert np.all(out[i, k] == F32(rgb[k])), (i, k)


def test_output_is_finite_with_both_clamps():
    rng = np.random.default_rng(3)
    for h, w in SMALL:
        p = rng.uniform(-0.5, 1.5, size=(2, 9, h, w)).astype(F32)
        wbs = rng.uniform(0.7, 2.2, size=(2, 3)).astype(F32)
        m = D.mosaic_xtrans(p, wbs)
        assert m.min() == 0.0 and m.max() == 1.0
        assert np.isfinite(X.linear_xtrans_dir(p, wbs)).all()
    flat = np.zeros((1, 9, 2, 2), F32)                      # no gradient anywhere: the weights' 1e-6 keeps the division finite
    assert np.array_equal(X.linear_xtrans_dir(flat, np.ones((1, 3), F32)), np.zeros((1, 3, 6, 6), F32))


# ---- 3. the pattern facts ---------------------------------------------------------------------------------------------------------------------
def test_pattern_facts():
    """every R and B site has one solitary axis (both neighbours and both second neighbours are G) and one paired axis (neighbour a is G, the
    site at 2a has the site's colour, the one at -a the other colour, the one at -2a is G)"""
    col = D.xtrans_colour_map(18, 18)
    a_h, a_v = X.axis_maps(col)
    n = 0
    for y in range(6, 12):
        for x in range(6, 12):
            own = col[y, x]
            if own == 1:
                assert a_h[y, x] == 0 and a_v[y, x] == 0
                continue
            n += 1
            kinds = []
            for a, (dy, dx) in ((a_h[y, x], (0, 1)), (a_v[y, x], (1, 0))):
                line = [col[y + k * dy, x + k * dx] for k in range(-2, 3)]
                solitary = line[0] == line[1] == line[3] == line[4] == 1
                kinds.append(solitary)
                if solitary:
                    assert a == 0
                else:
                    assert a in (-1, 1)
                    assert line[2 + a] == 1 and line[2 + 2 * a] == own and line[2 - a] == 2 - own and line[2 - 2 * a] == 1, (y, x)
            assert kinds[0] != kinds[1], (y, x)             # solitary xor paired
    assert n == 16


def test_extension_preserves_colour():
    """the extended colour map equals the periodic one for frames from 6 x 6 upwards; a 6-site side folds twice"""
    for H in (6, 12, 18, 24):
        for W in (6, 12, 18, 30):
            col = D.xtrans_colour_map(H, W)
            iy, ix = X.ext_indices(H, 0), X.ext_indices(W, 1)
            assert iy.min() >= 0 and iy.max() < H and ix.min() >= 0 and ix.max() < W
            assert np.array_equal(col[iy][:, ix], D.xtrans_colour_map(H + 12, W + 12)), (H, W)
    assert X.ext_index(-6, 6, 0) == 0 and X.ext_index(-6, 6, 1) == 0 and X.ext_index(11, 6, 0) == 5 and X.ext_index(11, 6, 1) == 5
    assert X.ext_index(-1, 12, 0) == 1 and X.ext_index(12, 12, 0) == 6 and X.ext_index(-1, 12, 1) == 5 and X.ext_index(12, 12, 1) == 10
    cell = D.xtrans_cell_colours()                          # no other mirror: rows only about 0 and 3, columns only about 2 and 5
    assert [r for r in range(6) if all(np.array_equal(cell[(r + k) % 6], cell[(r - k) % 6]) for k in range(6))] == [0, 3]
    assert [c for c in range(6) if all(np.array_equal(cell[:, (c + k) % 6], cell[:, (c - k) % 6]) for k in range(6))] == [2, 5]


# ---- 4. quality against the normalised convolution -----------------------------------------------------------------------------------------------
def both(img):
    """(PSNR of the directional demosaic, PSNR of the normalised convolution), both float32, of the picture sampled on the X-Trans cell"""
    p = X.sample(img).astype(F32)
    ones = np.ones((1, 3), F32)
    return psnr(X.linear_xtrans_dir(p, ones)[0], img), psnr(D.linear_xtrans(p, ones)[0], img)


@pytest.mark.parametrize('seed', [5, 6, 7])
def test_quality_on_gratings(seed):
    """fine oriented gratings whose three channels share one luminance: a wrong direction choice or a swapped weight gives up the gain.
    Measured in float32 (equal to float64 at this precision): seed 5 18.46 -> 20.72 dB (+2.25), seed 6 19.76 -> 23.15 dB (+3.38),
    seed 7 18.53 -> 20.56 dB (+2.02); the margin asked is half of the smallest, 1.0 dB"""
    img = E.gratings(seed, 192, 258)
    assert img.shape == (3, 192, 258)
    xdir, norm = both(img)
    print('gratings seed %d PSNR: normalised convolution %.2f dB, directional %.2f dB (%+.2f)' % (seed, norm, xdir, xdir - norm))
    assert xdir >= norm + 1.0, seed


@pytest.mark.parametrize('seed', [7, 1])
def test_quality_on_the_existing_scenes(seed):
    """smooth sinusoids with step edges (tests/test_demosaic_cpu.py scene()): no loss beyond 0.1 dB (measured in float32: seed 7 36.46 ->
    36.74 dB (+0.29), seed 1 36.77 -> 36.84 dB (+0.07))"""
    xdir, norm = both(scene(seed=seed))
    print('scene seed %d PSNR: normalised convolution %.2f dB, directional %.2f dB (%+.2f)' % (seed, norm, xdir, xdir - norm))
    assert xdir >= norm - 0.1, seed


# ---- 5. the per-site functions of the kernel under AddressSanitizer ------------------------------------------------------------------------------
def hostcheck_case(H, W, seed):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-0.2, 1.2, size=(1, H, W)).clip(0, 1).astype(F32)        # both clamps among the values
    want = X.directional_xtrans(v)
    return struct.pack('<II', H, W) + v.tobytes() + want.tobytes(), want


def test_arithmetic_under_address_sanitizer(tmp_path):
    cxx = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'demosaic_xdir_hostcheck')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
                           os.path.join(ROOT, 'tools', 'demosaic_xdir_hostcheck.cpp')])
    shapes = [(12, 18), (6, 6), (6, 12), (12, 6), (18, 30), (30, 24)]
    cases = [hostcheck_case(H, W, 50 + i) for i, (H, W) in enumerate(shapes)]
    path = str(tmp_path / 'cases.bin')
    with open(path, 'wb') as fh:
        fh.write(struct.pack('<I', len(cases)) + b''.join(c[0] for c in cases))
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and 'hostcheck OK' in r.stdout, r.stdout
    assert '%d values of %d cases' % (3 * sum(H * W for H, W in shapes), len(shapes)) in r.stdout
    lines = r.stdout.split('\n')
    at = lines.index('frame 12 18')                          # the printed frame, compared here: the same bits as the restatement
    words = np.array([[int(x, 16) for x in ln.split()] for ln in lines[at + 1:at + 1 + 36]], np.uint32)
    assert np.array_equal(words.reshape(3, 12, 18), cases[0][1][0].view(np.uint32))


# ---- 6. the entry point's refusals (before any launch: fake pointers do) and the tile it reports -------------------------------------------------
def test_entry_point_refusals_and_tile(eld_lib):
    P = ctypes.c_void_p

    def call(fn, packed=0x1000, wbs=0x2000, ccms=0x3000, out=0x4000, mode=1, N=1, h=4, w=4, gamma=2.2, e=None, f=None, cn=0):
        return fn(P(packed), P(wbs), P(ccms), P(out), mode, N, h, w, gamma, e, f, cn, None)
    bad_args = [dict(packed=None), dict(wbs=None), dict(out=None), dict(packed=0x1004), dict(out=0x4008), dict(wbs=0x2002), dict(ccms=0x3001),
                dict(N=0), dict(N=-1), dict(N=65536), dict(h=0), dict(w=-2), dict(h=1), dict(w=1), dict(h=3), dict(w=5), dict(mode=2),
                dict(mode=-1), dict(gamma=0.0), dict(gamma=-1.0), dict(cn=1), dict(cn=-1), dict(cn=8), dict(cn=8, e=P(0x5000)),
                dict(cn=8, e=P(0x5002), f=P(0x6000))]
    for kw in bad_args:                                     # everything eld_render_xtrans refuses, eld_render_xtrans_dir refuses
        assert call(eld_lib.eld_render_xtrans, **kw) == -1, kw
        assert call(eld_lib.eld_render_xtrans_dir, **kw) == -1, kw
    assert call(eld_lib.eld_render_xtrans_dir, h=(1 << 28) + 2) == -1
    th, tw, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert eld_lib.eld_render_xtrans_dir_tile(ctypes.byref(th), ctypes.byref(tw), ctypes.byref(lds)) == 0
    assert th.value >= 6 and th.value % 6 == 0 and tw.value >= 6 and tw.value % 6 == 0                     # whole cells
    assert (th.value + 12) * (tw.value + 12) * 4 <= lds.value <= 80 * 1024      # at least v on tile + 12; two workgroups share a CU's 160 KiB
    assert eld_lib.eld_render_xtrans_dir_tile(None, ctypes.byref(tw), None) == -1 and eld_lib.eld_render_xtrans_dir_tile(ctypes.byref(th), None, None) == -1
    th2, tw2 = ctypes.c_int(), ctypes.c_int()
    assert eld_lib.eld_render_xtrans_dir_tile(ctypes.byref(th2), ctypes.byref(tw2), None) == 0 and (th2.value, tw2.value) == (th.value, tw.value)


# ---- 7. argument handling ------------------------------------------------------------------------------------------------------------------
class FakeNet:
    def parameters(self):
        raise AssertionError('device work before the argument checks')


def fake(cfa):
    from eld_amd.denoise import PLANES
    return types.SimpleNamespace(cfa=cfa, in_channels=PLANES[cfa], out_channels=PLANES[cfa], net=FakeNet())


class NoTensor:                                               # any use of the frame is device work
    def __getattr__(self, name):
        raise AssertionError('device work before the argument checks')


COLOUR = dict(wb=[2.0, 1.0, 1.5], ccm=np.eye(3))


def test_the_names():
    from eld_amd import isp
    assert isp.DEMOSAICS == ('mhc', 'edge', 'directional')
    isp.check_demosaic('mhc', 'xtrans', 'full')
    isp.check_demosaic('mhc', 'xtrans', 'packed')
    isp.check_demosaic('directional', 'xtrans', 'full')
    for args in (('directional', 'bayer', 'full'), ('directional',), ('directional', 'xtrans', 'packed'), ('edge', 'xtrans', 'full'),
                 ('Directional', 'xtrans', 'full'), (None, 'xtrans', 'full')):
        with pytest.raises(ValueError, match='demosaic'):
            isp.check_demosaic(*args)


@pytest.mark.parametrize('cfa,kw', [
    ('bayer', dict(demosaic='directional', srgb_size='full', **COLOUR)),   # an X-Trans demosaic
    ('xtrans', dict(demosaic='directional', **COLOUR)),                    # without srgb_size='full'
    ('xtrans', dict(demosaic='directional')),
    ('xtrans', dict(demosaic='edge', srgb_size='full', **COLOUR)),         # 'edge' stays a Bayer demosaic
    ('xtrans', dict(demosaic='markesteijn', srgb_size='full', **COLOUR)),  # an unknown value
])
def test_denoise_raw_demosaic_errors(cfa, kw):
    from eld_amd.denoise import denoise_raw
    with pytest.raises(ValueError, match='demosaic'):
        denoise_raw(fake(cfa), np.full((12, 24), 1100, np.uint16), cfa, **kw)


def test_renders_refuse_before_the_frame_is_touched():
    from eld_amd.isp import render_bayer, render_xtrans
    with pytest.raises(ValueError, match='demosaic'):
        render_bayer(NoTensor(), [[0, 1], [3, 2]], np.ones((1, 4), F32), np.eye(3)[None], demosaic='directional')
    for bad in ('edge', 'ahd', 'DIRECTIONAL', None, 1):
        with pytest.raises(ValueError, match='demosaic'):
            render_xtrans(NoTensor(), np.ones((1, 3), F32), np.eye(3)[None], demosaic=bad)
        with pytest.raises(ValueError, match='demosaic'):
            render_xtrans(NoTensor(), np.ones((1, 3), F32), np.eye(3)[None], demosaic=bad, warp=object())


def test_cli_and_sidecar_demosaic(tmp_path):
    from eld_amd.denoise import build_parser, parse_args, read_sidecar
    base = ['--ckpt', 'm.pt', 'a.npy', '-o', 'x', '--cfa', 'xtrans']
    colour = ['--wb', '2', '1', '1.5', '--ccm', '1', '0', '0', '0', '1', '0', '0', '0', '1']
    full = colour + ['--srgb-size', 'full']
    assert 'demosaic' not in parse_args(base)[3] and 'demosaic' not in parse_args(base + full)[3]          # the default adds nothing
    assert parse_args(base + full + ['--demosaic', 'directional'])[3]['demosaic'] == 'directional'
    assert parse_args(base + full + ['--demosaic', 'mhc'])[3]['demosaic'] == 'mhc'
    with pytest.raises(ValueError, match='demosaic'):
        parse_args(base + colour + ['--demosaic', 'directional'])             # packed resolution has no demosaic
    with pytest.raises(ValueError, match='demosaic'):
        parse_args(['--ckpt', 'm.pt', 'a.npy', '-o', 'x'] + full + ['--demosaic', 'directional'])         # a Bayer frame
    with pytest.raises(ValueError, match='demosaic'):
        parse_args(base + full + ['--demosaic', 'edge'])
    with pytest.raises(SystemExit):
        parse_args(base + full + ['--demosaic', 'markesteijn'])
    text = build_parser().format_help()
    at = text.index('--demosaic')
    assert 'Bayer' in text[at:] and 'X-Trans' in text[at:] and 'directional' in text[at:]                  # which value belongs to which CFA
    meta = tmp_path / 'meta.json'
    meta.write_text(json.dumps({'cfa': 'xtrans', 'demosaic': 'directional', 'srgb_size': 'full', 'wb': [2, 1, 1.5], 'ccm': np.eye(3).tolist()}))
    assert read_sidecar(str(meta))['demosaic'] == 'directional'
    plain = ['--ckpt', 'm.pt', 'a.npy', '-o', 'x']
    assert parse_args(plain + ['--meta', str(meta)])[3]['demosaic'] == 'directional'                       # the sidecar's key is read
    assert parse_args(plain + ['--meta', str(meta), '--demosaic', 'mhc'])[3]['demosaic'] == 'mhc'          # the command line overrides it
    meta.write_text(json.dumps({'cfa': 'bayer', 'demosaic': 'directional', 'srgb_size': 'full', 'wb': [2, 1, 1.5], 'ccm': np.eye(3).tolist()}))
    with pytest.raises(ValueError, match='demosaic'):
        parse_args(plain + ['--meta', str(meta)])
    assert parse_args(plain + ['--meta', str(meta), '--cfa', 'xtrans'])[3]['demosaic'] == 'directional'
