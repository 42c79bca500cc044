"""CPU tests of the edge-directed Bayer demosaic: the NumPy restatement (tests/demosaic_edge_ref.py) has the properties a
demosaic must have (sampled values pass through, constant colours come back exact at every small size) and beats Malvar-He-Cutler where an
edge-directed method must (fine oriented gratings) without losing on the existing scene; the per-site functions of csrc/demosaic_edge_dev.h
give the restatement's bits under AddressSanitizer (tools/demosaic_edge_hostcheck.cpp, a plain executable); render_bayer, denoise_raw and the
command line refuse bad `demosaic` arguments before any device work.  The kernel is compared with the restatement in
tests/test_demosaic_edge_gpu.py."""
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
from test_demosaic_cpu import CONST, PATTERNS, psnr, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ---- 1. sampled values pass through -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pat', PATTERNS)
def test_sampled_values_pass_through(pat):
    rng = np.random.default_rng(1)
    p = rng.uniform(0, 1, size=(2, 4, 9, 13)).astype(F32)
    ones = np.ones((2, 4), F32)
    rgb = E.linear_bayer_edge(p, pat, ones)
    m = D.mosaic_bayer(p, pat, ones)
    col = D.bayer_colour_map(pat, 18, 26)
    assert rgb.dtype == F32 and rgb.shape == (2, 3, 18, 26) and np.isfinite(rgb).all()
    for k in range(3):
        assert np.array_equal(rgb[:, k][:, col == k], m[:, col == k])
    for k in range(4):                                      # ... and every plane sits where raw_pattern puts it
        (oy,), (ox,) = np.where(np.asarray(pat) == k)
        assert np.array_equal(rgb[:, D.CODE_COLOUR[k], oy::2, ox::2], p[:, k])


# ---- 2. constant colours come back exact, down to one packed pixel -----------------------------------------------------------------------------
@pytest.mark.parametrize('pat', PATTERNS)
@pytest.mark.parametrize('hw', [(1, 1), (1, 4), (2, 2), (5, 7)])
def test_constant_colour_is_exact(pat, hw):
    h, w = hw
    p = np.zeros((len(CONST), 4, h, w), F32)
    for i, rgb in enumerate(CONST):
        for k in range(4):
            p[i, k] = rgb[D.CODE_COLOUR[k]]
    out = E.linear_bayer_edge(p, pat, np.ones((len(CONST), 4), F32))
    for i, rgb in enumerate(CONST):
        for k in range(3):
            assert np.all(out[i, k] == F32(rgb[k])), (i, k)


# ---- 3. quality against Malvar-He-Cutler ------------------------------------------------------------------------------------------------------
def both(img, pat):
    """(PSNR of the edge-directed demosaic, PSNR of Malvar-He-Cutler), both float32, of the picture sampled with `pat`"""
    p = E.sample(img, pat).astype(F32)
    ones = np.ones((1, 4), F32)
    return psnr(E.linear_bayer_edge(p, pat, ones)[0], img), psnr(D.linear_bayer(p, pat, ones)[0], img)


@pytest.mark.parametrize('seed', [5, 6, 7])
def test_quality_on_gratings(seed):
    """fine oriented gratings whose three channels share one luminance: a wrong direction choice or a swapped weight gives up the whole gain
    (measured: +2.00 to +2.55 dB), the margin asked is half of the smallest"""
    img = E.gratings(seed)
    assert img.shape == (3, 192, 256)
    for pat in PATTERNS:
        edge, mhc = both(img, pat)
        print('gratings seed %d %s PSNR: Malvar %.2f dB, edge-directed %.2f dB (%+.2f)' % (seed, pat, mhc, edge, edge - mhc))
        assert edge >= mhc + 1.0, (seed, pat)


def test_quality_on_the_existing_scene():
    """smooth sinusoids with step edges (tests/test_demosaic_cpu.py scene(), seed 7): no loss (measured: +0.03 to +0.06 dB)"""
    img = scene()
    for pat in PATTERNS:
        edge, mhc = both(img, pat)
        print('scene seed 7 %s PSNR: Malvar %.2f dB, edge-directed %.2f dB (%+.2f)' % (pat, mhc, edge, edge - mhc))
        assert edge >= mhc - 0.1, pat


# ---- 4. the per-site functions of the kernel under AddressSanitizer ------------------------------------------------------------------------------
def hostcheck_case(H, W, pat, seed):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-0.2, 1.2, size=(1, H, W)).clip(0, 1).astype(F32)        # both clamps among the values
    want = E.edge_directed(v, pat)
    return struct.pack('<II4i', H, W, *np.asarray(pat).reshape(-1).tolist()) + v.tobytes() + want.tobytes(), want


def test_arithmetic_under_address_sanitizer(tmp_path):
    cxx = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'demosaic_edge_hostcheck')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
                           os.path.join(ROOT, 'tools', 'demosaic_edge_hostcheck.cpp')])
    shapes = [(10, 14), (2, 2), (2, 8), (4, 4), (6, 10), (18, 26), (34, 22)]
    cases = [hostcheck_case(H, W, PATTERNS[i % 4], 40 + i) for i, (H, W) in enumerate(shapes)]
    path = str(tmp_path / 'cases.bin')
    with open(path, 'wb') as fh:
        fh.write(struct.pack('<I', len(cases)) + b''.join(c[0] for c in cases))
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and 'hostcheck OK' in r.stdout, r.stdout
    assert '%d values of %d cases' % (3 * sum(H * W for H, W in shapes), len(shapes)) in r.stdout
    lines = r.stdout.split('\n')
    at = lines.index('frame 10 14')                          # the printed frame, compared here: the same bits as the restatement
    words = np.array([[int(x, 16) for x in ln.split()] for ln in lines[at + 1:at + 1 + 30]], np.uint32)
    assert np.array_equal(words.reshape(3, 10, 14), cases[0][1][0].view(np.uint32))


# ---- 5. the entry point's refusals (before any launch: fake pointers do) and the tile it reports -------------------------------------------------
def test_entry_point_refusals_and_tile(eld_lib):
    import ctypes
    P = ctypes.c_void_p
    pat = (ctypes.c_int * 4)(0, 1, 3, 2)

    def call(packed=0x1000, pattern=pat, wbs=0x2000, ccms=0x3000, out=0x4000, mode=1, N=1, h=4, w=4, gamma=2.2, e=None, f=None, cn=0):
        return eld_lib.eld_render_bayer_edge(P(packed), pattern, P(wbs), P(ccms), P(out), mode, N, h, w, gamma, e, f, cn, None)
    bad = [call(packed=None), call(wbs=None), call(out=None), call(pattern=None), call(packed=0x1004), call(out=0x4008), call(wbs=0x2002),
           call(ccms=0x3001), call(N=0), call(N=65536), call(h=0), call(w=-2), call(h=(1 << 28) + 1), call(mode=2), call(mode=-1), call(gamma=0.0),
           call(cn=1), call(cn=-1), call(cn=8)]
    assert bad == [-1] * len(bad), bad
    for bad_pat in ((0, 1, 2, 2), (0, 1, 2, 4), (-1, 0, 1, 2), (0, 0, 0, 0), (0, 2, 1, 3)):
        assert call(pattern=(ctypes.c_int * 4)(*bad_pat)) == -1, bad_pat
    th, tw, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert eld_lib.eld_render_bayer_edge_tile(ctypes.byref(th), ctypes.byref(tw), ctypes.byref(lds)) == 0
    assert th.value >= 2 and th.value % 2 == 0 and tw.value >= 4 and tw.value % 4 == 0
    assert (th.value + 8) * (tw.value + 8) * 4 <= lds.value <= 80 * 1024          # at least v on tile + 4; two workgroups share a CU's 160 KiB
    assert eld_lib.eld_render_bayer_edge_tile(None, ctypes.byref(tw), None) == -1 and eld_lib.eld_render_bayer_edge_tile(ctypes.byref(th), None, None) == -1


# ---- 6. argument handling ------------------------------------------------------------------------------------------------------------------
class FakeNet:
    def parameters(self):
        raise AssertionError('device work before the argument checks')


def fake(cfa):
    from eld_amd.denoise import PLANES
    return types.SimpleNamespace(cfa=cfa, in_channels=PLANES[cfa], out_channels=PLANES[cfa], net=FakeNet())


COLOUR = dict(wb=[2.0, 1.0, 1.5], ccm=np.eye(3))


@pytest.mark.parametrize('cfa,kw', [
    ('bayer', dict(demosaic='ahd', srgb_size='full', **COLOUR)),          # an unknown value
    ('bayer', dict(demosaic=None, srgb_size='full', **COLOUR)),
    ('bayer', dict(demosaic='malvar')),                                    # ... also where no render would use it
    ('xtrans', dict(demosaic='edge', srgb_size='full', **COLOUR)),        # a Bayer demosaic
    ('bayer', dict(demosaic='edge', **COLOUR)),                            # without srgb_size='full'
    ('bayer', dict(demosaic='edge')),
])
def test_denoise_raw_demosaic_errors(cfa, kw):
    from eld_amd.denoise import denoise_raw
    with pytest.raises(ValueError, match='demosaic'):
        denoise_raw(fake(cfa), np.full((12, 24), 1100, np.uint16), cfa, **kw)


def test_render_bayer_refuses_an_unknown_demosaic():
    from eld_amd.isp import render_bayer

    class NoTensor:                                           # any use of the frame is device work
        def __getattr__(self, name):
            raise AssertionError('device work before the argument checks')
    for bad in ('ahd', 'MHC', None, 1):
        with pytest.raises(ValueError, match='demosaic'):
            render_bayer(NoTensor(), PATTERNS[0], np.ones((1, 4), F32), np.eye(3)[None], demosaic=bad)


def test_cli_and_sidecar_demosaic(tmp_path):
    from eld_amd.denoise import parse_args, read_sidecar
    base = ['--ckpt', 'm.pt', 'a.npy', '-o', 'x']
    colour = ['--wb', '2', '1', '1.5', '--ccm', '1', '0', '0', '0', '1', '0', '0', '0', '1']
    full = colour + ['--srgb-size', 'full']
    assert 'demosaic' not in parse_args(base)[3] and 'demosaic' not in parse_args(base + full)[3]          # the default adds nothing
    assert parse_args(base + full + ['--demosaic', 'edge'])[3]['demosaic'] == 'edge'
    assert parse_args(base + full + ['--demosaic', 'mhc'])[3]['demosaic'] == 'mhc'
    with pytest.raises(ValueError, match='demosaic'):
        parse_args(base + colour + ['--demosaic', 'edge'])                    # packed resolution has no demosaic
    with pytest.raises(ValueError, match='demosaic'):
        parse_args(base + full + ['--cfa', 'xtrans', '--demosaic', 'edge'])
    with pytest.raises(SystemExit):
        parse_args(base + full + ['--demosaic', 'ahd'])
    meta = tmp_path / 'meta.json'
    meta.write_text(json.dumps({'demosaic': 'edge', 'srgb_size': 'full', 'wb': [2, 1, 1.5], 'ccm': np.eye(3).tolist()}))
    assert read_sidecar(str(meta))['demosaic'] == 'edge'
    assert parse_args(base + ['--meta', str(meta)])[3]['demosaic'] == 'edge'                                 # the sidecar's key is read
    assert parse_args(base + ['--meta', str(meta), '--demosaic', 'mhc'])[3]['demosaic'] == 'mhc'            # the command line overrides it
    meta.write_text(json.dumps({'demosaic': 'ahd', 'srgb_size': 'full', 'wb': [2, 1, 1.5], 'ccm': np.eye(3).tolist()}))
    with pytest.raises(ValueError, match='demosaic'):
        parse_args(base + ['--meta', str(meta)])
