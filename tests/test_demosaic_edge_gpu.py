"""GPU tests of the edge-directed Bayer render (csrc/demosaic_edge.hip eld_render_bayer_edge, eld_amd.isp.render_bayer(demosaic='edge'),
denoise_raw(demosaic='edge')): the linear output bit for bit against the NumPy float32 restatement
(tests/demosaic_edge_ref.py), the 8-bit codes, guarded output buffers, agreement with the Malvar-He-Cutler render on frames of constant colour,
the identity warp, denoise_raw end to end and determinism.

Packed shapes, the smallest at which the kernel can go wrong: 1 x 1 and 1 x 4 (a mosaic of two rows: every stage mirrors more than once),
2 x 2 .. 9 x 13 (every border inside one tile), 17 x 133 (a width that is no multiple of 4 mosaic sites: the narrow stores and the half-lane
in front of the right edge; three tiles), and tile + 3 x 2 tiles + 5 from the kernel's own constants (two tiles down, three across, ragged
last tiles both ways)."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import demosaic_edge_ref as E          # noqa: E402
import demosaic_ref as D              # noqa: E402
import warp_ref as W                  # noqa: E402
from guarded import Guards            # noqa: E402

F32 = np.float32
PATTERNS = [[[0, 1], [3, 2]], [[2, 3], [1, 0]], [[1, 0], [2, 3]], [[3, 2], [0, 1]]]      # RGGB, BGGR, GRBG, GBRG
SMALL = [(1, 1), (1, 4), (2, 2), (3, 5), (5, 7), (9, 13)]
CRF_E = np.linspace(0, 1, 1024, dtype=F32)
CRF = (CRF_E, (CRF_E ** 0.45).astype(F32))


@pytest.fixture(scope='module')
def lib(eld_lib):
    assert torch.cuda.is_available()
    return eld_lib


def tile_shape():
    from eld_amd.isp import edge_tile
    th, tw = edge_tile()
    assert th >= 1 and tw >= 1
    return th + 3, 2 * tw + 5


def inputs(h, w, seed, N=2):
    """packed values in [-0.1, 1.3] with both ends present, per-frame gains that differ and drive sites to both clamps, per-frame matrices"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.1, 1.3, size=(N, 4, h, w)).astype(F32)
    p[:, 0, 0, 0], p[:, 1, 0, 0] = -0.1, 1.3
    wbs = rng.uniform(0.8, 2.2, size=(N, 4)).astype(F32)
    assert N < 2 or not np.array_equal(wbs[0], wbs[1])
    ccms = (np.eye(3)[None] * rng.uniform(1.2, 1.7, size=(N, 1, 1)) + rng.uniform(-0.35, 0.1, size=(N, 3, 3))).astype(F32)
    return p, wbs, ccms


def dev(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()           # a copy: the shared references are read-only


def bits_equal(got, want):
    return got.shape == want.shape and got.dtype == want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


_REF = {}


def reference(h, w, pi):
    """(inputs, restatement with the matrix, restatement without) of one shape and pattern: computed once, shared, never written to"""
    if (h, w, pi) not in _REF:
        p, wbs, ccms = inputs(h, w, 100 + 7 * pi + h)
        m = D.mosaic_bayer(p, PATTERNS[pi], wbs)
        for n in range(p.shape[0]):
            assert m[n].min() == 0.0 and m[n].max() == 1.0           # both clamps, in every frame
        cam = E.linear_bayer_edge(p, PATTERNS[pi], wbs)
        lin = D.apply_ccm(cam, ccms)
        for a in (p, cam, lin):
            a.setflags(write=False)
        _REF[(h, w, pi)] = (p, wbs, ccms, lin, cam)
    return _REF[(h, w, pi)]


# ---- 1. linear output, bit for bit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', SMALL + [(17, 133), 'tile'])
def test_linear_equals_the_restatement(lib, hw):
    from eld_amd.isp import render_bayer
    h, w = tile_shape() if hw == 'tile' else hw
    for pi, pat in enumerate(PATTERNS):
        p, wbs, ccms, lin, cam = reference(h, w, pi)
        x = dev(p)
        got = render_bayer(x, pat, wbs, ccms, linear=True, demosaic='edge')
        assert got.dtype == torch.float32 and got.shape == (2, 3, 2 * h, 2 * w) and got.is_cuda
        assert bits_equal(got.cpu().numpy(), lin), pat
        assert bits_equal(render_bayer(x, pat, wbs, None, linear=True, demosaic='edge').cpu().numpy(), cam), pat      # camera RGB


# ---- 2. the 8-bit codes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', [(5, 7), (17, 133), 'tile'])
def test_srgb8_codes(lib, hw):
    """gamma 2.2 (the threshold table) and a CRF (float32 interpolation, one rounding per operation, as the restatement's): every code equal"""
    from eld_amd.isp import render_bayer
    h, w = tile_shape() if hw == 'tile' else hw
    for pi in ((0, 3) if hw == 'tile' else (1, 2)):
        pat = PATTERNS[pi]
        p, wbs, ccms, lin, _ = reference(h, w, pi)
        x = dev(p)
        got = render_bayer(x, pat, wbs, ccms, demosaic='edge').cpu().numpy()
        assert got.dtype == np.uint8 and got.shape == lin.shape
        want = D.srgb8(lin)
        print('gamma 2.2: %d of %d codes differ' % (int((got != want).sum()), want.size))
        assert np.array_equal(got, want)
        got = render_bayer(x, pat, wbs, ccms, CRF=CRF, demosaic='edge').cpu().numpy()
        want = D.srgb8(lin, CRF=CRF)
        print('CRF: %d of %d codes differ' % (int((got != want).sum()), want.size))
        assert np.array_equal(got, want)


# ---- 3. guarded, poisoned buffers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', [(1, 1), (5, 7), (17, 133), 'tile'])
def test_guarded_buffers(lib, hw):
    """every operand between guard bands, the outputs poisoned with 0xFF (NaN): nothing outside is written, every element inside is, no NaN"""
    from eld_amd import _lib as L
    h, w = tile_shape() if hw == 'tile' else hw
    pi = 2
    p, wbs, ccms, lin, _ = reference(h, w, pi)
    g = Guards()
    x, wb, cm = g.ro(dev(p), 'packed'), g.ro(dev(wbs), 'wbs'), g.ro(dev(ccms.reshape(2, 9)), 'ccms')
    o32 = g.new((2, 3, 2 * h, 2 * w), torch.float32, 'linear out')
    o8 = g.new((2, 3, 2 * h, 2 * w), torch.uint8, 'srgb out')
    pat = (ctypes.c_int * 4)(*np.asarray(PATTERNS[pi]).reshape(-1).tolist())
    for out, mode in ((o32, L.RENDER_LINEAR_F32), (o8, L.RENDER_SRGB8)):
        L.check(lib.eld_render_bayer_edge(L.dptr(x), pat, L.dptr(wb), L.dptr(cm), L.dptr(out), mode, 2, h, w, 2.2, None, None, 0, L.cur_stream()),
                'eld_render_bayer_edge')
    torch.cuda.synchronize()
    g.check()
    got = o32.cpu().numpy()
    assert not np.isnan(got).any()
    assert bits_equal(got, lin) and np.array_equal(o8.cpu().numpy(), D.srgb8(lin))


# ---- 4. agreement with the Malvar-He-Cutler render where both are exact ----------------------------------------------------------------------------
GAINS = np.array([0.75, 1.0, 1.5, 2.0], F32)


@pytest.mark.parametrize('pat', PATTERNS)
def test_constant_colour_gives_the_codes_of_the_mhc_render(lib, pat):
    """frames of one colour on the 2^-8 grid with gains from GAINS: both demosaics return the colour exactly, so both renders write one code"""
    from eld_amd.isp import render_bayer
    rng = np.random.default_rng(5)
    N = 4
    rgb = rng.integers(0, 257, size=(N, 3)).astype(F32) / F32(256)
    rgb[0] = (1.0, 0.0, 0.5)
    wbs = GAINS[rng.integers(0, 4, size=(N, 4))]
    wbs[:, 3] = wbs[:, 1]                                     # one green
    ccms = (np.eye(3)[None] * rng.uniform(1.2, 1.7, size=(N, 1, 1)) + rng.uniform(-0.35, 0.1, size=(N, 3, 3))).astype(F32)
    for h, w in ((1, 1), (2, 2), (37, 53)):
        p = np.ascontiguousarray(np.broadcast_to(rgb[:, list(D.CODE_COLOUR), None, None], (N, 4, h, w)))
        x = dev(p)
        for kw in (dict(), dict(CRF=CRF), dict(linear=True)):
            edge = render_bayer(x, pat, wbs, ccms, demosaic='edge', **kw)
            if h >= 2:
                assert torch.equal(edge, render_bayer(x, pat, wbs, ccms, **kw)), (h, w, sorted(kw))
            for n in range(N):
                for c in range(3):
                    assert float(edge[n, c].min()) == float(edge[n, c].max()), (h, w, n, c)       # ... also at 1 x 1, which MHC refuses


# ---- 5. behind the warp, denoise_raw, determinism ---------------------------------------------------------------------------------------------
def test_identity_warp_returns_the_unwarped_bits(lib):
    from eld_amd.dng_opcodes import Warp
    from eld_amd.isp import render_bayer
    h, w = 17, 133
    p, wbs, ccms, lin, _ = reference(h, w, 1)
    x = dev(p)
    ident = Warp(W.IDENTITY, 0.4871, 0.5123)
    for kw in (dict(), dict(CRF=CRF), dict(linear=True)):
        want = render_bayer(x, PATTERNS[1], wbs, ccms, demosaic='edge', **kw)
        got = render_bayer(x, PATTERNS[1], wbs, ccms, demosaic='edge', warp=ident, **kw)
        assert got.dtype == want.dtype and torch.equal(got.view(torch.uint8), want.view(torch.uint8)), sorted(kw)
    assert bits_equal(render_bayer(x, PATTERNS[1], wbs, ccms, demosaic='edge', warp=ident, linear=True).cpu().numpy(), lin)


def test_two_calls_return_identical_bytes(lib):
    from eld_amd.isp import render_bayer
    h, w = tile_shape()
    p, wbs, ccms, _, _ = reference(h, w, 3)
    x = dev(p)
    for kw in (dict(), dict(linear=True)):
        a = render_bayer(x, PATTERNS[3], wbs, ccms, demosaic='edge', **kw)
        b = render_bayer(x, PATTERNS[3], wbs, ccms, demosaic='edge', **kw)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_denoise_raw_end_to_end(lib, tmp_path):
    """denoise_raw(srgb_size='full', demosaic='edge') returns the edge render of its own written-back network output; the default is untouched"""
    from test_demosaic_gpu import CCM, WB4, make_opt, noisy_frame
    from eld_amd.denoise import denoise_raw, load_denoiser
    from eld_amd.isp import render_bayer
    from eld_amd.model import ELDModel
    torch.manual_seed(2022)
    m = ELDModel()
    m.initialize(make_opt(tmp_path, 4))
    m.save('latest')
    den = load_denoiser(os.path.join(m.save_dir, 'model_latest.pt'), cfa='bayer')
    del m
    pat = [[2, 3], [1, 0]]
    u = noisy_frame((2, 64, 96), 512, 1)
    kw = dict(raw_pattern=pat, black_level=512, ratio=40.0, wb=WB4, ccm=CCM, srgb_size='full')
    res = denoise_raw(den, u, 'bayer', linear=True, demosaic='edge', **kw)
    base = denoise_raw(den, u, 'bayer', linear=True, **kw)
    assert np.array_equal(res['mosaic'], base['mosaic']) and np.array_equal(res['packed'], base['packed'])
    assert res['srgb'].dtype == np.uint8 and res['srgb'].shape == (2, 3, 64, 96) and res['linear'].dtype == np.float32
    wbs = np.tile(np.asarray(WB4, np.float64) / WB4[1], (2, 1)).astype(F32)
    ccms = np.tile(CCM, (2, 1, 1))
    x = dev(res['packed'])
    assert np.array_equal(res['srgb'], render_bayer(x, pat, wbs, ccms, demosaic='edge').cpu().numpy())
    assert bits_equal(res['linear'], render_bayer(x, pat, wbs, ccms, linear=True, demosaic='edge').cpu().numpy())
    assert bits_equal(res['linear'], E.linear_bayer_edge(res['packed'], pat, wbs, ccms))
    assert np.array_equal(base['srgb'], render_bayer(x, pat, wbs, ccms).cpu().numpy())                      # the default: Malvar-He-Cutler, as before
    assert np.array_equal(denoise_raw(den, u, 'bayer', demosaic='mhc', **kw)['srgb'], base['srgb'])
    assert not np.array_equal(res['linear'], base['linear'])
