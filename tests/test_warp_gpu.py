"""GPU tests of DNG WarpRectilinear (csrc/warp.hip through eld_amd.isp.warp_rgb) against the NumPy restatement tests/warp_ref.py, bit for bit,
and of the warp through the renders and the command lines.

Shapes (Hm, Wm), the smallest at which the kernel can go wrong: 5 x 7 (smaller than the 4 x 4 footprint's reach: every tap clamps somewhere,
one workgroup mostly outside the image), 33 x 70 (odd, one row and six columns into a second tile in each direction), 96 x 160 with N = 2
(3 x 3 tiles, two frames; large enough for the violent case's source boxes to exceed even the largest LDS budget, so that launch runs both
paths)."""
import functools
import json
import os

import numpy as np
import pytest

import dng_opcodes_ref as R
import dng_ref as DR
import demosaic_ref as DM
import warp_ref as W
from guarded import Guards

pytestmark = pytest.mark.gpu

SHAPES = ((1, 5, 7), (1, 33, 70), (2, 96, 160))
MIXED = (0.96, 0.06, -0.01, 0.002, 0.001, -0.001)
THREE = ((1.002, 0.01, 0.0, 0.0, 0.0, 0.0), (1.0, 0.01, 0.0, 0.0, 0.0, 0.0), (0.998, 0.01, 0.0, 0.0, 0.0, 0.0))
CASES = {'identity': (W.IDENTITY, 0.5, 0.5), 'barrel': ((1.0, 0.05, 0.0, 0.0, 0.0, 0.0), 0.5, 0.5), 'mixed': (MIXED, 0.47, 0.53),
         'three': (THREE, 0.5, 0.5), 'violent': ((3.0, 0.0, 0.0, 0.0, 0.0, 0.0), 0.5, 0.5)}
CM = ((8000, 10000), (-2000, 10000), (-500, 10000), (-3000, 10000), (11000, 10000), (2000, 10000), (-500, 10000), (1500, 10000), (6000, 10000))
BUDGETS = (-1, 0, 65536)


@pytest.fixture(scope='module')
def isp(eld_lib):
    import torch
    if not torch.cuda.is_available():
        pytest.fail('these tests need a GPU')
    from eld_amd import isp
    return isp


def O():
    from eld_amd import dng_opcodes
    return dng_opcodes


@functools.lru_cache(maxsize=None)
def frames(N, Hm, Wm):
    """(camera RGB in [-0.1, 1.1], per-frame matrices), computed once and left unchanged"""
    rng = np.random.default_rng(1000 * Hm + Wm)
    rgb = rng.uniform(-0.1, 1.1, (N, 3, Hm, Wm)).astype(np.float32)
    ccms = (np.eye(3)[None] * rng.uniform(1.2, 1.7, size=(N, 1, 1)) + rng.uniform(-0.35, 0.1, size=(N, 3, 3))).astype(np.float32)
    rgb.setflags(write=False)
    ccms.setflags(write=False)
    return rgb, ccms


@functools.lru_cache(maxsize=None)
def resampled(name, N, Hm, Wm):
    """the restatement's resampled planes of a case, before the tail; computed once"""
    sets, cx, cy = CASES[name]
    out = W.warp(frames(N, Hm, Wm)[0], sets, cx, cy)
    out.setflags(write=False)
    return out


def expected(name, N, Hm, Wm, linear, with_ccm):
    w, ccms = resampled(name, N, Hm, Wm), frames(N, Hm, Wm)[1]
    if linear:
        return DM.apply_ccm(w, ccms) if with_ccm else w
    eye = np.tile(np.eye(3, dtype=np.float32).reshape(1, 9), (N, 1))
    return DM.srgb8(DM.apply_ccm(w, ccms if with_ccm else eye))


def same_bits(t, want):
    a, b = t.cpu().numpy(), np.ascontiguousarray(want)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class budget:
    """eld_amd.isp.WARP_LDS_BYTES for the length of a with block"""
    def __init__(self, isp, value):
        self.isp, self.value = isp, value

    def __enter__(self):
        self.old, self.isp.WARP_LDS_BYTES = self.isp.WARP_LDS_BYTES, self.value

    def __exit__(self, *exc):
        self.isp.WARP_LDS_BYTES = self.old


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
@pytest.mark.parametrize('name', sorted(CASES))
def test_warp_matches_the_restatement_on_both_paths(isp, name, shape):
    """LINEAR and SRGB8, with and without a CCM, at the default LDS budget, with the direct path forced (0) and staged at the cap (65536)"""
    import torch
    N, Hm, Wm = shape
    rgb, ccms = frames(N, Hm, Wm)
    sets, cx, cy = CASES[name]
    warp = O().Warp(sets, cx, cy)
    x = torch.from_numpy(rgb.copy()).cuda()
    if name == 'violent':                                            # most coordinates leave the image and are clamped to the replicated edge
        rec = W.record(sets, cx, cy, Hm, Wm)
        u, v = W.coords(rec['k'][0], rec, Hm, Wm)
        assert ((u < -1) | (u > Wm) | (v < -1) | (v > Hm)).mean() > 0.5
    for linear in (True, False):
        for with_ccm in (True, False):
            want = expected(name, N, Hm, Wm, linear, with_ccm)
            for b in BUDGETS:
                with budget(isp, b):
                    got = isp.warp_rgb(x, warp, ccms.copy() if with_ccm else None, linear=linear)
                assert got.dtype == (torch.float32 if linear else torch.uint8) and tuple(got.shape) == (N, 3, Hm, Wm)
                assert same_bits(got, want), (name, shape, linear, with_ccm, b)


def test_the_violent_case_exceeds_the_lds_budget():
    """what makes the direct path run beside the staged one at the largest budget: the centre tile of 96 x 160 under kr0 = 3 samples a box of more
    than 64 KiB"""
    Hm, Wm = 96, 160
    sets, cx, cy = CASES['violent']
    rec = W.record(sets, cx, cy, Hm, Wm)
    u, v = W.coords(rec['k'][0], rec, Hm, Wm)
    i0, _ = W.cell(v[32:64, 64:128], Hm)
    j0, _ = W.cell(u[32:64, 64:128], Wm)
    box = (int(i0.max() - i0.min()) + 4) * (int(j0.max() - j0.min()) + 4)
    assert 3 * 4 * box > 65536
    i0, _ = W.cell(v[:32, :64], Hm)                                  # ... and the corner tile's box is small: the staged path runs in the same launch
    j0, _ = W.cell(u[:32, :64], Wm)
    assert 3 * 4 * (int(i0.max() - i0.min()) + 4) * (int(j0.max() - j0.min()) + 4) < 65536


def test_three_sets_are_three_one_set_warps(isp):
    import torch
    N, Hm, Wm = 2, 96, 160
    rgb, _ = frames(N, Hm, Wm)
    x = torch.from_numpy(rgb.copy()).cuda()
    sets = (MIXED, (1.0, 0.05, 0.0, 0.0, 0.0, 0.0), (1.01, -0.03, 0.01, 0.0, -0.002, 0.001))
    got = isp.warp_rgb(x, O().Warp(sets, 0.47, 0.53), linear=True)
    for c in range(3):
        one = isp.warp_rgb(x, O().Warp(sets[c], 0.47, 0.53), linear=True)
        assert same_bits(got[:, c], one[:, c].cpu().numpy()), c
    assert same_bits(got, W.warp(rgb, sets, 0.47, 0.53))


def test_guard_bytes_and_the_empty_batch(isp, eld_lib):
    import ctypes
    import torch
    from eld_amd import _lib as L
    N, Hm, Wm = 1, 33, 70
    rgb, ccms = frames(N, Hm, Wm)
    g = Guards()
    x = g.ro(torch.from_numpy(rgb.copy()).cuda(), 'rgb')
    m = g.ro(torch.from_numpy(ccms.copy()).cuda().reshape(N, 9), 'ccms')
    rec = O().Warp(MIXED, 0.47, 0.53).record(Hm, Wm)
    for mode, dtype, linear in ((L.RENDER_SRGB8, torch.uint8, False), (L.RENDER_LINEAR_F32, torch.float32, True)):
        for b in BUDGETS:
            out = g.new((N, 3, Hm, Wm), dtype, 'out mode %d budget %d' % (mode, b))

            def call(n):
                return eld_lib.eld_warp_rgb_f32(L.dptr(x), L.dptr(out), mode, n, Hm, Wm, ctypes.c_void_p(rec.ctypes.data), L.dptr(m), 2.2, None, None, 0, b,
                                                L.cur_stream())
            assert call(0) == 0
            torch.cuda.synchronize()
            assert bool((out.view(torch.uint8) == 0xFF).all())       # N = 0 writes nothing: the buffer is as the guard filled it
            assert call(N) == 0
            torch.cuda.synchronize()
            g.check()
            assert same_bits(out, expected('mixed', N, Hm, Wm, linear, True))
    # out right behind rgb and right in front of it, in one arena: no overlap, accepted, and the operand unchanged
    arena = g.new((2, N, 3, Hm, Wm), torch.float32, 'rgb and out side by side')
    arena[0].copy_(x)
    assert eld_lib.eld_warp_rgb_f32(L.dptr(arena[0]), L.dptr(arena[1]), L.RENDER_LINEAR_F32, N, Hm, Wm, ctypes.c_void_p(rec.ctypes.data), L.dptr(m), 2.2,
                                    None, None, 0, -1, L.cur_stream()) == 0
    torch.cuda.synchronize()
    g.check()
    assert same_bits(arena[1], expected('mixed', N, Hm, Wm, True, True)) and same_bits(arena[0], rgb)
    assert eld_lib.eld_warp_rgb_f32(L.dptr(arena[0]), L.dptr(arena[0]), L.RENDER_LINEAR_F32, N, Hm, Wm, ctypes.c_void_p(rec.ctypes.data), L.dptr(m), 2.2,
                                    None, None, 0, -1, L.cur_stream()) == -1        # in place is refused


def test_a_nan_pixel_reaches_its_footprints_only(isp):
    import torch
    N, Hm, Wm = 1, 33, 70
    rgb = frames(N, Hm, Wm)[0].copy()
    sites = ((0, 0, 0), (1, 16, 35), (2, 32, 69), (1, 20, 63))        # (plane, y, x): corners, the middle, a tile's last column
    for c, y, x in sites:
        rgb[0, c, y, x] = np.nan
    xin = torch.from_numpy(rgb).cuda()
    for name in ('identity', 'mixed', 'three'):
        sets, cx, cy = CASES[name]
        want = W.warp(rgb, sets, cx, cy)
        rec = W.record(sets, cx, cy, Hm, Wm)
        for b in (-1, 65536):
            with budget(isp, b):
                got = isp.warp_rgb(xin, O().Warp(sets, cx, cy), linear=True).cpu().numpy()
            assert np.array_equal(np.isnan(got), np.isnan(want)), name
            assert np.array_equal(got[~np.isnan(want)].view(np.uint32), want[~np.isnan(want)].view(np.uint32)), name
        for c in range(3):                                           # the restatement's NaNs are the pixels whose 4 x 4 footprint holds a NaN site
            u, v = W.coords(rec['k'][c if len(rec['k']) == 3 else 0], rec, Hm, Wm)
            rows, cols = W.footprint(u, v, Hm, Wm)
            hit = np.zeros((Hm, Wm), bool)
            for pc, y, x in sites:
                if pc == c:
                    hit |= (rows == y).any(0) & (cols == x).any(0)
            assert np.array_equal(np.isnan(want[0, c]), hit) and hit.sum() >= 4, (name, c)


# ---- the identity ties the tail to the renders ------------------------------------------------------------------------------------------------
def packed_inputs(N, planes, h, w, seed, gains):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.2, 1.3, size=(N, planes, h, w)).astype(np.float32)
    wbs = rng.uniform(0.7, 2.2, size=(N, gains)).astype(np.float32)
    ccms = (np.eye(3)[None] * rng.uniform(1.2, 1.7, size=(N, 1, 1)) + rng.uniform(-0.35, 0.1, size=(N, 3, 3))).astype(np.float32)
    return p, wbs, ccms


@pytest.mark.parametrize('cfa', ('bayer', 'xtrans'))
def test_identity_warp_gives_the_renders_own_output(isp, cfa):
    """warp_rgb(render(x, no matrix, linear), identity, ccm) == render(x, ccm): as uint8 codes (gamma 2.2, another gamma, a CRF) and as float32"""
    import torch
    pat = [[2, 3], [1, 0]]
    if cfa == 'bayer':
        p, wbs, ccms = packed_inputs(2, 4, 45, 67, 7, 4)
        render = lambda c, **kw: isp.render_bayer(x, pat, wbs, c, **kw)
    else:
        p, wbs, ccms = packed_inputs(2, 9, 30, 44, 8, 3)
        render = lambda c, **kw: isp.render_xtrans(x, wbs, c, **kw)
    x = torch.from_numpy(p).cuda()
    cam = render(None, linear=True)
    ident = O().Warp(W.IDENTITY, 0.4871, 0.5123)
    E = np.linspace(0, 1, 1024, dtype=np.float32)
    for kw in (dict(), dict(gamma=2.7), dict(CRF=(E, (E ** 0.45).astype(np.float32))), dict(linear=True)):
        want = render(ccms, **kw)
        for b in (-1, 65536):
            with budget(isp, b):
                assert same_bits(isp.warp_rgb(cam, ident, ccms, **kw), want.cpu().numpy()), (cfa, sorted(kw), b)
        assert same_bits(render(ccms, warp=ident, **kw), want.cpu().numpy()), (cfa, sorted(kw))        # the renders' own warp= goes the same way
    assert same_bits(isp.warp_rgb(cam, ident, None, linear=True), cam.cpu().numpy())
    # and a real warp through the renders is the restatement on the linear render
    sets, cx, cy = CASES['mixed']
    got = render(ccms, warp=O().Warp(sets, cx, cy))
    assert same_bits(got, W.warp_srgb8(cam.cpu().numpy(), sets, cx, cy, ccms))
    with pytest.raises(ValueError, match='cam2rgbs'):
        render(None, warp=ident)
    with pytest.raises(ValueError, match='Warp'):
        isp.warp_rgb(cam, {'sets': W.IDENTITY}, ccms)
    with pytest.raises(ValueError, match='CUDA'):
        isp.warp_rgb(cam.cpu(), ident, ccms)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
AA = (2, 4, 50, 68)                                                  # the visible mosaic is 48 x 64 of a stored 52 x 70
E2E = ((0.97, 0.05, -0.01, 0.0, 0.002, -0.001), 0.48, 0.53)


@pytest.fixture(scope='module')
def dng_file(isp, tmp_path_factory):
    d = tmp_path_factory.mktemp('warp')
    rng = np.random.default_rng(4)
    yy, xx = np.mgrid[0:52, 0:70]
    img = np.clip(900 + 600 * np.sin(xx / 5.0) * np.cos(yy / 7.0) + rng.normal(0, 20, (52, 70)), 512, 4095).astype(np.uint16)
    specs3 = [{'id': 3, 'flags': 0, 'k': (0.3, -0.1, 0.0, 0.0, 0.0), 'cx': 0.5, 'cy': 0.5}, W.spec(*E2E)]
    info = DR.write_dng_file(str(d / 'f.dng'), img, bits=12, compression=7, tile=(16, 32), ljpeg=dict(P=12, geometry='nf2'),
                             tags={50714: (DR.SHORT, (512,)), 50717: (DR.LONG, (4095,)), 50829: (DR.LONG, AA),
                                   51022: (DR.UNDEFINED, R.pack_list(specs3))},
                             tags0={50728: (DR.RATIONAL, ((1, 2), (1, 1), (2, 3))), 50721: (DR.SRATIONAL, CM), 50778: (DR.SHORT, (21,))})
    return {'dir': d, 'path': info['path'], 'visible': img[AA[0]:AA[2], AA[1]:AA[3]].copy(), 'specs3': specs3}


def test_denoise_command_line_warps_the_render_only(isp, dng_file):
    """classical.main (no checkpoint) on a DNG whose list 3 holds a warp: --warp opcodes against the restatement on the unwarped linear render"""
    import torch
    import eld_amd.dng as D
    from eld_amd import classical, denoise
    d = dng_file['dir']
    args = ['--method', 'nlm', '--K', '2.0', '--sigma', '3.0', '--srgb-size', 'full', '--dng']
    runs = {'plain': [dng_file['path']], 'warp': [dng_file['path'], '--warp', 'opcodes'],
            'apply': [dng_file['path'], '--opcodes', 'apply'], 'both': [dng_file['path'], '--opcodes', 'apply', '--warp', 'opcodes']}
    wfile = str(d / 'warp.json')
    with open(wfile, 'w') as fh:
        json.dump({'sets': [list(E2E[0])], 'cx': E2E[1], 'cy': E2E[2]}, fh)
    runs['file'] = [dng_file['path'], '--warp', wfile]
    outs = {}
    for name, argv in runs.items():
        out = str(d / ('out_' + name))
        assert classical.main(argv + ['-o', out] + args) == 0
        outs[name] = {k: np.load(os.path.join(out, 'f_%s.npy' % k)) for k in ('denoised', 'srgb')}
    # the written-back mosaic is not warped; neither is the raw frame --dng writes, which still carries list 3 with its warp
    assert np.array_equal(outs['warp']['denoised'], outs['plain']['denoised']) and np.array_equal(outs['both']['denoised'], outs['apply']['denoised'])
    assert not np.array_equal(outs['warp']['srgb'], outs['plain']['srgb']) and not np.array_equal(outs['both']['srgb'], outs['apply']['srgb'])
    assert np.array_equal(outs['file']['srgb'], outs['warp']['srgb'])
    source = O().read_opcodes(dng_file['path'])
    for name in ('warp', 'both'):
        carried = O().read_opcodes(os.path.join(str(d / ('out_' + name)), 'f_denoised.dng'))
        assert carried[2] == source[2] and carried[2][1].id == 1 and carried[2][1].data == W.pack_params(*E2E), name
        back, _ = D.read_dng(os.path.join(str(d / ('out_' + name)), 'f_denoised.dng'))
        assert np.array_equal(back, outs[name]['denoised'])
    assert O().read_opcodes(os.path.join(str(d / 'out_plain'), 'f_denoised.dng'))[2] == []       # without either option nothing is carried, as before
    # the prediction: the same denoiser through denoise_raw, no warp -> its packed output -> camera RGB -> the restatement with the file's matrix
    a = classical.parse_method_args(classical.build_parser(), runs['plain'] + ['-o', str(d / 'unused')] + args)
    o = denoise.options_from(a)[3]
    den = classical.ClassicalDenoiser('bayer', 2.0, sigma=3.0, camera=None, search=a.search, patch=a.patch, strength=a.strength, method='nlm', step=a.step,
                                      group=a.group, mix=None)
    kw = {k: o.get(k) for k in ('raw_pattern', 'black_level', 'white_point', 'ratio', 'wb', 'ccm', 'chop', 'rounding', 'srgb_size')}
    res = denoise.denoise_raw(den, dng_file['visible'], 'bayer', **kw)
    assert np.array_equal(np.moveaxis(res['srgb'], 1, -1)[0], outs['plain']['srgb'])           # the command without --warp matches the API without warp
    wbs, ccms = denoise.colour_args('bayer', o['wb'], o['ccm'], 1)
    pat = np.asarray(o['raw_pattern']).reshape(-1).tolist()
    cam = isp.render_bayer(torch.from_numpy(res['packed']).cuda(), pat, wbs, None, linear=True).cpu().numpy()
    want = W.warp_srgb8(cam, E2E[0], E2E[1], E2E[2], ccms)
    assert np.array_equal(np.moveaxis(want, 1, -1)[0], outs['warp']['srgb'])
    assert (want != res['srgb']).mean() > 0.2                         # the warp moves this picture
    # denoise_raw with warp= and linear=True returns the warped linear RGB too
    res_w = denoise.denoise_raw(den, dng_file['visible'], 'bayer', linear=True, warp=O().Warp(*E2E), **kw)
    assert np.array_equal(res_w['srgb'], want) and np.array_equal(res_w['mosaic'], res['mosaic'])
    assert np.array_equal(res_w['linear'].view(np.uint32), W.warp_linear(cam, E2E[0], E2E[1], E2E[2], ccms).view(np.uint32))
    with pytest.raises(ValueError, match='.dng inputs'):
        np.save(str(d / 'g.npy'), dng_file['visible'])
        classical.main([str(d / 'g.npy'), '--warp', 'opcodes', '--wb', '2', '1', '1.5', '--ccm', '1', '0', '0', '0', '1', '0', '0', '0', '1', '-o', str(d / 'x')] + args)
