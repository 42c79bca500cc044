"""GPU tests of the validation step: eld_hist_u16 / eld_hist_f32 bit for bit against tests/validate_ref.py, the defect bitmap, the ELD_EINVAL
cases, and validate_camera end to end (exactly, statistically, on X-Trans and through the command line)."""
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from eld_amd import _lib as L
from eld_amd import validate as V

from test_calib_cpu import PATTERNS
from validate_ref import clean_from_flat_pair_ref, groups_f32, groups_u16, hist_f32_ref, hist_u16_ref
from xtrans_ref import xtrans_pattern

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XPAT = xtrans_pattern(g2=((1, 1), (4, 4)))
RADII = (1, 16, 256, 4096)
# the issue's sizes, then sizes whose width is a multiple of 8 (the 16-byte path of the kernel; none of the issue's is)
BAYER_SIZES = [(2, 2), (4, 6), (34, 50), (66, 130), (40, 258), (6, 8), (50, 136)]
XTRANS_SIZES = [(6, 6), (13, 20), (45, 262), (14, 24), (45, 264)]


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def hist_abi(u, p, group, G, centre, R, v=None, bitmap=None):
    """The raw ABI call on CUDA int16 tensors -> int64 ndarray (F,G,2R+1); the output starts as garbage: every counter must be written."""
    torch = _torch()
    F, Hm, Wm = u.shape
    counts = torch.full((F, G, 2 * R + 1), -7, dtype=torch.int64, device='cuda')
    cen = None if centre is None else (ctypes.c_int32 * G)(*[int(c) for c in centre])
    L.check(L.lib().eld_hist_u16(L.dptr(u), L.dptr(v), F, Hm, Wm, p, (ctypes.c_int * (p * p))(*[int(g) for g in group]), G, cen, R,
                                 L.dptr(bitmap), L.dptr(counts), L.cur_stream()), 'eld_hist_u16')
    return counts.cpu().numpy()


def laws(rng, F, Hm, Wm):
    """name -> (u, v): a constant frame (one bin: the contention extreme), rint(N(512, 3)), uniform over all 65536 codes (both end bins)."""
    shape = (F, Hm, Wm)
    return {'constant': (np.full(shape, 515, np.uint16), np.full(shape, 509, np.uint16)),
            'normal': tuple(np.clip(np.rint(rng.normal(512, 3, shape)), 0, 65535).astype(np.uint16) for _ in range(2)),
            'uniform': tuple(rng.integers(0, 65536, shape).astype(np.uint16) for _ in range(2))}


def check_u16(shape, F, p, group, G, centre, seed):
    rng = np.random.default_rng(seed)
    Hm, Wm = shape
    gm = np.asarray(group).reshape(p, p)[np.arange(Hm)[:, None] % p, np.arange(Wm)[None, :] % p]
    npix = np.array([(gm == g).sum() for g in range(G)])
    for name, (u, v) in laws(rng, F, Hm, Wm).items():
        ud, vd = _dev(u), _dev(v)
        for R in RADII:
            got = hist_abi(ud, p, group, G, centre, R)
            assert np.array_equal(got, hist_u16_ref(u, p, group, G, centre, R)), (name, R)
            assert np.array_equal(got.sum(axis=2), np.broadcast_to(npix, (F, G))), (name, R)
            got = hist_abi(ud, p, group, G, None, R, v=vd)
            assert np.array_equal(got, hist_u16_ref(u, p, group, G, None, R, v=v)), (name, R, 'subtract')
            assert np.array_equal(got.sum(axis=2), np.broadcast_to(npix, (F, G))), (name, R, 'subtract')


@pytest.mark.parametrize('F', [1, 3])
@pytest.mark.parametrize('shape', BAYER_SIZES)
@pytest.mark.parametrize('pattern', PATTERNS)
def test_hist_u16_bayer_equals_bincount(eld_lib, pattern, shape, F):
    p, gm, G = groups_u16('bayer', pattern)
    check_u16(shape, F, p, gm.reshape(-1).tolist(), G, [512, 510, 515, 513], 1000 * PATTERNS.index(pattern) + shape[0] + shape[1] + F)


@pytest.mark.parametrize('F', [1, 3])
@pytest.mark.parametrize('shape', XTRANS_SIZES)
def test_hist_u16_xtrans_equals_bincount(eld_lib, shape, F):
    p, gm, G = groups_u16('xtrans', XPAT)
    check_u16(shape, F, p, gm.reshape(-1).tolist(), G, [512, 510, 515], 77 + shape[0] + shape[1] + F)


def test_hist_u16_with_uncounted_cells(eld_lib):
    check_u16((34, 50), 2, 2, [1, -1, 0, 1], 2, [512, 500], 5)
    check_u16((50, 136), 1, 2, [-1, -1, 2, -1], 3, [1, 2, 512], 6)
    g6 = groups_u16('xtrans', XPAT)[1].reshape(-1).copy()
    g6[g6 == 1] = -1                                              # no green
    check_u16((45, 264), 2, 6, g6.tolist(), 3, [512, 0, 512], 7)


@pytest.mark.parametrize('shape', [(514, 1030), (520, 1024)])
def test_hist_u16_constant_frame_across_many_workgroups(eld_lib, shape):
    """F = 2 constant frames of 514 x 1030 (32-bit path) and 520 x 1024 (16-byte path): hundreds of workgroups add to one bin.  With every
    cell in one group the hot counter ends at 529 420 (532 480) > 2^19 per frame; per Bayer channel it is a quarter of that, > 2^16.
    (How many of these a single workgroup sees is the library's choice of grid; its LDS counters are 32 bits wide.)"""
    Hm, Wm = shape
    u = np.full((2, Hm, Wm), 512, np.uint16)
    ud = _dev(u)
    got = hist_abi(ud, 2, [0, 0, 0, 0], 1, [512], 256)
    assert got[:, 0, 256].tolist() == [Hm * Wm] * 2 and got.sum() == 2 * Hm * Wm and Hm * Wm > 2 ** 19
    got = hist_abi(ud, 2, [0, 1, 3, 2], 4, [512, 511, 512, 514], 256)
    assert np.array_equal(got, hist_u16_ref(u, 2, [0, 1, 3, 2], 4, [512, 511, 512, 514], 256)) and Hm * Wm // 4 > 2 ** 16


def test_hist_u16_every_radius_works(eld_lib):
    """R = 32767 with four groups is a 1 MiB table: no LDS stage, the lanes count in global memory.  R = 4859 / 4860: the last radius with an
    LDS table and the first without (4 x 9719 counters, padded to a stride of 1 modulo 32 words, are 152 KiB less 124 bytes)."""
    rng = np.random.default_rng(9)
    u = rng.integers(0, 65536, (2, 40, 264)).astype(np.uint16)
    for R in (32767, 4859, 4860):
        assert np.array_equal(hist_abi(_dev(u), 2, [0, 1, 3, 2], 4, [32768, 512, 0, 65535], R), hist_u16_ref(u, 2, [0, 1, 3, 2], 4, [32768, 512, 0, 65535], R))
    # counting in global memory on the other three load paths: Bayer 32-bit words, X-Trans 32-bit words, X-Trans 16-byte loads
    g6 = groups_u16('xtrans', XPAT)[1].reshape(-1).tolist()
    for p, group, centre, shape in ((2, [0, 1, 3, 2], [32768, 512, 0, 65535], (6, 130)), (6, g6, [32768, 512, 0], (12, 18)), (6, g6, [32768, 512, 0], (12, 24))):
        u = rng.integers(0, 65536, (2,) + shape).astype(np.uint16)
        assert np.array_equal(hist_abi(_dev(u), p, group, len(centre), centre, 32767), hist_u16_ref(u, p, group, len(centre), centre, 32767))


@pytest.mark.parametrize('shape,cfa', [((34, 50), 'bayer'), ((34, 64), 'bayer'), ((45, 264), 'xtrans'), ((13, 70), 'xtrans')])
def test_defect_bitmap_sites_are_not_counted(eld_lib, shape, cfa):
    from eld_amd.defects import pack_bitmap
    Hm, Wm = shape
    rng = np.random.default_rng(Hm + Wm)
    u = rng.integers(480, 545, (2, Hm, Wm)).astype(np.uint16)
    v = rng.integers(480, 545, (2, Hm, Wm)).astype(np.uint16)
    mask = rng.random((Hm, Wm)) < 0.03
    for y, x in ((0, 0), (0, Wm - 1), (Hm - 1, Wm - 1), (3, 31), (3, 32), (5, 31), (6, 32), (Hm - 1, 0)):
        mask[y, x] = True
    mask[2, 30:34] = False
    u[:, mask] = 7                                                # a flagged site that were counted would land in the low end bin
    p, gm, G = groups_u16(cfa, XPAT if cfa == 'xtrans' else PATTERNS[1])
    bm = _torch().from_numpy(pack_bitmap(mask).view(np.int32).copy()).cuda()
    centre = [512] * G
    got = hist_abi(_dev(u), p, gm.reshape(-1).tolist(), G, centre, 40, bitmap=bm)
    assert np.array_equal(got, hist_u16_ref(u, p, gm.reshape(-1), G, centre, 40, mask=mask))
    assert got[:, :, 0].sum() == 0 and got.sum() == 2 * int((~mask).sum())
    got = hist_abi(_dev(u), p, gm.reshape(-1).tolist(), G, None, 40, v=_dev(v), bitmap=bm)
    assert np.array_equal(got, hist_u16_ref(u, p, gm.reshape(-1), G, None, 40, v=v, mask=mask))


def test_histogram_u16_module_with_a_defect_map(eld_lib):
    from eld_amd.defects import DefectMap
    rng = np.random.default_rng(3)
    u = rng.integers(500, 525, (2, 34, 64)).astype(np.uint16)
    dm = DefectMap.from_sites([(0, 0), (5, 31), (5, 32), (33, 63)], (34, 64))
    got = V.histogram_u16(u, 'bayer', PATTERNS[2], [512] * 4, 16, defects=dm)
    assert got.dtype == np.int64 and np.array_equal(got, hist_u16_ref(u, 2, np.asarray(PATTERNS[2]).reshape(-1), 4, [512] * 4, 16, mask=dm.mask))
    got = V.histogram_u16(_dev(u), 'bayer', PATTERNS[2], None, 16, subtract=_dev(u[::-1].copy()))
    assert np.array_equal(got, hist_u16_ref(u, 2, np.asarray(PATTERNS[2]).reshape(-1), 4, None, 16, v=u[::-1]))


# ---- eld_hist_f32 ----------------------------------------------------------------------------------------------------------------------
def f32_values(rng, N, C, H, W, scales):
    """Normal values around the radius, then planted: exact k +- 0.5 after scaling (scales are powers of two), negatives, +-1e30, +-inf, NaN."""
    x = rng.normal(0, 6, (N, C, H, W)).astype(np.float32)
    special = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 7.5, -8.5, 1e30, -1e30, np.inf, -np.inf, np.nan, 3.0, -3.0], np.float32)
    for n in range(N):
        flat = x[n].reshape(-1)
        k = min(flat.size, special.size * 2)
        idx = rng.permutation(flat.size)[:k]
        flat[idx] = (np.resize(special, k) / np.float32(scales[n])).astype(np.float32)
    return x


@pytest.mark.parametrize('N', [1, 3])
@pytest.mark.parametrize('hw', [(1, 1), (3, 5), (17, 33), (64, 64), (96, 200)])
@pytest.mark.parametrize('C', [4, 9])
def test_hist_f32_equals_bincount(eld_lib, C, hw, N):
    torch = _torch()
    cfa = 'bayer' if C == 4 else 'xtrans'
    group, G = groups_f32(cfa)
    rng = np.random.default_rng(100 * C + hw[0] + N)
    scales = [2.0, 0.5, 4.0][:N]
    x, x2 = f32_values(rng, N, C, hw[0], hw[1], scales), f32_values(rng, N, C, hw[0], hw[1], scales)
    xd, x2d = torch.from_numpy(x).cuda(), torch.from_numpy(x2).cuda()
    for R in (1, 16, 256, 20000):                                 # 20000: a 156 KiB table, counted in global memory
        got = V.histogram_f32(xd, scales, R, cfa)
        assert got.dtype == np.int64 and got.shape == (N, G, 2 * R + 1)
        assert np.array_equal(got, hist_f32_ref(x, group, G, scales, R)), R
        got = V.histogram_f32(xd, scales, R, cfa, subtract=x2d)
        assert np.array_equal(got, hist_f32_ref(x, group, G, scales, R, x2=x2)), (R, 'subtract')


def test_hist_f32_skips_planes_of_group_minus_one(eld_lib):
    torch = _torch()
    rng = np.random.default_rng(4)
    x = rng.normal(0, 3, (2, 4, 17, 33)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    sc = torch.tensor([1.0, 3.0], device='cuda')
    counts = torch.full((2, 2, 33), -1, dtype=torch.int64, device='cuda')
    L.check(L.lib().eld_hist_f32(L.dptr(xd), None, 2, 4, 17, 33, (ctypes.c_int * 4)(1, -1, 0, 1), 2, L.dptr(sc), 16, L.dptr(counts), L.cur_stream()))
    assert np.array_equal(counts.cpu().numpy(), hist_f32_ref(x, [1, -1, 0, 1], 2, [1.0, 3.0], 16))


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
def test_einval_cases_on_device_pointers(eld_lib):
    torch = _torch()
    buf = torch.zeros(4 * 8 + 8, dtype=torch.int16, device='cuda')
    counts = torch.zeros((1, 4, 17), dtype=torch.int64, device='cuda')
    g = (ctypes.c_int * 4)(0, 1, 3, 2)
    c = (ctypes.c_int32 * 4)(512, 512, 512, 512)

    def call(u=buf.data_ptr(), Wm=8, p=2, group=g, G=4, R=8):
        return L.lib().eld_hist_u16(ctypes.c_void_p(u), None, 1, 4, Wm, p, group, G, c, R, None, L.dptr(counts), L.cur_stream())
    assert call() == 0
    assert call(Wm=7) == -1 and call(G=0) == -1 and call(G=5) == -1 and call(R=0) == -1 and call(p=3) == -1
    assert call(group=(ctypes.c_int * 4)(0, 1, 4, 2)) == -1
    assert call(u=buf.data_ptr() + 2) == -1                       # a view that starts at an odd element
    torch.cuda.synchronize()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
LAM, TL_SCALE = -0.25, 2.0
# standard deviation of Tukey-lambda(lam), lam > -1/2: var = (2 / lam^2) (1 / (1 + 2 lam) - Gamma(lam + 1)^2 / Gamma(2 lam + 2))
TL_SD = math.sqrt(2 / LAM ** 2 * (1 / (1 + 2 * LAM) - math.gamma(LAM + 1) ** 2 / math.gamma(2 * LAM + 2)))
BLACK, WHITE, BAYER = [512.0] * 4, 16383, [[0, 1], [3, 2]]
KS = (0.8, 3.0)


def _params(K, ncb=4):
    return {'K': K, 'g_scale': TL_SCALE * TL_SD, 'tl_lambda': LAM, 'tl_scale': TL_SCALE, 'row_scale': 0.0, 'color_bias': [0.0] * ncb}


def mint(id_of, cfa='bayer', packed=(4, 65, 97), nsess=2, F=3, ncb=4, black=BLACK):
    """Sessions of F 'real' bias frames of the law PG (Tukey-lambda(-0.25), scale 2 DN) minted by synthesize_codes at the ids id_of(s, f),
    one flat pair per session at 2000 DN under 'Pg', and the diag that names those parameters."""
    torch = _torch()
    sat = WHITE - max(black)
    sessions, frames = [], []
    for s in range(nsess):
        prm = _params(KS[s], ncb)
        bias = torch.stack([V.synthesize_codes(None, prm, 'PG', cfa, 2018, id_of(s, f), WHITE, black, shape=packed) for f in range(F)])
        clean = np.full(packed, 2000.0 / sat, np.float32)
        flats = torch.stack([V.synthesize_codes(clean, prm, 'Pg', cfa, 2018, 900000 + 10 * s + d, WHITE, black) for d in range(2)])[None]
        sessions.append({'iso': 100 * (s + 1), 'bias': bias.cpu().numpy(), 'flats': flats.cpu().numpy()})
        frames += [{'session': s, 'iso': 100 * (s + 1), 'K': KS[s], 'lambda': LAM, 'G_scale': TL_SCALE, 'R_scale': 0.0,
                    'g_scale': TL_SCALE * TL_SD, 'color_bias': np.zeros(ncb)} for _ in range(F)]
    return sessions, {'frames': frames, 'K': np.array(KS[:nsess])}


def test_end_to_end_exact(eld_lib):
    """Frames minted at the very ids validate_camera draws at, under the model and parameters it is told: the 'PG' histogram of draw 0 IS the
    real one, so kl is exactly 0.0 -- scale, centre, rounding and the id layout agree through every layer."""
    sessions, diag = mint(lambda s, f: V.sample_id(s, f, 1, 0))
    assert sessions[0]['bias'].shape == (3, 130, 194) and sessions[0]['bias'].dtype == np.uint16
    rep = V.validate_camera(sessions, BAYER, BLACK, WHITE, models=('Pg', 'PG'), source='frames', diag=diag, keep_hist=True)
    for s in rep['sessions']:
        assert len(s['frames']) == 3
        for fr in s['frames']:
            assert fr['models']['PG']['kl'] == 0.0 and fr['models']['PG']['kl_groups'] == [0.0] * 4
            assert fr['models']['Pg']['kl'] > 0 and fr['models']['PG']['floor'] > 0
        assert all(np.isfinite(p['models'][m]['kl_flat']) and p['models'][m]['kl_flat'] >= 0 for p in s['flats'] for m in ('Pg', 'PG'))
    assert rep['best'] == 'PG' and rep['radius'] == 256 and rep['alpha'] == 1.0 and rep['seed'] == 2018
    h = rep['hist']
    assert np.array_equal(h['s0_real'][1], h['s0_f1_PG'][0]) and h['s0_real'].sum() == 3 * 130 * 194
    json.dumps(V.to_jsonable({k: v for k, v in rep.items() if k != 'hist'}))


def test_end_to_end_statistical(eld_lib):
    """The same law at OTHER ids: 'PG' is now a fresh draw of the right law, 'Pg' a Gaussian of the same standard deviation.
    The factor 4 is a condition, not a measurement: on the CPU, Tukey-lambda(-0.25, scale 2) against a Gaussian of its standard deviation gave
    KL ~ 0.09-0.10 against 0.004 for a fresh draw at n = 24 576 (add-one smoothing, R = 256, 5 seeds): a ratio of 23 and more; a frame of
    130 x 194 has 25 220 pixels, 6 305 per Bayer channel."""
    sessions, diag = mint(lambda s, f: V.sample_id(s + 8, f, 1, 0))
    rep = V.validate_camera(sessions, BAYER, BLACK, WHITE, models=('Pg', 'PG'), source='frames', diag=diag)
    for s in rep['sessions']:
        for fr in s['frames']:
            m = fr['models']
            print('kl PG %.5f  kl Pg %.5f  floor PG %.5f  floor Pg %.5f' % (m['PG']['kl'], m['Pg']['kl'], m['PG']['floor'], m['Pg']['floor']))
            assert 0 < m['PG']['kl'] and m['PG']['kl'] * 4 < m['Pg']['kl']
            for k in ('Pg', 'PG'):
                assert 0 < m[k]['floor'] < m['Pg']['kl']
    assert rep['best'] == 'PG'


def test_flat_clean_image_equals_the_restatement(eld_lib):
    """clip((((a + b) / 2 - black_c) - cb_c) / sat, 0, 1) in float32 against tests/validate_ref.py: the subtraction chain is exact-per-op, the
    division may differ by its last bit (the device's float32 division need not be correctly rounded): one ulp, rtol 2^-23."""
    rng = np.random.default_rng(12)
    a, b = rng.integers(400, 16384, (2, 34, 50)).astype(np.uint16)
    blk, cb, sat = [512.0, 511.5, 500.0, 512.0], [0.25, -1.5, 0.0, 2.0], 15871.0
    for pat in PATTERNS:
        got = V.clean_from_flat_pair(_dev(a), _dev(b), 'bayer', pat, blk, cb, sat).cpu().numpy()
        ref = clean_from_flat_pair_ref(a, b, 'bayer', pat, blk, cb, sat)
        assert got.shape == ref.shape == (4, 17, 25) and got.dtype == np.float32
        np.testing.assert_allclose(got, ref, rtol=2.0 ** -23, atol=0)
    a, b = rng.integers(400, 16384, (2, 48, 66)).astype(np.uint16)
    got = V.clean_from_flat_pair(_dev(a), _dev(b), 'xtrans', XPAT, [1024.0, 1023.0, 1022.0, 1023.0], [0.5, -0.5, 1.0], 15359.0).cpu().numpy()
    ref = clean_from_flat_pair_ref(a, b, 'xtrans', XPAT, [1024.0, 1023.0, 1022.0, 1023.0], [0.5, -0.5, 1.0], 15359.0)
    assert got.shape == ref.shape == (9, 16, 22)
    np.testing.assert_allclose(got, ref, rtol=2.0 ** -23, atol=0)


def test_xtrans_smoke(eld_lib):
    black = [1024.0] * 4
    sessions, diag = mint(lambda s, f: V.sample_id(s + 3, f, 1, 0), cfa='xtrans', packed=(9, 16, 22), nsess=1, F=2, ncb=3, black=black)
    assert sessions[0]['bias'].shape == (2, 48, 66)
    rep = V.validate_camera(sessions, XPAT, black, WHITE, models=('Pg', 'PGR'), diag=diag, cfa='xtrans', radius=64, flat_radius=512)
    assert rep['groups'] == 3 and rep['cfa'] == 'xtrans' and len(rep['sessions']) == 1
    for fr in rep['sessions'][0]['frames']:
        for m in ('Pg', 'PGR'):
            assert len(fr['models'][m]['kl_groups']) == 3 and np.all(np.isfinite(fr['models'][m]['kl_groups'])) and np.isfinite(fr['models'][m]['floor'])
    assert np.isfinite(rep['means']['PGR']['kl_flat']) and rep['best'] in ('Pg', 'PGR')


def test_cli_writes_the_report(eld_lib, tmp_path):
    from test_calib_gpu import SAMPLER_PATTERN, make_sessions
    sessions = make_sessions()
    man = {'raw_pattern': SAMPLER_PATTERN, 'black_level': [512.0] * 4, 'white_level': 16383, 'sessions': []}
    for i, s in enumerate(sessions):
        ent = {'iso': s['iso'], 'bias': [], 'flats': []}
        for f in range(s['bias'].shape[0]):
            np.save(tmp_path / ('b%d_%d.npy' % (i, f)), s['bias'][f])
            ent['bias'].append('b%d_%d.npy' % (i, f))
        for j in range(s['flats'].shape[0]):
            names = ['f%d_%d%s.npy' % (i, j, ab) for ab in 'ab']
            for k, nm in enumerate(names):
                np.save(tmp_path / nm, s['flats'][j, k])
            ent['flats'].append(names)
        man['sessions'].append(ent)
    (tmp_path / 'manifest.json').write_text(json.dumps(man))
    out, hist = tmp_path / 'report.json', tmp_path / 'hist.npz'
    r = subprocess.run([sys.executable, '-m', 'eld_amd.validate', str(tmp_path / 'manifest.json'), '--models', 'Pg,PGR', '--radius', '128',
                        '--out', str(out), '--hist', str(hist)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rep = json.loads(out.read_text())
    here = V.validate_camera([{k: s[k] for k in ('iso', 'bias', 'flats')} for s in sessions], SAMPLER_PATTERN, [512.0] * 4, 16383,
                             models=('Pg', 'PGR'), radius=128)
    assert rep['best'] == here['best'] and 'best model: %s' % here['best'] in r.stdout
    assert rep['means'] == V.to_jsonable(here['means']) and rep['radius'] == 128 and len(rep['sessions']) == 5
    assert r.stdout.count('session ') == 10
    with np.load(hist, allow_pickle=False) as z:
        assert z['s0_real'].shape == (sessions[0]['bias'].shape[0], 4, 257)
