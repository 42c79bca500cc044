"""CPU tests of eld_amd.validate: the KL divergence, the reference binning rules (tests/validate_ref.py), the sample-id layout, every argument
error (reached before any device work) and the ABI of the histogram entry points."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from eld_amd import validate as V

from validate_ref import bincount_groups, clean_from_flat_pair_ref, groups_f32, groups_u16, hist_f32_ref, hist_u16_ref, kl_ref, quant_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RGGB = [[0, 1], [3, 2]]


# ---- kl_divergence ---------------------------------------------------------------------------------------------------------------------
def test_kl_of_a_histogram_with_itself_is_exactly_zero():
    rng = np.random.default_rng(0)
    n = rng.integers(0, 1000, (3, 4, 65))
    for alpha in (1.0, 0.5, 1e-3):
        assert np.all(V.kl_divergence(n, n, alpha) == 0.0)
    assert np.all(V.kl_divergence(n + 1, n + 1, 0.0) == 0.0)


def test_kl_three_bins_by_hand():
    """p counts (1, 2, 1), q counts (2, 1, 1), alpha = 1, B = 3: p = (2, 3, 2) / 7, q = (3, 2, 2) / 7, so
    KL = 2/7 ln(2/3) + 3/7 ln(3/2) + 2/7 ln 1 = (1/7) ln(3/2) = 0.057923586874..."""
    got = V.kl_divergence([1, 2, 1], [2, 1, 1])
    assert abs(got - math.log(1.5) / 7) < 1e-15
    assert abs(got - 0.05792358687) < 1e-10
    assert abs(kl_ref([1, 2, 1], [2, 1, 1]) - got) < 1e-15


def test_kl_is_asymmetric_and_matches_the_restatement():
    # alpha = 0: p = (3/4, 1/4), q = (1/2, 1/2): KL(p||q) = 3/4 ln(3/2) + 1/4 ln(1/2), KL(q||p) = 1/2 ln(2/3) + 1/2 ln 2
    a = V.kl_divergence([3, 1], [1, 1], alpha=0.0)
    b = V.kl_divergence([1, 1], [3, 1], alpha=0.0)
    assert abs(a - (0.75 * math.log(1.5) + 0.25 * math.log(0.5))) < 1e-15
    assert abs(b - (0.5 * math.log(2 / 3) + 0.5 * math.log(2))) < 1e-15
    assert a != b
    rng = np.random.default_rng(1)
    p, q = rng.integers(0, 50, (2, 3, 33)), rng.integers(0, 50, (2, 3, 33))
    np.testing.assert_allclose(V.kl_divergence(p, q, 1.0), kl_ref(p, q, 1.0), rtol=1e-12, atol=1e-15)
    assert V.kl_divergence(p, q).shape == (2, 3) and np.all(V.kl_divergence(p, q) > 0)
    assert V.kl_divergence([0, 4, 0], [1, 2, 1], alpha=0.0) == pytest.approx(math.log(2))     # 0 log 0 = 0


def test_kl_value_errors():
    with pytest.raises(ValueError, match='infinite'):
        V.kl_divergence([1, 1, 1], [1, 0, 1], alpha=0.0)
    with pytest.raises(ValueError):
        V.kl_divergence([1, 1], [1, 1], alpha=-1.0)
    with pytest.raises(ValueError):
        V.kl_divergence([0, 0], [1, 1], alpha=0.0)
    with pytest.raises(ValueError):
        V.kl_divergence([1, 1, 1], [1, 1])
    with pytest.raises(ValueError):
        V.kl_divergence([1, -1], [1, 1])
    assert V.kl_divergence([1, 1, 1], [1, 0, 1], alpha=1.0) > 0      # smoothed: finite


# ---- the reference binning -------------------------------------------------------------------------------------------------------------
def test_reference_rounds_ties_to_even_and_clamps():
    q, nan = quant_ref(np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.25, np.nan, np.inf, -np.inf, 1e30, -1e30], np.float32), 1.0)
    assert q[:7].tolist() == [0, 2, 2, 0, -2, -2, 0]
    assert nan.tolist() == [False] * 7 + [True] + [False] * 4
    assert q[8] == 2 ** 29 and q[9] == -2 ** 29 and q[10] == 2 ** 29 and q[11] == -2 ** 29
    q, _ = quant_ref(np.array([0.25, 0.75, 1.25], np.float32), 2.0)              # exact k + 0.5 after scaling
    assert q.tolist() == [0, 2, 2]
    x = np.array([0.5, 2.5, -7.0, 9.0, np.nan, np.inf, -np.inf, 1.0], np.float32).reshape(1, 4, 1, 2)
    h = hist_f32_ref(x, [0, 1, -1, 0], 2, [1.0], 2)
    assert h.shape == (1, 2, 5)
    assert h[0, 0].tolist() == [1, 0, 1, 1, 1]        # planes 0 and 3: 0.5 -> 0, 2.5 -> 2 (end bin), -inf -> the low end bin, 1.0 -> 1
    assert h[0, 1].tolist() == [1, 0, 0, 0, 1]        # plane 1: -7 and 9 land in the end bins
    assert h.sum() == 6                                # plane 2 (group -1) is skipped, its NaN and +inf with it
    x[0, 0, 0, 0] = np.nan
    assert hist_f32_ref(x, [0, 1, -1, 0], 2, [1.0], 2)[0, 0].tolist() == [1, 0, 0, 1, 1]     # a NaN in a counted plane is dropped


def test_reference_u16_groups_end_bins_and_mask():
    u = np.array([[[512, 0, 65535, 511], [513, 512, 512, 600]]], np.uint16)
    h = hist_u16_ref(u, 2, [0, 1, -1, 0], 2, [512, 512], 2)
    # group 0: cells (0,0) and (1,1): 512, 65535, 512, 600 -> bins 2, 4, 2, 4; group 1: cell (0,1): 0, 511 -> bins 0, 1; cell (1,0) skipped
    assert h[0, 0].tolist() == [0, 0, 2, 0, 2] and h[0, 1].tolist() == [1, 1, 0, 0, 0]
    mask = np.zeros((2, 4), bool)
    mask[0, 2] = True
    assert hist_u16_ref(u, 2, [0, 1, -1, 0], 2, [512, 512], 2, mask=mask)[0, 0].tolist() == [0, 0, 2, 0, 1]
    d = hist_u16_ref(u, 2, [0, 0, 0, 0], 1, None, 1, v=u[:, ::-1].copy())
    assert d.sum() == 8 and d[0, 0, 1] == 0
    assert bincount_groups([0, 5, -5], np.array([0, 0, -1]), 1, 1).tolist() == [[0, 1, 1]]


def test_group_maps():
    assert V.group_map_u16('bayer', [[2, 3], [1, 0]]) == (2, [2, 3, 1, 0], 4)
    assert V.group_map_f32('bayer') == (4, [0, 1, 2, 3], 4)
    C, g, G = V.group_map_f32('xtrans')
    assert (C, G) == (9, 3) and g == [0, 1, 2, 0, 2, 1, 1, 1, 1] == groups_f32('xtrans')[0].tolist()
    from xtrans_ref import xtrans_pattern
    xp = xtrans_pattern(g2=((1, 1),))
    p, g, G = V.group_map_u16('xtrans', xp)
    assert (p, G) == (6, 3) and g == groups_u16('xtrans', xp)[1].reshape(-1).tolist() and sorted(set(g)) == [0, 1, 2]
    assert np.bincount(g).tolist() == [8, 20, 8]
    assert V.group_black('bayer', [512.4, 511.6, 512, 513]).tolist() == [512, 512, 512, 513]
    assert V.group_black('xtrans', [1024, 1023.6, 1022, 1024.2]).tolist() == [1024, 1024, 1022]
    with pytest.raises(ValueError):
        V.group_black('xtrans', [1024, 1024, 1024, 1020])


def test_clean_image_restatement():
    a = np.array([[600, 700], [800, 16383]], np.uint16)
    b = np.array([[601, 700], [400, 16383]], np.uint16)
    y = clean_from_flat_pair_ref(a, b, 'bayer', [[1, 0], [2, 3]], [512, 512, 500, 512], [0.5, 0, 0, -1.0], 15871.0)
    assert y.dtype == np.float32 and y.shape == (4, 1, 1)
    assert y[0, 0, 0] == np.float32(np.float32(700 - 512 - 0.5) / np.float32(15871))        # channel 0 sits at (0, 1)
    assert y[1, 0, 0] == np.float32(np.float32(88.5) / np.float32(15871))
    assert y[2, 0, 0] == np.float32(np.float32(100.0) / np.float32(15871)) and y[3, 0, 0] == 1.0


def test_sample_id_is_injective():
    ids = {V.sample_id(s, f, m, d) for s in range(64) for f in range(64) for m in range(16) for d in range(2)}
    assert len(ids) == 64 * 64 * 16 * 2
    assert all(0 <= i < 2 ** 64 for i in (min(ids), max(ids)))
    assert V.sample_id(1, 2, 3, 1) == (1 << 62) + (1 << 40) + (2 << 8) + 7
    for bad in ((-1, 0, 0, 0), (0, 0, 128, 0), (0, 0, 0, 2), (1 << 20, 0, 0, 0)):
        with pytest.raises(ValueError):
            V.sample_id(*bad)


# ---- argument errors -------------------------------------------------------------------------------------------------------------------
def _sessions():
    return [{'iso': 100 * (i + 1), 'bias': np.full((2, 8, 8), 512, np.uint16), 'flats': np.full((1, 2, 8, 8), 900, np.uint16)} for i in range(2)]


def test_validate_camera_argument_errors_before_device_work():
    s, blk = _sessions(), [512.0] * 4
    with pytest.raises(ValueError, match='unknown noise model'):
        V.validate_camera(s, RGGB, blk, 16383, models=('Pg', 'PX'))
    with pytest.raises(ValueError, match='no noise model'):
        V.validate_camera(s, RGGB, blk, 16383, models=())
    for r in (0, 32768, -3, 2.5):
        with pytest.raises(ValueError, match='radius'):
            V.validate_camera(s, RGGB, blk, 16383, radius=r)
    with pytest.raises(ValueError, match='flat_radius'):
        V.validate_camera(s, RGGB, blk, 16383, flat_radius=40000)
    with pytest.raises(ValueError, match='source'):
        V.validate_camera(s, RGGB, blk, 16383, source='both')
    xt_table = {'cfa': 'xtrans'}
    with pytest.raises(ValueError, match='colour bias'):
        V.validate_camera(s, RGGB, blk, 16383, table=xt_table, models=('PGRB',))
    with pytest.raises(ValueError, match='alpha'):
        V.validate_camera(s, RGGB, blk, 16383, alpha=-1.0)
    # calibrate's own checks
    with pytest.raises(ValueError, match='raw_pattern'):
        V.validate_camera(s, [[0, 1], [1, 2]], blk, 16383)
    with pytest.raises(ValueError, match='black_level'):
        V.validate_camera(s, RGGB, [512.0] * 3, 16383)
    with pytest.raises(ValueError, match='cfa'):
        V.validate_camera(s, RGGB, blk, 16383, cfa='foveon')
    with pytest.raises(ValueError, match='at least 2 sessions'):
        V.validate_camera([dict(s[0], bias=np.full((3, 8, 8), 512, np.uint16))], RGGB, blk, 16383)
    with pytest.raises(ValueError, match='white level'):
        V.validate_camera(s, RGGB, blk, 500)
    with pytest.raises(ValueError, match='defects'):
        V.validate_camera(s, RGGB, blk, 16383, defects=3)


def test_histogram_argument_errors_before_device_work():
    u = np.zeros((1, 4, 8), np.uint16)
    for r in (0, 32768):
        with pytest.raises(ValueError, match='radius'):
            V.histogram_u16(u, 'bayer', RGGB, [0] * 4, r)
    with pytest.raises(ValueError, match='even'):
        V.histogram_u16(np.zeros((1, 4, 7), np.uint16), 'bayer', RGGB, [0] * 4, 4)
    with pytest.raises(ValueError, match='uint16'):
        V.histogram_u16(u.astype(np.int32), 'bayer', RGGB, [0] * 4, 4)
    with pytest.raises(ValueError, match='F, Hm, Wm'):
        V.histogram_u16(u[0], 'bayer', RGGB, [0] * 4, 4)
    with pytest.raises(ValueError, match='centre'):
        V.histogram_u16(u, 'bayer', RGGB, [0] * 3, 4)
    with pytest.raises(ValueError, match='centre'):
        V.histogram_u16(u, 'bayer', RGGB, [0.5, 0, 0, 0], 4)
    with pytest.raises(ValueError, match='subtract'):
        V.histogram_u16(u, 'bayer', RGGB, None, 4, subtract=np.zeros((1, 4, 6), np.uint16))
    with pytest.raises(ValueError, match='raw_pattern'):
        V.histogram_u16(u, 'bayer', [[0, 0], [1, 2]], [0] * 4, 4)
    with pytest.raises(ValueError, match='raw_pattern'):
        V.histogram_u16(u, 'xtrans', RGGB, [0] * 3, 4)
    with pytest.raises(ValueError, match='cfa'):
        V.histogram_u16(u, 'quad', RGGB, [0] * 4, 4)
    import torch
    with pytest.raises(ValueError, match='CUDA'):
        V.histogram_u16(torch.zeros((1, 4, 8), dtype=torch.int16), 'bayer', RGGB, [0] * 4, 4)
    with pytest.raises(ValueError, match='CUDA float32'):
        V.histogram_f32(np.zeros((1, 4, 2, 2), np.float32), 1.0, 4, 'bayer')
    with pytest.raises(ValueError, match='CUDA float32'):
        V.histogram_f32(torch.zeros((1, 4, 2, 2)), 1.0, 4, 'bayer')
    with pytest.raises(ValueError, match='radius'):
        V.histogram_f32(torch.zeros((1, 4, 2, 2)), 1.0, 0, 'bayer')
    with pytest.raises(ValueError, match='shape'):
        V.synthesize_codes(None, {'K': 1.0}, 'PG', 'bayer', 1, 0, 16383, [512] * 4)
    with pytest.raises(ValueError, match='unknown noise model'):
        V.synthesize_codes(None, {'K': 1.0}, 'Pz', 'bayer', 1, 0, 16383, [512] * 4, shape=(4, 2, 2))


def test_cli_parser_errors():
    ap = V.parser()
    a = ap.parse_args(['m.json'])
    assert a.models == ['Pg', 'PG', 'PGR', 'PGRB'] and a.source == 'frames' and a.radius == 256 and a.seed == 2018 and a.camera is None
    a = ap.parse_args(['m.json', '--models', 'Pg,PGRU', '--source', 'table', '--radius', '64', '--defects', 'auto', '--out', 'r.json', '--hist', 'h.npz'])
    assert a.models == ['Pg', 'PGRU'] and a.source == 'table' and a.radius == 64 and a.defects == 'auto'
    for bad in (['m.json', '--models', 'Pg,XY'], ['m.json', '--radius', '0'], ['m.json', '--radius', '40000'], ['m.json', '--source', 'none'], []):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)


def test_report_is_jsonable():
    import json
    rep = {'a': np.float64(1.5), 'b': np.arange(3), 'c': [np.int64(2), {'d': np.float32(0.5)}], 'e': None, 5: 'x'}
    assert json.loads(json.dumps(V.to_jsonable(rep))) == {'a': 1.5, 'b': [0, 1, 2], 'c': [2, {'d': 0.5}], 'e': None, '5': 'x'}


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_abi_declares_the_histogram_entry_points(eld_lib):
    from eld_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'eld_amd.h')).read()
    assert re.search(r'\bint eld_hist_u16\(', hdr) and re.search(r'\bint eld_hist_f32\(', hdr)
    assert int(re.search(r'#define ELD_ABI_VERSION (\d+)', hdr).group(1)) == 8 == _lib.ABI_VERSION == eld_lib.eld_abi_version()
    assert 'every version-7 call behaves as before' in hdr
    assert hasattr(eld_lib, 'eld_hist_u16') and hasattr(eld_lib, 'eld_hist_f32')


def test_abi_argument_errors_without_gpu(eld_lib):
    """ELD_EINVAL is decided before any launch, so it is reached without a device (pointers are never dereferenced)."""
    g = (ctypes.c_int * 4)(0, 1, 3, 2)
    c = (ctypes.c_int32 * 4)(512, 512, 512, 512)
    P = ctypes.c_void_p
    ok = dict(u=P(4096), v=None, F=1, Hm=4, Wm=8, p=2, group=g, G=4, centre=c, R=8, bitmap=None, counts=P(8192))

    def call(**kw):
        a = dict(ok, **kw)
        return eld_lib.eld_hist_u16(a['u'], a['v'], a['F'], a['Hm'], a['Wm'], a['p'], a['group'], a['G'], a['centre'], a['R'], a['bitmap'],
                                    a['counts'], None)
    assert call(Wm=7) == -1 and call(G=0) == -1 and call(G=5) == -1 and call(R=0) == -1 and call(R=32768) == -1 and call(p=3) == -1
    assert call(group=(ctypes.c_int * 4)(0, 1, 4, 2)) == -1 and call(group=(ctypes.c_int * 4)(0, -2, 1, 2)) == -1 and call(G=3) == -1
    assert call(u=P(4098)) == -1 and call(v=P(4098 + 64)) == -1 and call(bitmap=P(4097)) == -1 and call(counts=P(8196)) == -1
    assert call(u=None) == -1 and call(counts=None) == -1 and call(centre=None) == -1 and call(group=None) == -1
    assert call(Hm=1 << 16, Wm=1 << 15) == -1 and call(F=-1) == -1 and call(F=65536) == -1
    assert call(F=0) == 0                                               # nothing to do: no launch
    gf = (ctypes.c_int * 4)(0, 1, 2, 3)

    def callf(x=P(4096), x2=None, N=1, C=4, H=2, W=2, group=gf, G=4, scale=P(256), R=8, counts=P(8192)):
        return eld_lib.eld_hist_f32(x, x2, N, C, H, W, group, G, scale, R, counts, None)
    assert callf(G=0) == -1 and callf(G=5) == -1 and callf(R=0) == -1 and callf(C=0) == -1 and callf(C=65) == -1 and callf(G=3) == -1
    assert callf(x=None) == -1 and callf(scale=None) == -1 and callf(x=P(4098)) == -1 and callf(counts=None) == -1 and callf(N=-1) == -1
    assert callf(N=0) == 0
