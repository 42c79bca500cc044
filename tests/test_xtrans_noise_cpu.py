"""CPU tests of the X-Trans noise model and calibration: ELD_CFA_XTRANS and the cell-statistics argument checks of the C ABI, the
NoiseModel table / CFA rules, the launch flags, and the X-Trans estimators from exact cell sums against a float64 NumPy restatement."""
import ctypes
import os

import numpy as np
import pytest

from eld_amd import calibrate as CAL

from xtrans_ref import (CODE_COLOUR, cell_flat_sums_ref, cell_sums_ref, xtrans_bias_ref, xtrans_flat_ref, xtrans_pattern)

ROW, CBIAS, XT = 16, 64, 512


def test_noise_forward_cfa_arguments(eld_lib):
    from eld_amd import _lib as L
    assert L.CFA_XTRANS == XT
    f = eld_lib.eld_noise_forward
    assert f(None, 0, None, None, 1, 4, 8, 8, XT, 0, None, None, None) == -1               # ELD_CFA_XTRANS needs C == 9
    assert f(None, 0, None, None, 1, 4, 8, 8, ROW | XT, 0, None, None, None) == -1
    assert f(None, 0, None, None, 1, 9, 8, 8, ROW, 0, None, None, None) == -1              # 9 planes with row noise: say X-Trans
    assert f(None, 0, None, None, 1, 9, 8, 8, CBIAS, 0, None, None, None) == -1
    assert f(None, 0, None, None, 1, 3, 8, 8, ROW | XT, 0, None, None, None) == -1
    assert f(None, 0, None, None, 1, 9, 8, 8, ROW | XT, 0, None, None, None) == -1         # accepted flags, null pointers
    assert f(None, 0, None, None, 1, 9, 8, 8, ROW | CBIAS | XT, 0, None, None, None) == -1
    assert f(None, 0, None, None, 0, 9, 8, 8, ROW | CBIAS | XT, 0, None, None, None) == 0   # empty batch
    assert f(None, 0, None, None, 0, 9, 8, 8, XT, 0, None, None, None) == 0
    assert f(None, 0, None, None, 1, 9, 8, 8, XT | 1 | 4, 0, None, None, None) == -1        # per-pixel terms only: legal, null pointers
    assert f(None, 0, None, None, 1, 3, 8, 8, ROW, 0, None, None, None) == -1                # refused before, refused now


def test_cell_entry_points_refuse_bad_arguments(eld_lib):
    u, ws, out, t = ctypes.c_void_p(0x30000), ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000), ctypes.c_void_p(0x40000)
    blk = (ctypes.c_double * 36)(*([0.0] * 36))
    for p in (0, 1, 3, 4, 5, 7, 12, -6):
        assert eld_lib.eld_calib_cell_stats(u, 1, 12, 12, p, out, out, ws, 1 << 20, None) == -1
        assert eld_lib.eld_calib_cell_residual(u, 1, 12, 12, p, blk, out, out, t, None) == -1
        assert eld_lib.eld_calib_cell_flat_stats(u, 1, 12, 12, p, 16383, out, ws, 1 << 20, None) == -1
        assert eld_lib.eld_calib_cell_stats_workspace_bytes(1, 12, p) == 0
        assert eld_lib.eld_calib_cell_flat_stats_workspace_bytes(1, 12, p) == 0
    for p in (2, 6):
        assert eld_lib.eld_calib_cell_stats(u, 1, 12, 13, p, out, out, ws, 1 << 20, None) == -1          # odd Wm
        assert eld_lib.eld_calib_cell_residual(u, 1, 12, 13, p, blk, out, out, t, None) == -1
        assert eld_lib.eld_calib_cell_flat_stats(u, 1, 12, 13, p, 16383, out, ws, 1 << 20, None) == -1
        for base in (0x30002, 0x30001):                                                               # misaligned mosaics
            m = ctypes.c_void_p(base)
            assert eld_lib.eld_calib_cell_stats(m, 1, 12, 12, p, out, out, ws, 1 << 20, None) == -1
            assert eld_lib.eld_calib_cell_residual(m, 1, 12, 12, p, blk, out, out, t, None) == -1
            assert eld_lib.eld_calib_cell_flat_stats(m, 1, 12, 12, p, 16383, out, ws, 1 << 20, None) == -1
        assert eld_lib.eld_calib_cell_residual(u, 1, 12, 12, p, blk, out, out, ctypes.c_void_p(0x40004), None) == -1   # t not 8-aligned
        assert eld_lib.eld_calib_cell_stats(u, 1, 12, 12, p, out, out, ws, 8, None) == -3                   # aligned: on to ELD_EWS
        assert eld_lib.eld_calib_cell_flat_stats(u, 1, 12, 12, p, 16383, out, ws, 8, None) == -3
        assert eld_lib.eld_calib_cell_stats(u, 0, 12, 12, p, None, None, None, 0, None) == 0                # empty
        assert eld_lib.eld_calib_cell_stats_workspace_bytes(3, 13, p) == 3 * 13 * p * 2 * 8
        assert eld_lib.eld_calib_cell_flat_stats_workspace_bytes(3, 13, p) == 3 * 13 * p * 4 * 8


# ---- NoiseModel ---------------------------------------------------------------------------------------------------------------
def _xtrans_table(m=4, seed=0):
    rng = np.random.default_rng(seed)
    prof = {k: {'slope': np.float64(0.8), 'bias': np.float64(-1.0), 'sigma': np.float64(0.05)} for k in CAL.SIGMA_KEYS}
    return {'Kmin': np.float64(0.5), 'Kmax': np.float64(8.0), 'G_shape': rng.uniform(-0.2, 0.2, m), 'cfa': 'xtrans',
            'color_bias': rng.normal(0, 0.5, (m, 3)).astype(np.float32), 'Profile-1': prof}


def test_noise_model_table_cfa_rules(tmp_path, monkeypatch, capsys):
    from eld_amd.noise import ALL_CAMERAS, NoiseModel
    with pytest.raises(ValueError, match='CanonEOS5D4|CanonEOS70D|CanonEOS700D|NikonD850|SonyA7S2'):
        NoiseModel(model='PGRUB', cfa='xtrans')                       # release tables are Bayer
    with pytest.raises(ValueError):
        NoiseModel(model='B', cfa='xtrans', include=2)
    nm = NoiseModel(model='PGRU', cfa='xtrans')                       # G, R, U do not depend on the CFA
    assert nm.cameras == ALL_CAMERAS and nm.raw_packer.cfa == 'xtrans'
    NoiseModel(model='PGRUB', cfa='bayer')
    monkeypatch.chdir(tmp_path)
    tab = _xtrans_table()
    CAL.save_camera_params(tab, 'FujiSynth', os.path.join('camera_params', 'release'))
    with pytest.raises(ValueError, match='FujiSynth'):
        NoiseModel(model='PGRUB', cameras=['FujiSynth'])              # an X-Trans table on Bayer input
    with pytest.raises(ValueError, match='SonyA7S2'):
        NoiseModel(model='PGRUB', cfa='xtrans', cameras=['FujiSynth', 'SonyA7S2'])
    NoiseModel(model='PGRU', cameras=['FujiSynth'])                   # no colour bias asked for: any table
    nm = NoiseModel(model='PGRUB', cfa='xtrans', cameras=['FujiSynth'])
    np.random.seed(3)
    for _ in range(6):
        q = nm._sample_params()
        i = list(tab['G_shape']).index(q.tl_lambda)
        assert q.color_bias == tuple(float(v) for v in tab['color_bias'][i]) + (0.0,)
        rec = q.record(5)
        assert rec['color_bias'].tolist() == [float(v) for v in tab['color_bias'][i]] + [0.0]


def test_sample_params_draws_unchanged_on_xtrans(golden_dir, capsys):
    """np.random.seed reproduces the reference's five draws whatever the CFA; the withheld terms come after them."""
    from eld_amd.noise import NoiseModel
    recs = np.load(os.path.join(golden_dir, 'sample_params.npz'))['recs']
    i = 0
    for inc in (None, 4, 1):
        nm = NoiseModel(model='g', include=inc, cfa='xtrans')
        for s in (0, 1, 2018):
            np.random.seed(s)
            for _ in range(3):
                assert np.array_equal(np.array(tuple(nm._sample_params()), np.float64), recs[i][2:])
                i += 1
    np.random.seed(5)
    base = NoiseModel(model='Pg', include=4, cfa='xtrans')._sample_params()
    np.random.seed(5)
    full = NoiseModel(model='PGRU', include=4, cfa='xtrans')._sample_params()
    assert tuple(base) == tuple(full) and full.row_scale > 0


def test_flags_helper_sets_cfa_xtrans_exactly_for_xtrans(capsys):
    from eld_amd import _lib as L
    from eld_amd.noise import NoiseModel, model_flags, noise_model_flags
    for m in ('g', 'Pg', 'pg', 'PGRU', 'PGRUB', ''):
        assert model_flags(m, 'xtrans') == model_flags(m) | L.CFA_XTRANS
        assert model_flags(m, 'bayer') == model_flags(m) and not model_flags(m) & L.CFA_XTRANS
    assert NoiseModel(model='PGRU', cfa='xtrans').flags() == model_flags('PGRU') | L.CFA_XTRANS
    assert NoiseModel(model='PGRU').flags() == model_flags('PGRU')

    class Duck:                      # any object with .model (the reference's own NoiseModel has a raw_packer too)
        model = 'Pg'
    assert noise_model_flags(Duck()) == model_flags('Pg')


# ---- host derivations from cell sums -----------------------------------------------------------------------------------------
PATTERNS = [xtrans_pattern(), xtrans_pattern(g2=[(1, 0), (2, 4), (4, 1), (0, 2), (5, 3)])]


@pytest.mark.parametrize('shape', [(36, 48), (37, 50), (41, 62), (6, 6), (13, 8)])
@pytest.mark.parametrize('pi', [0, 1])
def test_xtrans_estimators_from_cell_sums_equal_numpy(shape, pi):
    pattern = PATTERNS[pi]
    rng = np.random.default_rng(shape[0] * 100 + shape[1] + pi)
    Hm, Wm = shape
    black = np.array([1024.0, 1023.0, 1025.5, 1021.0])
    F = 3
    u = np.clip(rng.normal(1030, 7, (F, Hm, Wm)) + rng.normal(0, 2, (F, Hm, 1)), 0, 65535).astype(np.uint16)
    u[2] = rng.integers(0, 65536, (Hm, Wm), dtype=np.uint16)                   # the whole code range
    cs, rs = cell_sums_ref(u, 6)
    st = CAL.xtrans_bias_stats_from_cell_sums(cs, rs, pattern, black, Hm, Wm)
    for f in range(F):
        cb, rho, g, R, _ = xtrans_bias_ref(u[f], pattern, black)
        np.testing.assert_allclose(st['color_bias'][f], cb, rtol=1e-12, atol=1e-9)
        np.testing.assert_allclose(st['row_offset'][f], rho, rtol=1e-10, atol=1e-8)
        assert abs(st['g_scale'][f] - g) <= 1e-9 * g
        assert abs(st['R_scale'][f] - R) <= 1e-7 * max(R, 1e-3)
    white = 16383
    ab = rng.integers(900, 16383, (3, 2, Hm, Wm), dtype=np.uint16)
    ab[1] = np.clip(rng.normal(3000, 50, (2, Hm, Wm)), 0, 65535).astype(np.uint16)
    ab[2, 0, 0, 0] = 16383
    cbm = np.array([0.5, -0.25, 0.125])
    fl = CAL.xtrans_flat_stats_from_cell_sums(cell_flat_sums_ref(ab, 6, white), pattern, black, white, cbm, Hm, Wm)
    for p in range(3):
        mu, var, ok = xtrans_flat_ref(ab[p, 0], ab[p, 1], pattern, black, white, cbm)
        np.testing.assert_allclose(fl['mu'][p], mu, rtol=1e-12, atol=1e-9)
        np.testing.assert_allclose(fl['var'][p], var, rtol=1e-10)
        assert np.array_equal(fl['usable'][p], ok)


def test_xtrans_pattern_and_arguments_are_checked():
    pat = xtrans_pattern()
    assert np.bincount(CODE_COLOUR[pat].reshape(-1)).tolist() == [8, 20, 8]
    assert pat[0].tolist() == [0, 2, 1, 2, 0, 1]                            # R B G B R G: the pack's phase
    bad = [pat[:2, :2], np.zeros((6, 6), int), pat.copy(), pat.copy(), np.full((6, 6), 4)]
    bad[2][0, 0] = 1                                                        # 7 R
    bad[3][0, 2] = 0                                                        # 9 R, 19 G
    u = np.full((2, 12, 12), 1024, np.uint16)
    ses = [{'bias': u, 'flats': np.zeros((2, 2, 12, 12), np.uint16)}] * 2
    for b in bad:
        with pytest.raises(ValueError, match='raw_pattern'):
            CAL.calibrate_camera(ses, b, [1024] * 4, 16383, cfa='xtrans')
        with pytest.raises(ValueError, match='raw_pattern'):
            CAL.xtrans_bias_stats_from_cell_sums(np.zeros((1, 6, 6, 2), np.int64), np.zeros((1, 12, 6), np.int64), b, [0] * 4, 12, 12)
    with pytest.raises(ValueError, match='cfa'):
        CAL.calibrate_camera(ses, pat, [1024] * 4, 16383, cfa='foveon')
    with pytest.raises(ValueError, match='even width'):
        CAL.calibrate_camera([{'bias': np.zeros((2, 12, 13), np.uint16), 'flats': np.zeros((2, 2, 12, 13), np.uint16)}] * 2, pat, [0] * 4,
                             16383, cfa='xtrans')
    with pytest.raises(ValueError, match='black_level'):
        CAL.calibrate_camera(ses, pat, [1024] * 3, 16383, cfa='xtrans')
