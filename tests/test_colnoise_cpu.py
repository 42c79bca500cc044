"""Host side of the column term (model letter C, flag COL): the restatement of the op chain is pinned to the oracle, the letter parses, its
scale travels in the record without moving a byte, its draw comes after every existing one, the calibration regresses it, and the
estimator recovers a planted column pattern.  No GPU: integer sums come from tests/structure_ref.py.

Bounds are 5 standard errors from the counts, with the two formulas tests/test_structure_cpu.py states: a variance estimated from N
independent values of variance v has s.e. v sqrt(2 / (N - 1)); a covariance of two series of variances va, vb and covariance c has s.e.
sqrt((va vb + c^2) / (N - 1))."""
import contextlib
import inspect
import io
import math

import numpy as np
import pytest

from eld_amd import _lib as L
from eld_amd import calibrate as CAL
from eld_amd import validate as V
from eld_amd.noise import NoiseModel, NoiseParams, load_camera_params, make_records, model_flags
from oracle import noise_ref as O

import colnoise_ref as CR
from structure_ref import sums_dict
from xtrans_ref import plane_bias

FULL = O.SHOT_POISSON | O.READ_TL | O.ROW | O.QUANT
# the flag sets of the sampler's replay tests (tests/test_noise_gpu.py, tests/test_xtrans_noise_gpu.py)
FLAGSETS = [FULL, FULL | O.CBIAS | O.CLIP, FULL | O.CLIP, FULL | O.CBIAS, O.SHOT_GAUSS | O.READ_GAUSS, O.SHOT_POISSON | O.READ_GAUSS,
            O.READ_GAUSS | O.READ_TL | O.ROW | O.QUANT | O.CBIAS, 0]
PAT = [[0, 1], [3, 2]]
C_LAW = {'slope': np.float64(0.5), 'bias': np.float64(math.log(0.6)), 'sigma': np.float64(0.25)}


# ---- the restatement is the oracle's chain ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(4, 6, 8), (9, 4, 6)])
@pytest.mark.parametrize('flags', FLAGSETS)
def test_restatement_without_col_equals_the_oracle(shape, flags):
    rng = np.random.default_rng(100 * shape[0] + flags)
    y = (np.floor(65535.0 * rng.uniform(size=shape) ** 2.2) / 65535.0).astype(np.float32)
    cb = (1.5, -1.0, 0.25, 4.0) if shape[0] == 4 else plane_bias((1.5, -1.0, 0.25))
    p = O.Params(K=2.288, g_scale=6.451, saturation=15583, ratio=208.98, tl_lambda=-0.14285714, tl_scale=3.3, row_scale=0.9, color_bias=cb)
    v = {'counts': rng.poisson(O.poisson_lambda(y, p)), 'n_shot': rng.standard_normal(shape).astype(np.float32),
         'n_read': rng.standard_normal(shape).astype(np.float32), 't_tl': (3 * rng.standard_normal(shape)).astype(np.float32),
         'n_row': np.broadcast_to(rng.standard_normal(shape[:2] + (1,)).astype(np.float32), shape), 'u_q': rng.uniform(size=shape).astype(np.float32)}
    want = O.noise_arith(y, p, flags, **v)
    got = CR.noise_arith_col(y, p, flags, col_scale=7.5, n_col=rng.standard_normal(shape).astype(np.float32), **v)      # COL off: both ignored
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # and with COL on the term is there: z moves by n_col * col_scale before the tail of the chain
    n_col = rng.standard_normal(shape).astype(np.float32)
    on = CR.noise_arith_col(y, p, flags | CR.COL, col_scale=7.5, n_col=n_col, **v)
    assert not np.array_equal(on, want)


def test_sensor_column_maps_are_the_pack_maps():
    """Bayer: packing a mosaic whose value is its column index gives sensor_cols; X-Trans the same through pack_raw_xtrans."""
    H, W = 5, 7
    mos = np.broadcast_to(np.arange(2 * W, dtype=np.float32)[None, :], (2 * H, 2 * W))
    assert np.array_equal(O.pack_raw_bayer(mos), CR.sensor_cols(4, H, W).astype(np.float32))
    assert CR.sensor_cols(4, H, W)[:, 0, 0].tolist() == [0, 1, 1, 0]              # planes 0 and 3 even, 1 and 2 odd
    H, W = 4, 6
    mos = np.broadcast_to(np.arange(3 * W, dtype=np.float32)[None, :], (3 * H, 3 * W))
    cols = CR.sensor_cols(9, H, W)
    assert np.array_equal(O.pack_raw_xtrans(mos), cols.astype(np.float32))
    j = np.arange(W)[None, None, :]
    assert np.all((cols >= 3 * j) & (cols <= 3 * j + 2))                            # packed column j holds sensor columns 3j .. 3j + 2


# ---- letters, flags, records ---------------------------------------------------------------------------------------------------------------
def test_letter_parses_to_the_flag():
    assert L.COL == 2048 == CR.COL and L.PLANE_NCOL == 6 and L.NPLANES_COL == 7 and L.NPLANES == 6
    assert L.PLANE == {'counts': 0, 'n_shot': 1, 'n_read': 2, 't_tl': 3, 'n_row': 4, 'u_q': 5}      # the six planes are what they were
    assert model_flags('C') == L.COL
    assert model_flags('PGRCU') == L.SHOT_POISSON | L.READ_TL | L.ROW | L.COL | L.QUANT
    assert model_flags('PGRCU', 'xtrans') == model_flags('PGRCU') | L.CFA_XTRANS
    assert model_flags('PGRU') & L.COL == 0
    assert L.COL & (L.SHOT_POISSON | L.SHOT_GAUSS | L.READ_GAUSS | L.READ_TL | L.ROW | L.QUANT | L.CBIAS | L.CLIP | L.AUG_NOTRANSPOSE
                    | L.CFA_XTRANS | L.DARK) == 0


def test_record_carries_the_scale_in_reserved0():
    assert L.NOISE_PARAMS_DTYPE.itemsize == 64
    p = NoiseParams(2.0, 3.0, 15583, 150.0, tl_lambda=0.1, tl_scale=2.0, row_scale=0.5, col_scale=1.25)
    rec = p.record((7 << 32) | 5)
    assert rec.dtype.itemsize == 64 and rec['reserved'].tolist() == [0x3fa00000, 0]
    assert rec['reserved'][:1].view(np.float32)[0] == np.float32(1.25)
    plain = NoiseParams(2.0, 3.0, 15583, 150.0, tl_lambda=0.1, tl_scale=2.0, row_scale=0.5).record((7 << 32) | 5)
    assert plain['reserved'].tolist() == [0, 0]
    for name in L.NOISE_PARAMS_DTYPE.names:
        if name != 'reserved':
            assert np.array_equal(rec[name], plain[name]), name
    assert NoiseParams(2.0, 3.0, 15583, 150.0, col_scale=0.1).record(0)['reserved'][:1].view(np.float32)[0] == np.float32(0.1)
    # a dark range keeps the field (the two letters exclude each other)
    assert NoiseParams(2.0, 3.0, 15583, 150.0, dark=(3, 4), col_scale=1.25).record(0)['reserved'].tolist() == [3, 4]
    # keyword after the existing ones; the dict key
    names = list(inspect.signature(NoiseParams.__new__).parameters)
    assert names[-2:] == ['dark', 'col_scale'] and inspect.signature(NoiseParams.__new__).parameters['col_scale'].default == 0.0
    q = NoiseParams.coerce({'K': 2.0, 'g_scale': 3.0, 'ratio': 150.0, 'col_scale': 0.75})
    assert q.col_scale == 0.75 and NoiseParams.coerce({'K': 2.0, 'g_scale': 3.0, 'ratio': 150.0}).col_scale == 0.0
    assert NoiseParams.coerce((2.0, 3.0, 15583, 150.0)).col_scale == 0.0
    recs = make_records([p, q], [1, 2])
    assert recs['reserved'][:, 0].view(np.float32).tolist() == [1.25, 0.75]


def _table_with_column_law(tmp_path, name='Col'):
    t = load_camera_params('SonyA7S2')
    t['Profile-1'] = dict(t['Profile-1'], C_scale=dict(C_LAW))
    CAL.save_camera_params(t, name, str(tmp_path))
    return t


def _nm(**kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return NoiseModel(**kw)


def test_sample_params_prefix_property(tmp_path):
    t = _table_with_column_law(tmp_path)
    a = _nm(model='PGRU', cameras=['Col'], param_dir=str(tmp_path))
    b = _nm(model='PGRCU', cameras=['Col'], param_dir=str(tmp_path))
    for seed in (0, 7, 2018):
        np.random.seed(seed)
        pa = a._sample_params()
        nxt = np.random.standard_normal()                          # the draw that follows every draw of 'PGRU'
        np.random.seed(seed)
        pb = b._sample_params()
        after = np.random.uniform()
        assert tuple(pa) == tuple(pb)
        for k in ('tl_lambda', 'tl_scale', 'row_scale', 'q_step', 'color_bias', 'dark'):
            assert getattr(pa, k) == getattr(pb, k), k
        assert pa.col_scale == 0.0
        np.random.seed(seed)                                       # log K as _sample_params draws it: two choices, then the uniform
        np.random.choice(['Col'])
        np.random.choice(['Profile-1'])
        log_K = np.random.uniform(low=np.log(1e-1), high=np.log(30))
        assert pb.col_scale == float(np.exp(nxt * C_LAW['sigma'] + C_LAW['slope'] * log_K + C_LAW['bias']))
        np.random.seed(seed)                                       # exactly one draw more than 'PGRU'
        a._sample_params()
        np.random.standard_normal()
        assert np.random.uniform() == after
    # 'C' alone takes the withheld-terms branch too
    np.random.seed(3)
    assert _nm(model='C', cameras=['Col'], param_dir=str(tmp_path))._sample_params().col_scale > 0
    assert t['Profile-1']['C_scale']['slope'] == 0.5


def test_noise_model_refuses_c_with_d_and_tables_without_the_law(tmp_path):
    with pytest.raises(ValueError, match='excludes C'):
        _nm(model='PDCU')
    with pytest.raises(ValueError, match=r'calibrate --column'):
        _nm(model='PGRCU', cameras=['SonyA7S2'])
    with pytest.raises(ValueError, match=r'C_scale'):
        _nm(model='PGRCU')                                         # no release table has the key
    _table_with_column_law(tmp_path)
    assert _nm(model='PGRCU', cameras=['Col'], param_dir=str(tmp_path)).flags() & L.COL


# ---- calibration -----------------------------------------------------------------------------------------------------------------------------
def _frames(with_c):
    Ks = [0.5, 0.5, 2.0, 2.0, 8.0, 8.0]
    out = []
    for j, K in enumerate(Ks):
        fr = {'session': j // 2, 'iso': 100 * K, 'K': K, 'lambda': 0.1, 'G_scale': 1.7 * K ** 0.46 * (1 + 0.01 * j), 'R_scale': 0.55 * K ** 0.52 * (1 - 0.01 * j),
              'g_scale': 3.4 * K ** 0.54, 'color_bias': np.zeros(4)}
        if with_c:
            fr['C_scale'] = 0.6 * K ** 0.5 * (1 + 0.02 * (-1) ** j)
        out.append(fr)
    return out, [0.5, 2.0, 8.0]


def test_params_from_samples_with_and_without_the_column_samples():
    fr, Ks = _frames(False)
    plain = CAL.params_from_samples(fr, Ks)
    assert set(plain) == {'Kmin', 'Kmax', 'G_shape', 'color_bias', 'Profile-1'} and set(plain['Profile-1']) == set(CAL.SIGMA_KEYS)
    frc, _ = _frames(True)
    col = CAL.params_from_samples(frc, Ks)
    assert set(col['Profile-1']) == set(CAL.SIGMA_KEYS) | {'C_scale'}
    for k in CAL.SIGMA_KEYS:                                        # the three existing regressions keep their bits
        assert col['Profile-1'][k] == plain['Profile-1'][k]
    want = CAL.fit_log_linear([f['K'] for f in frc], [f['C_scale'] for f in frc])
    assert col['Profile-1']['C_scale'] == want and set(want) == {'slope', 'bias', 'sigma'}
    assert abs(want['slope'] - 0.5) < 0.02 and abs(want['bias'] - math.log(0.6)) < 0.02
    frc[3]['C_scale'] = 0.0
    with pytest.raises(ValueError, match='drop --column'):
        CAL.params_from_samples(frc, Ks)
    part, _ = _frames(True)
    del part[0]['C_scale']                                          # not every frame has one: no fourth regression
    assert set(CAL.params_from_samples(part, Ks)['Profile-1']) == set(CAL.SIGMA_KEYS)


def test_calibrate_signature():
    sig = inspect.signature(CAL.calibrate_camera)
    assert list(sig.parameters)[-1] == 'column' and sig.parameters['column'].default is False


HM, WM = 256, 384
SW, SR, SC = 6.0, 1.5, 1.0
Q = 1.0 / 12.0


def _planted(seed, F, fixed):
    """F frames of white noise SW, a temporal row term SR and a column term SC that is one pattern for all frames (fixed) or a fresh one per
    frame."""
    rng = np.random.default_rng(seed)
    shared = SC * rng.standard_normal(WM)
    out = []
    for f in range(F):
        col = shared if fixed else SC * rng.standard_normal(WM)
        out.append(np.rint(2048.0 + SW * rng.standard_normal((HM, WM)) + SR * rng.standard_normal(HM)[:, None] + col[None, :]))
    return np.stack(out).astype(np.uint16)


@pytest.mark.parametrize('fixed', [True, False])
def test_host_estimator_recovers_a_planted_column_pattern(fixed):
    F = 3
    u = _planted(77 + fixed, F, fixed)
    sums = sums_dict(u, 2, [2048] * 4, pairs=[(a, b) for a in range(F) for b in range(a + 1, F)])
    samples, rep = CAL.column_samples_from_sums(sums, 'bayer', PAT)
    site, n_c, N_c = SW ** 2 + Q, HM // 2, WM // 2
    vc = SC ** 2 + site / n_c                                       # a column mean of one row phase; the two phases share the column term only
    se = math.sqrt((vc * vc + SC ** 4) / (WM - 1))
    assert samples.shape == (F,)
    print('samples', samples.tolist(), 'expect', SC ** 2, 'se', se, rep)
    assert np.all(np.abs(samples - SC ** 2) < 5 * se)
    # the fixed share: what two frames share of the column variance (per group, over the N_c column entries of a row phase)
    cc = SC ** 2 if fixed else 0.0
    se_fix = math.sqrt((vc * vc + cc * cc) / (N_c - 1))
    se_var = vc * math.sqrt(2.0 / (N_c - 1))
    assert abs(rep['col_fixed_var'] - cc) < 5 * se_fix
    assert abs(rep['col_var'] - SC ** 2) < 5 * se_var
    assert rep['fixed_share'] == rep['col_fixed_var'] / rep['col_var']
    assert (rep['fixed_share'] > 0.5) == fixed
    # one frame: samples, no share
    one, none = CAL.column_samples_from_sums(sums_dict(u[:1], 2, [2048] * 4), 'bayer', PAT)
    assert none is None and one[0] == samples[0]


# ---- validate's letter rules -----------------------------------------------------------------------------------------------------------------
def test_validate_letter_rules():
    assert 'C' in V.MODEL_LETTERS and 'C' in V.DARK_EXCLUDES
    assert V._models('PGR,PGRC') == ['PGR', 'PGRC']
    for bad in ('PDC', 'PCDU'):
        with pytest.raises(ValueError, match='excludes'):
            V._models([bad])
    p = V._noise_params({'K': 2.0, 'g_scale': 0.0, 'tl_scale': 3.0, 'row_scale': 1.5, 'tl_lambda': 0.14, 'color_bias': [0.0] * 4, 'col_scale': 0.8}, 15871.0)
    assert p.col_scale == 0.8 and p[3] == 1.0 and p[2] == 15871.0
    assert V._noise_params({'K': 2.0}, 100.0).col_scale == 0.0
    rec = {'K': 2.0, 'g_scale': 0.0, 'G_scale': 3.0, 'R_scale': 1.5, 'lambda': 0.14, 'color_bias': [0.0] * 4}
    assert 'col_scale' not in V._frame_params(rec, 4)                # a diag without the sample: the record is what it was
    assert V._frame_params(dict(rec, C_scale=0.8), 4)['col_scale'] == 0.8
    fp = [V._frame_params(dict(rec, C_scale=c), 4) for c in (0.6, 1.0)]
    assert V._mean_params(fp)['col_scale'] == 0.8 and 'col_scale' not in V._mean_params([V._frame_params(rec, 4)])
    t = load_camera_params('SonyA7S2')
    assert 'col_scale' not in V._table_params(t, 2.0, 4)
    t['Profile-1'] = dict(t['Profile-1'], C_scale=dict(C_LAW))
    assert V._table_params(t, 2.0, 4)['col_scale'] == pytest.approx(0.6 * math.sqrt(2.0), rel=1e-12)
