"""validate_camera(structure=True) end to end: frames with a planted column and pixel pattern, the report must show what PGR misses and
what PD carries.  Bounds are 5 standard errors from the counts (tests/test_structure_cpu.py states the two formulas); where the report
averages estimates over frames and groups that share data, the s.e. of one estimate is used: the mean of correlated estimates has no more."""
import math

import numpy as np
import pytest
import torch

from eld_amd import validate as V

pytestmark = pytest.mark.gpu

PAT = [[0, 1], [3, 2]]
BLACK, WHITE = [512.0] * 4, 16383
HM, WM, F = 256, 384, 3
K, TL, LAM, ROW = 2.0, 3.0, 0.14, 1.5          # G: Tukey-lambda read noise of scale TL and shape LAM
PRM = {'K': K, 'g_scale': 0.0, 'tl_scale': TL, 'row_scale': ROW, 'tl_lambda': LAM, 'color_bias': [0.0] * 4}
REC = {'K': K, 'g_scale': 0.0, 'G_scale': TL, 'R_scale': ROW, 'lambda': LAM, 'color_bias': [0.0] * 4}
Q = 1.0 / 12.0
# variance of the Tukey-lambda distribution of shape l and scale 1: (2 / l^2) (1 / (1 + 2 l) - Gamma(l + 1)^2 / Gamma(2 l + 2))
TL_VAR = 2.0 / LAM ** 2 * (1.0 / (1 + 2 * LAM) - math.gamma(LAM + 1) ** 2 / math.gamma(2 * LAM + 2))


@pytest.fixture(scope='module')
def run(eld_lib):
    rng = np.random.default_rng(31)
    colfix = np.rint(2.0 * rng.standard_normal(WM)).astype(np.int64)
    pixfix = np.rint(3.0 * rng.standard_normal((HM, WM))).astype(np.int64)
    sessions = []
    for si in range(2):
        bias = []
        for f in range(F + 2):
            clean = None if f < F else np.full((4, HM // 2, WM // 2), 0.05, np.float32)
            code = V.synthesize_codes(clean, PRM, 'PGR', 'bayer', 99, 1000 + 16 * si + f, WHITE, BLACK, shape=(4, HM // 2, WM // 2))
            code = code.cpu().numpy().astype(np.int64) + colfix[None, :] + pixfix
            bias.append(np.clip(code, 0, 65535).astype(np.uint16))
        sessions.append({'iso': 800 * (si + 1), 'bias': np.stack(bias[:F]), 'flats': np.stack(bias[F:])[None]})
    diag = {'frames': [dict(REC) for _ in range(2 * F)]}
    kw = dict(diag=diag, models=('PGR', 'PD'), source='frames', radius=64, flat_radius=256)
    plain = V.validate_camera(sessions, PAT, BLACK, WHITE, **kw)
    rep = V.validate_camera(sessions, PAT, BLACK, WHITE, structure=True, lags=4, **kw)
    torch.cuda.synchronize()
    return plain, rep, float(np.var(colfix)), float(np.var(pixfix))


def test_report_without_the_flag_is_unchanged(run):
    plain, rep, _, _ = run
    assert 'structure' not in plain
    assert set(plain) == {'models', 'source', 'cfa', 'groups', 'radius', 'flat_radius', 'alpha', 'seed', 'sessions', 'means', 'best'}
    assert {k: v for k, v in rep.items() if k != 'structure'} == plain            # the histogram pass keeps its bits with the report on


def test_structure_report(run):
    _, rep, vc, vf = run
    st = rep['structure']
    assert st['lags'] == 4 and len(st['sessions']) == 2
    n_r, n_c, N_r, N_c, N = WM // 2, HM // 2, HM // 2, WM // 2, (HM // 2) * (WM // 2)
    site_syn = TL ** 2 * TL_VAR + Q              # a dark frame under PGR: no shot noise; read noise and the rounding to codes
    site = site_syn + vf
    sr = ROW ** 2
    total, fixed = site + sr + vc, vf + vc
    col_a = vc + site / n_c                      # variance of a column entry's mean in one real frame
    col_c = vc + vf / n_c                        # what two real frames share of it
    se_colfix = math.sqrt((col_a ** 2 + col_c ** 2) / (N_c - 1))
    se_pixfix = math.sqrt((total ** 2 + fixed ** 2) / N + 2 * vc ** 2 / (N_c - 1) + sr ** 2 / (N_r - 1))
    row_a = sr + site / n_r
    se_rowsens_real = math.sqrt((row_a ** 2 + sr ** 2) / (HM - 1))
    row_s = sr + site_syn / n_r
    se_rowsens_syn = math.sqrt((row_s ** 2 + sr ** 2) / (HM - 1))
    for s in st['sessions']:
        real = s['real']
        print('real', real)
        for m in ('PGR', 'PD'):
            print(m, s['models'][m]['synthetic'])
        # the real side shows what was planted
        assert abs(real['col_fixed_var'] - vc) < 5 * se_colfix
        assert abs(real['pix_fixed_var'] - fixed) < 5 * se_pixfix
        assert abs(real['row_fixed_var']) < 5 * math.sqrt((row_a ** 2 + (vf / n_r) ** 2) / (N_r - 1))
        # PGR: the row law is right, the column and fixed terms are missing
        pgr = s['models']['PGR']['synthetic']
        assert abs(pgr['row_var_sensor'] - real['row_var_sensor']) < 5 * math.sqrt(se_rowsens_real ** 2 / F + se_rowsens_syn ** 2 / (2 * F))
        assert abs(pgr['col_var']) < 5 * (site_syn / n_c) * math.sqrt(2.0 / (N_c - 1))
        assert abs(pgr['pix_fixed_var']) < 5 * math.sqrt((site_syn + sr) ** 2 / N + sr ** 2 / (N_r - 1))
        assert s['models']['PGR']['log_ratio']['col_fixed_var'] is None or s['models']['PGR']['log_ratio']['col_fixed_var'] < 0
        # PD (leave-one-out): the column and fixed terms are those of the sensor
        pd = s['models']['PD']
        assert pd['dark'] == 'leave-one-out' and 'split' not in pd
        assert abs(pd['synthetic']['col_fixed_var'] - real['col_fixed_var']) < 5 * math.sqrt(2.0) * se_colfix
        assert abs(pd['synthetic']['pix_fixed_var'] - real['pix_fixed_var']) < 5 * math.sqrt(2.0) * se_pixfix
    lines = V.structure_lines(rep)
    assert len(lines) == 1 + 2 * 2


def test_two_bias_frames_give_no_split_for_dark_models(run, eld_lib):
    rng = np.random.default_rng(5)
    bias = rng.integers(480, 545, size=(2, 32, 48)).astype(np.uint16)
    flats = rng.integers(900, 1100, size=(1, 2, 32, 48)).astype(np.uint16)
    rep = V.validate_camera([{'iso': 100, 'bias': bias, 'flats': flats}], PAT, BLACK, WHITE, diag={'frames': [dict(REC), dict(REC)]},
                            models=('PD',), radius=64, flat_radius=256, structure=True)
    pd = rep['structure']['sessions'][0]['models']['PD']
    assert pd['synthetic']['pix_fixed_var'] is None and pd['log_ratio']['pix_fixed_var'] is None and 'fewer than 3' in pd['split']
    assert pd['synthetic']['pix_var'] is not None
