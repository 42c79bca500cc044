"""The structure estimators on planted components (no GPU: the integer sums come from the NumPy restatement, tests/structure_ref.py).

Every bound is 5 standard errors, the standard error derived from the counts: a variance estimated from N independent values of variance v
has s.e. v sqrt(2 / (N - 1)); a covariance of two series of variances va, vb and covariance c has s.e. sqrt((va vb + c^2) / (N - 1))."""
import inspect
import math

import numpy as np
import pytest

from eld_amd import structure as ST
from eld_amd import validate as V

from structure_ref import stats_ref, sums_dict

PAT = [[0, 1], [3, 2]]
GROUPS = np.array(PAT)
HM, WM = 256, 384
SW, SR, SC, SF = 6.0, 1.5, 1.0, 3.0              # white, temporal per sensor row, fixed per column, fixed per pixel (sigma, DN)
Q = 1.0 / 12.0                                   # rounding to integer codes adds a uniform error of variance 1/12 to the white part


def planted(seed, F=2, sw=SW, sr=SR, sc=SC, sf=SF, hm=HM, wm=WM, rows=None):
    rng = np.random.default_rng(seed)
    colfix = sc * rng.standard_normal(wm)
    pixfix = sf * rng.standard_normal((hm, wm))
    out = []
    for f in range(F):
        r = sr * rng.standard_normal(hm) if rows is None else rows[f]
        out.append(np.rint(2048.0 + sw * rng.standard_normal((hm, wm)) + r[:, None] + colfix[None, :] + pixfix))
    return np.stack(out).astype(np.uint16)


@pytest.fixture(scope='module')
def planted_stats():
    u = planted(2024)
    sums = sums_dict(u, 2, [2048] * 4, pairs=[(0, 1)])
    return sums, ST.structure_stats(sums, 'bayer', PAT, lags=8)


def within(values, expect, se):
    v = np.asarray(values, np.float64)
    assert np.all(np.abs(v - expect) < 5.0 * se), (v.tolist(), expect, se)


def test_planted_components_are_recovered(planted_stats):
    _, st = planted_stats
    n_r, n_c = WM // 2, HM // 2                  # sites behind a row entry, a column entry (a Bayer group is one cell)
    N_r, N_c, N = HM // 2, WM // 2, (HM // 2) * (WM // 2)
    site = SW ** 2 + Q + SF ** 2                 # what is independent from site to site within a frame
    total = site + SR ** 2 + SC ** 2
    for fr in st['frames']:
        within(fr['pix_var'], total, math.sqrt(2 * (site ** 2 / N + SR ** 4 / (N_r - 1) + SC ** 4 / (N_c - 1))))
        within(fr['row_var'], SR ** 2, (SR ** 2 + site / n_r) * math.sqrt(2.0 / (N_r - 1)))
        within(fr['col_var'], SC ** 2, (SC ** 2 + site / n_c) * math.sqrt(2.0 / (N_c - 1)))
        va = SR ** 2 + site / n_r                # a row mean of one column phase; the two phases share the row term only
        within(fr['row_var_sensor'], SR ** 2, math.sqrt((va * va + SR ** 4) / (HM - 1)))
        vc = SC ** 2 + site / n_c                # a column mean of one row phase; the two phases share the column offset only
        within(fr['col_var_sensor'], SC ** 2, math.sqrt((vc * vc + SC ** 4) / (WM - 1)))
    pr = st['pairs'][0]
    fixed = SF ** 2 + SC ** 2                    # per site, what the two frames share: the pixel and the column pattern
    within(pr['pix_fixed_var'], fixed, math.sqrt((total ** 2 + fixed ** 2) / N + 2 * SC ** 4 / (N_c - 1) + SR ** 4 / (N_r - 1)))
    cc = SC ** 2 + SF ** 2 / n_c
    within(pr['col_fixed_var'], SC ** 2, math.sqrt((vc * vc + cc * cc) / (N_c - 1)))
    cr = SF ** 2 / n_r
    within(pr['row_fixed_var'], 0.0, math.sqrt((va * va + cr * cr) / (N_r - 1)))
    se_row = (SR ** 2 + site / n_r) * math.sqrt(2.0 / (N_r - 1))
    within(pr['row_temporal_var'], SR ** 2, math.sqrt(se_row ** 2 / 2 + (va * va + cr * cr) / (N_r - 1)))
    se_pix = math.sqrt(2 * (site ** 2 / N + SR ** 4 / (N_r - 1) + SC ** 4 / (N_c - 1)))
    se_fix = math.sqrt((total ** 2 + fixed ** 2) / N + 2 * SC ** 4 / (N_c - 1) + SR ** 4 / (N_r - 1))
    within(pr['pix_temporal_var'], SW ** 2 + Q + SR ** 2, math.sqrt(se_pix ** 2 / 2 + se_fix ** 2))      # mean of two totals minus the fixed part


def test_stats_equal_the_restatement(planted_stats):
    sums, st = planted_stats
    ref = stats_ref(sums, GROUPS, 4)
    for a, b in zip(st['frames'], ref['frames']):
        for k in ('pix_var', 'row_var', 'col_var', 'row_var_sensor', 'col_var_sensor'):
            np.testing.assert_allclose(a[k], b[k], rtol=1e-9, atol=1e-9)
    for a, b in zip(st['pairs'], ref['pairs']):
        for k in ('pix_fixed_var', 'row_fixed_var', 'col_fixed_var'):
            np.testing.assert_allclose(a[k], b[k], rtol=1e-9, atol=1e-9)


def test_white_noise_alone_shows_no_structure():
    u = planted(7, sr=0.0, sc=0.0, sf=0.0)
    st = ST.structure_stats(sums_dict(u, 2, [2048] * 4, pairs=[(0, 1)]), 'bayer', PAT, lags=8)
    w = SW ** 2 + Q
    n_r, n_c, N_r, N_c, N = WM // 2, HM // 2, HM // 2, WM // 2, (HM // 2) * (WM // 2)
    for fr in st['frames']:
        within(fr['row_var'], 0.0, w / n_r * math.sqrt(2.0 / (N_r - 1)))
        within(fr['col_var'], 0.0, w / n_c * math.sqrt(2.0 / (N_c - 1)))
        within(fr['row_var_sensor'], 0.0, w / n_r / math.sqrt(HM - 1))
        within(fr['col_var_sensor'], 0.0, w / n_c / math.sqrt(WM - 1))
        assert np.all(np.abs(fr['row_acf']) < 5.0 / math.sqrt(HM))
        assert np.all(np.abs(fr['col_acf']) < 5.0 / math.sqrt(WM))
    pr = st['pairs'][0]
    within(pr['pix_fixed_var'], 0.0, w / math.sqrt(N))
    within(pr['row_fixed_var'], 0.0, w / n_r / math.sqrt(N_r - 1))
    within(pr['col_fixed_var'], 0.0, w / n_c / math.sqrt(N_c - 1))


def test_ar1_banding_shows_in_the_row_autocorrelation():
    """Bartlett: for an AR(1) series var r_1 ~ (1 - rho^2) / N.  The white part dilutes the expectation to rho s / (s + w / n), s the row
    variance, w / n the sampling share of the white noise in a sensor-row mean."""
    rho, hm, wm, s, sw = 0.8, 1024, 128, 4.0, 2.0
    rng = np.random.default_rng(11)
    e = rng.standard_normal(hm) * math.sqrt(s * (1 - rho ** 2))
    r = np.empty(hm)
    r[0] = rng.standard_normal() * math.sqrt(s)
    for i in range(1, hm):
        r[i] = rho * r[i - 1] + e[i]
    u = planted(12, F=1, sw=sw, sc=0.0, sf=0.0, hm=hm, wm=wm, rows=[r])
    st = ST.structure_stats(sums_dict(u, 2, [2048] * 4), 'bayer', PAT, lags=4)
    expect = rho * s / (s + (sw ** 2 + Q) / wm)
    se = math.sqrt((1 - rho ** 2) / hm)
    assert abs(st['frames'][0]['row_acf'][0] - expect) < 5 * se
    assert abs(st['frames'][0]['row_acf'][0] - rho) < 5 * se          # the dilution is far inside the bound at this size
    assert abs(st['frames'][0]['col_acf'][0]) < 5.0 / math.sqrt(wm)


def test_fully_masked_lines_are_dropped():
    u = planted(5, F=2, hm=48, wm=64)
    mask = np.zeros((48, 64), bool)
    mask[10, :] = True
    mask[:, 33] = True
    sums = sums_dict(u, 2, [2048] * 4, pairs=[(0, 1)], mask=mask)
    assert np.all(sums['row'][:, 10] == 0) and np.all(sums['col'][:, 33] == 0)
    st = ST.structure_stats(sums, 'bayer', PAT, lags=3)
    ref = stats_ref(sums, GROUPS, 4)
    for k in ('pix_var', 'row_var', 'col_var'):
        assert np.all(np.isfinite(st['frames'][0][k]))
        np.testing.assert_allclose(st['frames'][0][k], ref['frames'][0][k], rtol=1e-9, atol=1e-9)
    assert np.all(np.isfinite(st['frames'][0]['row_acf']))


def test_xtrans_groups():
    from xtrans_ref import xtrans_pattern
    pat = xtrans_pattern()
    rng = np.random.default_rng(3)
    u = np.rint(1000 + 5 * rng.standard_normal((2, 72, 96))).astype(np.uint16)
    sums = sums_dict(u, 6, [1000] * 36, pairs=[(0, 1)])
    st = ST.structure_stats(sums, 'xtrans', pat, lags=2)
    assert st['groups'] == 3 and len(st['frames'][0]['pix_var']) == 3
    p, groups, G = V.group_map_u16('xtrans', pat)
    ref = stats_ref(sums, np.array(groups).reshape(6, 6), 3)
    for k in ('pix_var', 'row_var', 'col_var', 'row_var_sensor', 'col_var_sensor'):
        np.testing.assert_allclose(st['frames'][1][k], ref['frames'][1][k], rtol=1e-9, atol=1e-9)
    within(st['frames'][0]['pix_var'], 25 + Q, (25 + Q) * math.sqrt(2.0 / (72 * 96 * 8 / 36 - 1)))


def test_arguments():
    sums = sums_dict(planted(1, F=1, hm=8, wm=8), 2, [2048] * 4)
    for bad in (0, -1, True, 2.5, 5000):
        with pytest.raises(ValueError):
            ST.structure_stats(sums, 'bayer', PAT, lags=bad)
    with pytest.raises(ValueError):
        ST.structure_stats(sums, 'xtrans', __import__('xtrans_ref').xtrans_pattern())      # the sums were taken with period 2
    for bad in ([1, 2, 3], [0, 0, 0, 65536], [0, 0, 0, -1], [0.5, 0, 0, 0], None):
        with pytest.raises(ValueError):
            ST._centre(bad, 2)
    for bad in ([[0, 2]], [[0, -1]], [0, 1, 1]):
        with pytest.raises(ValueError):
            ST._pairs(bad, 2)
    assert ST.cell_centres('bayer', [[2, 3], [1, 0]], [512.2, 520, 500, 531.6]).tolist() == [[500, 532], [520, 512]]


def test_cli_and_signature():
    a = V.parser().parse_args(['m.json'])
    assert a.structure is False and a.lags == 8
    a = V.parser().parse_args(['m.json', '--structure', '--lags', '3'])
    assert a.structure is True and a.lags == 3
    for bad in ('0', '-2', 'x'):
        with pytest.raises(SystemExit):
            V.parser().parse_args(['m.json', '--structure', '--lags', bad])
    sig = inspect.signature(V.validate_camera)
    names = list(sig.parameters)
    assert names[:17] == ['sessions', 'raw_pattern', 'black_level', 'white_level', 'table', 'diag', 'models', 'source', 'cfa', 'defects', 'radius',
                          'flat_radius', 'seed', 'alpha', 'keep_hist', 'structure', 'lags']
    assert sig.parameters['structure'].default is False and sig.parameters['lags'].default == 8


def test_table_lines_and_log_ratio():
    real = {k: 1.0 for k in ST.COMPONENTS}
    syn = dict(real, col_var_sensor=-0.25, pix_fixed_var=None, row_var_sensor=math.e)
    lr = ST.log_ratio(real, syn)
    assert lr['row_var_sensor'] == pytest.approx(1.0) and lr['col_var_sensor'] is None and lr['pix_fixed_var'] is None
    rep = {'models': ['PGR'], 'structure': {'sessions': [{'iso': 800, 'real': real, 'models': {'PGR': {'synthetic': syn}}}]}}
    lines = V.structure_lines(rep)
    assert len(lines) == 2 and 'PGR' in lines[1] and '-0.500' in lines[1] and lines[1].count('|') == 4
