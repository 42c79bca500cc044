"""Burst stacking without a GPU: hand-worked cases of the NumPy restatement (tests/burst_ref.py), the operand widths of the rule, the
host half of eld_amd.burst (ptc_points, burst_gain, the flicker check, argument errors), the library's argument checks, calibrate's
manifest with "bursts", and the statistical recovery of K by the restatement alone.

The statistical bounds.  Scene 5 + 6000 ((x + 0.37 y) / (W + 0.37 H))^2 DN on 64 x 96, N = 16, K = 2 DN/e-, read noise 3 DN, black 512,
white 16383, seeds 0..11, k = 5, min_dev = 2, min_sites = 64, measured with this file's restatement:
    largest relative error of K            2.4385 %  (seed 8)    -> K_REL_BOUND = twice that
    largest relative error of sigma0^2     746.8 %   (seed 8: 76.9 against 9.083)    -> C_REL_BOUND = twice that
The intercept's spread is far beyond K's: a 64 x 96 frame gives 1536 sites per colour group, so only the bins above about 500 DN hold the
64 sites a point needs, and the intercept is an extrapolation of the line over 500 DN and more; its own measured spread is the bound, as
it is recorded in DESIGN.md sec. 20."""
import ctypes
import json
import os

import numpy as np
import pytest

import burst_ref as R
from pairstats_ref import bin_loop

K_REL_BOUND = 2 * 0.024385
C_REL_BOUND = 2 * 7.4682
C_TRUE = 3.0 ** 2 + 1.0 / 12.0
BAYER = (2, [0, 1, 3, 2], 4, [512] * 4, 16383)


def _one_site(samples, k2q=100, min_dev=2, white=16383):
    fr = np.asarray(samples, np.uint16).reshape(-1, 1, 1)
    fr = np.broadcast_to(fr, (fr.shape[0], 2, 2)).copy()
    mean, kept, ptc = R.stack(fr, 2, [0, 0, 0, 0], 1, [0] * 4, white, k2q, min_dev)
    return int(mean[0, 0]), int(kept[0, 0]), ptc


def test_outlier_is_rejected_at_four_frames_and_kept_at_three():
    mean, kept, ptc = _one_site([100, 102, 101, 900])
    # for 900: the others are 100, 102, 101 (mean 101, deviations far below 799); for 100: the others include 900
    assert (mean, kept) == (101, 3)
    assert R.site_loop([100, 102, 101, 900], 100, 2)[:3] == (101, 3, [False, False, False, True])
    assert not ptc.any()                                           # a site with a rejection is not eligible
    mean, kept, ptc = _one_site([100, 102, 900])                   # N = 3: the rule is off
    assert (mean, kept) == ((1102 * 2 + 3) // 6, 3) and ptc[0, :, 0].sum() == 4
    assert R.site_loop([100, 102, 900], 100, 2)[2] == [False] * 3


def test_one_dn_step_on_a_constant_site_is_kept_by_the_floor():
    xs = [700] * 7 + [701]
    assert _one_site(xs, min_dev=1)[:2] == (700, 8)               # (2 * 5601 + 8) // 16 = 700
    assert _one_site(xs, min_dev=2)[:2] == (700, 8)
    # without the floor V1 = 0 for the step's sample and any deviation at all rejects it
    assert _one_site(xs, min_dev=0)[:2] == (700, 7)
    assert R.site_loop(xs, 100, 0)[2] == [False] * 7 + [True]


def test_round_half_up():
    assert _one_site([10, 11], k2q=0)[0] == 11                     # 10.5 -> 11
    assert _one_site([10, 11, 11, 11], k2q=0)[0] == 11             # 10.75
    assert _one_site([10, 10, 10, 11], k2q=0)[0] == 10             # 10.25
    assert _one_site([0, 1, 0, 1, 0, 1], k2q=0)[0] == 1            # 0.5 -> 1
    assert _one_site([65535, 65534], k2q=0)[0] == 65535


def test_every_intermediate_fits_the_widths_claimed():
    for xs in ([0, 65535] * 128, [65535] * 256, [0] * 255 + [65535], [65535] * 255 + [0], [0] * 128 + [65535] * 128):
        for k2q, min_dev in ((256, 0), (1, 65535), (100, 2)):
            mean, n, flags, w = R.site_loop(xs, k2q, min_dev)
            assert w['S1'] < 1 << 24 and w['S2'] < 1 << 40 and w['d'] < 1 << 24 and w['d2'] < 1 << 48
            assert w['V1'] < 1 << 46 and w['V'] < 1 << 46 and w['left'] < 1 << 58 and w['right'] < 1 << 62
            assert 2 * sum(xs) + 256 < 1 << 26
            x = np.asarray(xs, np.int64).reshape(-1, 1, 1)
            assert R.reject_mask(x, k2q, min_dev).reshape(-1).tolist() == flags      # int64 NumPy and Python integers agree
    # alternating 0 / 65535: V1 is at its bound (N - 1)^2 R^2 / 4 up to the odd count's remainder
    w = R.site_loop([0, 65535] * 128, 256, 0)[3]
    assert w['V1'] == 255 * (127 * 65535 ** 2) - (127 * 65535) ** 2 or w['V1'] == 255 * (128 * 65535 ** 2) - (128 * 65535) ** 2
    assert R.site_loop([0, 65535] * 128, 100, 2)[:2] == (32768, 256)          # 32767.5 rounds up; nothing is rejected
    assert _one_site([0, 65535] * 128, white=65536)[1] == 0                  # kept 256 is written as 0


def test_the_rule_is_monotone_in_the_distance_from_the_mean():
    """What lets a kernel look twice only where the site's maximum or minimum is rejected: N V1 = (N - 1) V - d^2."""
    rng = np.random.default_rng(3)
    for _ in range(300):
        N = int(rng.integers(4, 12))
        xs = rng.integers(500, 520, size=N)
        xs[rng.integers(0, N, size=2)] += rng.integers(-400, 400, size=2)
        xs = np.clip(xs, 0, 65535)
        k2q, min_dev = int(rng.integers(1, 257)), int(rng.integers(0, 4))
        _, n, flags, _ = R.site_loop(xs, k2q, min_dev)
        S1, S2 = int(xs.sum()), int((xs * xs).sum())
        for v, r in zip(xs, flags):
            d = N * int(v) - S1
            assert N * ((N - 1) * (S2 - int(v) ** 2) - (S1 - int(v)) ** 2) == (N - 1) * (N * S2 - S1 * S1) - d * d
            assert all(r2 for v2, r2 in zip(xs, flags) if abs(N * int(v2) - S1) >= abs(d)) or not r
        # the rule as one test on the site's sums: d^2 A > V B; the furthest sample decides whether anything is rejected
        A, B, V = 4 * N * (N - 2) + k2q * (N - 1), k2q * (N - 1) ** 2, N * S2 - S1 * S1
        for v, r in zip(xs, flags):
            d = N * int(v) - S1
            assert r == (abs(d) > (N - 1) * min_dev and d * d * A > V * B)
        dmax = max(N * int(xs.max()) - S1, S1 - N * int(xs.min()))
        assert any(flags) == (dmax > (N - 1) * min_dev and dmax * dmax * A > V * B)
        if k2q >= 6:
            assert n >= 1                                          # 4 N <= k2q (N - 1): the rule cannot reject every sample
    assert R.site_loop([0, 0, 10, 10], 5, 0)[1] == 0               # ... below that it can: n = 0 writes mean 0
    assert R.site_loop([0, 0, 10, 10], 5, 0)[0] == 0 and R.site_loop([0, 0, 10, 10], 6, 0)[1] == 4


def test_eligibility_and_bins():
    # four sites of one group: clean, touching 0, saturated, flagged
    fr = np.zeros((4, 2, 2), np.uint16)
    fr[:, 0, 0] = [600, 602, 604, 602]
    fr[:, 0, 1] = [3, 0, 2, 1]
    fr[:, 1, 0] = [16383, 16000, 16100, 16200]
    fr[:, 1, 1] = [600, 602, 604, 602]
    mask = np.zeros((2, 2), bool)
    mask[1, 1] = True
    mean, kept, ptc = R.stack(fr, 2, [0, 0, 0, 0], 1, [512] * 4, 16383, 100, 2, mask=mask)
    assert mean.tolist() == [[602, 2], [16171, 602]] and kept.tolist() == [[4, 4], [4, 4]]       # a flagged site still gets its mean
    b = bin_loop(602, 512, 16383)
    S1, S2 = 2408, 600 ** 2 + 2 * 602 ** 2 + 604 ** 2
    want = np.zeros((1, R.NB, 4), np.int64)
    want[0, b] = [1, S1, 4 * S2 - S1 * S1, 0]
    assert np.array_equal(ptc, want)


def test_ptc_points_recombines_halves_beyond_32_bits():
    from eld_amd.burst import NB, ptc_points
    assert NB == R.NB
    ptc = np.zeros((2, NB, 4), np.int64)
    ptc[0, 30] = [1000, 16 * 1000 * 1512, (1 << 32) - 5, 7]       # sum V = 7 * 2^32 + 2^32 - 5
    ptc[1, 59] = [3, 16 * 3 * 60000, 12345, (1 << 21) + 1]        # sum V beyond 2^53
    q = ptc_points({'ptc': ptc, 'N': 16, 'group_black': [512, 500]})
    assert q['n'][0, 30] == 1000 and q['mu'][0, 30] == 1000.0 and q['mu'][1, 59] == 59500.0
    assert q['var'][0, 30] == (8 * (1 << 32) - 5) / (16 * 15 * 1000)
    assert q['var'][1, 59] == ((((1 << 21) + 1) << 32) + 12345) / (16 * 15 * 3)
    assert np.isnan(q['mu'][0, 0]) and np.isnan(q['var'][1, 1]) and q['n'].sum() == 1003
    n, mu, var = R.points(ptc, 16, [512, 500])
    assert np.array_equal(mu, q['mu'], equal_nan=True) and np.array_equal(var, q['var'], equal_nan=True)


def _line_ptc(K, c, bins, n=1000, N=16):
    from eld_amd.evaluate import bin_lower_edges
    ptc = np.zeros((1, R.NB, 4), np.int64)
    for b in bins:
        mu = int(bin_lower_edges()[b]) + 1
        V = int(round((K * mu + c) * N * (N - 1))) * n
        ptc[0, b] = [n, N * n * (mu + 512), V % (1 << 32), V >> 32]
    return {'ptc': ptc, 'N': N, 'group_black': [512]}


def test_burst_gain_fits_the_line_and_refuses_what_it_cannot():
    from eld_amd.burst import burst_gain
    fit = burst_gain([_line_ptc(2.0, 9.0, (20, 30, 40, 50))])
    assert abs(fit['K'] - 2.0) < 1e-3 and abs(fit['sigma0_sq'] - 9.0) < 0.1 and fit['mu'].size == 4
    two = burst_gain([_line_ptc(2.0, 9.0, (20, 30)), _line_ptc(2.0, 9.0, (40,))])     # points of several stacks are pooled
    assert abs(two['K'] - 2.0) < 1e-3 and two['mu'].size == 3
    with pytest.raises(ValueError, match='fewer than two usable'):
        burst_gain([_line_ptc(2.0, 9.0, (30,))])                                      # one point
    with pytest.raises(ValueError, match='fewer than two usable'):
        burst_gain([_line_ptc(2.0, 9.0, (30, 40), n=63)])                             # below min_sites
    with pytest.raises(ValueError, match='fewer than two usable'):
        burst_gain([_line_ptc(2.0, 9.0, (0, 60, 30))])                                # bins 0 and 60 never count
    with pytest.raises(ValueError, match='not a positive gain'):
        burst_gain([_line_ptc(0.0, 50.0, (20, 30, 40))])                              # flat slope
    with pytest.raises(ValueError, match='not a positive gain'):
        burst_gain([_line_ptc(-0.001, 500.0, (20, 30, 40))])
    assert burst_gain([_line_ptc(2.0, 9.0, (30, 40), n=63)], min_sites=10)['mu'].size == 2


def test_flicker_check():
    from eld_amd.burst import FLICKER_FACTOR, flicker_check
    stack = _line_ptc(2.0, 9.0, (30, 40), n=50000)
    sum_v = sum((int(v[3]) << 32) + int(v[2]) for v in stack['ptc'].reshape(-1, 4))
    expected = np.sqrt(sum_v / (16 * 15)) / 100000
    calm = flicker_check(1000.0 + expected * np.array([1.0, -1.0] * 8), 100000, stack)
    assert calm['warning'] is None and abs(calm['expected'] - expected) < 1e-12 and 0.9 < calm['ratio'] < 1.1
    lit = flicker_check(1000.0 * (1.0 + 0.01 * np.array([1.0, -1.0] * 8)), 100000, stack)
    assert lit['ratio'] > FLICKER_FACTOR and 'not constant' in lit['warning'] and abs(lit['rel_spread'] - 0.0103) < 1e-3


def test_stack_burst_refuses_on_the_host():
    from eld_amd.burst import stack_burst
    ok = np.zeros((4, 4, 8), np.uint16)
    bad = [((np.zeros((1, 4, 8), np.uint16),), {}), ((np.zeros((257, 2, 2), np.uint16),), {}), ((np.zeros((4, 8), np.uint16),), {}),
           ((ok.astype(np.int32),), {}), ((np.zeros((4, 3, 8), np.uint16),), {}), ((ok, 'foveon'), {}), ((ok,), {'k': 8.1}), ((ok,), {'k': -1}),
           ((ok,), {'k': float('nan')}), ((ok,), {'min_dev': -1}), ((ok,), {'min_dev': 1.5}), ((ok,), {'min_dev': 65536}),
           ((ok,), {'white_level': 0}), ((ok,), {'black_level': [1, 2, 3]}), ((ok,), {'raw_pattern': [[0, 1], [1, 2]]}),
           ((np.zeros((4, 4, 8), np.uint16), 'xtrans'), {}), ((ok,), {'defects': 'no/such/map.npz'})]
    for args, kw in bad:
        with pytest.raises(ValueError):
            stack_burst(*args, **kw)


def test_library_argument_errors_without_gpu(eld_lib):
    E = -1

    def call(frames=ctypes.c_void_p(16), N=4, Hm=4, Wm=8, p=2, group=(0, 1, 3, 2), G=4, black=(512,) * 4, white=16383, k2q=100, min_dev=2,
             mean=ctypes.c_void_p(16), ptc=None, ws_bytes=0):
        g = None if group is None else (ctypes.c_int * len(group))(*group)
        b = None if black is None else (ctypes.c_int32 * len(black))(*black)
        return eld_lib.eld_burst_stack_u16(frames, N, Hm, Wm, p, g, G, b, white, None, k2q, min_dev, mean, None, ptc, None, ws_bytes, None)

    for kw in (dict(N=1), dict(N=257), dict(N=0), dict(k2q=257), dict(k2q=-1), dict(min_dev=-1), dict(min_dev=65536), dict(p=3), dict(frames=None),
               dict(mean=None), dict(G=0), dict(G=5), dict(group=None), dict(black=None), dict(group=(0, 1, 4, 2)), dict(black=(512, 65536, 0, 0)),
               dict(white=0), dict(white=65537), dict(Hm=1 << 16, Wm=1 << 15), dict(Hm=-1), dict(frames=ctypes.c_void_p(17)),
               dict(mean=ctypes.c_void_p(17)), dict(ptc=ctypes.c_void_p(20))):
        assert call(**kw) == E, kw
    assert call(Hm=0, frames=None, mean=None) == 0                 # an empty image without ptc: nothing to zero, nothing to launch
    assert call(Wm=0, frames=None, mean=None) == 0
    assert eld_lib.eld_burst_stack_workspace_bytes(16, 4000, 6000) == 0      # no workspace in this implementation: ELD_EWS cannot occur


def _write_session_files(tmp_path, with_gain):
    rng = np.random.default_rng(0)
    names = []
    for i in range(5):
        np.save(tmp_path / ('f%d.npy' % i), rng.integers(500, 530, size=(4, 8)).astype(np.uint16))
        names.append('f%d.npy' % i)
    s0 = {'iso': 100, 'bias': names[:2]}
    s1 = {'iso': 400, 'bias': names[2:4]}
    if with_gain:
        s0['bursts'] = [names[:4], names[1:5]]
        s1['bursts'] = [names[:3]]
        s1['flats'] = [[names[0], names[1]]]
    m = {'raw_pattern': [[0, 1], [3, 2]], 'black_level': [512] * 4, 'white_level': 16383, 'sessions': [s0, s1]}
    path = tmp_path / 'manifest.json'
    path.write_text(json.dumps(m))
    return str(path)


def test_manifest_accepts_bursts(tmp_path):
    from eld_amd import calibrate as CAL
    sessions = CAL.load_manifest(_write_session_files(tmp_path, True))[0]
    assert 'flats' not in sessions[0] and [b.shape for b in sessions[0]['bursts']] == [(4, 4, 8), (4, 4, 8)]
    assert sessions[1]['flats'].shape == (1, 2, 4, 8) and sessions[1]['bursts'][0].shape == (3, 4, 8)
    assert np.array_equal(sessions[0]['bursts'][1][0], np.load(os.path.join(str(tmp_path), 'f1.npy')))
    CAL._check_sessions(sessions)
    with pytest.raises(ValueError, match="'flats'.*'bursts'"):
        CAL.load_manifest(_write_session_files(tmp_path, False))


def test_session_with_neither_flats_nor_bursts_names_both():
    from eld_amd import calibrate as CAL
    bias = np.zeros((2, 4, 8), np.uint16)
    burst = np.zeros((4, 4, 8), np.uint16)
    with pytest.raises(ValueError, match="neither 'flats'.*nor 'bursts'"):
        CAL.calibrate_camera([{'iso': 1, 'bias': bias}, {'iso': 2, 'bias': bias, 'bursts': [burst]}], [[0, 1], [3, 2]], [512] * 4, 16383)
    for bursts in ([], burst, [burst[:1]], [np.zeros((4, 4, 6), np.uint16)], [burst.astype(np.int32)]):
        with pytest.raises(ValueError):
            CAL._check_sessions([{'iso': 1, 'bias': bias, 'bursts': bursts}, {'iso': 2, 'bias': bias, 'bursts': [burst]}])
    CAL._check_sessions([{'iso': 1, 'bias': bias, 'bursts': [burst]}, {'iso': 2, 'bias': bias, 'bursts': [burst, burst]}])


@pytest.fixture(scope='module')
def recovered():
    out = []
    for seed in range(12):
        fr = R.scene_burst(seed)
        mean, kept, ptc = R.stack(fr, *BAYER, 100, 2)
        K, c = R.gain([R.points(ptc, 16, [512] * 4)])
        out.append((K, c, float(np.mean(kept != 16)), ptc))
    return out


def test_restatement_recovers_the_gain(recovered):
    from eld_amd.burst import burst_gain
    errs = [abs(K - 2.0) / 2.0 for K, _, _, _ in recovered]
    cerr = [abs(c - C_TRUE) / C_TRUE for _, c, _, _ in recovered]
    print('largest relative error of K %.5f, of the intercept %.4f; share of sites with a rejection %.4f'
          % (max(errs), max(cerr), np.mean([r for _, _, r, _ in recovered])))
    assert max(errs) <= K_REL_BOUND and max(cerr) <= C_REL_BOUND
    assert max(errs) > K_REL_BOUND / 4                             # the bound is twice the measured maximum, not a loose guess
    assert 0.001 < np.mean([r for _, _, r, _ in recovered]) < 0.01          # about 0.4 % of the sites lose a sample at N = 16, k = 5
    for K, c, _, ptc in recovered[:3]:                             # the package's fit is the restatement's
        fit = burst_gain([{'ptc': ptc, 'N': 16, 'group_black': [512] * 4}])
        assert abs(fit['K'] - K) < 1e-9 * K and abs(fit['sigma0_sq'] - c) < 1e-6
