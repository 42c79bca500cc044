"""CPU tests of the defective-pixel maps (eld_amd/defects.py): the NumPy restatement (tests/defects_ref.py) on hand-made cases, the
X-Trans neighbour-count claim by brute force, DefectMap, every argument error before device work, the count-aware host derivations of
the calibration, and the detector's quality on the restatement alone (which lets the GPU tests be pure equality tests)."""
import types

import numpy as np
import pytest

import defects_ref as R
from eld_amd import calibrate as CAL
from eld_amd import defects as DF
from eld_amd.defects import DefectMap

from test_calib_cpu import PATTERNS, flat_sums_ref, sums_ref, tukey_quantile
from xtrans_ref import cell_flat_sums_ref, cell_sums_ref, xtrans_pattern

XPAT = xtrans_pattern()
RGGB = [[0, 1], [3, 2]]


# ---- 1. the restatement on hand-made cases ------------------------------------------------------------------------------------------
def test_lower_median_and_ties():
    assert R.lower_median([5]) == 5
    assert R.lower_median([4, 9]) == 4                       # rank (2 - 1) // 2 = 0
    assert R.lower_median([7, 1, 7, 3]) == 3                 # 1 3 7 7 -> rank 1
    assert R.lower_median([2, 2, 9, 9, 9, 9, 2, 2]) == 2     # a tie across the middle: rank 3 of 2 2 2 2 9 9 9 9
    assert R.lower_median([3, 1, 2]) == 2


def test_bayer_corner_and_interior_by_hand():
    cls = R.class_map(8, 8, 'bayer', RGGB)
    assert R.neighbours(cls, 0, 0, 2) == [(0, 2), (2, 0), (2, 2)]                                  # 3 in a corner
    assert len(R.neighbours(cls, 0, 3, 2)) == 5 and len(R.neighbours(cls, 4, 4, 2)) == 8
    S = np.arange(64, dtype=np.uint16).reshape(1, 8, 8) * 3
    S[0, 0, 0], S[0, 4, 4] = 1000, 0
    D = R.deviation(S, cls, 2)
    assert D[0, 0] == 1000 - sorted([6, 48, 54])[1]                                                # lower median of 3 = the middle
    nb = sorted(int(S[0, y, x]) for y, x in R.neighbours(cls, 4, 4, 2))
    assert D[4, 4] == 0 - nb[3]
    for y, x in [(0, 0), (7, 7), (0, 5), (3, 0), (4, 4)]:                                          # the vectorised form equals the loops
        assert D[y, x] == int(S[0, y, x]) - R.lower_median([S[0, yy, xx] for yy, xx in R.neighbours(cls, y, x, 2)])


@pytest.mark.parametrize('cfa,pat,rad,shape', [('bayer', RGGB, 2, (10, 12)), ('bayer', PATTERNS[2], 2, (6, 6)), ('xtrans', XPAT, 3, (13, 16))])
def test_repair_cluster_partly_flagged_neighbours_and_borders(cfa, pat, rad, shape):
    rng = np.random.default_rng(3)
    Hm, Wm = shape
    cls = R.class_map(Hm, Wm, cfa, pat)
    u = rng.integers(500, 530, (Hm, Wm)).astype(np.uint16)
    mask = np.zeros((Hm, Wm), bool)
    mask[2:4, 2:4] = True                                     # a 2 x 2 cluster: four classes (Bayer), mixed colours (X-Trans)
    mask[0, 0] = mask[Hm - 1, Wm - 1] = mask[0, Wm - 1] = mask[Hm - 1, 0] = True
    mask[4, 4] = mask[4, 2] = True                            # (4, 4)'s neighbour (4, 2) [Bayer] is flagged too
    u[mask] = 60000
    got = R.repair(u, mask, cls, rad)
    assert np.array_equal(got, R.repair_loops(u, mask, cls, rad))
    assert np.array_equal(got[~mask], u[~mask]) and got[mask].max() < 530
    for y, x in np.argwhere(mask):                            # no flagged site fed a repair
        vals = [u[yy, xx] for yy, xx in R.neighbours(cls, y, x, rad) if not mask[yy, xx]]
        assert 60000 not in vals and got[y, x] == R.lower_median(vals)
    assert np.array_equal(R.repair(np.stack([u, u]), mask, cls, rad), np.stack([got, got]))


def test_bitmap_packing():
    rng = np.random.default_rng(0)
    for Wm in (6, 31, 32, 33, 64, 70):
        mask = rng.random((5, Wm)) < 0.3
        words = R.pack_bitmap(mask)
        assert words.shape == (5, (Wm + 31) // 32) and np.array_equal(words, DF.pack_bitmap(mask))
        assert np.array_equal(DF.unpack_bitmap(words, Wm), mask)
        for y in range(5):
            for x in range(Wm):
                assert bool((int(words[y, x >> 5]) >> (x & 31)) & 1) == bool(mask[y, x])
    with pytest.raises(ValueError, match='beyond the row width'):
        DF.unpack_bitmap(np.array([[1 << 7]], np.uint32), 6)


# ---- 2. the X-Trans radius ------------------------------------------------------------------------------------------------------------
def test_xtrans_radius_is_the_smallest_with_three_neighbours(eld_lib):
    t = DF.xtrans_tables()
    sides = range(6, 19)
    assert R.xtrans_min_neighbours(XPAT, t['R'], sides) >= 3
    assert R.xtrans_min_neighbours(XPAT, t['R'] - 1, sides) < 3
    assert t['R'] == 3                                         # what DESIGN.md sec. 14 states


# ---- 3. DefectMap ----------------------------------------------------------------------------------------------------------------------
def test_defect_map_round_trip_and_from_sites(eld_lib, tmp_path):
    sites = [[5, 7], [0, 0], [5, 8], [9, 11]]
    m = DefectMap.from_sites(sites, (10, 12), 'bayer', PATTERNS[1])
    assert m.count == 4 and m.sites.dtype == np.int32 and m.sites.tolist() == [[0, 0], [5, 7], [5, 8], [9, 11]]      # row-major
    assert m.shape == (10, 12) and m.cfa == 'bayer' and np.array_equal(m.raw_pattern, PATTERNS[1])
    assert np.array_equal(m.words, R.pack_bitmap(m.mask)) and m.mask.sum() == 4
    p = m.save(str(tmp_path / 'd.npz'))
    with np.load(p, allow_pickle=False) as z:                  # readable without pickle
        assert sorted(z.files) == ['cfa', 'raw_pattern', 'shape', 'sites']
    b = DefectMap.load(p)
    assert b.shape == m.shape and b.cfa == m.cfa and np.array_equal(b.sites, m.sites) and np.array_equal(b.words, m.words)
    x = DefectMap.from_sites([[6, 6]], (12, 18), 'xtrans', XPAT)
    assert DefectMap.load(x.save(str(tmp_path / 'x.npz'))).cfa == 'xtrans'
    bare = x.save(str(tmp_path / 'bare'))                     # a name without the suffix: the path written comes back
    assert bare.endswith('bare.npz') and DefectMap.load(bare).count == 1
    assert DefectMap.from_sites(np.zeros((0, 2), np.int64), (12, 18), 'xtrans').count == 0
    assert np.array_equal(DefectMap.from_sites([], (4, 4)).raw_pattern, [[0, 1], [3, 2]])


def test_defect_map_refuses_bad_sites_and_an_all_flagged_neighbourhood(eld_lib):
    for bad in ([[10, 0]], [[0, -1]], [[1, 1], [1, 1]], [[0.5, 1.0]], [[1, 2, 3]]):
        with pytest.raises(ValueError):
            DefectMap.from_sites(bad, (10, 12))
    with pytest.raises(ValueError, match='cfa'):
        DefectMap.from_sites([[1, 1]], (10, 12), 'foveon')
    with pytest.raises(ValueError, match='at least 6'):
        DefectMap.from_sites([[1, 1]], (4, 12), 'xtrans')
    with pytest.raises(ValueError, match='not the 6x6 cell'):
        DefectMap.from_sites([[1, 1]], (12, 12), 'xtrans', np.roll(XPAT, 1, axis=1))
    corner = [[0, 0], [0, 2], [2, 0], [2, 2]]                   # (0, 0) and all three of its neighbours
    with pytest.raises(ValueError, match='no unflagged neighbour'):
        DefectMap.from_sites(corner, (10, 12))
    assert DefectMap.from_sites(corner[:3], (10, 12)).count == 3
    assert len(DF.stranded_sites(np.ones((6, 6), bool), np.asarray(RGGB), 2)) == 36


# ---- 4. argument errors, all before device work ---------------------------------------------------------------------------------------
class FakeNet:
    inference_precision = 'fp32'

    def parameters(self):
        raise AssertionError('device work before the argument checks')


def fake(cfa):
    from eld_amd.denoise import PLANES
    return types.SimpleNamespace(cfa=cfa, in_channels=PLANES[cfa], out_channels=PLANES[cfa], net=FakeNet())


def test_find_defects_and_repair_argument_errors(eld_lib):
    u = np.full((2, 8, 12), 512, np.uint16)
    for kw in (dict(k=0), dict(k=float('nan')), dict(k='8'), dict(floor_dn=-1), dict(thresholds=(5,)), dict(thresholds=(-1, 3)),
               dict(thresholds=(2.5, 3)), dict(thresholds=(1 << 31, 3)), dict(cfa='foveon'), dict(raw_pattern=[[0, 1], [1, 2]])):
        with pytest.raises(ValueError):
            DF.find_defects(u, **{'cfa': 'bayer', 'raw_pattern': RGGB, **kw})
    for bad in (u.astype(np.int32), u[:, :7], u[:, :, :7], np.zeros((0, 8, 12), np.uint16), u[None]):
        with pytest.raises(ValueError):
            DF.find_defects(bad, 'bayer', RGGB)
    with pytest.raises(ValueError):
        DF.find_defects(np.full((1, 4, 12), 512, np.uint16), 'xtrans', XPAT)
    m = DefectMap.from_sites([[1, 1]], (8, 12))
    for bad in (u.astype(np.float32), u[:, :6], np.zeros((8, 10), np.uint16), u[None], 'x'):
        with pytest.raises(ValueError):
            DF.repair(bad, m)
    with pytest.raises(ValueError, match='DefectMap'):
        DF.repair(u, 'map.npz')
    with pytest.raises(ValueError, match='out='):
        DF.repair(u, m, out=u.copy())
    # the raw binding refuses a Bayer pattern that is no permutation of 0..3 before any launch: every other argument is in order, and the
    # pointers are never dereferenced
    import ctypes
    p = ctypes.c_void_p(0x10000)
    for bad in ((ctypes.c_int * 4)(0, 1, 1, 2), (ctypes.c_int * 4)(0, 1, 4, 2), (ctypes.c_int * 4)(0, -1, 3, 2), None):
        assert eld_lib.eld_defect_deviation(p, 2, 8, 12, 2, bad, p, p, 1 << 20, None) == -1
        assert eld_lib.eld_defect_repair_u16(p, p, 2, 8, 12, 2, bad, p, None) == -1


def test_pipeline_argument_errors(eld_lib, tmp_path):
    from eld_amd.denoise import denoise_raw
    from eld_amd.framepool import FramePool
    m = DefectMap.from_sites([[1, 1]], (12, 24))
    mx = DefectMap.from_sites([[1, 1]], (12, 24), 'xtrans')
    raw = np.full((12, 24), 1100, np.uint16)
    for cfa, d in (('bayer', mx), ('xtrans', m), ('bayer', DefectMap.from_sites([], (12, 26))), ('bayer', 3), ('bayer', str(tmp_path / 'no.npz'))):
        with pytest.raises(ValueError):
            denoise_raw(fake(cfa), raw, cfa, defects=d)
        with pytest.raises(ValueError):
            FramePool([raw], cfa=cfa, defects=d)
    with pytest.raises(ValueError, match='frame 1'):
        FramePool([raw, np.full((14, 24), 1100, np.uint16)], defects=m)
    sess = [{'iso': 100 * (i + 1), 'bias': np.full((2, 12, 24), 512, np.uint16), 'flats': np.full((2, 2, 12, 24), 900, np.uint16)} for i in range(2)]
    for cfa, pat, d in (('bayer', RGGB, mx), ('xtrans', XPAT, m), ('bayer', RGGB, DefectMap.from_sites([], (12, 26))), ('bayer', RGGB, 'map.npz')):
        with pytest.raises(ValueError, match='defect'):
            CAL.calibrate_camera(sess, pat, [512] * 4, 16383, cfa=cfa, defects=d)
    with pytest.raises(ValueError, match='defect'):
        CAL.bias_frame_stats(sess[0]['bias'], RGGB, [512] * 4, defects=mx)
    with pytest.raises(ValueError, match='defect'):
        CAL.xtrans_flat_pair_stats(sess[0]['flats'], XPAT, [512] * 4, 16383, [0] * 3, defects=m)


# ---- 5. the count-aware host derivations --------------------------------------------------------------------------------------------------
def masked_bias_ref(u, group, blackmap, keep):
    """float64 evaluation over the unflagged pixels of one frame: (cb per group, rho, g_scale, R_scale, t of the kept sites)."""
    d = u.astype(np.float64) - blackmap
    cb = np.array([d[keep & (group == k)].mean() for k in range(group.max() + 1)])
    e = d - cb[group]
    n_y = keep.sum(axis=1)
    rho = np.where(keep, e, 0.0).sum(axis=1) / n_y
    t = e - rho[:, None]
    g = np.sqrt(np.mean(e[keep] ** 2))
    Rs = np.sqrt(max(0.0, np.mean(rho * rho) - np.mean(t[keep] ** 2) * np.mean(1.0 / n_y)))
    t32 = (((u.astype(np.float64) - blackmap) - cb[group]) - rho[:, None]).astype(np.float32)[keep]
    return cb, rho, g, Rs, t32


def masked_flat_ref(a, b, group, blackmap, white, cbm, keep):
    a, b = a.astype(np.int64), b.astype(np.int64)
    K = group.max() + 1
    mu, var, ok = np.empty(K), np.empty(K), np.empty(K, bool)
    for k in range(K):
        m = keep & (group == k)
        bbar = blackmap[m].mean()
        mu[k] = np.mean((a[m] + b[m]) / 2.0) - bbar - cbm[k]
        var[k] = np.var(a[m] - b[m]) / 2.0
        ok[k] = not np.any((a[m] >= white) | (b[m] >= white)) and 0 < mu[k] <= 0.8 * (white - bbar)
    return mu, var, ok


def _frames(rng, F, Hm, Wm):
    return np.clip(np.round(rng.normal(512, 4, (F, Hm, Wm)) + rng.normal(0, 2, (F, Hm, 1))), 0, 65535).astype(np.uint16)


def _defect_sites(rng, Hm, Wm, n):
    idx = rng.choice(Hm * Wm, n, replace=False)
    return np.stack([idx // Wm, idx % Wm], axis=1)


@pytest.mark.parametrize('pattern', PATTERNS)
def test_bayer_masked_derivations(eld_lib, pattern):
    rng = np.random.default_rng(21)
    F, Hm, Wm, white = 3, 34, 50, 4095
    black = np.array([512.0, 510.0, 514.0, 509.0])
    pat = np.asarray(pattern)
    u = _frames(rng, F, Hm, Wm)
    ab = rng.integers(500, 4000, (3, 2, Hm, Wm)).astype(np.uint16)
    dm = DefectMap.from_sites(_defect_sites(rng, Hm, Wm, 25), (Hm, Wm), 'bayer', pattern)
    ys, xs = dm.sites[:, 0], dm.sites[:, 1]
    u[:, ys, xs] = 9000
    ab[:, :, ys, xs] = 4095                                       # saturated: they must leave the saturation count too
    keep = ~dm.mask
    ch = R.class_map(Hm, Wm, 'bayer', pattern)
    uk = np.where(keep, u, 0)                                     # zeroed sites add nothing to any sum
    cs, rs = sums_ref(uk, pattern)
    cell_n, row_n = CAL._site_counts(dm, Hm, Wm, 2)
    nc = np.array([cell_n[pat == c][0] for c in range(4)])
    assert nc.sum() == Hm * Wm - 25 and row_n.sum() == Hm * Wm - 25
    d = CAL.bias_stats_from_sums_masked(cs, rs, pattern, black, Hm, Wm, nc, row_n)
    for f in range(F):
        cb, rho, g, Rs, _ = masked_bias_ref(u[f], ch, black[ch], keep)
        np.testing.assert_allclose(d['color_bias'][f], cb, rtol=0, atol=1e-9)
        np.testing.assert_allclose(d['row_offset'][f], rho, rtol=0, atol=1e-9)
        assert abs(d['g_scale'][f] - g) < 1e-9 and abs(d['R_scale'][f] - Rs) < 1e-9
    abk = np.where(keep, ab, 0)
    fs = flat_sums_ref(abk, pattern, white)
    cbm = d['color_bias'].mean(axis=0)
    fl = CAL.flat_stats_from_sums_masked(fs, black, white, cbm, Hm, Wm, nc)
    for p in range(3):
        mu, var, ok = masked_flat_ref(ab[p, 0], ab[p, 1], ch, black[ch], white, cbm, keep)
        np.testing.assert_allclose(fl['mu'][p], mu, rtol=0, atol=1e-9)
        np.testing.assert_allclose(fl['var'][p], var, rtol=1e-12)
        assert np.array_equal(fl['usable'][p], ok) and ok.all()
    # no flagged site: the bits of the existing functions
    cs, rs = sums_ref(u, pattern)
    full, full_r = np.full(4, Hm * Wm // 4), np.full((Hm, 2), Wm // 2)
    for a in (CAL.bias_stats_from_sums_masked(cs, rs, pattern, black, Hm, Wm), CAL.bias_stats_from_sums_masked(cs, rs, pattern, black, Hm, Wm, full, full_r)):
        b = CAL.bias_stats_from_sums(cs, rs, pattern, black, Hm, Wm)
        assert all(np.array_equal(a[k], b[k]) for k in b)
    fs = flat_sums_ref(ab, pattern, white)
    a, b = CAL.flat_stats_from_sums_masked(fs, black, white, cbm, Hm, Wm, full), CAL.flat_stats_from_sums(fs, black, white, cbm, Hm, Wm)
    assert all(np.array_equal(a[k], b[k]) for k in b)


def test_xtrans_masked_derivations(eld_lib):
    rng = np.random.default_rng(22)
    F, Hm, Wm, white = 2, 38, 52, 4095
    black = np.array([512.0, 510.0, 514.0, 510.0])
    u = _frames(rng, F, Hm, Wm)
    ab = rng.integers(500, 4000, (2, 2, Hm, Wm)).astype(np.uint16)
    dm = DefectMap.from_sites(_defect_sites(rng, Hm, Wm, 30), (Hm, Wm), 'xtrans', XPAT)
    ys, xs = dm.sites[:, 0], dm.sites[:, 1]
    u[:, ys, xs] = 9000
    ab[:, :, ys, xs] = 4095
    keep = ~dm.mask
    col = R.class_map(Hm, Wm, 'xtrans', XPAT)
    blackmap = black[XPAT[np.arange(Hm)[:, None] % 6, np.arange(Wm)[None, :] % 6]]
    cs, rs = cell_sums_ref(np.where(keep, u, 0), 6)
    cell_n, row_n = CAL._site_counts(dm, Hm, Wm, 6)
    d = CAL.xtrans_bias_stats_from_cell_sums_masked(cs, rs, XPAT, black, Hm, Wm, cell_n, row_n)
    for f in range(F):
        cb, rho, g, Rs, _ = masked_bias_ref(u[f], col, blackmap, keep)
        np.testing.assert_allclose(d['color_bias'][f], cb, rtol=0, atol=1e-9)
        np.testing.assert_allclose(d['row_offset'][f], rho, rtol=0, atol=1e-9)
        assert abs(d['g_scale'][f] - g) < 1e-9 and abs(d['R_scale'][f] - Rs) < 1e-9
    cbm = d['color_bias'].mean(axis=0)
    fs = cell_flat_sums_ref(np.where(keep, ab, 0), 6, white)
    fl = CAL.xtrans_flat_stats_from_cell_sums_masked(fs, XPAT, black, white, cbm, Hm, Wm, cell_n)
    for p in range(2):
        mu, var, ok = masked_flat_ref(ab[p, 0], ab[p, 1], col, blackmap, white, cbm, keep)
        np.testing.assert_allclose(fl['mu'][p], mu, rtol=0, atol=1e-9)
        np.testing.assert_allclose(fl['var'][p], var, rtol=1e-12)
        assert np.array_equal(fl['usable'][p], ok) and ok.all()
    cs, rs = cell_sums_ref(u, 6)
    a, b = CAL.xtrans_bias_stats_from_cell_sums_masked(cs, rs, XPAT, black, Hm, Wm), CAL.xtrans_bias_stats_from_cell_sums(cs, rs, XPAT, black, Hm, Wm)
    assert all(np.array_equal(a[k], b[k]) for k in b)
    full = CAL.cell_counts(Hm, Wm)
    a = CAL.xtrans_bias_stats_from_cell_sums_masked(cs, rs, XPAT, black, Hm, Wm, full, np.broadcast_to(CAL.cell_counts(1, Wm)[0], (Hm, 6)))
    assert all(np.array_equal(a[k], b[k]) for k in b)
    fs = cell_flat_sums_ref(ab, 6, white)
    a = CAL.xtrans_flat_stats_from_cell_sums_masked(fs, XPAT, black, white, cbm, Hm, Wm, full)
    b = CAL.xtrans_flat_stats_from_cell_sums(fs, XPAT, black, white, cbm, Hm, Wm)
    assert all(np.array_equal(a[k], b[k]) for k in b)


# ---- 6. detector quality, on the restatement alone ------------------------------------------------------------------------------------------
def synthetic_bias_stack(cfa, seed=5, F=4, Hm=192, Wm=240, n_hot=40, n_dead=20):
    """A bias stack with Gaussian row noise plus Tukey-lambda read noise at a release-table scale (SonyA7S2 at K ~ 2: G_scale ~ 3 DN,
    lambda -0.14, R_scale ~ 0.5 DN) on black 512, and injected defects at seeded sites: hot sites sit `amp` DN above their value in
    every frame (amp from 40 to 4000), dead sites read 0."""
    rng = np.random.default_rng(seed)
    t = 3.0 * tukey_quantile(rng.uniform(1e-9, 1 - 1e-9, (F, Hm, Wm)), -0.14)
    u = np.clip(np.round(512 + t + rng.normal(0, 0.5, (F, Hm, 1))), 0, 65535).astype(np.uint16)
    idx = rng.choice(Hm * Wm, n_hot + n_dead, replace=False)
    sites = np.stack([idx // Wm, idx % Wm], axis=1)
    amp = np.round(np.exp(rng.uniform(np.log(40), np.log(4000), n_hot))).astype(np.int64)
    hot, dead = sites[:n_hot], sites[n_hot:]
    u[:, hot[:, 0], hot[:, 1]] = np.clip(u[:, hot[:, 0], hot[:, 1]].astype(np.int64) + amp[None, :], 0, 65535).astype(np.uint16)
    u[:, dead[:, 0], dead[:, 1]] = 0
    return u, hot, amp, dead


@pytest.mark.parametrize('cfa,pat,rad', [('bayer', RGGB, 2), ('xtrans', XPAT, 3)])
def test_detector_finds_the_injected_sites(cfa, pat, rad):
    """Thresholds by find_defects' rule (k = 8, floor 16 DN per frame) evaluated on the restatement: T = max(ceil(8 * 1.4826 * median|D|),
    4 * 16).  Stated margin: an injected site must be found when its amplitude per frame exceeds T / F by 16 DN (the median of its
    neighbours sits within a few sigma / sqrt(F) of the black level, far inside that margin); every dead site (512 DN below) must be
    found.  Cap on false positives: 5 of 46080 sites -- the noise has Tukey-lambda tails (lambda -0.14), so a handful of genuine
    outliers beyond 8 robust sigma is expected; Gaussian noise would give none.
    Observed on the CPU: Bayer T = 119 (sigma-hat 14.83 on the stack sum), 40 of 40 hot (37 required) and 20 of 20 dead found,
    1 false positive; X-Trans T = 107 (sigma-hat 13.34), 40 of 40 hot (38 required), 20 of 20 dead, 1 false positive."""
    F = 4
    u, hot, amp, dead = synthetic_bias_stack(cfa)
    Hm, Wm = u.shape[1:]
    cls = R.class_map(Hm, Wm, cfa, pat)
    D = R.deviation(u, cls, rad)
    sigma = 1.4826 * float(np.sort(np.abs(D).reshape(-1))[(D.size - 1) // 2])
    T = max(int(np.ceil(8.0 * sigma)), F * 16)
    mask = R.flags(D, T, T)
    must = amp > T / F + 16
    found_hot = mask[hot[:, 0], hot[:, 1]]
    print(cfa, 'T', T, 'sigma', sigma, 'hot found', int(found_hot.sum()), 'of', len(hot), 'required', int(must.sum()),
          'dead found', int(mask[dead[:, 0], dead[:, 1]].sum()), 'false positives', int(mask.sum() - found_hot.sum() - mask[dead[:, 0], dead[:, 1]].sum()))
    assert must.sum() >= 30 and found_hot[must].all()
    assert mask[dead[:, 0], dead[:, 1]].all()
    inj = np.zeros_like(mask)
    inj[hot[:, 0], hot[:, 1]] = inj[dead[:, 0], dead[:, 1]] = True
    assert int((mask & ~inj).sum()) <= 5
    assert (D[mask & (D > 0)] > T).all() and np.array_equal(R.pack_bitmap(mask), DF.pack_bitmap(mask))
