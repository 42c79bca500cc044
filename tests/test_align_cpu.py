"""The burst alignment's restatement (tests/align_ref.py) against its own definition, and the host logic of eld_amd.burst: no GPU.
The closed loop shifts a synthetic scene by whole CFA periods and asks for every tile's displacement back, exactly; where all frames are
present the aligned merge must then be the tripod merge of the same noisy frames, bit for bit."""
import numpy as np
import pytest

import align_ref as A
import burst_ref as R

BAYER = (2, [0, 1, 3, 2], 4, [512] * 4)
XT_COLOUR = [0, 2, 1, 2, 0, 1, 1, 1, 0, 1, 1, 2, 1, 1, 2, 1, 1, 0, 2, 0, 1, 0, 2, 1, 1, 1, 2, 1, 1, 0, 1, 1, 0, 1, 1, 2]
XTRANS = (6, XT_COLOUR, 3, [512] * 36)
WHITE = 16383
SEEDS = (0, 1, 2, 3, 4, 5)
LOOP = {'bayer': (BAYER, 104, 136), 'xtrans': (XTRANS, 204, 300)}


@pytest.mark.parametrize('name', ['bayer', 'xtrans'])
def test_closed_loop(name):
    layout, Hm, Wm = LOOP[name]
    p = layout[0]
    assert A.default_levels(Hm, Wm, p) == 2
    (TY, oy), (TX, ox) = A.tiles(Hm // p), A.tiles(Wm // p)
    assert oy[-1] != (TY - 1) * A.T and ox[-1] != (TX - 1) * A.T          # both have shifted-back last tiles
    wrong = total = 0
    for seed in SEEDS:
        frames, shifts, noisy = A.shifted_burst(seed, Hm, Wm, p)
        assert np.all(shifts[0] == 0) and np.abs(shifts).max() <= 6 and np.abs(shifts[1:]).max() > 0
        disp, cost = A.align(frames, p)
        assert disp.shape == (5, TY, TX, 2) and cost.shape == (5, TY, TX) and not disp[0].any() and not cost[0].any()
        bad = (disp.astype(np.int64) != -shifts[:, None, None, :]).any(axis=3)
        wrong += int(bad.sum())
        total += bad[1:].size
        print('%s seed %d: shifts %s, wrong tiles %d' % (name, seed, shifts[1:].tolist(), int(bad.sum())))
        if bad.any():
            continue
        # the exact merge: where all five samples are present the aligned stack is the tripod stack of the same noisy frames
        mean, kept, present, ptc = A.stack_aligned(frames, *layout, WHITE, 100, 2, disp)
        o = 12 * p
        tripod = noisy[:, o:o + Hm, o:o + Wm]
        assert np.array_equal(tripod[0], frames[0])
        tm, tk, _ = R.stack(tripod, *layout, WHITE, 100, 2)
        full = present == 5
        assert 0.5 < full.mean() < 1.0
        assert np.array_equal(mean[full], tm[full]) and np.array_equal(kept[full], tk[full])
        lo = np.abs(shifts).max(axis=0) * p                              # outside this border every frame is present
        assert full[lo[0]:Hm - lo[0], lo[1]:Wm - lo[1]].all()
    assert total == len(SEEDS) * 4 * TY * TX and wrong == 0


@pytest.mark.parametrize('layout,shape', [(BAYER, (36, 40)), (XTRANS, (96, 102))], ids=['bayer', 'xtrans'])
def test_zero_field_is_the_tripod_stack(layout, shape):
    rng = np.random.default_rng(3)
    fr = np.clip(900 + rng.integers(-40, 41, size=(6,) + shape) + 3000 * (rng.uniform(size=(6,) + shape) < 0.01), 0, 65535).astype(np.uint16)
    p = layout[0]
    disp = np.zeros((6, -(-(shape[0] // p) // A.T), -(-(shape[1] // p) // A.T), 2), np.int16)
    mask = rng.uniform(size=shape) < 0.1
    for m in (None, mask):
        mean, kept, present, ptc = A.stack_aligned(fr, *layout, WHITE, 100, 2, disp, mask=m)
        want = R.stack(fr, *layout, WHITE, 100, 2, mask=m)
        assert np.array_equal(mean, want[0]) and np.array_equal(kept, want[1]) and np.array_equal(ptc, want[2])
        assert np.all(present == 6) and (kept != 6).any() and ptc[..., 0].sum() > 0


def test_absent_samples_and_small_m():
    """A field that pushes frames out: M varies over the frame, rejection stops below M = 4, a site nobody reaches but the zero frame keeps it."""
    rng = np.random.default_rng(4)
    fr = (1000 + rng.integers(-8, 9, size=(5, 32, 64))).astype(np.uint16)
    fr[4, 10:20, 40:60] = 9000                                           # an outlier wherever frame 4 is present
    disp = np.zeros((5, 1, 2, 2), np.int16)
    disp[1, 0, 0] = (60, 0)                                              # frame 1 leaves tile 0 altogether (32 rows, 2 * 60 > 32)
    disp[2, 0, 1] = (0, -60)
    disp[3, 0, 1] = (-3, 5)
    mean, kept, present, ptc = A.stack_aligned(fr, *BAYER, WHITE, 100, 2, disp)
    assert np.all(present[:, :32] == 4) and set(np.unique(present[:, 32:])) == {3, 4}
    s, pr = A.gather(fr, 2, disp)
    for y, x in ((12, 44), (12, 56), (0, 0), (31, 63), (15, 33)):
        xs = [int(s[i, y, x]) for i in range(5) if pr[i, y, x]]
        m, n, _, _ = R.site_loop(xs, 100, 2)
        assert (mean[y, x], kept[y, x], present[y, x]) == (m, n, len(xs))
    assert (present[12, 44], kept[12, 44]) == (4, 3) and mean[12, 44] < 1100     # M = 4 rejects the outlier
    assert (present[12, 56], kept[12, 56]) == (3, 3) and mean[12, 56] > 3000     # M = 3 cannot
    assert ptc[..., 0].sum() == 0                                        # no site has all five present
    with pytest.raises(ValueError):
        A.stack_aligned(fr, *BAYER, WHITE, 100, 2, disp + np.int16(61) * (disp == 60))


def test_ties_fall_to_the_smallest_move():
    fr = np.full((3, 64, 96), 777, np.uint16)
    for levels in (1, 2):
        disp, cost = A.align(fr, 2, ref=1, levels=levels)
        assert not disp.any() and not cost.any()
    assert A.RANK[A._CANDS.index((0, 0))] == 0 and sorted(A.RANK) == list(range(81))
    assert [A._CANDS[k] for k in np.argsort(A.RANK)[:5]] == [(0, 0), (-1, 0), (0, -1), (0, 1), (1, 0)]
    assert A._CANDS[int(np.argmax(A.RANK))] == (4, 4)
    costs = np.full(81, 5, np.int64)
    assert A.pick(costs)[:3] == (0, 0, 5)
    costs[A._CANDS.index((0, 0))] = 6
    assert A.pick(costs)[:2] == (-1, 0)


def test_key_width_at_the_extreme_tile():
    ref = np.zeros((16, 16), np.uint16)
    alt = np.full((16, 16), 65535, np.uint16)
    costs = A.tile_costs(ref, alt, 0, 0, 0, 0)
    assert np.all(costs == 256 * 65535) and 256 * 65535 < 1 << 24
    v, u, c, key = A.pick(costs)
    assert (v, u, c) == (0, 0, 256 * 65535) and key == (256 * 65535) << 7 and ((256 * 65535) << 7 | 80) < 1 << 31
    fr = np.stack([np.zeros((32, 32), np.uint16), np.full((32, 32), 65535, np.uint16)])
    disp, cost = A.align(fr, 2, levels=1)
    assert not disp.any() and cost[1, 0, 0] == 256 * 65535 and cost.dtype == np.uint32
    assert A.MAX_DISP == 60 == 4 * (1 + 2 + 4 + 8)


def test_pyramid_sides_and_clamped_downsample():
    rng = np.random.default_rng(5)
    fr = rng.integers(0, 65536, size=(2, 66, 70)).astype(np.uint16)
    pyr = A.pyramid(fr, 2, 2)
    assert [q.shape[1:] for q in pyr] == [(33, 35), (17, 18)] == A.level_sides(66, 70, 2, 2)
    x = fr.astype(np.int64)
    assert pyr[0][1, 5, 7] == (x[1, 10, 14] + x[1, 10, 15] + x[1, 11, 14] + x[1, 11, 15] + 2) // 4
    l0 = pyr[0].astype(np.int64)
    assert pyr[1][0, 3, 4] == (l0[0, 6, 8] + l0[0, 6, 9] + l0[0, 7, 8] + l0[0, 7, 9] + 2) >> 2
    assert pyr[1][0, 16, 17] == (2 * l0[0, 32, 34] + 2 * l0[0, 32, 34] + 2) >> 2      # the last row and column repeat
    assert pyr[1][0, 16, 0] == (2 * l0[0, 32, 0] + 2 * l0[0, 32, 1] + 2) >> 2
    xt = rng.integers(0, 65536, size=(1, 100, 106)).astype(np.uint16)                 # sides no multiples of 6: rows 96.., columns 102.. do not enter
    lx = A.luma(xt, 6)
    assert lx.shape == (1, 16, 17) and lx[0, 15, 16] == (int(xt[0, 90:96, 96:102].astype(np.int64).sum()) + 18) // 36


def test_parent_mapping_and_shifted_back_origins():
    assert A.tiles(33) == (3, [0, 16, 17]) and A.tiles(35) == (3, [0, 16, 19]) and A.tiles(16) == (1, [0]) and A.tiles(32) == (2, [0, 16])
    assert A.tiles(17) == (2, [0, 1]) and A.tiles(18) == (2, [0, 2])
    # level 0 of 33 x 35 over level 1 of 17 x 18 (2 x 2 tiles): the tile centre, halved, picks the parent; the count above bounds it
    assert [A.parent(o, 2) for o in (0, 16, 17)] == [0, 0, 0] and [A.parent(o, 2) for o in (0, 16, 19)] == [0, 0, 0]
    # 68 wide over 34: origins 0, 16, 32, 48, 52 -> centres 8, 24, 40, 56, 60 -> halved 4, 12, 20, 28, 30 -> parents 0, 0, 1, 1, 1 of 3
    n, o = A.tiles(68)
    assert (n, o) == (5, [0, 16, 32, 48, 52]) and [A.parent(v, 3) for v in o] == [0, 0, 1, 1, 1]
    assert A.parent(120, 3) == 2 and A.parent(56, 2) == 1 and A.parent(88, 2) == 1     # clamped to the last tile above


def test_levels_rule():
    assert A.default_levels(32, 32, 2) == 1 and A.default_levels(64, 64, 2) == 2 and A.default_levels(62, 64, 2) == 2 and A.default_levels(60, 64, 2) == 1
    assert A.default_levels(136, 200, 2) == 3 and A.default_levels(4000, 6000, 2) == 4 and A.default_levels(100, 106, 6) == 1
    with pytest.raises(ValueError):
        A.default_levels(30, 64, 2)
    for bad in (0, 5, True, 2.0):
        with pytest.raises(ValueError):
            A.check_levels(256, 256, 2, bad)
    with pytest.raises(ValueError):
        A.check_levels(66, 70, 2, 3)
    with pytest.raises(ValueError):
        A.align(np.zeros((3, 32, 32), np.uint16), 2, ref=3)


def test_argument_errors_come_before_device_work(monkeypatch):
    from eld_amd import _lib as L
    from eld_amd import burst as B

    def no_device(*a, **k):
        raise AssertionError('device work before the argument checks')
    monkeypatch.setattr(L, 'lib', no_device)
    fr = np.zeros((3, 66, 70), np.uint16)
    for kw in (dict(ref=3), dict(ref=-1), dict(ref=True), dict(levels=0), dict(levels=5), dict(levels=3), dict(cfa='foveon')):
        with pytest.raises(ValueError):
            B.align_burst(fr, **kw)
    with pytest.raises(ValueError):
        B.align_burst(np.zeros((3, 30, 70), np.uint16))                 # level 0 is below one tile
    with pytest.raises(ValueError):
        B.align_burst(np.zeros((3, 90, 200), np.uint16), 'xtrans')       # 15 x 33 luma pixels
    with pytest.raises(ValueError):
        B.stack_burst(np.zeros((3, 30, 70), np.uint16), align=True)
    assert B.align_levels(66, 70, 2) == 2 and B.align_levels(66, 70, 2, 1) == 1 and B.align_levels(4000, 6000, 2) == 4
    good = B.BurstAlignment(np.zeros((3, 3, 3, 2), np.int16), None, 2)
    for bad in (B.BurstAlignment(np.zeros((2, 3, 3, 2), np.int16), None, 2), B.BurstAlignment(np.zeros((3, 3, 2, 2), np.int16), None, 2),
                B.BurstAlignment(np.zeros((3, 3, 3, 2), np.int16), None, 6), np.zeros((3, 3, 3, 2), np.int16), 'yes'):
        with pytest.raises(ValueError):
            B.stack_burst(fr, align=bad)
    with pytest.raises(ValueError):
        B.BurstAlignment(np.full((3, 3, 3, 2), 61, np.int16))
    with pytest.raises(ValueError):
        B.BurstAlignment(np.zeros((3, 3, 3), np.int16))
    with pytest.raises(ValueError):
        B.BurstAlignment(np.zeros((3, 3, 3, 2), np.int16), np.zeros((3, 3, 2)))
    with pytest.raises(AssertionError):
        B.stack_burst(fr, align=good)                                    # a good field passes every check and reaches the device


def test_alignment_summaries():
    from eld_amd.burst import BurstAlignment
    disp = np.zeros((2, 2, 5, 2), np.int16)
    disp[1] = (3, -4)
    disp[1, 0, 0] = (3, -2)                                              # two luma pixels off the median: an outlier
    disp[1, 1, 1] = (4, -4)                                              # one off: not
    al = BurstAlignment(disp, None, 6, levels=2, ref=0)
    assert np.array_equal(al.shift_px(), [[0, 0], [18, -24]]) and np.allclose(al.outlier_share(), [0.0, 0.1])
    assert (al.period, al.tile, al.levels, al.ref, al.cost) == (6, 16, 2, 0, None)
