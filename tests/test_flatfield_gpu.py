"""Flat-field maps on the device: the entry points of csrc/flatfield.hip against their NumPy restatement (tests/flatfield_ref.py), bit for bit,
and the wiring end to end.  Shapes are the smallest at which each code path can go wrong: the 16-byte and the 4-byte path, a ragged last lane,
sides that are no multiple of the period, a frame off the 16-byte grid, windows larger than the plane, the largest radius on a plane larger
than its window, and a shape that crosses the tiles of both box passes with a ragged tail."""
import ctypes
import types

import numpy as np
import pytest

import flatfield_ref as R

pytestmark = pytest.mark.gpu

PAT = [[0, 1], [3, 2]]
PATTERNS = ([[0, 1], [3, 2]], [[1, 0], [2, 3]], [[3, 2], [0, 1]], [[2, 3], [1, 0]])
SHAPES = [('bayer', (4, 8)), ('bayer', (6, 10)), ('bayer', (10, 24)), ('bayer', (130, 1032)), ('xtrans', (6, 6)), ('xtrans', (12, 18)),
          ('xtrans', (14, 20))]
WHITE = 16383


@pytest.fixture(scope='module')
def dev(eld_lib):
    import torch
    assert torch.cuda.is_available(), 'these tests need a GPU'
    return torch.device('cuda', 0)


def _period(cfa):
    return 2 if cfa == 'bayer' else 6


def _codes(rng, shape, lo=2000, hi=9000):
    """Flat-field codes with 0, 65535 and values on both sides of the white level among them."""
    u = rng.integers(lo, hi, size=shape).astype(np.uint16)
    flat = u.reshape(-1)
    idx = rng.choice(flat.size, size=max(5, flat.size // 12), replace=False)
    for k, v in enumerate((0, 65535, WHITE - 1, WHITE, WHITE + 1)):
        flat[idx[k::5]] = v
    return u


def _mask(rng, shape, on):
    if not on:
        return None
    m = rng.random(shape) < 0.1
    m[0, 0] = m[-1, -1] = True
    return m


def _bitmap(mask, dev):
    import torch
    return None if mask is None else torch.from_numpy(R.pack_bitmap(mask).view(np.int32).copy()).to(dev)


def _defects(mask, dev):
    """What flat_sums takes: anything with bitmap_on (a DefectMap refuses masks that flag whole neighbourhoods, which these random ones may)."""
    return None if mask is None else types.SimpleNamespace(bitmap_on=lambda d: _bitmap(mask, dev))


def _u32(t):
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


def _unpack(words, Wm):
    bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8).reshape(words.shape[0], -1), axis=1, bitorder='little')
    assert not bits[:, Wm:].any(), 'pad bits of the flag bitmap are set'
    return bits[:, :Wm].astype(bool)


def _same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))


# ---- pass 1 -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cfa,shape', SHAPES)
@pytest.mark.parametrize('pairs', [1, 3])
@pytest.mark.parametrize('nses', [1, 2])
@pytest.mark.parametrize('masked', [False, True])
def test_sums_equal_the_restatement(eld_lib, dev, cfa, shape, pairs, nses, masked):
    """Through the pool upload fit_flat_field uses: a session without flats between the others is skipped."""
    from eld_amd import flatfield as FF
    from eld_amd.framepool import FramePool
    rng = np.random.default_rng(hash((shape, pairs, nses, masked)) % 2 ** 31)
    sessions = [{'flats': _codes(rng, (pairs, 2) + shape)} for _ in range(nses)]
    sessions.insert(1, {'bias': _codes(rng, (2,) + shape)})
    mask = _mask(rng, shape, masked)
    frames = FF.flat_frames(sessions, cfa)
    assert len(frames) == 2 * pairs * nses
    pool = FramePool(frames, cfa=cfa, white_point=65535, device=dev)
    S, D, bad = FF.flat_sums(pool, WHITE, _defects(mask, dev))
    wS, wD, wbad = R.sums(np.stack(frames), WHITE, mask)
    assert np.array_equal(_u32(S), wS)
    assert np.array_equal(D.cpu().numpy(), wD)
    assert np.array_equal(bad.cpu().numpy().view(np.uint32), R.pack_bitmap(wbad))
    assert np.array_equal(FF.unpack_bad(bad, shape[1]).cpu().numpy(), wbad)
    assert wbad.any() and not wbad.all()


def _sums_raw(lib, dev, frames, white, mask=None, skew=0):
    """The raw binding on a hand-made pool: frames start on 16-byte boundaries, except that `skew` elements (even) are put in front of the second
    frame and all after it."""
    import torch
    from eld_amd import _lib as L
    Hm, Wm = frames[0].shape
    step = -(-Hm * Wm // 8) * 8
    table = np.zeros(len(frames), L.POOL_FRAME_DTYPE)
    for i in range(len(frames)):
        table[i] = (i * step + (skew if i else 0), Hm, Wm)
    elems = len(frames) * step + skew
    buf = np.zeros(elems, np.uint16)
    for e, f in zip(table, frames):
        buf[int(e['offset']):int(e['offset']) + Hm * Wm] = f.reshape(-1)
    pool = torch.from_numpy(buf.view(np.int16)).to(dev)
    tab = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
    S = torch.full((Hm, Wm), -7, dtype=torch.int32, device=dev)
    D = torch.full((Hm, Wm), -7, dtype=torch.int64, device=dev)
    bad = torch.full((Hm, (Wm + 31) // 32), -1, dtype=torch.int32, device=dev)
    rc = lib.eld_flat_sums_u16(L.dptr(pool), elems, L.dptr(tab), len(frames), Hm, Wm, white, L.dptr(_bitmap(mask, dev)), L.dptr(S), L.dptr(D),
                               L.dptr(bad), L.cur_stream())
    assert rc == 0
    torch.cuda.synchronize()
    return _u32(S), D.cpu().numpy(), bad.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize('shape', [(4, 8), (10, 24)])
def test_sums_with_a_frame_off_the_16_byte_grid(eld_lib, dev, shape):
    """The second frame starts at a byte offset that is a multiple of 4 and not of 16: its group of frames takes the 4-byte path."""
    rng = np.random.default_rng(11)
    frames = list(_codes(rng, (6,) + shape))
    S, D, bad = _sums_raw(eld_lib, dev, frames, WHITE, skew=2)
    wS, wD, wbad = R.sums(np.stack(frames), WHITE)
    assert np.array_equal(S, wS) and np.array_equal(D, wD) and np.array_equal(bad, R.pack_bitmap(wbad))


def test_sums_widths(eld_lib, dev):
    """18 frames of pairs (65535, 0): S needs more than 16 + 4 bits and D more than 32; white 65536 flags nothing."""
    frames = [np.full((4, 40), v, np.uint16) for _ in range(9) for v in (65535, 0)]
    S, D, bad = _sums_raw(eld_lib, dev, frames, 65536)
    assert np.all(S == 9 * 65535) and np.all(D == 9 * 65535 ** 2) and 9 * 65535 ** 2 > 2 ** 32 and not bad.any()
    assert _unpack(_sums_raw(eld_lib, dev, frames, 65535)[2], 40).all()


def test_sums_einval_before_any_launch(eld_lib, dev):
    import torch
    from eld_amd import _lib as L
    Hm, Wm, F = 4, 8, 4
    pool = torch.zeros(F * Hm * Wm + 8, dtype=torch.int16, device=dev)
    table = np.zeros(F, L.POOL_FRAME_DTYPE)
    for i in range(F):
        table[i] = (i * Hm * Wm, Hm, Wm)
    tab = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
    S = torch.zeros((Hm, Wm), dtype=torch.int32, device=dev)
    D = torch.zeros((Hm, Wm), dtype=torch.int64, device=dev)
    bad = torch.zeros((Hm, 1), dtype=torch.int32, device=dev)
    s = L.cur_stream()

    def run(pool_=L.dptr(pool), tab_=L.dptr(tab), F_=F, Hm_=Hm, Wm_=Wm, white=WHITE, bm=None, S_=L.dptr(S), D_=L.dptr(D), bad_=L.dptr(bad)):
        return eld_lib.eld_flat_sums_u16(pool_, pool.numel(), tab_, F_, Hm_, Wm_, white, bm, S_, D_, bad_, s)
    assert run() == 0 and run(bm=L.dptr(bad)) == 0
    for kw in (dict(pool_=None), dict(tab_=None), dict(S_=None), dict(D_=None), dict(bad_=None), dict(F_=3), dict(F_=0), dict(F_=65538), dict(Wm_=7),
               dict(Hm_=-1), dict(white=0), dict(white=65537), dict(pool_=ctypes.c_void_p(pool.data_ptr() + 2)),
               dict(D_=ctypes.c_void_p(D.data_ptr() + 4)), dict(bm=ctypes.c_void_p(bad.data_ptr() + 2))):
        assert run(**kw) == -1, kw
    assert run(Hm_=0) == 0 and run(Wm_=0) == 0
    torch.cuda.synchronize()


# ---- pass 2 -----------------------------------------------------------------------------------------------------------------------------------
def _box(lib, dev, S, bad, p, radius):
    import torch
    from eld_amd import _lib as L
    Hm, Wm = S.shape
    St = torch.from_numpy(S.astype(np.uint32).view(np.int32)).to(dev)
    bt = _bitmap(bad, dev)
    Bsum = torch.full((Hm, Wm), -7, dtype=torch.int64, device=dev)
    Bcnt = torch.full((Hm, Wm), -7, dtype=torch.int32, device=dev)
    nbytes = lib.eld_flat_box_workspace_bytes(Hm, Wm)
    assert nbytes == Hm * Wm * 8
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    assert lib.eld_flat_box_u32(L.dptr(St), L.dptr(bt), Hm, Wm, p, radius, L.dptr(Bsum), L.dptr(Bcnt), L.dptr(ws), nbytes, L.cur_stream()) == 0
    torch.cuda.synchronize()
    return Bsum.cpu().numpy(), Bcnt.cpu().numpy().astype(np.int64)


def _box_inputs(rng, shape, masked, p):
    """Sums over the whole uint32 range (a window's sum then needs more than 32 bits); with bad sites, a block of them so large that the windows
    of its middle are wholly bad at radius 0 and 1."""
    S = rng.integers(0, 2 ** 32, size=shape, dtype=np.int64)
    S.reshape(-1)[:2] = (2 ** 32 - 1, 0)
    bad = np.zeros(shape, bool)
    if masked:
        bad = rng.random(shape) < 0.15
        bad[:min(shape[0], 3 * p), :min(shape[1], 3 * p)] = True
    return S, bad


def _check_box(lib, dev, S, bad, p, radius):
    Bsum, Bcnt = _box(lib, dev, S, bad, p, radius)
    wsum, wcnt = R.box(S, bad, p, radius)
    assert np.array_equal(Bcnt, wcnt)
    assert np.array_equal(Bsum, wsum)
    return wcnt


@pytest.mark.parametrize('cfa,shape', SHAPES)
@pytest.mark.parametrize('radius', [0, 1, 3])
@pytest.mark.parametrize('masked', [False, True])
def test_box_equals_the_restatement(eld_lib, dev, cfa, shape, radius, masked):
    p = _period(cfa)
    rng = np.random.default_rng(hash((shape, radius, masked)) % 2 ** 31)
    S, bad = _box_inputs(rng, shape, masked, p)
    wcnt = _check_box(eld_lib, dev, S, bad, p, radius)
    if masked and radius <= 1 and min(shape) >= 3 * p:
        assert wcnt[p, p] == 0                                   # a window that lies wholly on bad sites
    if not masked:
        assert wcnt.max() == min(2 * radius + 1, -(-shape[0] // p)) * min(2 * radius + 1, -(-shape[1] // p))


@pytest.mark.parametrize('cfa,shape,radius', [('bayer', (6, 10), 8), ('bayer', (10, 24), 64), ('xtrans', (12, 18), 5), ('xtrans', (14, 20), 64)])
def test_box_with_a_radius_larger_than_the_plane(eld_lib, dev, cfa, shape, radius):
    p = _period(cfa)
    rng = np.random.default_rng(radius)
    for masked in (False, True):
        S, bad = _box_inputs(rng, shape, masked, p)
        wcnt = _check_box(eld_lib, dev, S, bad, p, radius)
        if not masked:                                           # every window is its whole position plane
            assert np.array_equal(wcnt, R.cell_map(np.outer([-(-(shape[0] - r) // p) for r in range(p)], [-(-(shape[1] - c) // p) for c in range(p)]), *shape))


@pytest.mark.parametrize('cfa,shape', [('bayer', (266, 272)), ('xtrans', (790, 800))])
def test_box_with_the_largest_radius_inside_a_larger_plane(eld_lib, dev, cfa, shape):
    p = _period(cfa)
    assert min(shape) // p > 129
    rng = np.random.default_rng(64)
    S, bad = _box_inputs(rng, shape, True, p)
    _check_box(eld_lib, dev, S, bad, p, 64)
    wcnt = _check_box(eld_lib, dev, S, np.zeros(shape, bool), p, 64)
    assert wcnt.max() == 129 * 129


def _tiles(lib, p):
    tw, th = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.eld_flat_box_tile(p, ctypes.byref(tw), ctypes.byref(th)) == 0
    return tw.value, th.value


@pytest.mark.parametrize('cfa', ['bayer', 'xtrans'])
@pytest.mark.parametrize('radius', [2, 64])
def test_box_across_the_tiles_of_both_passes(eld_lib, dev, cfa, radius):
    """The library names the columns a workgroup of the row pass covers and the rows a workgroup of the column pass covers: the shape takes two
    whole tiles of rows and one of columns, plus a ragged tail that is no multiple of the period or of 8."""
    p = _period(cfa)
    tw, th = _tiles(eld_lib, p)
    assert tw % p == 0 and th % p == 0 and tw >= p and th >= p
    shape = (2 * th + p + 1, tw + 2 * p + 2)
    assert shape[1] % 2 == 0 and (p == 2 or shape[1] % p) and shape[1] % 8 and shape[0] % p
    rng = np.random.default_rng(radius)
    S, bad = _box_inputs(rng, shape, True, p)
    _check_box(eld_lib, dev, S, bad, p, radius)


def test_box_einval_before_any_launch(eld_lib, dev):
    import torch
    from eld_amd import _lib as L
    Hm, Wm = 4, 8
    S = torch.zeros((Hm, Wm), dtype=torch.int32, device=dev)
    bad = torch.zeros((Hm, 1), dtype=torch.int32, device=dev)
    Bs = torch.zeros((Hm, Wm), dtype=torch.int64, device=dev)
    Bc = torch.zeros((Hm, Wm), dtype=torch.int32, device=dev)
    ws = torch.zeros(Hm * Wm, dtype=torch.int64, device=dev)

    def run(S_=L.dptr(S), bad_=L.dptr(bad), Hm_=Hm, Wm_=Wm, p=2, r=1, Bs_=L.dptr(Bs), Bc_=L.dptr(Bc), ws_=L.dptr(ws), n=Hm * Wm * 8):
        return eld_lib.eld_flat_box_u32(S_, bad_, Hm_, Wm_, p, r, Bs_, Bc_, ws_, n, L.cur_stream())
    assert run() == 0 and run(p=6) == 0 and run(r=0) == 0 and run(r=64) == 0
    for kw in (dict(S_=None), dict(bad_=None), dict(Bs_=None), dict(Bc_=None), dict(ws_=None), dict(p=3), dict(r=-1), dict(r=65), dict(Wm_=7), dict(Hm_=-1),
               dict(Bs_=ctypes.c_void_p(Bs.data_ptr() + 4)), dict(ws_=ctypes.c_void_p(ws.data_ptr() + 4))):
        assert run(**kw) == -1, kw
    assert run(n=Hm * Wm * 8 - 1) == -3                              # ELD_EWS
    assert run(Hm_=0) == 0 and eld_lib.eld_flat_box_workspace_bytes(4, 7) == 0
    assert eld_lib.eld_flat_box_tile(3, ctypes.byref(ctypes.c_int()), ctypes.byref(ctypes.c_int())) == -1
    torch.cuda.synchronize()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------
def _planted_sessions(rng, shape, F):
    Hm, Wm = shape
    yy, xx = np.mgrid[0:Hm, 0:Wm]
    fall = 1.0 - 0.4 * (((yy - Hm / 2) / Hm) ** 2 + ((xx - Wm / 2) / Wm) ** 2)
    g = 1.0 + 0.02 * rng.standard_normal(shape)
    mean = 3000.0 * fall * g
    flats = (600 + rng.poisson(mean, size=(F // 2, 2) + shape)).astype(np.uint16)
    flats[0, 1, 5, 7] = WHITE + 5                                 # one saturated code
    flats[:, :, 2, 3] = 590                                       # a site below black: r <= 0
    return flats


@pytest.mark.parametrize('cfa,shape,black', [('bayer', (36, 50), [600, 601, 599, 600]), ('xtrans', (32, 44), 600)])
@pytest.mark.parametrize('radius', [2, 16])
def test_fit_flat_field_is_the_restatement(dev, cfa, shape, black, radius):
    from eld_amd.defects import DefectMap
    from eld_amd.flatfield import fit_flat_field
    rng = np.random.default_rng(radius + shape[0])
    a, b = _planted_sessions(rng, shape, 4), _planted_sessions(rng, shape, 2)
    dmap = DefectMap.from_sites([(0, 0), (9, 14), (shape[0] - 1, shape[1] - 1)], shape, cfa)
    sessions = [{'iso': 100, 'bias': a[0], 'flats': a}, {'iso': 200, 'bias': a[0]}, {'iso': 400, 'flats': b}]
    ff = fit_flat_field(sessions, cfa, PAT if cfa == 'bayer' else None, black, white_level=WHITE, radius=radius, defects=dmap, device=dev)
    p = _period(cfa)
    blk = np.broadcast_to(np.asarray(black, np.float64).reshape(-1), (4,)) if np.ndim(black) == 0 else np.asarray(black, np.float64)
    centre = np.rint(blk).astype(np.int64)[ff.raw_pattern]
    assert centre.shape == (p, p)
    frames = np.concatenate([a.reshape((-1,) + shape), b.reshape((-1,) + shape)])
    want = R.fit(frames, centre, R.CODE_COLOUR[ff.raw_pattern], WHITE, radius, dmap.mask)
    assert _same_bits(ff.lens, want['lens']) and _same_bits(ff.prnu, want['prnu'])
    assert ff.report == want['report'] and ff.invalid == want['invalid'] >= 5
    assert (ff.frames, ff.radius, ff.white_level, ff.shape, ff.cfa) == (6, radius, WHITE, shape, cfa)
    for y, x in ((0, 0), (9, 14), (5, 7), (2, 3)):
        assert ff.lens[y, x] == 1.0 and ff.prnu[y, x] == 1.0
    assert ff.lens[want['ok']].min() >= 1.0 and all(0 < ff.report[c]['falloff'] <= 1 for c in 'RGB')
    assert ff.on(dev, 'lens').data_ptr() == ff.on(dev, 'lens').data_ptr() and _same_bits(ff.on(dev, 'prnu').cpu().numpy(), ff.prnu)


def test_fit_on_tensors_gives_the_same_map(dev):
    import torch
    from eld_amd.flatfield import fit_flat_field
    flats = _planted_sessions(np.random.default_rng(3), (12, 16), 4)
    a = fit_flat_field([{'flats': flats}], 'bayer', PAT, 600, radius=1, device=dev)
    b = fit_flat_field([{'flats': torch.from_numpy(flats.view(np.int16)).to(dev)}], 'bayer', PAT, 600, radius=1, device=dev)
    assert _same_bits(a.lens, b.lens) and _same_bits(a.prnu, b.prnu) and a.report == b.report


# ---- the integer path -------------------------------------------------------------------------------------------------------------------------
def _gain_case(rng, shape, p):
    """Codes, a gain plane and per-cell black levels (integers: w + black then hits exact .5 ties) with ties, both clamps and saturated codes."""
    black = (512 + 2 * rng.integers(0, 3, size=(p, p))).astype(np.float32)          # even: black + k + 0.5 rounds to the even one of black + k, black + k + 1
    g = (1 + 0.3 * rng.random(shape)).astype(np.float32)
    u = _codes(rng, shape, 400, 9000)
    b = R.cell_map(black, *shape).astype(np.int64)
    fu, fg = u.reshape(-1), g.reshape(-1)
    fb = b.reshape(-1)
    spec = [(1, 0.5), (3, 1.5), (5, 0.5), (7, 2.5), (188, 400.0), (-412, 3.0), (-1, 0.5), (2, 1.25)]          # (u - black, gain)
    n = min(len(spec), fu.size)
    for k in range(n):
        fu[k], fg[k] = fb[k] + spec[k][0], spec[k][1]
    fu[-1], fu[-2] = 65535, WHITE                                 # saturated codes, whatever the draw
    return u, g, black, n


@pytest.mark.parametrize('cfa,shape', SHAPES + [('xtrans', (12, 24))])     # (12, 24): X-Trans on the 16-byte path
@pytest.mark.parametrize('N', [1, 3])
def test_apply_equals_the_restatement(eld_lib, dev, cfa, shape, N):
    import torch
    from eld_amd import _lib as L
    p = _period(cfa)
    rng = np.random.default_rng(hash((shape, N)) % 2 ** 31)
    u0, g, black, n = _gain_case(rng, shape, p)
    u = np.stack([u0] + [_codes(rng, shape, 400, 9000) for _ in range(N - 1)])
    blk = (ctypes.c_float * (p * p))(*black.reshape(-1).tolist())
    for mask in (None, _mask(rng, shape, True)):
        want = R.apply(u, g, black, WHITE, mask)
        ut, gt, bm = torch.from_numpy(u.view(np.int16)).to(dev), torch.from_numpy(g).to(dev), _bitmap(mask, dev)
        out = torch.zeros_like(ut)
        assert eld_lib.eld_flat_apply_u16(L.dptr(ut), L.dptr(out), N, shape[0], shape[1], L.dptr(gt), blk, p, WHITE, L.dptr(bm), L.cur_stream()) == 0
        assert eld_lib.eld_flat_apply_u16(L.dptr(ut), L.dptr(ut), N, shape[0], shape[1], L.dptr(gt), blk, p, WHITE, L.dptr(bm), L.cur_stream()) == 0
        got = out.cpu().numpy().view(np.uint16)
        assert np.array_equal(got, want)
        assert np.array_equal(ut.cpu().numpy().view(np.uint16), want)              # in place
        sat = u >= WHITE
        assert sat.any() and np.array_equal(got[sat], u[sat])                      # clipping stays detectable
        if mask is not None:
            assert np.array_equal(got[:, mask], u[:, mask])
    # the planted sites: ties go to even (0.5 -> 0, 4.5 -> 4, 2.5 -> 2, 17.5 -> 18), then both clamps, then -0.5 -> -0 and 2.5 -> 2
    b = R.cell_map(black, *shape).astype(np.int64).reshape(-1)
    ref = R.apply(u, g, black, WHITE)[0].reshape(-1)
    assert (ref[:n].astype(np.int64) - b[:n] * (np.arange(n) != 4) * (np.arange(n) != 5)).tolist() == [0, 4, 2, 18, 65535, 0, 0, 2][:n]


def test_apply_on_an_unaligned_gain_plane_takes_the_word_path(eld_lib, dev):
    import torch
    from eld_amd import _lib as L
    rng = np.random.default_rng(5)
    shape = (4, 16)
    u, g, black, _ = _gain_case(rng, shape, 2)
    ut = torch.from_numpy(u.view(np.int16)).to(dev)
    store = torch.zeros(g.size + 1, dtype=torch.float32, device=dev)
    store[1:] = torch.from_numpy(g.reshape(-1)).to(dev)
    gt = store[1:].view(shape)
    assert gt.data_ptr() % 16 == 4
    out = torch.zeros_like(ut)
    blk = (ctypes.c_float * 4)(*black.reshape(-1).tolist())
    assert eld_lib.eld_flat_apply_u16(L.dptr(ut), L.dptr(out), 1, 4, 16, L.dptr(gt), blk, 2, WHITE, None, L.cur_stream()) == 0
    assert np.array_equal(out.cpu().numpy().view(np.uint16), R.apply(u, g, black, WHITE))


def _map(rng, shape, cfa='bayer', pattern=PAT, white=WHITE):
    from eld_amd.flatfield import FlatField
    lens = (1 + 0.5 * rng.random(shape)).astype(np.float32)
    prnu = (1 + 0.02 * rng.standard_normal(shape)).astype(np.float32)
    return FlatField(lens, prnu, cfa, pattern, radius=4, frames=8, white_level=white)


@pytest.mark.parametrize('part', ['prnu', 'lens', 'both'])
def test_flat_field_apply_parts_and_conventions(dev, part):
    import torch
    from eld_amd.defects import DefectMap
    rng = np.random.default_rng(21)
    shape = (12, 24)
    ff = _map(rng, shape)
    u = _codes(rng, (2,) + shape, 400, 9000)
    black = [512, 513, 511, 512]
    bc = np.asarray(black, np.float32)[np.asarray(PAT)]
    gain = {'prnu': ff.prnu, 'lens': ff.lens, 'both': (ff.lens * ff.prnu).astype(np.float32)}[part]
    dmap = DefectMap.from_sites([(0, 0), (5, 7)], shape)
    want = R.apply(u, gain, bc, WHITE, dmap.mask)
    got = ff.apply(u, part, black_level=black, defects=dmap)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint16 and np.array_equal(got, want)
    assert np.array_equal(ff.apply(u[0], part, black_level=black, defects=dmap), want[0])                      # one frame
    assert np.array_equal(ff.apply(u, part), R.apply(u, gain, np.full((2, 2), 512, np.float32), WHITE))       # the default black level
    t = torch.from_numpy(u.view(np.int16)).to(dev)
    o = ff.apply(t, part, black_level=black, defects=dmap)
    assert o.data_ptr() != t.data_ptr() and o.dtype == t.dtype and np.array_equal(o.cpu().numpy().view(np.uint16), want)
    assert np.array_equal(t.cpu().numpy().view(np.uint16), u)
    dst = torch.zeros_like(t)
    assert ff.apply(t, part, black_level=black, defects=dmap, out=dst) is dst and np.array_equal(dst.cpu().numpy().view(np.uint16), want)
    assert ff.apply(t, part, black_level=black, defects=dmap, out=t) is t and np.array_equal(t.cpu().numpy().view(np.uint16), want)
    with pytest.raises(ValueError, match='out'):
        ff.apply(t, part, out=torch.zeros((2, 12, 26), dtype=torch.int16, device=dev))
    assert not np.array_equal(want, u)


# ---- the input stage --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('hw', [(3, 4), (5, 7), (4, 130)])
@pytest.mark.parametrize('N', [1, 2])
def test_flat_bayer_pack(eld_lib, dev, pattern, hw, N):
    import torch
    from eld_amd import _lib as L
    h, w = hw
    rng = np.random.default_rng(hash((hw, N)) % 2 ** 31)
    u = _codes(rng, (N, 2 * h, 2 * w), 400, 3000)
    a = (3 * rng.standard_normal((2 * h, 2 * w))).astype(np.float32)
    b = (rng.standard_normal((2 * h, 2 * w)) / 500).astype(np.float32)
    g = (1 + 0.05 * rng.standard_normal((2 * h, 2 * w))).astype(np.float32)
    one = np.ones_like(g)
    black, white, ratios, t = [512.0, 510.0, 515.0, 512.0], 16383.0, np.array([100.0, 250.0][:N], np.float32), np.float32(-733.5)
    ut, rt = torch.from_numpy(u.view(np.int16)).to(dev), torch.from_numpy(ratios).to(dev)
    at, bt = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    pat, blk = (ctypes.c_int * 4)(*np.asarray(pattern).reshape(-1).tolist()), (ctypes.c_float * 4)(*black)

    def new():
        return torch.full((N, 4, h, w), float('nan'), dtype=torch.float32, device=dev)

    def flat(g_, shade=True, ratio=True):
        out, gt = new(), torch.from_numpy(g_).to(dev)
        assert eld_lib.eld_pack_raw_bayer_u16_flat(L.dptr(ut), L.dptr(out), N, h, w, pat, blk, white, L.dptr(rt) if ratio else None,
                                                   L.dptr(at) if shade else None, L.dptr(bt) if shade else None, float(t), L.dptr(gt),
                                                   L.cur_stream()) == 0
        return out.cpu().numpy()
    # a non-trivial gain against the restatement, with and without the dark shading, with and without the ratio
    assert _same_bits(flat(g), R.pack_bayer_flat(u, pattern, black, white, ratios, g, a, b, t))
    assert _same_bits(flat(g, shade=False), R.pack_bayer_flat(u, pattern, black, white, ratios, g))
    assert _same_bits(flat(g, shade=False, ratio=False), R.pack_bayer_flat(u, pattern, black, white, None, g))
    # a gain of ones gives the bits of the three existing entry points
    ref = new()
    assert eld_lib.eld_pack_raw_bayer_u16_shaded(L.dptr(ut), L.dptr(ref), N, h, w, pat, blk, white, L.dptr(rt), L.dptr(at), L.dptr(bt), float(t),
                                                 L.cur_stream()) == 0
    assert _same_bits(flat(one), ref.cpu().numpy())
    ref = new()
    assert eld_lib.eld_pack_raw_bayer_u16_gain(L.dptr(ut), L.dptr(ref), N, h, w, pat, blk, white, L.dptr(rt), L.cur_stream()) == 0
    assert _same_bits(flat(one, shade=False), ref.cpu().numpy())
    ref = new()
    assert eld_lib.eld_pack_raw_bayer_u16(L.dptr(ut), L.dptr(ref), N, h, w, pat, blk, white, L.cur_stream()) == 0
    assert _same_bits(flat(one, shade=False, ratio=False), ref.cpu().numpy())
    assert not _same_bits(flat(g, ratio=False), flat(one, ratio=False))      # without the ratio few values clip: the gain shows


def _off_by_a_float(arr, dev):
    """`arr` on the device, 4 bytes past a 16-byte boundary."""
    import torch
    store = torch.zeros(arr.size + 1, dtype=torch.float32, device=dev)
    store[1:] = torch.from_numpy(arr.reshape(-1)).to(dev)
    t = store[1:].view(arr.shape)
    assert t.data_ptr() % 16 == 4
    return t


@pytest.mark.parametrize('pattern', PATTERNS)
def test_flat_bayer_pack_with_one_plane_off_the_16_byte_grid(eld_lib, dev, pattern):
    """A row pitch that allows the 8-byte code reads (2w % 4 == 0) with ONE plane that forbids the 16-byte plane reads -- the gain alone, or
    the slope map alone: every plane is then read by the word.  The same bits as the restatement and as the call on aligned planes."""
    import torch
    from eld_amd import _lib as L
    h, w, N = 3, 4, 2
    rng = np.random.default_rng(29)
    u = _codes(rng, (N, 2 * h, 2 * w), 400, 3000)
    a = (3 * rng.standard_normal((2 * h, 2 * w))).astype(np.float32)
    b = (rng.standard_normal((2 * h, 2 * w)) / 500).astype(np.float32)
    g = (1 + 0.05 * rng.standard_normal((2 * h, 2 * w))).astype(np.float32)
    black, white, ratios, t = [512.0, 510.0, 515.0, 512.0], 16383.0, np.array([100.0, 250.0], np.float32), np.float32(-733.5)
    ut, rt = torch.from_numpy(u.view(np.int16)).to(dev), torch.from_numpy(ratios).to(dev)
    at, bt, gt = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), torch.from_numpy(g).to(dev)
    assert at.data_ptr() % 16 == 0 and bt.data_ptr() % 16 == 0 and gt.data_ptr() % 16 == 0
    pat, blk = (ctypes.c_int * 4)(*np.asarray(pattern).reshape(-1).tolist()), (ctypes.c_float * 4)(*black)

    def flat(a_, b_, g_):
        out = torch.full((N, 4, h, w), float('nan'), dtype=torch.float32, device=dev)
        assert eld_lib.eld_pack_raw_bayer_u16_flat(L.dptr(ut), L.dptr(out), N, h, w, pat, blk, white, L.dptr(rt), L.dptr(a_), L.dptr(b_), float(t),
                                                   L.dptr(g_), L.cur_stream()) == 0
        return out.cpu().numpy()
    want = R.pack_bayer_flat(u, pattern, black, white, ratios, g, a, b, t)
    aligned = flat(at, bt, gt)
    assert _same_bits(aligned, want)
    for planes in ((at, bt, _off_by_a_float(g, dev)), (at, _off_by_a_float(b, dev), gt)):
        got = flat(*planes)
        assert _same_bits(got, want) and _same_bits(got, aligned)
    want = R.pack_bayer_flat(u, pattern, black, white, ratios, g)             # no map: the gain is the only plane
    aligned, got = flat(None, None, gt), flat(None, None, _off_by_a_float(g, dev))
    assert _same_bits(aligned, want) and _same_bits(got, want)


@pytest.mark.parametrize('shape', [(6, 6), (12, 18), (14, 20)])
@pytest.mark.parametrize('N', [1, 2])
def test_flat_xtrans_pack(eld_lib, dev, shape, N):
    import torch
    from eld_amd import _lib as L
    Hm, Wm = shape
    rng = np.random.default_rng(hash((shape, N)) % 2 ** 31)
    u = _codes(rng, (N, Hm, Wm), 900, 4000)
    a = (3 * rng.standard_normal(shape)).astype(np.float32)
    b = (rng.standard_normal(shape) / 500).astype(np.float32)
    g = (1 + 0.05 * rng.standard_normal(shape)).astype(np.float32)
    one = np.ones_like(g)
    black, white, ratios, t = 1024.0, 16383.0, np.array([100.0, 250.0][:N], np.float32), np.float32(366.25)
    ut, rt = torch.from_numpy(u.view(np.int16)).to(dev), torch.from_numpy(ratios).to(dev)
    at, bt = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    h, w = 2 * (Hm // 6), 2 * (Wm // 6)

    def new():
        return torch.full((N, 9, h, w), float('nan'), dtype=torch.float32, device=dev)

    def flat(g_, shade=True, ratio=True):
        out, gt = new(), torch.from_numpy(g_).to(dev)
        assert eld_lib.eld_pack_raw_xtrans_u16_flat(L.dptr(ut), L.dptr(out), N, Hm, Wm, black, white, L.dptr(rt) if ratio else None,
                                                    L.dptr(at) if shade else None, L.dptr(bt) if shade else None, float(t), L.dptr(gt),
                                                    L.cur_stream()) == 0
        return out.cpu().numpy()
    assert _same_bits(flat(g), R.pack_xtrans_flat(u, black, white, ratios, g, a, b, t))
    assert _same_bits(flat(g, shade=False), R.pack_xtrans_flat(u, black, white, ratios, g))
    assert _same_bits(flat(g, shade=False, ratio=False), R.pack_xtrans_flat(u, black, white, None, g))
    ref = new()
    assert eld_lib.eld_pack_raw_xtrans_u16_shaded(L.dptr(ut), L.dptr(ref), N, Hm, Wm, black, white, L.dptr(rt), L.dptr(at), L.dptr(bt), float(t),
                                                  L.cur_stream()) == 0
    assert _same_bits(flat(one), ref.cpu().numpy())
    ref = new()
    assert eld_lib.eld_pack_raw_xtrans_u16_gain(L.dptr(ut), L.dptr(ref), N, Hm, Wm, black, white, L.dptr(rt), L.cur_stream()) == 0
    assert _same_bits(flat(one, shade=False), ref.cpu().numpy())
    ref = new()
    assert eld_lib.eld_pack_raw_xtrans_u16(L.dptr(ut), L.dptr(ref), N, Hm, Wm, black, white, L.cur_stream()) == 0
    assert _same_bits(flat(one, shade=False, ratio=False), ref.cpu().numpy())
    assert not _same_bits(flat(g, ratio=False), flat(one, ratio=False))      # without the ratio few values clip: the gain shows


def test_apply_and_pack_einval_before_any_launch(eld_lib, dev):
    import torch
    from eld_amd import _lib as L
    Hm, Wm = 4, 8
    s = L.cur_stream()
    u = torch.zeros((2, Hm, Wm), dtype=torch.int16, device=dev)
    g = torch.ones((Hm, Wm), dtype=torch.float32, device=dev)
    bm = torch.zeros((Hm, 1), dtype=torch.int32, device=dev)
    blk = (ctypes.c_float * 4)(512, 512, 512, 512)

    def app(in_=L.dptr(u), out_=L.dptr(u), N=2, Hm_=Hm, Wm_=Wm, g_=L.dptr(g), blk_=blk, p=2, white=WHITE, bm_=None):
        return eld_lib.eld_flat_apply_u16(in_, out_, N, Hm_, Wm_, g_, blk_, p, white, bm_, s)
    assert app() == 0 and app(bm_=L.dptr(bm)) == 0
    for kw in (dict(in_=None), dict(out_=None), dict(g_=None), dict(blk_=None), dict(Wm_=7), dict(N=-1), dict(p=4), dict(white=0), dict(white=65537),
               dict(blk_=(ctypes.c_float * 4)(512, -1, 512, 512)), dict(blk_=(ctypes.c_float * 4)(512, float('nan'), 512, 512)),
               dict(in_=ctypes.c_void_p(u.data_ptr() + 2)), dict(bm_=ctypes.c_void_p(bm.data_ptr() + 1))):
        assert app(**kw) == -1, kw
    assert app(N=0) == 0 and app(Hm_=0) == 0
    packed = torch.zeros((1, 4, 2, 4), dtype=torch.float32, device=dev)
    r = torch.ones(1, dtype=torch.float32, device=dev)
    pat = (ctypes.c_int * 4)(0, 1, 3, 2)

    def pb(m=L.dptr(u), o=L.dptr(packed), N=1, pat_=pat, blk_=blk, r_=L.dptr(r), a_=L.dptr(g), b_=L.dptr(g), g_=L.dptr(g)):
        return eld_lib.eld_pack_raw_bayer_u16_flat(m, o, N, 2, 4, pat_, blk_, 16383.0, r_, a_, b_, 1.0, g_, s)
    assert pb() == 0 and pb(N=0) == 0 and pb(r_=None) == 0 and pb(a_=None, b_=None) == 0
    for kw in (dict(m=None), dict(o=None), dict(g_=None), dict(a_=None), dict(b_=None), dict(pat_=None), dict(blk_=None), dict(N=-1),
               dict(pat_=(ctypes.c_int * 4)(0, 1, 1, 2)), dict(pat_=(ctypes.c_int * 4)(0, 1, 4, 2)), dict(g_=ctypes.c_void_p(g.data_ptr() + 2))):
        assert pb(**kw) == -1, kw
    x = torch.zeros((1, 6, 6), dtype=torch.int16, device=dev)
    xg = torch.ones((6, 6), dtype=torch.float32, device=dev)
    xo = torch.zeros((1, 9, 2, 2), dtype=torch.float32, device=dev)

    def px(m=L.dptr(x), o=L.dptr(xo), N=1, white=16383.0, r_=L.dptr(r), a_=L.dptr(xg), b_=L.dptr(xg), g_=L.dptr(xg)):
        return eld_lib.eld_pack_raw_xtrans_u16_flat(m, o, N, 6, 6, 1024.0, white, r_, a_, b_, 1.0, g_, s)
    assert px() == 0 and px(N=0) == 0 and px(r_=None) == 0 and px(a_=None, b_=None) == 0
    for kw in (dict(m=None), dict(o=None), dict(g_=None), dict(a_=None), dict(b_=None), dict(N=-1), dict(white=1024.0)):
        assert px(**kw) == -1, kw
    torch.cuda.synchronize()


# ---- the wiring -------------------------------------------------------------------------------------------------------------------------------
def test_packed_lens_is_the_pack_of_the_lens_plane(dev):
    rng = np.random.default_rng(4)
    for pattern in PATTERNS:
        ff = _map(rng, (8, 12), 'bayer', pattern)
        got = ff.packed_lens(dev)
        assert got.data_ptr() == ff.packed_lens(dev).data_ptr()                    # packed once per device
        assert _same_bits(got.cpu().numpy()[0], R.pack_plane_bayer(ff.lens, pattern))
    ff = _map(rng, (14, 20), 'xtrans', None)
    assert _same_bits(ff.packed_lens(dev).cpu().numpy()[0], R.pack_plane_xtrans(ff.lens))


@pytest.fixture(scope='module')
def denoiser(dev):
    import torch
    from eld_amd.denoise import load_denoiser
    from eld_amd.unet import UNetSeeInDark
    torch.manual_seed(7)
    net = UNetSeeInDark(4, 4)
    with torch.no_grad():
        net.conv10_1.bias.fill_(0.3)                 # outputs inside (0, 1): a gain on them shows in the codes
    return load_denoiser(net, cfa='bayer', device=dev)


def test_denoise_raw_with_a_flat_field(dev, denoiser):
    import torch
    from eld_amd.denoise import denoise_raw, pack_input
    from eld_amd.flatfield import FlatField
    from eld_amd.shading import DarkShading
    rng = np.random.default_rng(8)
    Hm, Wm = 64, 96
    pattern = PATTERNS[1]
    u = _codes(rng, (2, Hm, Wm), 500, 700)
    ff = _map(rng, (Hm, Wm), 'bayer', pattern)
    flat_lens = FlatField(np.ones((Hm, Wm), np.float32), ff.prnu, 'bayer', pattern)
    sh = DarkShading((3 * rng.standard_normal((Hm, Wm))).astype(np.float32), (rng.standard_normal((Hm, Wm)) / 800).astype(np.float32),
                     1500.0, 800, 3200, 'bayer', pattern)
    ratios = np.array([100.0, 200.0], np.float32)
    kw = dict(raw_pattern=pattern, black_level=512, ratio=[100.0, 200.0], wb=[2.0, 1.0, 1.5], ccm=np.eye(3))
    t = torch.from_numpy(u.view(np.int16)).to(dev)
    codes = [int(v) for v in np.asarray(pattern).reshape(-1)]
    # the network input gets the PRNU plane only
    x = pack_input(t, 'bayer', codes, [512.0] * 4, 16383.0, ratios, None, None, ff)
    assert _same_bits(x.cpu().numpy(), R.pack_bayer_flat(u, pattern, [512.0] * 4, 16383.0, ratios, ff.prnu))
    xs = pack_input(t, 'bayer', codes, [512.0] * 4, 16383.0, ratios, sh, sh.t(1600), ff)
    assert _same_bits(xs.cpu().numpy(), R.pack_bayer_flat(u, pattern, [512.0] * 4, 16383.0, ratios, ff.prnu, sh.a, sh.b, sh.t(1600)))
    off = denoise_raw(denoiser, u, 'bayer', flatfield=ff, lens='off', **kw)
    ones = denoise_raw(denoiser, u, 'bayer', flatfield=flat_lens, lens='all', **kw)
    srgb = denoise_raw(denoiser, u, 'bayer', flatfield=ff, **kw)                    # the default: 'srgb'
    both = denoise_raw(denoiser, u, 'bayer', flatfield=ff, lens='all', **kw)
    plain = denoise_raw(denoiser, u, 'bayer', **kw)
    from eld_amd.denoise import run_network
    assert _same_bits(off['packed'], run_network(denoiser, x).cpu().numpy())
    for k in ('packed', 'mosaic', 'srgb'):                                          # 'off' is a run whose lens plane is all ones
        assert np.array_equal(off[k], ones[k]), k
    inside = (off['packed'] > 0.01) & (off['packed'] < 0.6)                        # there the lens gain (<= 1.5) shows below the clip
    assert inside.mean() > 0.5, 'the random network writes too few values inside (0, 1) for this test to see a gain'
    assert np.array_equal(srgb['mosaic'], off['mosaic']) and not np.array_equal(srgb['srgb'], off['srgb'])
    assert not np.array_equal(both['mosaic'], off['mosaic']) and np.array_equal(both['srgb'], srgb['srgb'])
    for r in (srgb, both):
        assert _same_bits(r['packed'], off['packed'])                               # the network's own output in every mode
    assert not np.array_equal(plain['packed'], off['packed'])
    # the written-back mosaic of 'all' is the write-back of output x packed lens plane
    from eld_amd.denoise import write_back
    lifted = torch.from_numpy(off['packed'] * R.pack_plane_bayer(ff.lens, pattern)[None]).to(dev)
    want = write_back(lifted, t.clone(), 'bayer', codes, [512.0] * 4, 16383.0)
    assert np.array_equal(both['mosaic'], want.cpu().numpy().view(np.uint16))
    with_shading = denoise_raw(denoiser, u, 'bayer', flatfield=ff, lens='off', shading=sh, iso=1600, **kw)
    assert _same_bits(with_shading['packed'], run_network(denoiser, xs).cpu().numpy())


def test_frame_pool_holds_the_corrected_frames(dev):
    from eld_amd.framepool import FramePool
    rng = np.random.default_rng(13)
    shape = (12, 24)
    ff = _map(rng, shape)
    frames = _codes(rng, (3,) + shape, 400, 9000)
    pool = FramePool(frames, cfa='bayer', raw_pattern=PAT, black_level=[512, 513, 511, 512], flatfield=ff, device=dev)
    want = ff.apply(frames, part='prnu', black_level=[512, 513, 511, 512])
    assert np.array_equal(want, R.apply(frames, ff.prnu, np.asarray([512, 513, 511, 512], np.float32)[np.asarray(PAT)], WHITE))
    got = pool.buffer.cpu().numpy().view(np.uint16)
    for f, w in zip(pool.frames, want):
        assert np.array_equal(got[int(f['offset']):int(f['offset']) + w.size].reshape(shape), w)
    plain = FramePool(frames, cfa='bayer', raw_pattern=PAT, black_level=[512, 513, 511, 512], device=dev)
    assert plain.flatfield is None and np.array_equal(plain.buffer.cpu().numpy().view(np.uint16)[:frames[0].size].reshape(shape), frames[0])
    assert not np.array_equal(want, frames)


def test_evaluate_pairs_corrects_both_exposures(dev, denoiser):
    from eld_amd.evaluate import evaluate_pairs
    rng = np.random.default_rng(17)
    Hm, Wm = 64, 96
    pattern = PATTERNS[1]
    ff = _map(rng, (Hm, Wm), 'bayer', pattern)
    short, long_ = _codes(rng, (Hm, Wm), 500, 700), _codes(rng, (Hm, Wm), 600, 9000)
    seen = {}
    evaluate_pairs(denoiser, [{'short': short, 'long': long_, 'ratio': 100.0}], 'bayer', raw_pattern=pattern, black_level=512, levels=False,
                   flatfield=ff, on_pair=lambda i, row, t: seen.update({k: v.cpu().numpy() for k, v in t.items()}))
    one = np.ones((Hm, Wm), np.float32)
    assert _same_bits(seen['input'], R.pack_bayer_flat(short[None], pattern, [512.0] * 4, 16383.0, [100.0], ff.prnu))
    fixed = R.apply(long_, ff.prnu, np.full((2, 2), 512, np.float32), WHITE)
    assert _same_bits(seen['target'], R.pack_bayer_flat(fixed[None], pattern, [512.0] * 4, 16383.0, [1.0], one))
    assert not np.array_equal(fixed, long_)
