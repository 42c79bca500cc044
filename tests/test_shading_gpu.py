"""Dark shading on the device: the four entry points of csrc/shading.hip against their NumPy restatement (tests/shading_ref.py), bit for
bit, and the wiring end to end.  Shapes are the smallest at which each code path can go wrong: the 16-byte and the 4-byte path, more than
one workgroup's column span with a ragged tail, a frame at an offset that forbids wide loads, sides that are no multiple of the period."""
import ctypes
import math

import numpy as np
import pytest

import shading_ref as R

pytestmark = pytest.mark.gpu

PAT = [[0, 1], [3, 2]]
PATTERNS = ([[0, 1], [3, 2]], [[1, 0], [2, 3]], [[3, 2], [0, 1]], [[2, 3], [1, 0]])
EINVAL = -1
SHAPES = [('bayer', (4, 8)), ('bayer', (10, 24)), ('bayer', (6, 10)), ('bayer', (130, 1032)), ('xtrans', (6, 6)), ('xtrans', (12, 18)),
          ('xtrans', (14, 20))]


@pytest.fixture(scope='module')
def dev(eld_lib):
    import torch
    assert torch.cuda.is_available(), 'these tests need a GPU'
    return torch.device('cuda', 0)


def _codes(rng, shape, lo=480, hi=560):
    """Codes around a black level, with 0 and 65535 among them."""
    u = rng.integers(lo, hi, size=shape).astype(np.uint16)
    flat = u.reshape(-1)
    idx = rng.choice(flat.size, size=max(2, flat.size // 16), replace=False)
    flat[idx[::2]] = 0
    flat[idx[1::2]] = 65535
    return u


def _mask(rng, shape, on):
    if not on:
        return None
    m = rng.random(shape) < 0.1
    m[0, 0] = m[-1, -1] = True
    return m


def _bitmap(mask, dev):
    import torch
    from eld_amd.defects import pack_bitmap
    return None if mask is None else torch.from_numpy(pack_bitmap(mask).view(np.int32).copy()).to(dev)


def _centre(cfa, rng):
    p = 2 if cfa == 'bayer' else 6
    return rng.integers(500, 530, size=(p, p)).astype(np.int64)


def _fit_raw(lib, dev, sessions, alpha, beta, centre, mask=None, skew=0):
    """The raw binding on a hand-made pool: frames start on 16-byte boundaries, except that `skew` elements (even) are put in front of the
    second frame and all after it."""
    import torch
    from eld_amd import _lib as L
    frames = [f for s in sessions for f in s]
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
    S = len(sessions)
    firsts = np.cumsum([0] + [len(s) for s in sessions])
    ses = (ctypes.c_int32 * (2 * S))(*[int(v) for i, s in enumerate(sessions) for v in (firsts[i], len(s))])
    p = centre.shape[0]
    a = torch.full((Hm, Wm), float('nan'), dtype=torch.float32, device=dev)
    b = torch.full((Hm, Wm), float('nan'), dtype=torch.float32, device=dev)
    rc = lib.eld_shading_fit_u16(L.dptr(pool), elems, L.dptr(tab), len(frames), Hm, Wm, ses, S, (ctypes.c_double * S)(*alpha),
                                 (ctypes.c_double * S)(*beta), (ctypes.c_int32 * (p * p))(*[int(v) for v in centre.reshape(-1)]), p,
                                 L.dptr(_bitmap(mask, dev)), L.dptr(a), L.dptr(b), L.cur_stream())
    assert rc == 0
    torch.cuda.synchronize()
    return a.cpu().numpy(), b.cpu().numpy()


def _same_bits(got, want):
    return np.array_equal(np.ascontiguousarray(got).view(np.int32), np.ascontiguousarray(want).view(np.int32))


# ---- the fit --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cfa,shape', SHAPES)
@pytest.mark.parametrize('counts', [(1,), (2, 3), (3, 1, 2)])
@pytest.mark.parametrize('masked', [False, True])
def test_fit_equals_the_restatement(eld_lib, dev, cfa, shape, counts, masked):
    rng = np.random.default_rng(hash((shape, counts, masked)) % 2 ** 31)
    sessions = [_codes(rng, (n,) + shape) for n in counts]
    isos = [800, 1600, 3200][:len(counts)]
    _, alpha, beta = R.coefficients(isos, counts)
    centre, mask = _centre(cfa, rng), _mask(rng, shape, masked)
    a, b = _fit_raw(eld_lib, dev, sessions, alpha, beta, centre, mask)
    wa, wb = R.fit(sessions, alpha, beta, centre, mask)
    assert _same_bits(a, wa) and _same_bits(b, wb)
    if masked:
        assert np.all(a.view(np.int32)[mask] == 0) and np.all(b.view(np.int32)[mask] == 0)          # exactly +0.0


@pytest.mark.parametrize('shape', [(4, 8), (10, 24)])
def test_fit_with_a_frame_off_the_16_byte_grid(eld_lib, dev, shape):
    """The second frame starts at a byte offset that is a multiple of 4 and not of 16: its group of frames takes the 4-byte path."""
    rng = np.random.default_rng(11)
    sessions = [_codes(rng, (2,) + shape), _codes(rng, (5,) + shape)]
    _, alpha, beta = R.coefficients([400, 1600], [2, 5])
    centre = _centre('bayer', rng)
    a, b = _fit_raw(eld_lib, dev, sessions, alpha, beta, centre, skew=2)
    wa, wb = R.fit(sessions, alpha, beta, centre)
    assert _same_bits(a, wa) and _same_bits(b, wb)


def test_fit_sum_width(eld_lib, dev):
    """17 frames all at 65535: the session sum needs more than 16 + 4 bits."""
    sessions = [np.full((17, 4, 8), 65535, np.uint16), np.zeros((3, 4, 8), np.uint16)]
    _, alpha, beta = R.coefficients([800, 3200], [17, 3])
    centre = np.array([[0, 65535], [512, 1]])
    a, b = _fit_raw(eld_lib, dev, sessions, alpha, beta, centre)
    wa, wb = R.fit(sessions, alpha, beta, centre)
    assert _same_bits(a, wa) and _same_bits(b, wb)
    assert abs(float(a[0, 0]) + float(b[0, 0]) * (800 - (17 * 800 + 3 * 3200) / 20.0) - 65535) < 0.01


# ---- the integer path -----------------------------------------------------------------------------------------------------------------------
def _maps(rng, shape):
    """Planes whose step a + b t at t = 2 holds ties (+-0.5, +-1.5), both signs and values large enough to clamp."""
    a = (4 * rng.standard_normal(shape)).astype(np.float32)
    b = (rng.standard_normal(shape) / 4).astype(np.float32)
    ties = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5], np.float32)
    flat_a, flat_b = a.reshape(-1), b.reshape(-1)
    n = min(ties.size, flat_a.size // 2)
    flat_a[:n], flat_b[:n] = ties[:n], 0.0
    flat_a[-1], flat_b[-1] = 3.0, 1.0                    # + 5 under codes 0..3
    flat_a[-2], flat_b[-2] = -3.0, -1.0                  # - 5 under codes 65533..65535
    return a, b


@pytest.mark.parametrize('cfa,shape', SHAPES)
@pytest.mark.parametrize('N', [1, 3])
def test_apply_equals_the_restatement(eld_lib, dev, cfa, shape, N):
    import torch
    from eld_amd import _lib as L
    rng = np.random.default_rng(hash((shape, N)) % 2 ** 31)
    a, b = _maps(rng, shape)
    t = np.float32(2.0)
    u = _codes(rng, (N,) + shape)
    u.reshape(N, -1)[:, -1] = rng.integers(0, 4, size=N)
    u.reshape(N, -1)[:, -2] = rng.integers(65533, 65536, size=N)
    for mask in (None, _mask(rng, shape, True)):
        want = R.apply(u, a, b, t, mask)
        ut = torch.from_numpy(u.view(np.int16)).to(dev)
        at, bt, bm = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), _bitmap(mask, dev)
        out = torch.zeros_like(ut)
        assert eld_lib.eld_shading_apply_u16(L.dptr(ut), L.dptr(out), N, shape[0], shape[1], L.dptr(at), L.dptr(bt), float(t), L.dptr(bm),
                                             L.cur_stream()) == 0
        assert eld_lib.eld_shading_apply_u16(L.dptr(ut), L.dptr(ut), N, shape[0], shape[1], L.dptr(at), L.dptr(bt), float(t), L.dptr(bm),
                                             L.cur_stream()) == 0                                   # in place
        got = out.cpu().numpy().view(np.uint16)
        assert np.array_equal(got, want)
        assert np.array_equal(ut.cpu().numpy().view(np.uint16), want)
        if mask is not None:
            assert np.array_equal(got[:, mask], u[:, mask])
        else:
            assert want.reshape(N, -1)[:, -1].max() == 0 and want.reshape(N, -1)[:, -2].min() == 65535       # both clamps act
    # ties go to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    ref = R.apply(np.full((1,) + shape, 1000, np.uint16), a, b, t)
    n = min(6, a.size // 2)
    assert ref.reshape(-1)[:n].tolist() == [1000, 1000, 998, 1002, 998, 1002][:n]


def test_apply_on_unaligned_planes_takes_the_word_path(eld_lib, dev):
    """Wm % 8 == 0 with a map plane that starts 4 bytes past a 16-byte boundary."""
    import torch
    from eld_amd import _lib as L
    rng = np.random.default_rng(5)
    shape = (4, 16)
    a, b = _maps(rng, shape)
    u = _codes(rng, (2,) + shape)
    ut = torch.from_numpy(u.view(np.int16)).to(dev)
    store = torch.zeros(a.size + 1, dtype=torch.float32, device=dev)
    store[1:] = torch.from_numpy(a.reshape(-1)).to(dev)
    at, bt = store[1:].view(shape), torch.from_numpy(b).to(dev)
    assert at.data_ptr() % 16 == 4
    out = torch.zeros_like(ut)
    assert eld_lib.eld_shading_apply_u16(L.dptr(ut), L.dptr(out), 2, 4, 16, L.dptr(at), L.dptr(bt), 2.0, None, L.cur_stream()) == 0
    assert np.array_equal(out.cpu().numpy().view(np.uint16), R.apply(u, a, b, np.float32(2.0)))


# ---- the fused input stage ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('hw', [(3, 4), (5, 7), (4, 130)])
@pytest.mark.parametrize('N', [1, 2])
def test_shaded_bayer_pack(eld_lib, dev, pattern, hw, N):
    import torch
    from eld_amd import _lib as L
    h, w = hw
    rng = np.random.default_rng(hash((hw, N)) % 2 ** 31)
    u = _codes(rng, (N, 2 * h, 2 * w), 400, 3000)
    a = (3 * rng.standard_normal((2 * h, 2 * w))).astype(np.float32)
    b = (rng.standard_normal((2 * h, 2 * w)) / 500).astype(np.float32)
    black, white, ratios, t = [512.0, 510.0, 515.0, 512.0], 16383.0, np.array([100.0, 250.0][:N], np.float32), np.float32(-733.5)
    ut, rt = torch.from_numpy(u.view(np.int16)).to(dev), torch.from_numpy(ratios).to(dev)
    pat, blk = (ctypes.c_int * 4)(*np.asarray(pattern).reshape(-1).tolist()), (ctypes.c_float * 4)(*black)

    def shaded(a_, b_):
        out = torch.full((N, 4, h, w), float('nan'), dtype=torch.float32, device=dev)
        at, bt = torch.from_numpy(a_).to(dev), torch.from_numpy(b_).to(dev)
        assert eld_lib.eld_pack_raw_bayer_u16_shaded(L.dptr(ut), L.dptr(out), N, h, w, pat, blk, white, L.dptr(rt), L.dptr(at), L.dptr(bt), float(t),
                                                     L.cur_stream()) == 0
        return out.cpu().numpy()
    assert _same_bits(shaded(a, b), R.pack_bayer_shaded(u, pattern, black, white, ratios, a, b, t))
    plain = torch.full((N, 4, h, w), float('nan'), dtype=torch.float32, device=dev)
    assert eld_lib.eld_pack_raw_bayer_u16_gain(L.dptr(ut), L.dptr(plain), N, h, w, pat, blk, white, L.dptr(rt), L.cur_stream()) == 0
    z = np.zeros_like(a)
    assert _same_bits(shaded(z, z), plain.cpu().numpy())


def _off_by_a_float(arr, dev):
    """`arr` on the device, 4 bytes past a 16-byte boundary."""
    import torch
    store = torch.zeros(arr.size + 1, dtype=torch.float32, device=dev)
    store[1:] = torch.from_numpy(arr.reshape(-1)).to(dev)
    t = store[1:].view(arr.shape)
    assert t.data_ptr() % 16 == 4
    return t


@pytest.mark.parametrize('pattern', PATTERNS)
def test_shaded_bayer_pack_with_planes_off_the_16_byte_grid(eld_lib, dev, pattern):
    """A row pitch that allows the 8-byte code reads (2w % 4 == 0) with map planes that forbid the 16-byte plane reads: the same bits as
    the restatement and as the call on aligned planes."""
    import torch
    from eld_amd import _lib as L
    h, w, N = 3, 4, 2
    rng = np.random.default_rng(23)
    u = _codes(rng, (N, 2 * h, 2 * w), 400, 3000)
    a = (3 * rng.standard_normal((2 * h, 2 * w))).astype(np.float32)
    b = (rng.standard_normal((2 * h, 2 * w)) / 500).astype(np.float32)
    black, white, ratios, t = [512.0, 510.0, 515.0, 512.0], 16383.0, np.array([100.0, 250.0], np.float32), np.float32(-733.5)
    ut, rt = torch.from_numpy(u.view(np.int16)).to(dev), torch.from_numpy(ratios).to(dev)
    pat, blk = (ctypes.c_int * 4)(*np.asarray(pattern).reshape(-1).tolist()), (ctypes.c_float * 4)(*black)

    def shaded(at, bt):
        out = torch.full((N, 4, h, w), float('nan'), dtype=torch.float32, device=dev)
        assert eld_lib.eld_pack_raw_bayer_u16_shaded(L.dptr(ut), L.dptr(out), N, h, w, pat, blk, white, L.dptr(rt), L.dptr(at), L.dptr(bt), float(t),
                                                     L.cur_stream()) == 0
        return out.cpu().numpy()
    at, bt = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    assert at.data_ptr() % 16 == 0 and bt.data_ptr() % 16 == 0
    want = R.pack_bayer_shaded(u, pattern, black, white, ratios, a, b, t)
    aligned = shaded(at, bt)
    assert _same_bits(aligned, want)
    for planes in ((_off_by_a_float(a, dev), _off_by_a_float(b, dev)), (_off_by_a_float(a, dev), bt), (at, _off_by_a_float(b, dev))):
        got = shaded(*planes)
        assert _same_bits(got, want) and _same_bits(got, aligned)


@pytest.mark.parametrize('shape', [(6, 6), (12, 18), (14, 20)])
@pytest.mark.parametrize('N', [1, 2])
def test_shaded_xtrans_pack(eld_lib, dev, shape, N):
    import torch
    from eld_amd import _lib as L
    Hm, Wm = shape
    rng = np.random.default_rng(hash((shape, N)) % 2 ** 31)
    u = _codes(rng, (N, Hm, Wm), 900, 4000)
    a = (3 * rng.standard_normal(shape)).astype(np.float32)
    b = (rng.standard_normal(shape) / 500).astype(np.float32)
    black, white, ratios, t = 1024.0, 16383.0, np.array([100.0, 250.0][:N], np.float32), np.float32(366.25)
    ut, rt = torch.from_numpy(u.view(np.int16)).to(dev), torch.from_numpy(ratios).to(dev)
    h, w = 2 * (Hm // 6), 2 * (Wm // 6)

    def shaded(a_, b_):
        out = torch.full((N, 9, h, w), float('nan'), dtype=torch.float32, device=dev)
        at, bt = torch.from_numpy(a_).to(dev), torch.from_numpy(b_).to(dev)
        assert eld_lib.eld_pack_raw_xtrans_u16_shaded(L.dptr(ut), L.dptr(out), N, Hm, Wm, black, white, L.dptr(rt), L.dptr(at), L.dptr(bt), float(t),
                                                      L.cur_stream()) == 0
        return out.cpu().numpy()
    assert _same_bits(shaded(a, b), R.pack_xtrans_shaded(u, black, white, ratios, a, b, t))
    plain = torch.full((N, 9, h, w), float('nan'), dtype=torch.float32, device=dev)
    assert eld_lib.eld_pack_raw_xtrans_u16_gain(L.dptr(ut), L.dptr(plain), N, Hm, Wm, black, white, L.dptr(rt), L.cur_stream()) == 0
    z = np.zeros_like(a)
    assert _same_bits(shaded(z, z), plain.cpu().numpy())


# ---- argument errors, through the raw binding -----------------------------------------------------------------------------------------------
def test_einval_before_any_launch(eld_lib, dev):
    import torch
    from eld_amd import _lib as L
    Hm, Wm, F = 4, 8, 3
    pool = torch.zeros(F * Hm * Wm + 8, dtype=torch.int16, device=dev)
    table = np.zeros(F, L.POOL_FRAME_DTYPE)
    for i in range(F):
        table[i] = (i * Hm * Wm, Hm, Wm)
    tab = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
    a = torch.zeros((Hm, Wm), dtype=torch.float32, device=dev)
    b = torch.zeros((Hm, Wm), dtype=torch.float32, device=dev)
    bm = torch.zeros((Hm, 1), dtype=torch.int32, device=dev)
    d1, i4 = (ctypes.c_double * 16)(*([1.0] * 16)), (ctypes.c_int32 * 36)(*([512] * 36))
    s = L.cur_stream()

    def fit(pool_=pool, tab_=tab, F_=F, Hm_=Hm, Wm_=Wm, ses=(0, 3), S=1, al=d1, be=d1, cen=i4, p=2, bm_=None, a_=a, b_=b):
        sess = None if ses is None else (ctypes.c_int32 * len(ses))(*ses)
        return eld_lib.eld_shading_fit_u16(None if pool_ is None else (pool_ if isinstance(pool_, ctypes.c_void_p) else L.dptr(pool_)), pool.numel(),
                                           L.dptr(tab_), F_, Hm_, Wm_, sess, S, al, be, cen, p,
                                           bm_ if isinstance(bm_, ctypes.c_void_p) else L.dptr(bm_), L.dptr(a_), L.dptr(b_), s)
    assert fit() == 0
    assert fit(bm_=bm) == 0
    odd = ctypes.c_void_p(pool.data_ptr() + 2)
    cases = [dict(pool_=None), dict(tab_=None), dict(ses=None), dict(al=None), dict(be=None), dict(cen=None), dict(a_=None), dict(b_=None),
             dict(Wm_=7), dict(p=3), dict(p=4), dict(pool_=odd), dict(bm_=ctypes.c_void_p(bm.data_ptr() + 2)),
             dict(S=0), dict(S=17, ses=(0, 1) * 17), dict(ses=(0, 0)), dict(ses=(0, 65537), F_=70000), dict(ses=(1, 3)), dict(ses=(-1, 2)),
             dict(cen=(ctypes.c_int32 * 4)(512, 512, 65536, 512)), dict(cen=(ctypes.c_int32 * 4)(-1, 512, 512, 512)), dict(Hm_=-1)]
    for kw in cases:
        assert fit(**kw) == EINVAL, kw
    assert fit(Hm_=0) == 0 and fit(Wm_=0) == 0 and fit(Hm_=0, pool_=None, a_=None, b_=None) == 0

    u = torch.zeros((2, Hm, Wm), dtype=torch.int16, device=dev)

    def app(in_=L.dptr(u), out_=L.dptr(u), N=2, Hm_=Hm, Wm_=Wm, a_=L.dptr(a), b_=L.dptr(b), bm_=None):
        return eld_lib.eld_shading_apply_u16(in_, out_, N, Hm_, Wm_, a_, b_, 1.0, bm_, s)
    assert app() == 0 and app(bm_=L.dptr(bm)) == 0
    for kw in (dict(in_=None), dict(out_=None), dict(a_=None), dict(b_=None), dict(Wm_=7), dict(N=-1), dict(in_=ctypes.c_void_p(u.data_ptr() + 2)),
               dict(out_=ctypes.c_void_p(u.data_ptr() + 2)), dict(bm_=ctypes.c_void_p(bm.data_ptr() + 1))):
        assert app(**kw) == EINVAL, kw
    assert app(N=0) == 0 and app(Hm_=0) == 0 and app(N=0, in_=None, out_=None) == 0

    packed = torch.zeros((1, 4, 2, 4), dtype=torch.float32, device=dev)
    r = torch.ones(1, dtype=torch.float32, device=dev)
    pat, blk = (ctypes.c_int * 4)(0, 1, 3, 2), (ctypes.c_float * 4)(512, 512, 512, 512)

    def pb(m=L.dptr(u), o=L.dptr(packed), N=1, pat_=pat, blk_=blk, r_=L.dptr(r), a_=L.dptr(a), b_=L.dptr(b)):
        return eld_lib.eld_pack_raw_bayer_u16_shaded(m, o, N, 2, 4, pat_, blk_, 16383.0, r_, a_, b_, 1.0, s)
    assert pb() == 0 and pb(N=0) == 0
    for kw in (dict(m=None), dict(o=None), dict(r_=None), dict(a_=None), dict(b_=None), dict(pat_=None), dict(blk_=None), dict(N=-1),
               dict(pat_=(ctypes.c_int * 4)(0, 1, 1, 2)), dict(pat_=(ctypes.c_int * 4)(0, 1, 4, 2))):
        assert pb(**kw) == EINVAL, kw
    x = torch.zeros((1, 6, 6), dtype=torch.int16, device=dev)
    xa = torch.zeros((6, 6), dtype=torch.float32, device=dev)
    xo = torch.zeros((1, 9, 2, 2), dtype=torch.float32, device=dev)

    def px(m=L.dptr(x), o=L.dptr(xo), N=1, white=16383.0, r_=L.dptr(r), a_=L.dptr(xa), b_=L.dptr(xa)):
        return eld_lib.eld_pack_raw_xtrans_u16_shaded(m, o, N, 6, 6, 1024.0, white, r_, a_, b_, 1.0, s)
    assert px() == 0 and px(N=0) == 0
    for kw in (dict(m=None), dict(o=None), dict(r_=None), dict(a_=None), dict(b_=None), dict(N=-1), dict(white=1024.0)):
        assert px(**kw) == EINVAL, kw
    torch.cuda.synchronize()


# ---- the closed loop on the device ----------------------------------------------------------------------------------------------------------
def test_closed_loop_planes_are_the_restatements(dev):
    """fit_dark_shading on the inputs of the CPU closed loop gives the restatement's planes bit for bit: the statistical bounds of
    tests/test_shading_cpu.py hold for the device's planes without being restated."""
    from eld_amd.shading import fit_dark_shading
    d, c = R.closed_loop_inputs(), R.LOOP
    sh = fit_dark_shading([{'iso': iso, 'bias': u} for iso, u in zip(c['isos'], d['sessions'])], 'bayer', PAT, c['black'], device=dev)
    x0, alpha, beta = R.coefficients(c['isos'], [c['frames']] * 3)
    wa, wb = R.fit(d['sessions'], alpha, beta, np.full((2, 2), c['black']))
    assert sh.x0 == x0 and (sh.iso_min, sh.iso_max, sh.counts, sh.shape) == (800.0, 3200.0, [8, 8, 8], (256, 384))
    assert _same_bits(sh.a, wa) and _same_bits(sh.b, wb)
    got = sh.apply(d['held'], 1600)
    assert np.array_equal(got, R.apply(d['held'], wa, wb, np.float32(1600 - x0)))
    import torch
    ht = torch.from_numpy(d['held'].view(np.int16)).to(dev)
    assert np.array_equal(sh.apply(ht, 1600).cpu().numpy().view(np.uint16), got)
    assert sh.apply(ht, 1600, out=ht) is ht and np.array_equal(ht.cpu().numpy().view(np.uint16), got)


def test_centred_fit_and_defects(dev):
    from eld_amd.defects import DefectMap
    from eld_amd.shading import fit_dark_shading
    rng = np.random.default_rng(9)
    shape = (12, 24)
    sessions = [{'iso': 400, 'bias': _codes(rng, (2,) + shape)}, {'iso': 1600, 'bias': _codes(rng, (3,) + shape)}]
    dmap = DefectMap.from_sites([(0, 0), (5, 7), (11, 23)], shape)
    sh = fit_dark_shading(sessions, 'bayer', PAT, [512, 513, 511, 512], defects=dmap, centred=True, device=dev)
    plain = fit_dark_shading(sessions, 'bayer', PAT, [512, 513, 511, 512], defects=dmap, device=dev)
    x0, alpha, beta = R.coefficients([400, 1600], [2, 3])
    wa, wb = R.fit([s['bias'] for s in sessions], alpha, beta, np.array([[512, 513], [512, 511]]), dmap.mask)
    assert _same_bits(plain.a, wa) and _same_bits(plain.b, wb) and sh.centred and not plain.centred
    good = ~dmap.mask
    for got, src in ((sh.a, wa), (sh.b, wb)):
        assert np.all(got[dmap.mask] == 0)
        for r in range(2):
            for c in range(2):
                g = good[r::2, c::2]
                m = np.float32(src[r::2, c::2][g].astype(np.float64).mean())
                assert np.allclose(got[r::2, c::2][g], src[r::2, c::2][g] - m, rtol=0, atol=np.finfo(np.float32).eps * np.abs(src).max())


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
HM, WM, F = 256, 384, 3
PLANT_ISOS, PLANT_SIGMA, FIT_FRAMES = (800, 1600), (2.0, 3.0), 8
REC = {'K': 2.0, 'g_scale': 2.5, 'G_scale': 2.5, 'R_scale': 0.0, 'lambda': 0.14, 'color_bias': [0.0] * 4}


@pytest.fixture(scope='module')
def plant(dev):
    """A pixel and a column pattern, both linear in ISO; per ISO three frames to validate and eight OTHER frames to fit the map from."""
    from eld_amd.shading import fit_dark_shading
    rng = np.random.default_rng(41)
    pix = [1.5 * rng.standard_normal((HM, WM)), 1.5 * rng.standard_normal((HM, WM)) / 1600.0]
    col = [1.0 * rng.standard_normal(WM), 1.0 * rng.standard_normal(WM) / 1600.0]

    def mint(iso, sigma, n):
        fixed = 512 + pix[0] + pix[1] * iso + (col[0] + col[1] * iso)[None, :]
        return np.rint(fixed[None] + sigma * rng.standard_normal((n, HM, WM))).astype(np.uint16)
    sessions, fit_sessions, vf, vc = [], [], [], []
    for iso, sg in zip(PLANT_ISOS, PLANT_SIGMA):
        fr = mint(iso, sg, F + 2)
        sessions.append({'iso': iso, 'bias': fr[:F], 'flats': fr[F:][None]})
        fit_sessions.append({'iso': iso, 'bias': mint(iso, sg, FIT_FRAMES)})
        vf.append(float(np.var(pix[0] + pix[1] * iso)))
        vc.append(float(np.var(col[0] + col[1] * iso)))
    sh = fit_dark_shading(fit_sessions, 'bayer', PAT, 512, device=dev)
    return sessions, sh, vf, vc


def test_validate_camera_shows_the_correction(plant):
    from eld_amd.validate import validate_camera
    sessions, sh, vf, vc = plant
    kw = dict(diag={'frames': [dict(REC) for _ in range(2 * F)]}, models=('Pg',), source='frames', radius=64, flat_radius=256, structure=True, lags=2)
    before = validate_camera(sessions, PAT, [512.0] * 4, 16383, **kw)
    after = validate_camera(sessions, PAT, [512.0] * 4, 16383, shading=sh, **kw)
    assert 'shading' not in before and after['shading']['x0'] == sh.x0
    N, N_c, n_c = (HM // 2) * (WM // 2), WM // 2, HM // 2        # sites of a colour group, its column entries, sites per column entry
    for si, sg in enumerate(PLANT_SIGMA):
        temporal = sg ** 2 + 1.0 / 12.0
        # without the map the report shows the plant (the bounds of tests/test_validate_structure_gpu.py, no row term)
        real = before['structure']['sessions'][si]['real']
        fixed, site = vf[si] + vc[si], temporal + vf[si]
        col_a, col_c = vc[si] + site / n_c, vc[si] + vf[si] / n_c
        print('iso %d before: pix_fixed %.4f (plant %.4f)  col_fixed %.4f (plant %.4f)' % (PLANT_ISOS[si], real['pix_fixed_var'], fixed,
                                                                                          real['col_fixed_var'], vc[si]))
        assert abs(real['pix_fixed_var'] - fixed) < 5 * math.sqrt(((site + vc[si]) ** 2 + fixed ** 2) / N + 2 * vc[si] ** 2 / (N_c - 1))
        assert abs(real['col_fixed_var'] - vc[si]) < 5 * math.sqrt((col_a ** 2 + col_c ** 2) / (N_c - 1))
        # with it: two sessions make the line pass through each session's own mean, so the map's error at that ISO is the noise of the
        # mean of its 8 fit frames, independent from site to site, plus the remainder of rint(ds): no column term is left
        rem = temporal / FIT_FRAMES + 1.0 / 12.0
        real = after['structure']['sessions'][si]['real']
        site = temporal + rem
        print('iso %d after:  pix_fixed %.4f (predicted %.4f)  col_fixed %.4f (predicted 0)' % (PLANT_ISOS[si], real['pix_fixed_var'], rem,
                                                                                               real['col_fixed_var']))
        assert abs(real['pix_fixed_var'] - rem) < 5 * math.sqrt((site ** 2 + rem ** 2) / N)
        assert abs(real['col_fixed_var']) < 5 * math.sqrt(((site / n_c) ** 2 + (rem / n_c) ** 2) / (N_c - 1))


def test_denoise_raw_is_the_manual_composition(dev):
    import torch
    from eld_amd.defects import DefectMap, repair_device
    from eld_amd.denoise import denoise_raw, load_denoiser, pack_input, run_network, write_back
    from eld_amd.shading import DarkShading
    from eld_amd.unet import UNetSeeInDark
    torch.manual_seed(7)
    den = load_denoiser(UNetSeeInDark(4, 4), cfa='bayer', device=dev)
    rng = np.random.default_rng(8)
    Hm, Wm = 64, 96
    u = _codes(rng, (2, Hm, Wm), 500, 700)
    sh = DarkShading((3 * rng.standard_normal((Hm, Wm))).astype(np.float32), (rng.standard_normal((Hm, Wm)) / 800).astype(np.float32),
                     1500.0, 800, 3200, 'bayer', PAT)
    dmap = DefectMap.from_sites([(3, 5), (40, 77)], (Hm, Wm))
    res = denoise_raw(den, u, 'bayer', raw_pattern=PAT, black_level=512, ratio=[100.0, 200.0], defects=dmap, shading=sh, iso=1600)
    t = repair_device(torch.from_numpy(u.view(np.int16)).to(dev), dmap)
    x = pack_input(t, 'bayer', [0, 1, 3, 2], [512.0] * 4, 16383.0, np.array([100.0, 200.0], np.float32), sh, sh.t(1600))
    want_x = R.pack_bayer_shaded(t.cpu().numpy().view(np.uint16), PAT, [512.0] * 4, 16383.0, [100.0, 200.0], sh.a, sh.b, sh.t(1600))
    assert _same_bits(x.cpu().numpy(), want_x)
    out = run_network(den, x)
    mosaic = write_back(out, t.clone(), 'bayer', [0, 1, 3, 2], [512.0] * 4, 16383.0)
    assert _same_bits(res['packed'], out.cpu().numpy())
    assert np.array_equal(res['mosaic'], mosaic.cpu().numpy().view(np.uint16))
    plain = denoise_raw(den, u, 'bayer', raw_pattern=PAT, black_level=512, ratio=[100.0, 200.0], defects=dmap)
    assert not np.array_equal(plain['packed'], res['packed'])


def test_dark_pool_corrects_its_frames_at_upload(dev):
    import torch
    from eld_amd import _lib as L
    from eld_amd.darkpool import DarkPool
    from eld_amd.noise import NoiseParams, sample_noise
    from eld_amd.shading import DarkShading
    rng = np.random.default_rng(12)
    Hm, Wm = 20, 28
    sessions = [{'iso': 800, 'bias': _codes(rng, (3, Hm, Wm))}, {'iso': 3200, 'bias': _codes(rng, (2, Hm, Wm))}]
    sh = DarkShading((3 * rng.standard_normal((Hm, Wm))).astype(np.float32), (rng.standard_normal((Hm, Wm)) / 500).astype(np.float32),
                     1500.0, 800, 3200, 'bayer', PAT)
    kw = dict(raw_pattern=PAT, black_level=512, white_level=16383, K=[1.5, 3.0], device=dev)
    pool = DarkPool(sessions, shading=sh, **kw)
    before = [{'iso': s['iso'], 'bias': sh.apply(s['bias'], s['iso'])} for s in sessions]
    for s, b in zip(sessions, before):
        assert np.array_equal(b['bias'], R.apply(s['bias'], sh.a, sh.b, sh.t(s['iso'])))
    ref = DarkPool(before, **kw)
    assert torch.equal(pool.pool.buffer, ref.pool.buffer)
    y = torch.from_numpy(rng.uniform(size=(4, 4, 8, 12)).astype(np.float32)).to(dev)
    prm = [NoiseParams(pool.K[i % 2], 0.0, pool.saturation, 120.0 + i, dark=pool.ranges[i % 2]) for i in range(4)]
    flags, ids = L.SHOT_POISSON | L.DARK, [3, 9, 1 << 40, 4]
    assert torch.equal(sample_noise(y, prm, flags, 2018, ids, dark=pool), sample_noise(y, prm, flags, 2018, ids, dark=ref))
    plain = DarkPool(sessions, **kw)
    assert not torch.equal(plain.pool.buffer, pool.pool.buffer)
