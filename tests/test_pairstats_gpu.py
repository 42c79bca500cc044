"""eld_pair_level_stats_u16 (csrc/pairstats.hip) against its NumPy restatement (tests/pairstats_ref.py), bit for bit: the outputs are exact
integer sums, so no case takes a tolerance.  The shapes are the smallest at which each path of the kernel can go wrong: the 16-byte path
inside rows (widths that are multiples of 8), the flat 16-byte path (other widths, odd ones and odd frame sizes included: frame starts move
off the 16-byte grid), the 2-byte path (a misaligned view), more than one workgroup per frame (32768 sites each), the crop, the bitmap."""
import ctypes

import numpy as np
import pytest

import pairstats_ref as R

pytestmark = pytest.mark.gpu

NB = R.NB
XT_COLOUR = np.array([[0, 2, 1, 2, 0, 1], [1, 1, 0, 1, 1, 2], [1, 1, 2, 1, 1, 0], [2, 0, 1, 0, 2, 1], [1, 1, 2, 1, 1, 0], [1, 1, 0, 1, 1, 2]])
ROTATIONS = ([0, 1, 3, 2], [1, 0, 2, 3], [3, 2, 0, 1], [2, 3, 1, 0])            # RGGB, GRBG, GBRG, BGGR as rawpy codes


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def _call(lib, est, ref, p, group, G, black, white, Hc=None, Wc=None, bitmap=None, F=None):
    """est, ref: CUDA int16 tensors (F,Hm,Wm) -> (rc, int64 ndarray (F,G,NB,4))"""
    import torch
    from eld_amd import _lib as L
    F_, Hm, Wm = ref.shape
    F = F_ if F is None else F
    out = torch.full((max(F, 1), G, NB, 4), -7, dtype=torch.int64, device=ref.device)       # the call must write every element
    need = lib.eld_pair_level_stats_workspace_bytes(F, Hm, Wm)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=ref.device)
    rc = lib.eld_pair_level_stats_u16(L.dptr(est), L.dptr(ref), F, Hm, Wm, Hm if Hc is None else Hc, Wm if Wc is None else Wc, p,
                                      (ctypes.c_int * (p * p))(*[int(v) for v in group]), G, (ctypes.c_int32 * (p * p))(*[int(v) for v in black]),
                                      white, L.dptr(bitmap), L.dptr(out), L.dptr(ws), need, L.cur_stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def _frames(rng, F, Hm, Wm, black, white):
    """Codes around every regime: below black, the small bins, the octaves, the white point and 65535."""
    pick = rng.integers(0, 4, size=(F, Hm, Wm))
    ref = np.where(pick == 0, rng.integers(max(black - 6, 0), black + 12, size=(F, Hm, Wm)),
                   np.where(pick == 1, rng.integers(0, 65536, size=(F, Hm, Wm)),
                            np.where(pick == 2, rng.integers(white - 3, white + 3, size=(F, Hm, Wm)), black + (1 << rng.integers(0, 14, size=(F, Hm, Wm))))))
    ref = np.clip(ref, 0, 65535).astype(np.uint16)
    est = np.clip(ref.astype(np.int64) + rng.integers(-40, 41, size=ref.shape) * rng.integers(0, 3, size=ref.shape) ** 6, 0, 65535).astype(np.uint16)
    return est, ref


BAYER_SHAPES = [(1, 2, 2), (3, 4, 10), (1, 6, 18), (3, 34, 70), (1, 8, 22), (3, 8, 22), (1, 16, 64), (1, 300, 256), (3, 130, 262)]


@pytest.mark.parametrize('F,Hm,Wm', BAYER_SHAPES)
def test_bayer_rotations(eld_lib, F, Hm, Wm):
    # (1, 300, 256): 76800 sites, three workgroups of the row path; (3, 130, 262): 34060 sites a frame, two of the flat path plus its edge group
    rng = np.random.default_rng(Hm * 1000 + Wm + F)
    blk4 = [512, 520, 500, 512]
    est, ref = _frames(rng, F, Hm, Wm, 512, 16383)
    de, dr = _dev(est), _dev(ref)
    for pat in ROTATIONS:
        black = [blk4[c] for c in pat]
        rc, out = _call(eld_lib, de, dr, 2, pat, 4, black, 16383)
        assert rc == 0
        assert np.array_equal(out, R.pair_level_sums(est, ref, 2, pat, 4, black, 16383)), pat


@pytest.mark.parametrize('Hm,Wm', [(12, 12), (16, 15), (22, 27)])
def test_xtrans(eld_lib, Hm, Wm):
    rng = np.random.default_rng(Hm + Wm)
    est, ref = _frames(rng, 2, Hm, Wm, 1024, 16383)
    group, black = XT_COLOUR.reshape(-1), [1024] * 36
    Hc, Wc = Hm // 6 * 6, Wm // 6 * 6
    rc, out = _call(eld_lib, _dev(est), _dev(ref), 6, group, 3, black, 16383, Hc, Wc)
    assert rc == 0
    want = R.pair_level_sums(est, ref, 6, group, 3, black, 16383, Hc, Wc)
    assert np.array_equal(out, want)
    assert int(out[..., 0].sum()) == 2 * Hc * Wc
    if (Hc, Wc) != (Hm, Wm):                                   # the border outside whole cells is really left out
        assert not np.array_equal(want, R.pair_level_sums(est, ref, 6, group, 3, black, 16383))


def test_misaligned_views_take_the_scalar_path(eld_lib):
    rng = np.random.default_rng(5)
    est, ref = _frames(rng, 2, 10, 14, 512, 16383)
    import torch
    be = torch.zeros(est.size + 8, dtype=torch.int16, device='cuda')
    br = torch.zeros(ref.size + 8, dtype=torch.int16, device='cuda')
    for off in (1, 3, 4):                                      # 2, 6 and 8 bytes off the 16-byte grid
        ve, vr = be[off:off + est.size].view(est.shape), br[off:off + ref.size].view(ref.shape)
        ve.copy_(_dev(est)); vr.copy_(_dev(ref))
        rc, out = _call(eld_lib, ve, vr, 2, [0, 1, 3, 2], 4, [512] * 4, 16383)
        assert rc == 0
        assert np.array_equal(out, R.pair_level_sums(est, ref, 2, [0, 1, 3, 2], 4, [512] * 4, 16383))
    est, ref = _frames(rng, 2, 12, 18, 1024, 16383)            # the same path under the X-Trans cell
    ve, vr = torch.zeros(est.size + 1, dtype=torch.int16, device='cuda')[1:].view(est.shape), torch.zeros(ref.size + 1, dtype=torch.int16, device='cuda')[1:].view(ref.shape)
    ve.copy_(_dev(est)); vr.copy_(_dev(ref))
    rc, out = _call(eld_lib, ve, vr, 6, XT_COLOUR.reshape(-1), 3, [1024] * 36, 16383)
    assert rc == 0 and ve.data_ptr() % 16 == 2
    assert np.array_equal(out, R.pair_level_sums(est, ref, 6, XT_COLOUR.reshape(-1), 3, [1024] * 36, 16383))


def test_every_bin_populated(eld_lib):
    black, white = 512, 16383
    codes = set([0, black - 1, black, white - 1, white, 65535])
    codes.update(black + s for s in range(0, 8))
    for o in range(3, 16):
        for q in range(4):
            lo = (4 + q) << (o - 2)                            # the first code of quarter q of octave o ...
            codes.update(c for c in (black + lo, black + lo + (1 << (o - 2)) - 1) if c <= 65535)     # ... and the last
    codes = sorted(codes)
    n = len(codes) * 4
    Wm = 16
    Hm = -(-n // Wm) + (-(-n // Wm)) % 2
    ref = np.full(Hm * Wm, black + 1, np.uint16)
    ref[:n] = np.repeat(codes, 4)                              # every code on four consecutive sites
    ref = ref.reshape(1, Hm, Wm)
    est = np.clip(ref.astype(np.int64) + np.arange(Hm * Wm).reshape(1, Hm, Wm) % 7 - 3, 0, 65535).astype(np.uint16)
    # white above every code: all 60 unsaturated bins; white = 16383: the saturated bin too
    rc, out = _call(eld_lib, _dev(est), _dev(ref), 2, [0, 0, 0, 0], 1, [black] * 4, 65536)
    assert rc == 0
    assert np.array_equal(out, R.pair_level_sums(est, ref, 2, [0, 0, 0, 0], 1, [black] * 4, 65536))
    assert np.all(out[0, 0, :NB - 1, 0] > 0) and out[0, 0, NB - 1, 0] == 0
    rc, out = _call(eld_lib, _dev(est), _dev(ref), 2, [0, 0, 0, 0], 1, [black] * 4, white)
    assert rc == 0
    assert np.array_equal(out, R.pair_level_sums(est, ref, 2, [0, 0, 0, 0], 1, [black] * 4, white))
    top = R.bin_loop(white - 1, black, white)
    assert np.all(out[0, 0, :top + 1, 0] > 0) and out[0, 0, NB - 1, 0] == int((ref >= white).sum())


def test_contention_all_sites_in_one_bin(eld_lib):
    Hm, Wm, black = 96, 512, 512                               # 49152 sites: two workgroups, every lane in bin 1
    ref = np.full((1, Hm, Wm), black + 1, np.uint16)
    est = (ref.astype(np.int64) + (np.arange(Hm * Wm).reshape(1, Hm, Wm) % 5) - 2).astype(np.uint16)
    rc, out = _call(eld_lib, _dev(est), _dev(ref), 2, [0, 1, 3, 2], 4, [black] * 4, 16383)
    assert rc == 0
    assert np.array_equal(out, R.pair_level_sums(est, ref, 2, [0, 1, 3, 2], 4, [black] * 4, 16383))
    assert np.array_equal(out[0, :, 1, 0], [Hm * Wm // 4] * 4) and int(out[..., 0].sum()) == Hm * Wm


def test_sum_of_squares_beyond_float64(eld_lib):
    Hm, Wm = 2048, 1100
    ref = np.zeros((1, Hm, Wm), np.uint16)
    est = np.full((1, Hm, Wm), 65535, np.uint16)
    rc, out = _call(eld_lib, _dev(est), _dev(ref), 2, [0, 0, 0, 0], 1, [0] * 4, 65536)
    assert rc == 0
    n = Hm * Wm
    want = np.zeros((1, 1, NB, 4), np.int64)
    want[0, 0, 0] = [n, 0, 65535 * n, 65535 * 65535 * n]        # Python integers: exact
    assert 65535 * 65535 * n > 2 ** 53
    assert np.array_equal(out, want)


def test_defect_bitmap(eld_lib):
    from eld_amd.defects import pack_bitmap
    rng = np.random.default_rng(9)
    for Hm, Wm in ((34, 70), (20, 64), (9, 37)):
        est, ref = _frames(rng, 2, Hm, Wm, 512, 16383)
        mask = rng.uniform(size=(Hm, Wm)) < 0.1
        mask[0, 0] = mask[Hm - 1, Wm - 1] = True
        import torch
        bm = torch.from_numpy(pack_bitmap(mask).view(np.int32).copy()).cuda()
        zero = torch.zeros_like(bm)
        args = (2, [0, 1, 3, 2], 4, [512] * 4, 16383)
        rc, out = _call(eld_lib, _dev(est), _dev(ref), *args, bitmap=bm)
        assert rc == 0
        assert np.array_equal(out, R.pair_level_sums(est, ref, *args, mask=mask))
        rc0, plain = _call(eld_lib, _dev(est), _dev(ref), *args)
        rcz, zeroed = _call(eld_lib, _dev(est), _dev(ref), *args, bitmap=zero)
        assert rc0 == 0 and rcz == 0
        assert np.array_equal(plain, zeroed)                   # a null bitmap and an all-zero one
        assert np.array_equal(plain[..., 0].sum(axis=(1, 2)) - out[..., 0].sum(axis=(1, 2)), [int(mask.sum())] * 2)


def test_repeat_call_and_group_minus_one(eld_lib):
    rng = np.random.default_rng(11)
    est, ref = _frames(rng, 2, 34, 70, 512, 16383)
    de, dr = _dev(est), _dev(ref)
    a = _call(eld_lib, de, dr, 2, [0, 1, -1, 1], 2, [512, 500, 0, 500], 16383)
    b = _call(eld_lib, de, dr, 2, [0, 1, -1, 1], 2, [512, 500, 0, 500], 16383)
    assert a[0] == 0 and b[0] == 0 and np.array_equal(a[1], b[1])
    assert np.array_equal(a[1], R.pair_level_sums(est, ref, 2, [0, 1, -1, 1], 2, [512, 500, 0, 500], 16383))


def test_empty_problems(eld_lib):
    rng = np.random.default_rng(2)
    est, ref = _frames(rng, 1, 4, 8, 512, 16383)
    de, dr = _dev(est), _dev(ref)
    rc, out = _call(eld_lib, de, dr, 2, [0, 1, 3, 2], 4, [512] * 4, 16383, Hc=0)
    assert rc == 0 and not out.any()                           # zeroed, nothing counted
    rc, out = _call(eld_lib, de, dr, 2, [0, 1, 3, 2], 4, [512] * 4, 16383, F=0)
    assert rc == 0 and np.all(out == -7)                       # F == 0: nothing is touched


def test_argument_errors(eld_lib):
    import torch
    from eld_amd import _lib as L
    E = -1
    est = torch.zeros((2, 4, 8), dtype=torch.int16, device='cuda')
    ref = torch.zeros_like(est)
    out = torch.full((2, 4, NB, 4), -7, dtype=torch.int64, device='cuda')

    def call(est_=est, ref_=ref, F=2, Hm=4, Wm=8, Hc=4, Wc=8, p=2, group=(0, 1, 3, 2), G=4, black=(512,) * 4, white=16383, bitmap=None, out_=out,
             ws_bytes=0):
        g = None if group is None else (ctypes.c_int * len(group))(*group)
        b = None if black is None else (ctypes.c_int32 * len(black))(*black)
        ptr = lambda t: t if (t is None or isinstance(t, ctypes.c_void_p)) else L.dptr(t)
        return eld_lib.eld_pair_level_stats_u16(ptr(est_), ptr(ref_), F, Hm, Wm, Hc, Wc, p, g, G, b, white, ptr(bitmap), ptr(out_), None, ws_bytes,
                                                L.cur_stream())

    assert call() == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:, :, 0], [[[8, -512 * 8, 0, 0]] * 4] * 2) and not got[:, :, 1:].any()      # code 0 everywhere: s = -512, bin 0
    out.fill_(-7)
    bad = [dict(p=3), dict(p=6), dict(F=-1), dict(F=65536), dict(Hm=-1), dict(Wm=-1), dict(Hc=5), dict(Wc=9), dict(Hc=-1), dict(G=0), dict(G=5),
           dict(group=None), dict(black=None), dict(group=(0, 1, 4, 2)), dict(group=(0, -2, 3, 2)), dict(black=(512, 512, -1, 512)),
           dict(black=(512, 65536, 0, 0)), dict(white=0), dict(white=65537), dict(Hm=1 << 16, Wm=1 << 15, Hc=0, Wc=0), dict(est_=None), dict(ref_=None),
           dict(out_=None), dict(out_=ctypes.c_void_p(out.data_ptr() + 4)), dict(est_=ctypes.c_void_p(est.data_ptr() + 1)),
           dict(ref_=ctypes.c_void_p(ref.data_ptr() + 1)), dict(bitmap=ctypes.c_void_p(est.data_ptr() + 2))]
    for kw in bad:
        if kw == dict(p=6):
            kw = dict(p=6, group=(0,) * 35 + (3,), black=(0,) * 36, G=3)          # a group outside [-1, G) in the last cell
        assert call(**kw) == E, kw
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == -7)                     # no launch happened: the output is untouched
    assert eld_lib.eld_pair_level_stats_workspace_bytes(2, 4, 8) == 0
