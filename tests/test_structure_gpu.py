"""eld_struct_sums_u16 / eld_struct_cross_u16 against the NumPy restatement: every integer output bit for bit (tests/structure_ref.py)."""
import ctypes

import numpy as np
import pytest
import torch

from eld_amd import _lib as L
from eld_amd.defects import pack_bitmap

from structure_ref import cross_ref, sums_ref

pytestmark = pytest.mark.gpu
EINVAL = -1


@pytest.fixture(scope='module')
def lib(eld_lib):
    assert torch.cuda.is_available()
    return eld_lib


def _cen(centre):
    c = [int(v) for v in np.asarray(centre).reshape(-1)]
    return (ctypes.c_int32 * len(c))(*c)


def _dev_u16(u, offset=0):
    """The stack on the device; offset > 0: a view starting `offset` elements into a 16-byte aligned buffer."""
    flat = torch.zeros(u.size + offset, dtype=torch.int16, device='cuda')
    flat[offset:] = torch.from_numpy(np.ascontiguousarray(u).view(np.int16).reshape(-1)).cuda()
    assert flat.data_ptr() % 16 == 0
    return flat[offset:].view(u.shape), flat


def run_sums(lib, u, p, centre, mask=None, offset=0):
    F, Hm, Wm = u.shape
    t, keep = _dev_u16(u, offset)
    bm = None if mask is None else torch.from_numpy(pack_bitmap(mask).view(np.int32).copy()).cuda()
    row = torch.full((F, Hm, p, 2), -7, dtype=torch.int64, device='cuda')
    col = torch.full((F, Wm, p, 2), -7, dtype=torch.int64, device='cuda')
    cell = torch.full((F, p * p, 3), -7, dtype=torch.int64, device='cuda')
    rc = lib.eld_struct_sums_u16(L.dptr(t), F, Hm, Wm, p, _cen(centre), L.dptr(bm), L.dptr(row), L.dptr(col), L.dptr(cell), L.cur_stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return row.cpu().numpy(), col.cpu().numpy(), cell.cpu().numpy()


def run_cross(lib, u, p, centre, pairs, mask=None, offset=0):
    F, Hm, Wm = u.shape
    t, keep = _dev_u16(u, offset)
    bm = None if mask is None else torch.from_numpy(pack_bitmap(mask).view(np.int32).copy()).cuda()
    q = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    cross = torch.full((len(q), p * p), -7, dtype=torch.int64, device='cuda')
    rc = lib.eld_struct_cross_u16(L.dptr(t), F, Hm, Wm, p, _cen(centre), L.dptr(bm), q.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(q),
                                  L.dptr(cross), L.cur_stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return cross.cpu().numpy()


def check_all(lib, u, p, centre, mask=None, offset=0, pairs=None):
    want = sums_ref(u, p, centre, mask)
    got = run_sums(lib, u, p, centre, mask, offset)
    for name, g, w in zip(('row', 'col', 'cell'), got, want):
        assert np.array_equal(g, w), '%s differs at %s' % (name, np.argwhere(g != w)[:4].tolist())
    F = u.shape[0]
    if pairs is None:
        pairs = [(a, b) for a in range(F) for b in range(a, F)][:3]
    gc = run_cross(lib, u, p, centre, pairs, mask, offset)
    wc = cross_ref(u, p, centre, pairs, mask)
    assert np.array_equal(gc, wc), 'cross differs at %s' % (np.argwhere(gc != wc)[:4].tolist(),)
    for q, (a, b) in enumerate(pairs):
        if a == b:
            assert np.array_equal(gc[q], got[2][a, :, 2])            # (a, a) is that frame's sum d^2
    return got


def stack(seed, shape, lo=0, hi=65536):
    return np.random.default_rng(seed).integers(lo, hi, size=shape).astype(np.uint16)


BAYER_CEN = [512, 520, 500, 531]


def test_bayer_word_path_width_not_a_multiple_of_8(lib):
    check_all(lib, stack(1, (3, 38, 46)), 2, BAYER_CEN)


def test_bayer_vector_path(lib):
    check_all(lib, stack(2, (2, 64, 72)), 2, BAYER_CEN)


def test_bayer_aligned_width_on_a_misaligned_view(lib):
    check_all(lib, stack(3, (2, 64, 72)), 2, BAYER_CEN, offset=2)


def test_bayer_several_bands_and_workgroups(lib):
    check_all(lib, stack(4, (1, 1100, 200)), 2, BAYER_CEN)
    check_all(lib, stack(5, (1, 300, 1040)), 2, BAYER_CEN)           # three column spans on the vector path
    check_all(lib, stack(6, (1, 40, 270)), 2, BAYER_CEN)             # three column spans on the word path


def test_bayer_with_bitmap(lib):
    u = stack(7, (2, 70, 96))
    mask = np.zeros((70, 96), bool)
    mask[[3, 17, 40, 69], [31, 32, 63, 64]] = True
    mask[11, :] = True
    mask[:, 50] = True
    row, col, cell = check_all(lib, u, 2, BAYER_CEN, mask)
    assert np.all(row[:, 11] == 0) and np.all(col[:, 50] == 0)       # n == 0 entries are (0, 0)


@pytest.mark.parametrize('code,centre', [(65535, 0), (0, 65535)])
def test_accumulator_width(lib, code, centre):
    """A column of 40000 rows sums to 2.6e9 > 2^31 over its two phases and a cell's sum d^2 to 6.9e14: any partial kept in 32 bits beyond
    its band wraps here."""
    u = np.full((1, 40000, 16), code, np.uint16)
    row, col, cell = check_all(lib, u, 2, [centre] * 4, pairs=[(0, 0)])
    assert abs(int(col[0, 0, :, 1].sum())) == 40000 * 65535 > 1 << 31
    assert int(cell[0, 0, 2]) == 20000 * 8 * 65535 ** 2


@pytest.mark.parametrize('shape', [(2, 40, 50), (2, 36, 48)])
@pytest.mark.parametrize('with_mask', [False, True])
def test_xtrans(lib, shape, with_mask):
    u = stack(8, shape)
    centre = 400 + 7 * np.arange(36)                                  # a different centre per cell
    mask = None
    if with_mask:
        mask = np.random.default_rng(9).uniform(size=shape[1:]) < 0.05
        mask[5, :] = True
        mask[:, 31] = True
        mask[:, 32] = True
    check_all(lib, u, 6, centre, mask)


def test_xtrans_several_spans_and_bands(lib):
    check_all(lib, stack(10, (1, 400, 1032)), 6, 300 + np.arange(36))   # vector path: three spans, three bands
    check_all(lib, stack(11, (1, 30, 134)), 6, 300 + np.arange(36))     # word path: two spans


def test_cross_pairs(lib):
    u = stack(12, (3, 38, 46))
    check_all(lib, u, 2, BAYER_CEN, pairs=[(0, 1), (2, 2), (2, 0)])
    u = stack(13, (3, 64, 72))
    check_all(lib, u, 2, BAYER_CEN, pairs=[(1, 1), (0, 2), (1, 0)])
    pairs = [(a, b) for a in range(3) for b in range(3)] * 8          # 72 pairs: more than one launch
    got = run_cross(lib, u, 2, BAYER_CEN, pairs)
    assert np.array_equal(got, cross_ref(u, 2, BAYER_CEN, pairs))


def test_empty_and_bad_input(lib):
    buf = torch.zeros(64 * 72 * 2 + 8, dtype=torch.int16, device='cuda')
    out = torch.full((8192,), -7, dtype=torch.int64, device='cuda')
    s = L.cur_stream()

    def sums(F=2, Hm=64, Wm=72, p=2, cen=BAYER_CEN, u=buf, row=out, col=out, cell=out):
        return lib.eld_struct_sums_u16(None if u is None else ctypes.c_void_p(u if isinstance(u, int) else u.data_ptr()), F, Hm, Wm, p,
                                       None if cen is None else _cen(cen), None,
                                       ctypes.c_void_p(row if isinstance(row, int) else row.data_ptr()),
                                       ctypes.c_void_p(col if isinstance(col, int) else col.data_ptr()),
                                       ctypes.c_void_p(cell if isinstance(cell, int) else cell.data_ptr()), s)

    assert sums(F=0) == 0
    torch.cuda.synchronize()
    assert int((out != -7).sum()) == 0                               # nothing written
    cell = torch.full((2 * 4 * 3,), -7, dtype=torch.int64, device='cuda')
    col = torch.full((2 * 72 * 2 * 2,), -7, dtype=torch.int64, device='cuda')
    assert sums(Hm=0, cell=cell, col=col) == 0                       # an empty frame: 0 after zeroing
    torch.cuda.synchronize()
    assert int(cell.abs().sum()) == 0 and int(col.abs().sum()) == 0
    assert sums(Wm=71) == EINVAL
    assert sums(p=3, cen=[0] * 9) == EINVAL
    assert sums(cen=[512, 520, 500, 65536]) == EINVAL
    assert sums(cen=[512, -1, 500, 531]) == EINVAL
    assert sums(cen=None) == EINVAL
    assert sums(F=-1) == EINVAL
    assert sums(Hm=1 << 16, Wm=1 << 15) == EINVAL
    assert sums(row=out.data_ptr() + 4) == EINVAL                    # a misaligned output
    assert sums(u=buf.data_ptr() + 2) == EINVAL
    assert sums(u=None) == EINVAL
    q = np.array([[0, 1], [1, 2]], np.int32)

    def cross(F=2, pairs=q, Q=1, out_=out, Wm=72):
        return lib.eld_struct_cross_u16(L.dptr(buf), F, 64, Wm, 2, _cen(BAYER_CEN), None,
                                        None if pairs is None else pairs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), Q,
                                        ctypes.c_void_p(out_ if isinstance(out_, int) else out_.data_ptr()), s)

    assert cross(Q=0) == 0
    assert cross(Q=2) == EINVAL                                      # frame 2 of a stack of 2
    assert cross(Q=1, pairs=None) == EINVAL
    assert cross(Q=-1) == EINVAL
    assert cross(Wm=71) == EINVAL
    assert cross(out_=out.data_ptr() + 4) == EINVAL
    torch.cuda.synchronize()
    assert int((out != -7).sum()) == 0                               # every refusal came before any launch
