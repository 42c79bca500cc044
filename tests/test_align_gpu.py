"""csrc/align.hip against its NumPy restatement (tests/align_ref.py), bit for bit: the luma pyramid, the displacement field and its costs,
and the stack through a field (mean, kept, present, ptc).  Everything is integer, so no case takes a tolerance.  The shapes are the
smallest that reach each branch: one tile and one level, odd luma sides (clamped downsample, shifted-back tiles), two and three levels,
X-Trans sides that are no multiples of 6, both load paths.  Then the public surface: stack_burst(align=...), and the command line."""
import ctypes

import numpy as np
import pytest

import align_ref as A
import burst_ref as R
from test_align_cpu import BAYER, WHITE, XTRANS

pytestmark = pytest.mark.gpu

NB = R.NB
EINVAL, EWS = -1, -3              # include/eld_amd.h


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def _odd_view(fr):
    """The same codes in a buffer that starts at an odd element: 2-byte aligned only, so every kernel takes its fallback loads."""
    import torch
    buf = torch.zeros(fr.size + 8, dtype=torch.int16, device='cuda')
    view = buf[1:1 + fr.size].view(fr.shape)
    view.copy_(_dev(fr))
    assert view.data_ptr() % 4 == 2
    return view


def _pyramid(lib, fr, p, levels):
    import torch
    from eld_amd import _lib as L
    N, Hm, Wm = fr.shape
    n = lib.eld_burst_luma_pyramid_elems(N, Hm, Wm, p, levels)
    out = torch.full((n,), -7, dtype=torch.int16, device=fr.device)
    assert lib.eld_burst_luma_pyramid_u16(L.dptr(fr), N, Hm, Wm, p, levels, L.dptr(out), L.cur_stream()) == 0
    torch.cuda.synchronize()
    flat, res, o = out.cpu().numpy().view(np.uint16), [], 0
    for h, w in A.level_sides(Hm, Wm, p, levels):
        res.append(flat[o:o + N * h * w].reshape(N, h, w))
        o += N * h * w
    assert o == n
    return res


def _align(lib, fr, p, ref, levels):
    """-> (rc, disp int16, cost uint32); the outputs start from a sentinel"""
    import torch
    from eld_amd import _lib as L
    N, Hm, Wm = fr.shape
    TY, TX = A.tiles(Hm // p)[0], A.tiles(Wm // p)[0]
    disp = torch.full((N, TY, TX, 2), -77, dtype=torch.int16, device=fr.device)
    cost = torch.full((N, TY, TX), -7, dtype=torch.int32, device=fr.device)
    need = lib.eld_burst_align_workspace_bytes(N, Hm, Wm, p, levels)
    ws = torch.empty(max(need, 4), dtype=torch.uint8, device=fr.device)
    rc = lib.eld_burst_align_u16(L.dptr(fr), N, Hm, Wm, p, ref, levels, L.dptr(disp), L.dptr(cost), L.dptr(ws), need, L.cur_stream())
    torch.cuda.synchronize()
    return rc, disp.cpu().numpy(), cost.cpu().numpy().view(np.uint32)


def _check_align(lib, fr, p, ref, levels, dev=None):
    d = _dev(fr) if dev is None else dev
    for got, want in zip(_pyramid(lib, d, p, levels), A.pyramid(fr, p, levels)):
        assert np.array_equal(got, want)
    rc, disp, cost = _align(lib, d, p, ref, levels)
    want = A.align(fr, p, ref, levels)
    assert rc == 0
    assert np.array_equal(disp, want[0])
    assert np.array_equal(cost, want[1])
    return want


def _textured(seed, N, Hm, Wm, p, span):
    """A small shifted burst of the closed loop's scene: margin and span sized to the frame."""
    return A.shifted_burst(seed, Hm, Wm, p, N=N, span=span, margin=2 * span + 2)[0]


@pytest.fixture(scope='module')
def loop():
    """The closed-loop bursts of seed 0 and their restated fields, computed once."""
    out = {}
    for name, (layout, Hm, Wm) in (('bayer', (BAYER, 104, 136)), ('xtrans', (XTRANS, 204, 300))):
        fr, shifts, noisy = A.shifted_burst(0, Hm, Wm, layout[0])
        out[name] = (layout, fr, shifts, noisy, A.align(fr, layout[0]))
    return out


CASES = [('bayer', (32, 32), 3, 1, 2), ('bayer', (66, 70), 4, 2, 5), ('bayer', (136, 200), 3, 3, 9), ('xtrans', (100, 106), 3, 1, 2)]


@pytest.mark.parametrize('cfa,shape,N,levels,span', CASES, ids=lambda v: 'x'.join(str(q) for q in v) if isinstance(v, tuple) else str(v))
def test_field_bit_equality(eld_lib, cfa, shape, N, levels, span):
    p = 2 if cfa == 'bayer' else 6
    assert A.default_levels(shape[0], shape[1], p) == levels
    fr = _textured(7 + shape[1], N, shape[0], shape[1], p, span)
    disp, _ = _check_align(eld_lib, fr, p, 0, levels)
    assert disp[1:].any()
    if levels > 1:
        _check_align(eld_lib, fr, p, 0, 1)                         # fewer levels than the frame allows


@pytest.mark.parametrize('name', ['bayer', 'xtrans'])
def test_closed_loop_field(eld_lib, loop, name):
    layout, fr, shifts, _, want = loop[name]
    rc, disp, cost = _align(eld_lib, _dev(fr), layout[0], 0, 2)
    assert rc == 0 and np.array_equal(disp, want[0]) and np.array_equal(cost, want[1])
    assert np.array_equal(disp.astype(np.int64), np.broadcast_to(-shifts[:, None, None, :], disp.shape))     # every tile finds its shift
    for got, ref in zip(_pyramid(eld_lib, _dev(fr), layout[0], 2), A.pyramid(fr, layout[0], 2)):
        assert np.array_equal(got, ref)


def test_field_special_bursts(eld_lib):
    const = np.full((3, 66, 70), 777, np.uint16)                   # all ties: the start wins at every level
    disp, cost = _check_align(eld_lib, const, 2, 1, 2)
    assert not disp.any() and not cost.any()
    fr = _textured(3, 3, 66, 70, 2, 5)
    sat = fr.copy()
    sat[:, :, 36:] = 65535                                         # a saturated half: flat tiles tie, tiles across the edge do not
    _check_align(eld_lib, sat, 2, 0, 2)
    ext = np.stack([np.zeros((32, 32), np.uint16), np.full((32, 32), 65535, np.uint16)])
    _, cost = _check_align(eld_lib, ext, 2, 0, 1)
    assert cost[1, 0, 0] == 256 * 65535                            # the widest key
    want = _check_align(eld_lib, fr, 2, 2, 2)                      # ref = the last frame
    assert not want[0][2].any() and want[0][:2].any()
    _check_align(eld_lib, fr, 2, 0, 2, dev=_odd_view(fr))          # 2-byte loads in the luma kernel
    xt = _textured(5, 3, 100, 106, 6, 2)
    _check_align(eld_lib, xt, 6, 1, 1, dev=_odd_view(xt))


def test_align_argument_errors(eld_lib):
    from eld_amd import _lib as L
    fr = _dev(np.zeros((3, 66, 70), np.uint16))
    assert eld_lib.eld_burst_align_workspace_bytes(3, 66, 70, 2, 3) == 0 and eld_lib.eld_burst_luma_pyramid_elems(3, 30, 70, 2, 1) == 0
    assert eld_lib.eld_burst_luma_pyramid_elems(3, 66, 70, 2, 2) == 3 * (33 * 35 + 17 * 18)
    for ref, levels in ((3, 2), (-1, 2), (0, 0), (0, 5), (0, 3)):
        assert _align(eld_lib, fr, 2, ref, levels)[0] == EINVAL
    import torch
    disp = torch.zeros((3, 3, 3, 2), dtype=torch.int16, device='cuda')
    ws = torch.empty(16, dtype=torch.uint8, device='cuda')
    assert eld_lib.eld_burst_align_u16(L.dptr(fr), 3, 66, 70, 2, 0, 2, L.dptr(disp), None, L.dptr(ws), 16, L.cur_stream()) == EWS


# ---- the stack through a field -----------------------------------------------------------------------------------------------------------------
def _stack(lib, fr, layout, disp, white=WHITE, k2q=100, min_dev=2, bitmap=None, grid=None):
    """fr: CUDA int16 (N,Hm,Wm), disp: int16 array -> (rc, mean, kept, present, ptc)"""
    import torch
    from eld_amd import _lib as L
    p, group, G, black = layout
    N, Hm, Wm = fr.shape
    TY, TX = disp.shape[1:3] if grid is None else grid
    mean = torch.full((Hm, Wm), -7, dtype=torch.int16, device=fr.device)
    kept = torch.full((Hm, Wm), 201, dtype=torch.uint8, device=fr.device)
    present = torch.full((Hm, Wm), 202, dtype=torch.uint8, device=fr.device)
    ptc = torch.full((G, NB, 4), -7, dtype=torch.int64, device=fr.device)
    d = torch.from_numpy(np.ascontiguousarray(disp)).cuda()
    need = lib.eld_burst_stack_aligned_workspace_bytes(N, Hm, Wm)
    ws = torch.empty(max(need, 4), dtype=torch.uint8, device=fr.device)
    rc = lib.eld_burst_stack_aligned_u16(L.dptr(fr), N, Hm, Wm, p, (ctypes.c_int * (p * p))(*group), G, (ctypes.c_int32 * (p * p))(*black), white,
                                         L.dptr(bitmap), k2q, min_dev, L.dptr(d), TY, TX, L.dptr(mean), L.dptr(kept), L.dptr(present), L.dptr(ptc),
                                         L.dptr(ws), need, L.cur_stream())
    torch.cuda.synchronize()
    return rc, mean.cpu().numpy().view(np.uint16), kept.cpu().numpy(), present.cpu().numpy(), ptc.cpu().numpy()


def _equal(got, want):
    assert got[0] == 0
    for g, w in zip(got[1:], want):
        assert np.array_equal(g, w)


@pytest.mark.parametrize('name', ['bayer', 'xtrans'])
def test_stack_through_the_closed_loop_field(eld_lib, loop, name):
    import torch
    from eld_amd.defects import pack_bitmap
    layout, fr, shifts, noisy, (disp, _) = loop[name]
    p = layout[0]
    want = A.stack_aligned(fr, *layout, WHITE, 100, 2, disp)
    assert (want[2] < 5).any() and (want[2] == 5).any() and want[3][..., 0].sum() > 0
    _equal(_stack(eld_lib, _dev(fr), layout, disp), want)
    _equal(_stack(eld_lib, _odd_view(fr), layout, disp), want)     # 2-byte loads
    mask = np.random.default_rng(2).uniform(size=fr.shape[1:]) < 0.15
    bm = torch.from_numpy(pack_bitmap(mask).view(np.int32).copy()).cuda()
    flagged = A.stack_aligned(fr, *layout, WHITE, 100, 2, disp, mask=mask)
    assert not np.array_equal(flagged[3], want[3])
    _equal(_stack(eld_lib, _dev(fr), layout, disp, bitmap=bm), flagged)
    # where all five are present this is the tripod stack of the same noisy frames
    o = 12 * p
    tm, tk, _ = R.stack(noisy[:, o:o + fr.shape[1], o:o + fr.shape[2]], *layout, WHITE, 100, 2)
    full = want[2] == 5
    assert np.array_equal(want[0][full], tm[full]) and np.array_equal(want[1][full], tk[full])


def _outlier_burst(rng, N, Hm, Wm):
    """Noise around a ramp, and in every frame a patch of outliers: whatever M a site ends with, some sites hold one."""
    fr = 800 + 20 * (np.arange(Wm)[None, None, :] % 50) + rng.integers(-6, 7, size=(N, Hm, Wm))
    hit = rng.uniform(size=(N, Hm, Wm)) < 0.03
    return np.clip(fr + 5000 * hit, 0, 65535).astype(np.uint16)


@pytest.mark.parametrize('layout,shape', [(BAYER, (64, 96)), (XTRANS, (96, 204))], ids=['bayer', 'xtrans'])
@pytest.mark.parametrize('N', [2, 3, 5, 16])
def test_stack_through_a_random_field(eld_lib, layout, shape, N):
    import torch
    from eld_amd.defects import pack_bitmap
    p = layout[0]
    rng = np.random.default_rng(100 * N + p)
    fr = _outlier_burst(rng, N, *shape)
    TY, TX = A.tiles(shape[0] // p)[0], A.tiles(shape[1] // p)[0]
    disp = rng.integers(-60, 61, size=(N, TY, TX, 2)).astype(np.int16)
    disp[rng.uniform(size=(N, TY, TX)) < 0.5] = 0                  # half the tiles stay, the others go anywhere in +-60: M spreads
    disp[0] = 0
    disp[1:3, 0, 0] = 0                                            # the first tile: frames 0..2 stay, every later one leaves the frame,
    disp[3:, 0, 0] = (60, -60)                                     # so M = min(N, 3) there
    disp[-1, 0, 0] = (60, -60)
    disp[:, -1, -1] = 0                                            # the last tile: every frame present (the last one but for a border)
    disp[-1, -1, -1] = (-1, 1)
    want = A.stack_aligned(fr, *layout, WHITE, 100, 2, disp)
    M = want[2].astype(np.int64)
    assert M.min() >= 1 and M.max() == N and len(np.unique(M)) >= 2
    if N >= 5:
        assert ((M >= 4) & (want[1] < M)).any() and ((M < 4) & (M > 1)).any()      # rejections where M allows, none below M = 4
        s, pr = A.gather(fr, p, disp)
        small = (M < 4) & ((s > 4000) & pr).any(axis=0)
        assert small.any() and np.all(want[1][small] == M[small])                    # a planted outlier stays where M < 4
    _equal(_stack(eld_lib, _dev(fr), layout, disp), want)
    mask = rng.uniform(size=shape) < 0.1
    bm = torch.from_numpy(pack_bitmap(mask).view(np.int32).copy()).cuda()
    _equal(_stack(eld_lib, _odd_view(fr), layout, disp, bitmap=bm), A.stack_aligned(fr, *layout, WHITE, 100, 2, disp, mask=mask))
    _equal(_stack(eld_lib, _dev(fr), layout, disp, k2q=0), A.stack_aligned(fr, *layout, WHITE, 0, 2, disp))


@pytest.mark.parametrize('layout,shape', [(BAYER, (64, 96)), (XTRANS, (96, 204))], ids=['bayer', 'xtrans'])
def test_zero_field_is_the_unaligned_kernel(eld_lib, layout, shape):
    from test_burst_gpu import _call, _frames
    p = layout[0]
    for N in (2, 3, 5, 16):
        fr = _frames(np.random.default_rng(N), N, shape[0], shape[1], layout[3][0])
        disp = np.zeros((N, A.tiles(shape[0] // p)[0], A.tiles(shape[1] // p)[0], 2), np.int16)
        rc, mean, kept, ptc = _call(eld_lib, _dev(fr), layout)
        got = _stack(eld_lib, _dev(fr), layout, disp)
        assert rc == 0 and got[0] == 0
        assert np.array_equal(got[1], mean) and np.array_equal(got[2], kept) and np.array_equal(got[4], ptc) and np.all(got[3] == N)
        if N >= 4:
            assert (kept != N).any() and ptc[..., 0].sum() > 0


def test_stack_argument_errors(eld_lib):
    fr = _dev(np.full((3, 64, 96), 900, np.uint16))
    disp = np.zeros((3, 2, 3, 2), np.int16)
    assert _stack(eld_lib, fr, BAYER, disp)[0] == 0
    for bad in (61, -61, 32767):
        d = disp.copy()
        d[2, 1, 2, 1] = bad
        rc, mean = _stack(eld_lib, fr, BAYER, d)[:2]
        assert rc == EINVAL and np.all(mean == np.uint16(-7 & 0xFFFF))       # refused before the stack ran
    d = disp.copy()
    d[1, 0, 0] = (60, -60)
    assert _stack(eld_lib, fr, BAYER, d)[0] == 0
    assert _stack(eld_lib, fr, BAYER, disp, grid=(2, 2))[0] == EINVAL
    assert _stack(eld_lib, fr, BAYER, disp, k2q=257)[0] == EINVAL
    assert _stack(eld_lib, _dev(np.zeros((3, 30, 96), np.uint16)), BAYER, np.zeros((3, 1, 3, 2), np.int16))[0] == EINVAL


# ---- the public surface ------------------------------------------------------------------------------------------------------------------------
def test_stack_burst_aligned(eld_lib, loop):
    import torch
    from eld_amd.burst import BurstAlignment, align_burst, stack_burst
    layout, fr, shifts, noisy, (disp, cost) = loop['bayer']
    pat = [[0, 1], [3, 2]]
    al = align_burst(fr, 'bayer')
    assert np.array_equal(al.disp, disp) and np.array_equal(al.cost, cost) and (al.period, al.tile, al.levels, al.ref) == (2, 16, 2, 0)
    assert np.array_equal(al.shift_px(), -2.0 * shifts) and not al.outlier_share().any()
    stack = stack_burst(fr, 'bayer', pat, 512, WHITE, align=True)
    want = A.stack_aligned(fr, *layout, WHITE, 100, 2, disp)
    assert stack.mean.dtype == torch.uint16 and stack.present.dtype == torch.uint8 and np.array_equal(stack.align.disp, disp)
    got = (stack.mean.cpu().numpy(), stack.kept.cpu().numpy(), stack.present.cpu().numpy(), stack.ptc)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    tm, tk, _ = R.stack(noisy[:, 24:24 + 104, 24:24 + 136], *layout, WHITE, 100, 2)
    full = got[2] == 5
    assert full.mean() > 0.5 and np.array_equal(got[0][full], tm[full]) and np.array_equal(got[1][full], tk[full])
    assert abs(stack.absent_share() - float(np.mean(~full))) < 1e-12
    assert abs(stack.rejected_share() - float(np.mean(want[1] != want[2]))) < 1e-12
    # the negative control: the same burst without alignment is not the tripod stack
    plain = stack_burst(fr, 'bayer', pat, 512, WHITE)
    assert plain.present is None and plain.align is None
    pm = plain.mean.cpu().numpy()
    assert np.mean(pm[full] != tm[full]) > 0.5
    assert np.abs(pm[full].astype(np.int64) - tm[full]).mean() > 20 * np.abs(got[0][full].astype(np.int64) - tm[full]).mean() + 20
    # ... and it is what it was before: the unaligned kernel's restatement
    wp = R.stack(fr, *layout, WHITE, 100, 2)
    assert np.array_equal(pm, wp[0]) and np.array_equal(plain.kept.cpu().numpy(), wp[1]) and np.array_equal(plain.ptc, wp[2])
    # a field given by hand, another reference frame, a device tensor
    again = stack_burst(torch.from_numpy(fr.view(np.int16)).cuda(), 'bayer', pat, 512, WHITE, align=BurstAlignment(disp, None, 2))
    assert torch.equal(again.mean, stack.mean) and torch.equal(again.present, stack.present)
    al3 = align_burst(fr, 'bayer', ref=3, levels=2)
    assert np.array_equal(al3.disp, A.align(fr, 2, 3, 2)[0]) and not al3.disp[3].any() and al3.ref == 3


def test_command_line_aligned(eld_lib, loop, tmp_path, capsys):
    import json
    from eld_amd.burst import main
    layout, fr, shifts, _, (disp, _) = loop['bayer']
    np.save(tmp_path / 'burst.npy', fr)
    (tmp_path / 'sensor.json').write_text(json.dumps({'raw_pattern': [[0, 1], [3, 2]], 'black_level_per_channel': [512] * 4, 'white_level': WHITE}))
    out = {k: str(tmp_path / k) for k in ('clean.npy', 'field.npy', 'ptc.json')}
    assert main([str(tmp_path / 'burst.npy'), '--meta', str(tmp_path / 'sensor.json'), '-o', out['clean.npy'], '--align', '--disp', out['field.npy'],
                 '--ptc', out['ptc.json']]) == 0
    want = A.stack_aligned(fr, *layout, WHITE, 100, 2, disp)
    assert np.array_equal(np.load(out['clean.npy']), want[0])
    field = np.load(out['field.npy'])
    assert field.dtype == np.int16 and np.array_equal(field, disp)
    text = capsys.readouterr().out
    assert 'aligned to frame 0 over 2 pyramid levels' in text and 'sites with a sample outside the frame' in text and 'tripod' in text
    for i in range(5):
        assert ('frame %d: shift %+.0f %+.0f px' % (i, -2 * shifts[i, 0], -2 * shifts[i, 1])) in text
    rep = json.load(open(out['ptc.json']))
    assert rep['ref'] == 0 and rep['levels'] == 2 and np.array_equal(np.asarray(rep['shift_px']), -2.0 * shifts) and 0 < rep['absent_share'] < 0.5
    with pytest.raises(SystemExit):
        main([str(tmp_path / 'burst.npy'), '-o', out['clean.npy'], '--disp', out['field.npy']])
