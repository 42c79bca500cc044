"""eld_burst_stack_u16 (csrc/burst.hip) against its NumPy restatement (tests/burst_ref.py), bit for bit: mean, kept and the photon-transfer
sums are integers, so no case takes a tolerance.  The shapes are the smallest that reach each path of the kernel: the 16-byte path (width a
multiple of 8, aligned base), the 32-bit path (other even widths), the 2-byte path (a view one element in), every N below, at and above
the rule's switch-on (4) and the depth of the load pipeline (4 frames in flight: N = 2, 3, 4, 5, 16, 37, 256), more than one workgroup.
Then the closed loop through eld_amd.burst.stack_burst and calibrate_camera on sessions that carry bursts."""
import ctypes

import numpy as np
import pytest

import burst_ref as R
from test_burst_cpu import C_REL_BOUND, C_TRUE, K_REL_BOUND

pytestmark = pytest.mark.gpu

NB = R.NB
XT_COLOUR = np.array([[0, 2, 1, 2, 0, 1], [1, 1, 0, 1, 1, 2], [1, 1, 2, 1, 1, 0], [2, 0, 1, 0, 2, 1], [1, 1, 2, 1, 1, 0], [1, 1, 0, 1, 1, 2]])
BAYER = (2, [0, 1, 3, 2], 4, [512, 520, 500, 512])
XTRANS = (6, [int(v) for v in XT_COLOUR.reshape(-1)], 3, [1024] * 36)
WHITE = 16383


def _frames(rng, N, Hm, Wm, black, white=WHITE):
    """Sites of six kinds: constant codes, noise around a level, noise with one outlier sample, codes touching 0, codes around the white
    point, and samples spread over the whole code range."""
    kind = rng.integers(0, 6, size=(Hm, Wm))
    level = rng.integers(black - 4, black + 9000, size=(Hm, Wm))
    level = np.where(kind == 3, rng.integers(0, 4, size=(Hm, Wm)), level)
    level = np.where(kind == 4, rng.integers(white - 6, white + 6, size=(Hm, Wm)), level)
    x = level[None] + rng.integers(-5, 6, size=(N, Hm, Wm)) * (kind != 0)
    hit = rng.integers(0, N, size=(Hm, Wm))
    x = x + (np.arange(N)[:, None, None] == hit[None]) * (kind == 2) * rng.integers(-3000, 3001, size=(Hm, Wm))
    x = np.where(kind == 5, rng.integers(0, 65536, size=(N, Hm, Wm)), x)
    return np.clip(x, 0, 65535).astype(np.uint16)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def _call(lib, fr, layout, white=WHITE, k2q=100, min_dev=2, bitmap=None, want_kept=True, want_ptc=True):
    """fr: CUDA int16 tensor (N,Hm,Wm) -> (rc, mean uint16, kept uint8 or None, ptc int64 or None); the outputs start from a sentinel."""
    import torch
    from eld_amd import _lib as L
    p, group, G, black = layout
    N, Hm, Wm = fr.shape
    mean = torch.full((Hm, Wm), -7, dtype=torch.int16, device=fr.device)
    kept = torch.full((Hm, Wm), 201, dtype=torch.uint8, device=fr.device) if want_kept else None
    ptc = torch.full((G, NB, 4), -7, dtype=torch.int64, device=fr.device) if want_ptc else None
    need = lib.eld_burst_stack_workspace_bytes(N, Hm, Wm)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=fr.device)
    rc = lib.eld_burst_stack_u16(L.dptr(fr), N, Hm, Wm, p, (ctypes.c_int * (p * p))(*group), G, (ctypes.c_int32 * (p * p))(*black), white,
                                 L.dptr(bitmap), k2q, min_dev, L.dptr(mean), L.dptr(kept), L.dptr(ptc), L.dptr(ws), need, L.cur_stream())
    torch.cuda.synchronize()
    return rc, mean.cpu().numpy().view(np.uint16), None if kept is None else kept.cpu().numpy(), None if ptc is None else ptc.cpu().numpy()


def _equal(got, want):
    rc, mean, kept, ptc = got
    assert rc == 0
    assert np.array_equal(mean, want[0])
    if kept is not None:
        assert np.array_equal(kept, want[1])
    if ptc is not None:
        assert np.array_equal(ptc, want[2])


SMALL_N = (2, 3, 4, 5, 16)
CASES = [(BAYER, s, N) for s in ((2, 2), (4, 8), (10, 24), (6, 130)) for N in SMALL_N]
CASES += [(XTRANS, s, N) for s in ((6, 6), (12, 18), (14, 20), (12, 24)) for N in SMALL_N]       # (12, 24): X-Trans on the 16-byte path
CASES += [(BAYER, (10, 24), 37), (BAYER, (6, 130), 256), (XTRANS, (12, 18), 37), (XTRANS, (12, 24), 256)]


@pytest.mark.parametrize('layout,shape,N', CASES, ids=lambda v: str(v) if not isinstance(v, tuple) or len(v) != 4 else 'p%d' % v[0])
def test_bit_equality(eld_lib, layout, shape, N):
    rng = np.random.default_rng(1000 * shape[0] + shape[1] + 7 * N + layout[0])
    fr = _frames(rng, N, shape[0], shape[1], layout[3][0])
    want = R.stack(fr, *layout, WHITE, 100, 2)
    if N >= 4 and shape[0] * shape[1] >= 96:
        assert (want[1] != N % 256).any() and (want[1] == N % 256).any()        # the case really rejects somewhere
        assert want[2][..., 0].sum() > 0
    _equal(_call(eld_lib, _dev(fr), layout), want)


@pytest.mark.parametrize('layout,shape', [(BAYER, (10, 24)), (BAYER, (6, 130)), (XTRANS, (12, 18)), (XTRANS, (12, 24))], ids=['b8', 'b2', 'x2', 'x8'])
def test_variants(eld_lib, layout, shape):
    import torch
    from eld_amd.defects import pack_bitmap
    rng = np.random.default_rng(shape[1])
    N = 9
    fr = _frames(rng, N, shape[0], shape[1], layout[3][0])
    d = _dev(fr)
    mask = rng.uniform(size=shape) < 0.15
    mask[0, 0] = mask[-1, -1] = True
    bm = torch.from_numpy(pack_bitmap(mask).view(np.int32).copy()).cuda()
    plain = R.stack(fr, *layout, WHITE, 100, 2)
    flagged = R.stack(fr, *layout, WHITE, 100, 2, mask=mask)
    assert np.array_equal(plain[0], flagged[0]) and not np.array_equal(plain[2], flagged[2])     # flagged sites keep their mean, leave ptc
    _equal(_call(eld_lib, d, layout, bitmap=bm), flagged)
    _equal(_call(eld_lib, d, layout, bitmap=torch.zeros_like(bm)), plain)
    _equal(_call(eld_lib, d, layout, want_kept=False), plain)
    _equal(_call(eld_lib, d, layout, want_ptc=False), plain)
    _equal(_call(eld_lib, d, layout, want_kept=False, want_ptc=False, bitmap=bm), flagged)
    off = R.stack(fr, *layout, WHITE, 0, 2)                        # k2q = 0: nothing is rejected
    assert np.all(off[1] == N)
    _equal(_call(eld_lib, d, layout, k2q=0), off)
    for k2q, min_dev in ((1, 0), (5, 0), (6, 1), (256, 0), (100, 65535)):       # the ends of both ranges; k2q <= 5 may reject every sample
        _equal(_call(eld_lib, d, layout, k2q=k2q, min_dev=min_dev), R.stack(fr, *layout, WHITE, k2q, min_dev))
    _equal(_call(eld_lib, d, layout, white=65536), R.stack(fr, *layout, 65536, 100, 2))
    _equal(_call(eld_lib, d, layout), plain)                       # a repeated call: ptc is zeroed by the call itself


@pytest.mark.parametrize('layout,shape', [(BAYER, (10, 24)), (XTRANS, (12, 24))], ids=['bayer', 'xtrans'])
def test_unaligned_base_takes_the_fallback_paths(eld_lib, layout, shape):
    import torch
    rng = np.random.default_rng(11)
    fr = _frames(rng, 7, shape[0], shape[1], layout[3][0])
    want = R.stack(fr, *layout, WHITE, 100, 2)
    buf = torch.zeros(fr.size + 8, dtype=torch.int16, device='cuda')
    for off in (1, 2, 4):                                          # 2 bytes off: 2-byte loads; 4 and 8 bytes off: 32-bit words
        view = buf[off:off + fr.size].view(fr.shape)
        view.copy_(_dev(fr))
        assert view.data_ptr() % 16 == 2 * off
        _equal(_call(eld_lib, view, layout), want)


def test_several_workgroups(eld_lib):
    """A workgroup covers TILE_UNITS = 2048 units of 8, 2 or 1 sites (csrc/burst.hip BS_UNITS; eld_amd.burst mirrors the constant): the
    frames below span two whole workgroups and a partial one on each path.  ptc is where the partial sums of different workgroups meet."""
    import torch
    from eld_amd.burst import TILE_UNITS
    rng = np.random.default_rng(21)
    for layout, Wm, cw in ((BAYER, 128, 8), (XTRANS, 120, 8), (BAYER, 52, 2)):
        Hm = -(-2 * TILE_UNITS * cw // Wm) + 2
        Hm += Hm % 2
        assert 2 * TILE_UNITS * cw < Hm * Wm < 3 * TILE_UNITS * cw
        fr = _frames(rng, 4, Hm, Wm, layout[3][0])
        want = R.stack(fr, *layout, WHITE, 100, 2)
        assert want[2][..., 0].sum() > TILE_UNITS * cw // 4
        _equal(_call(eld_lib, _dev(fr), layout), want)
    # the 2-byte path, and every site in one bin per group (a dark burst: the contention case)
    Hm, Wm = 2 * TILE_UNITS // 64 + 2, 64
    fr = (512 + rng.integers(0, 2, size=(4, Hm, Wm)) + 2 * (np.arange(Wm) % 2)).astype(np.uint16)
    want = R.stack(fr, *BAYER, WHITE, 100, 2)
    assert (want[2][..., 0] > 0).sum() <= 8 and want[2][..., 0].sum() == Hm * Wm
    buf = torch.zeros(fr.size + 8, dtype=torch.int16, device='cuda')
    view = buf[1:1 + fr.size].view(fr.shape)
    view.copy_(_dev(fr))
    _equal(_call(eld_lib, view, BAYER), want)


def test_widths(eld_lib):
    layout = (2, [0, 0, 0, 0], 1, [0] * 4)
    alt = np.broadcast_to(np.array([0, 65535] * 128, np.uint16)[:, None, None], (256, 4, 8)).copy()
    alt[:, 1] = alt[::-1, 1]                                       # one row starts with 65535
    full = np.full((256, 4, 8), 65535, np.uint16)
    edge = np.full((256, 4, 8), 65535, np.uint16)
    edge[0] = 0                                                    # the largest |d|: one sample at the other end of the range
    for fr in (alt, full, edge):
        for white, k2q, min_dev in ((65536, 100, 2), (WHITE, 256, 0), (65536, 256, 0), (65536, 1, 65535)):
            want = R.stack(fr, *layout, white, k2q, min_dev)
            _equal(_call(eld_lib, _dev(fr), layout, white=white, k2q=k2q, min_dev=min_dev), want)
    want = R.stack(full, *layout, 65536, 100, 2)
    assert want[0][0, 0] == 65535 and want[1][0, 0] == 0 and want[2][0, 59, 0] == 32 and want[2][0, 59, 1] == 32 * 256 * 65535
    assert R.stack(alt, *layout, 65536, 100, 2)[0][0, 0] == 32768


def _planted(seed=0, count=50):
    fr = R.scene_burst(seed).astype(np.int64)
    rng = np.random.default_rng(1000 + seed)
    sites = rng.choice(fr.shape[1] * fr.shape[2], size=count, replace=False)
    ys, xs = sites // fr.shape[2], sites % fr.shape[2]
    fs = rng.integers(0, fr.shape[0], size=count)
    fr[fs, ys, xs] += 4000                                         # over 30 sigma at the brightest site (sqrt(2 * 6000 + 9) = 110 DN), below white
    assert fr.max() < WHITE
    return fr.astype(np.uint16), ys, xs


def test_closed_loop_through_stack_burst(eld_lib):
    import torch
    from eld_amd.burst import burst_gain, ptc_points, stack_burst
    from eld_amd.framepool import FramePool
    fr, ys, xs = _planted()
    pat = [[0, 1], [3, 2]]
    stack = stack_burst(fr, 'bayer', pat, 512, WHITE, k=5.0, min_dev=2)
    want = R.stack(fr, 2, [0, 1, 3, 2], 4, [512] * 4, WHITE, 100, 2)
    mean, kept = stack.mean.cpu().numpy(), stack.kept.cpu().numpy()
    assert stack.mean.dtype == torch.uint16 and stack.mean.is_cuda and stack.N == 16 and stack.G == 4 and stack.k2q == 100
    assert np.all(kept[ys, xs] < 16) and np.all(kept[ys, xs] >= 14)                # every planted sample is rejected
    assert np.array_equal(mean[ys, xs], want[0][ys, xs])
    assert np.array_equal(mean, want[0]) and np.array_equal(kept, want[1]) and np.array_equal(stack.ptc, want[2])
    clean = R.scene_burst(0)
    assert np.max(np.abs(mean[ys, xs].astype(np.int64) - np.rint(clean.mean(axis=0))[ys, xs])) <= 60     # the hit left the mean: not + 4000 / 16 = 250
    fit = burst_gain([stack])
    print('K %.5f (relative error %.5f), sigma0^2 %.3f' % (fit['K'], abs(fit['K'] / 2.0 - 1.0), fit['sigma0_sq']))
    assert abs(fit['K'] / 2.0 - 1.0) <= K_REL_BOUND
    assert abs(fit['sigma0_sq'] - C_TRUE) / C_TRUE <= C_REL_BOUND
    assert abs(stack.rejected_share() - float(np.mean(want[1] != 16))) < 1e-12
    n, mu, var = R.points(want[2], 16, [512] * 4)
    q = ptc_points(stack)
    assert np.array_equal(q['mu'], mu, equal_nan=True) and np.array_equal(q['var'], var, equal_nan=True)
    # a device tensor on the int16 view gives the same stack
    again = stack_burst(torch.from_numpy(fr.view(np.int16)).cuda(), 'bayer', pat, 512, WHITE)
    assert torch.equal(again.mean, stack.mean) and np.array_equal(again.ptc, stack.ptc)
    # the stacked frame is a clean frame of the frame pool
    pool_t = FramePool([stack.mean], raw_pattern=pat, black_level=512, white_point=WHITE)
    pool_n = FramePool([mean], raw_pattern=pat, black_level=512, white_point=WHITE)
    grid = pool_t.grid((4, 16, 16), (4, 16, 16))
    assert len(grid) == 6 and torch.equal(pool_t.patches(grid), pool_n.patches(grid))


def test_flicker_warning_through_the_tool(eld_lib):
    from eld_amd.burst import run
    fr = R.scene_burst(3)
    o = {'cfa': 'bayer', 'raw_pattern': [[0, 1], [3, 2]], 'black_level': 512, 'white_point': WHITE}
    _, res = run(fr, o)
    assert res['warning'] is None and res['flicker']['ratio'] < 3.0 and res['N'] == 16 and abs(res['K'] / 2.0 - 1.0) <= K_REL_BOUND
    lit = fr.astype(np.float64) - 512.0
    lit *= (1.0 + 0.02 * np.cos(np.arange(16)))[:, None, None]     # 2 % flicker of the light
    _, res = run(np.clip(np.rint(lit + 512.0), 0, WHITE).astype(np.uint16), o)
    assert res['warning'] is not None and res['flicker']['ratio'] > 3.0 and 'not constant' in res['warning']


def _bias(rng, F, Hm, Wm):
    """Dark frames with Gaussian read noise (2 DN) and row noise (1 DN), black 512."""
    x = 512.0 + rng.normal(0.0, 2.0, size=(F, Hm, Wm)) + rng.normal(0.0, 1.0, size=(F, Hm, 1))
    return np.clip(np.rint(x), 0, 65535).astype(np.uint16)


def test_calibrate_camera_from_bursts(eld_lib):
    from eld_amd import calibrate as CAL
    rng = np.random.default_rng(5)
    pat, black = [[0, 1], [3, 2]], [512.0] * 4
    sessions, Kref = [], []
    for i, K in enumerate((1.0, 4.0)):
        bursts = [R.scene_burst(40 + 2 * i + j, K=K) for j in range(2)]
        sessions.append({'iso': 100 * (i + 1), 'bias': _bias(rng, 2, 64, 96), 'bursts': bursts})
        Kref.append(R.gain([R.points(R.stack(b, 2, [0, 1, 3, 2], 4, [512] * 4, WHITE, 100, 2)[2], 16, [512] * 4) for b in bursts])[0])
    params, diag = CAL.calibrate_camera(sessions, pat, black, WHITE)
    assert set(params) == {'Kmin', 'Kmax', 'G_shape', 'color_bias', CAL.PROFILE} and set(params[CAL.PROFILE]) == set(CAL.SIGMA_KEYS)
    assert all(set(params[CAL.PROFILE][k]) == {'slope', 'bias', 'sigma'} for k in CAL.SIGMA_KEYS)
    assert params['G_shape'].shape == (4,) and params['color_bias'].shape == (4, 4) and params['color_bias'].dtype == np.float32
    assert params['Kmin'] < params['Kmax']
    np.testing.assert_allclose(diag['K'], Kref, rtol=1e-9)         # the session gains are the restatement's fit of the restatement's sums
    assert abs(diag['K'][0] / 1.0 - 1.0) < 0.1 and abs(diag['K'][1] / 4.0 - 1.0) < 0.1
    assert all(pt['source'] == 'bursts' and pt['mu'].size >= 2 and pt['usable'].all() for pt in diag['ptc'])


def test_command_line(eld_lib, tmp_path, capsys):
    import json
    from eld_amd.burst import main
    fr = R.scene_burst(2, N=6)
    for i, f in enumerate(fr[:4]):
        np.save(tmp_path / ('f%d.npy' % i), f)
    np.save(tmp_path / 'g.npy', fr[4:])                            # a (2, Hm, Wm) file counts as two frames; 'g' sorts after the 'f' files
    (tmp_path / 'sensor.json').write_text(json.dumps({'raw_pattern': [[0, 1], [3, 2]], 'black_level_per_channel': [512] * 4, 'white_level': WHITE}))
    out = {k: str(tmp_path / k) for k in ('clean.npy', 'kept.npy', 'ptc.json')}
    assert main([str(tmp_path / '[fg]*.npy'), '--meta', str(tmp_path / 'sensor.json'), '-o', out['clean.npy'], '--kept', out['kept.npy'],
                 '--ptc', out['ptc.json'], '--k', '4', '--min-dev', '3']) == 0
    want = R.stack(fr, 2, [0, 1, 3, 2], 4, [512] * 4, WHITE, 64, 3)
    assert np.array_equal(np.load(out['clean.npy']), want[0]) and np.load(out['clean.npy']).dtype == np.uint16
    assert np.array_equal(np.load(out['kept.npy']), want[1])
    rep = json.load(open(out['ptc.json']))
    assert np.array_equal(np.asarray(rep['ptc']), want[2]) and rep['N'] == 6 and rep['k2q'] == 64 and rep['warning'] is None
    text = capsys.readouterr().out
    assert 'stacked 6 frames' in text and 'sites with a rejected sample' in text and ('K %.5g' % rep['K']) in text
