"""eld_tile_noise_sums_u16 (csrc/noiselevel.hip) against its NumPy restatement (tests/noiselevel_ref.py), bit for bit: the outputs are
exact integer sums, so no case takes a tolerance.  The shapes are the smallest at which each part of the kernel can go wrong: one site per
cell position, an empty grid, odd sizes with partial tiles both ways (the frame starts then leave the 16-byte grid and the stack ends in a
partial chunk), two tile rows, exactly one full tile, a crop, the X-Trans green layout at stride 3 and all colours at stride 6, a pointer
offset by one code (the 2-byte path), every G with uncounted cells, a defect bitmap on tile and frame borders, and the largest codes.
Then the host module on top: NumPy and CUDA input, the estimator on device sums, and python -m eld_amd.classical --K auto."""
import ctypes
import json
import re

import numpy as np
import pytest

import noiselevel_ref as R
import noiselevel_scene as SC

pytestmark = pytest.mark.gpu

RGGB = [0, 1, 3, 2]
XT_ALL = [int(v) for v in SC.XT_COLOUR.reshape(-1)]
XT_GREEN = [int(v) for v in SC.XT_GREEN]


def _dev(a, offset=0):
    """uint16 ndarray -> CUDA int16 tensor of the same bits; offset: codes by which the view starts off a fresh allocation"""
    import torch
    a = np.ascontiguousarray(a)
    buf = torch.zeros(a.size + offset, dtype=torch.int16, device='cuda')
    buf[offset:] = torch.from_numpy(a.view(np.int16).reshape(-1)).cuda()
    return buf[offset:].view(a.shape)


def _words(mask):
    Hm, Wm = mask.shape
    w = np.zeros((Hm, (Wm + 31) // 32), np.uint32)
    for y, x in zip(*np.nonzero(mask)):
        w[y, x >> 5] |= np.uint32(1) << np.uint32(x & 31)
    return w


def _call(lib, frames, Hc, Wc, p, s, group, G, black, white, mask=None, offset=0):
    """frames uint16 (F,Hm,Wm) on the host -> (rc, int64 ndarray) from the kernel; every element of out must be written"""
    import torch
    from eld_amd import _lib as L
    F, Hm, Wm = frames.shape
    d = _dev(frames, offset)
    nty, ntx = R.tiles_along(Hc, s), R.tiles_along(Wc, s)
    out = torch.full((F, nty, ntx, G, 4), -7, dtype=torch.int64, device='cuda')
    bm = None if mask is None else torch.from_numpy(_words(mask).view(np.int32)).cuda()
    need = lib.eld_tile_noise_workspace_bytes(F, Hm, Wm)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device='cuda')
    rc = lib.eld_tile_noise_sums_u16(L.dptr(d), F, Hm, Wm, Hc, Wc, p, s, (ctypes.c_int * (p * p))(*[int(v) for v in group]), G,
                                     (ctypes.c_int32 * (p * p))(*[int(v) for v in black]), white, L.dptr(bm), L.dptr(out), L.dptr(ws), need,
                                     L.cur_stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def _frames(rng, F, Hm, Wm, white, bad=0.02):
    """Codes over the whole range below white, with zeros and codes >= white sprinkled in."""
    fr = rng.integers(1, white, size=(F, Hm, Wm))
    pick = rng.random((F, Hm, Wm))
    fr = np.where(pick < bad / 2, 0, np.where(pick < bad, rng.integers(white, 65536, size=fr.shape) if white < 65536 else 0, fr))
    return fr.astype(np.uint16)


def _check(lib, fr, Hc, Wc, p, s, group, G, black, white, mask=None, offset=0):
    rc, out = _call(lib, fr, Hc, Wc, p, s, group, G, black, white, mask, offset)
    assert rc == 0
    want = R.tile_sums_ref(fr, Hc, Wc, p, s, group, G, black, white, mask)
    assert out.shape == want.shape
    assert np.array_equal(out, want)
    return want


@pytest.mark.parametrize('Hm,Wm,Hc,Wc', [(6, 6, 6, 6), (4, 40, 4, 40), (37, 45, 37, 45), (70, 100, 70, 100), (36, 36, 36, 36), (68, 68, 66, 50)])
def test_bayer(eld_lib, Hm, Wm, Hc, Wc):
    rng = np.random.default_rng(Hm * 1000 + Wm)
    fr = _frames(rng, 3, Hm, Wm, 16383)
    black = [512, 520, 500, 505]
    want = _check(eld_lib, fr, Hc, Wc, 2, 2, RGGB, 4, black, 16383)
    if (Hm, Wm) == (4, 40):
        assert want.size == 0
    else:
        assert want[..., 0].sum() > 0
    _check(eld_lib, fr, Hc, Wc, 2, 2, RGGB, 4, black, 16383, offset=1)              # the view starts one code into its allocation: 2-byte loads
    if (Hm, Wm) == (36, 36):
        clean = rng.integers(1, 16383, size=(1, Hm, Wm)).astype(np.uint16)
        assert _check(eld_lib, clean, Hc, Wc, 2, 2, RGGB, 4, black, 16383)[0, 0, 0, :, 0].tolist() == [256] * 4     # one full tile


@pytest.mark.parametrize('Hm,Wm,s,group', [(114, 125, 3, XT_GREEN), (54, 54, 3, XT_GREEN), (114, 125, 6, XT_ALL), (54, 61, 2, [0] * 36), (40, 47, 1, [0] * 36)])
def test_xtrans_layouts(eld_lib, Hm, Wm, s, group):
    # s = 2 and s = 1 under p = 6 are legal too (one group everywhere): their tiles are no multiple of the period
    rng = np.random.default_rng(Hm + Wm + s)
    fr = _frames(rng, 2, Hm, Wm, 16383)
    Hc, Wc = Hm // 6 * 6, Wm // 6 * 6
    G = 3 if s >= 3 else 1
    want = _check(eld_lib, fr, Hc, Wc, 6, s, group, G, [1024] * 36, 16383)
    assert want[..., 0].sum() > 0
    if group is XT_GREEN:
        assert not want[..., 0, :].any() and not want[..., 2, :].any()
        clean = rng.integers(1, 16383, size=(1, Hm, Wm)).astype(np.uint16)
        full = _check(eld_lib, clean, Hc, Wc, 6, s, group, G, [1024] * 36, 16383)
        assert full[0, 0, 0, 1, 0] == 48 * 48 * 20 // 36                              # 1280 green sites in a full stride-3 tile
    _check(eld_lib, fr, Hc, Wc, 6, s, group, G, [1024] * 36, 16383, offset=1)


@pytest.mark.parametrize('p,s,G,group', [(2, 1, 1, [0, 0, 0, 0]), (2, 2, 1, [0, -1, -1, 0]), (2, 2, 2, [0, 1, -1, 1]), (2, 2, 3, [2, -1, 1, 0]),
                                         (2, 2, 4, [3, 2, 1, 0]), (6, 6, 2, [{0: 0, 1: -1, 2: 1}[c] for c in XT_ALL]), (6, 3, 1, [0 if c == 1 else -1 for c in XT_ALL])])
def test_groups(eld_lib, p, s, G, group):
    rng = np.random.default_rng(p * 100 + s * 10 + G)
    Hm, Wm = (70, 100) if p == 2 else (120, 114)
    fr = _frames(rng, 1, Hm, Wm, 4000)
    black = rng.integers(0, 600, size=p * p)
    want = _check(eld_lib, fr, Hm, Wm, p, s, group, G, black, 4000)
    assert want[..., 0].sum() > 0
    if (p, s) == (2, 1):                                                              # the only Bayer case at stride 1: also on the 2-byte path
        _check(eld_lib, fr, Hm, Wm, p, s, group, G, black, 4000, offset=1)


@pytest.mark.parametrize('p,s,group,G,Hm,Wm', [(2, 2, RGGB, 4, 70, 100), (6, 3, XT_GREEN, 3, 114, 126)])
def test_bitmap(eld_lib, p, s, group, G, Hm, Wm):
    rng = np.random.default_rng(7 + p)
    fr = _frames(rng, 2, Hm, Wm, 16383, bad=0.0)
    side = 16 * s
    mask = np.zeros((Hm, Wm), bool)
    for y, x in ((s, s + 5), (s + side - 1, s + 7), (s + 9, s), (s + 11, s + side - 1), (s + side, s + side), (s + side + 3, s + side - 1),   # a tile's first and last row and column
                 (0, 0), (0, Wm - 1), (Hm - 1, 0), (Hm - 1, Wm - 1), (0, 33), (Hm - 1, 64), (31, 0), (32, Wm - 1), (20, 31), (20, 32), (21, 63), (21, 64)):
        mask[y, x] = True
    with_map = _check(eld_lib, fr, Hm, Wm, p, s, group, G, [512] * (p * p), 16383, mask)
    without = _check(eld_lib, fr, Hm, Wm, p, s, group, G, [512] * (p * p), 16383)
    assert with_map[..., 0].sum() < without[..., 0].sum()
    _check(eld_lib, fr, Hm, Wm, p, s, group, G, [512] * (p * p), 16383, mask, offset=1)


@pytest.mark.parametrize('p,s,group,G', [(2, 2, RGGB, 4), (6, 3, XT_GREEN, 3), (6, 6, XT_ALL, 3)])
def test_largest_codes(eld_lib, p, s, group, G):
    """1 and 65535 alternating at the stride with white = 65536: |r| = 8 * 65534, the largest there is, at every site."""
    Hm, Wm = 18 * s + p, 34 * s                                                       # one full tile row and a partial one, two full tile columns
    y, x = np.mgrid[:Hm, :Wm]
    fr = np.where((y // s + x // s) % 2 == 0, 65535, 1).astype(np.uint16)[None]
    want = _check(eld_lib, fr, Hm, Wm, p, s, group, G, [0] * (p * p), 65536)
    n = want[..., 0]
    assert n.sum() > 0 and np.array_equal(want[..., 2], n * (8 * 65534) ** 2) and not want[..., 3].any()
    assert int(want[..., 1].max()) >= 4 * 65535 * int(n.max())


# ---- the host module ----------------------------------------------------------------------------------------------------------------------
def test_tile_sums_numpy_and_cuda_input(eld_lib):
    import torch
    from eld_amd.noiselevel import tile_sums
    rng = np.random.default_rng(11)
    fr = _frames(rng, 2, 70, 100, 16383)
    a = tile_sums(fr, 'bayer', [[0, 1], [3, 2]], [512, 520, 500, 505], 16383)
    b = tile_sums(torch.from_numpy(fr.view(np.int16)).cuda(), 'bayer', [[0, 1], [3, 2]], [512, 520, 500, 505], 16383)
    assert np.array_equal(a.sums, b.sums) and (a.period, a.stride, a.group, a.G, a.shape) == (2, 2, RGGB, 4, (70, 100))
    # black_level is per colour code (R, G1, B, G2); the cells of RGGB hold the codes 0, 1, 3, 2
    assert np.array_equal(a.sums, R.tile_sums_ref(fr, 70, 100, 2, 2, RGGB, 4, [512, 520, 505, 500], 16383))
    one = tile_sums(fr[0], 'bayer', [[0, 1], [3, 2]], [512, 520, 500, 505], 16383)    # a single frame: F = 1
    assert np.array_equal(one.sums, a.sums[:1])
    xt = _frames(rng, 1, 114, 125, 16383)
    c = tile_sums(xt, 'xtrans', SC.XT_COLOUR, 1024, 16383)                      # the defaults: greens at stride 3 over the whole cells
    assert (c.period, c.stride, c.G) == (6, 3, 3)
    assert np.array_equal(c.sums, R.tile_sums_ref(xt, 114, 120, 6, 3, XT_GREEN, 3, [1024] * 36, 16383))


def test_estimate_from_device_sums_equals_the_restatement(eld_lib):
    from eld_amd.noiselevel import TileSums, estimate_noise
    K, sigma, tex = SC.CASES[0]
    u = SC.synth_frame(K, sigma, tex, 0)
    dev = estimate_noise(u, 'bayer', [[0, 1], [3, 2]], SC.BLACK, SC.WHITE)
    ref = estimate_noise(TileSums(R.tile_sums_ref(u, 768, 1024, 2, 2, RGGB, 4, [SC.BLACK] * 4, SC.WHITE), 2, 2, RGGB, 4))
    assert dev.K == ref.K and dev.sigma0_sq == ref.sigma0_sq and dev.kept_share == ref.kept_share
    assert np.array_equal(dev.points['n'], ref.points['n']) and np.array_equal(dev.points['var'], ref.points['var'])
    assert {g: d['K'] for g, d in dev.groups.items()} == {g: d['K'] for g, d in ref.groups.items()}


def test_command_line(eld_lib, tmp_path, capsys):
    """python -m eld_amd.noiselevel: the table, and --json with --camera on a table shipped with the package."""
    from eld_amd import noiselevel
    K, sigma, tex = SC.CASES[0]
    np.save(tmp_path / 'frame.npy', SC.synth_frame(K, sigma, tex, 0))
    with open(tmp_path / 'sensor.json', 'w') as fh:
        json.dump({'cfa': 'bayer', 'raw_pattern': [[0, 1], [3, 2]], 'black_level': SC.BLACK, 'white_point': SC.WHITE}, fh)
    args = [str(tmp_path / 'frame.npy'), '--meta', str(tmp_path / 'sensor.json')]
    assert noiselevel.main(args + ['--camera', 'SonyA7S2']) == 0
    text = capsys.readouterr().out
    m = re.search(r'^K ([0-9.eE+-]+) DN/e-  sigma ([0-9.eE+-]+) DN', text, re.M)
    assert m and 'tiles kept' in text and 'table SonyA7S2: K in [' in text and 'inside' in text, text
    assert len(re.findall(r'^\s*\d+\s+\d+\s+[0-9.]+\s+[0-9.]+$', text, re.M)) >= 30           # the table of points
    assert noiselevel.main(args + ['--camera', 'SonyA7S2', '--json']) == 0
    res = json.loads(capsys.readouterr().out)
    assert '%.5g' % res['K'] == m.group(1) and '%.4g' % res['sigma'] == m.group(2)
    assert abs(res['K'] / K - 1.0) < 0.05 and res['camera']['K_inside'] is True and res['camera']['sigma_table'] > 0
    assert sorted(res['groups']) == ['0', '1', '2', '3'] and len(res['points']['bin']) >= 30


def test_classical_with_auto_gain(eld_lib, tmp_path, capsys):
    """python -m eld_amd.classical --K auto on a 256 x 384 frame of the scene (K 2, sigma 3, no texture, seed 0; the restatement gives
    K +1.95 % on it): runs, prints a K inside the CPU test's bound, writes its output."""
    from eld_amd import classical
    from test_noiselevel_cpu import BOUNDS
    u = SC.synth_frame(2.0, 3.0, 0.0, 0, 256, 384)
    np.save(tmp_path / 'small.npy', u)
    with open(tmp_path / 'sensor.json', 'w') as fh:
        json.dump({'cfa': 'bayer', 'raw_pattern': [[0, 1], [3, 2]], 'black_level': SC.BLACK, 'white_point': SC.WHITE}, fh)
    assert classical.main([str(tmp_path / 'small.npy'), '-o', str(tmp_path / 'out'), '--meta', str(tmp_path / 'sensor.json'), '--K', 'auto']) == 0
    text = capsys.readouterr().out
    m = re.search(r'using K ([0-9.eE+-]+) DN/e-, sigma ([0-9.eE+-]+) DN', text)
    assert m, text
    assert abs(float(m.group(1)) / 2.0 - 1.0) <= BOUNDS[2][0]
    den = np.load(tmp_path / 'out' / 'small_denoised.npy')
    assert den.shape == u.shape and den.dtype == np.uint16
    twin = classical.ClassicalDenoiser.from_frames(u, 'bayer', [[0, 1], [3, 2]], SC.BLACK, SC.WHITE)
    assert '%.5g' % twin.K == m.group(1) and twin.estimate.K == twin.K
