"""CPU tests of BM3D on stabilised codes: the two NumPy forms of the kernel's contract agree, every group size occurs in
the inputs the GPU tests rely on, the filter has the properties the contract implies, the tables are what the header says, the C entry
refuses bad arguments before any device work, and the reference pipeline alone beats non-local means on a Bayer frame."""
import ctypes

import numpy as np
import pytest

import bm3d_ref as R
import nlm_ref as NR

# (N, C, h, w), S, step, Gmax, mix, frac: every shape, S in {0, 2, 5}, step in {1, 3, 8}, Gmax in {1, 4, 16}, frac in {0, 4}, mix 0 and 1
FORMS = [((1, 1, 8, 8), 0, 1, 1, 0, 0), ((1, 1, 8, 8), 2, 3, 4, 1, 4),
         ((1, 1, 8, 9), 2, 3, 4, 1, 4), ((1, 1, 8, 9), 5, 8, 16, 0, 0),
         ((2, 2, 9, 8), 2, 1, 4, 1, 0), ((1, 2, 9, 8), 0, 8, 1, 0, 4),
         ((1, 3, 11, 13), 5, 3, 16, 0, 4), ((1, 3, 11, 13), 2, 8, 4, 0, 0),
         ((1, 4, 15, 17), 2, 8, 16, 1, 4), ((1, 4, 15, 17), 5, 3, 4, 0, 0), ((1, 4, 15, 17), 2, 3, 1, 1, 4)]


@pytest.mark.parametrize('shape,S,step,Gmax,mix,frac', FORMS)
def test_direct_and_vectorised_forms_agree(shape, S, step, Gmax, mix, frac):
    N, C, h, w = shape
    x = R.flat_noise_x(N, C, h, w, 7 * h + w + S)
    fwd = R.identity_tables(C)
    tau1, thr, tau2, s2, win = R.bm3d_tables(C, mix)
    sa, sb = {}, {}
    a = R.bm3d_direct(x, 65535.0, fwd, None, S, step, Gmax, mix, tau1 // 2, thr, win, frac, sa)            # 2 Q^2 n: the expected distance
    b = R.bm3d_fast(x, 65535.0, fwd, None, S, step, Gmax, mix, tau1 // 2, thr, win, frac, sb)
    assert a.dtype == b.dtype == np.int32 and a.shape == shape and np.array_equal(a, b)
    assert sa == sb and sum(sa.values()) == N * len(R.grid(h, step)) * len(R.grid(w, step))
    sa, sb = {}, {}
    a2 = R.bm3d_direct(x, 65535.0, fwd, a, S, step, Gmax, mix, tau2, s2, win, frac, sa)
    b2 = R.bm3d_fast(x, 65535.0, fwd, a, S, step, Gmax, mix, tau2, s2, win, frac, sb)
    assert np.array_equal(a2, b2) and sa == sb
    assert not np.array_equal(a, a2)


def test_wiener_ratio_without_the_wide_product():
    """the restatement's vectorised form and the kernel form floor(4096 E / (E + p)) as 4096 - ceil(4096 p / (E + p)): E << 12 needs 70 bits"""
    rng = np.random.default_rng(3)
    E = np.concatenate([np.array([0, 1, 2, 4095, 4096, (1 << 29) ** 2 - 1, (32767 * 16384) ** 2]), rng.integers(0, 1 << 40, 200)]).astype(np.int64)
    for p in (1, 2, 4096, 16384, 4194304, (1 << 32) - 1):
        got = R._wiener_ratio(E, p)
        want = [((int(e) << 12) // (int(e) + p)) for e in E]
        assert got.tolist() == want
        assert got.min() >= 0 and got.max() <= 4095


@pytest.mark.parametrize('name', sorted(R.GROUP_SIZE_CASES))
def test_every_group_size_occurs(name):
    x, fwd, S, step, Gmax, mix, tables = R.group_size_case(name)
    stats = {}
    R.bm3d_two_steps(x, 65535.0, fwd, S, step, Gmax, mix, tables, 4, stats)
    print(name, stats)
    assert set(stats[1]) == set(stats[2]) == {0, 1, 2, 3, 4}


def test_one_block_alone_returns_its_mean():
    """Gmax = 1, S = 0 on an 8 x 8 plane with a threshold above every AC coefficient: only the DC term survives, nnz = 1, and every site
    gets (sum + 32) >> 6 in units of 2^-frac"""
    rng = np.random.default_rng(11)
    codes = rng.integers(700, 900, size=(1, 2, 8, 8))
    x = (codes.astype(np.float32) / np.float32(65535.0)).astype(np.float32)
    thr = np.full(5, 200 * 64, np.uint32)                                       # |AC| <= 200 * 64 / 2 ... < the DC term 700 * 64
    for frac in (0, 4):
        out = R.bm3d_fast(x, 65535.0, R.identity_tables(2), None, 0, 1, 1, 0, 0, thr, R.WIN.reshape(-1), frac)
        for c in range(2):
            s = int(codes[0, c].sum())
            assert s > 200 * 64
            assert np.all(out[0, c] == (s + (1 << (5 - frac))) >> (6 - frac))


def test_tau_0_groups_only_exact_duplicates():
    rng = np.random.default_rng(12)
    tile = rng.integers(500, 1500, size=(1, 1, 8, 8))
    codes = np.tile(tile, (1, 1, 2, 3))                                          # 16 x 24: a block and its five exact copies
    codes[0, 0, 0, 23] += 1                                                      # the top-right copy is spoilt
    x = (codes.astype(np.float32) / np.float32(65535.0)).astype(np.float32)
    _, thr, _, _, win = R.bm3d_tables(1, 0)
    stats = {}
    R.bm3d_fast(x, 65535.0, R.identity_tables(1), None, 16, 8, 16, 0, 0, thr, win, 0, stats)
    # the grid is the 6 tiles; 5 of them see 4 more exact copies (5 candidates -> 4 blocks), the spoilt one only itself
    assert stats == {2: 5, 0: 1}
    stats = {}
    R.bm3d_fast(x, 65535.0, R.identity_tables(1), None, 7, 8, 16, 0, 0, thr, win, 0, stats)              # |d| <= 7 reaches no copy
    assert stats == {0: 6}


def test_wiener_limits():
    """The largest noise energy shrinks a faint frame to nearly 0; par = 1 with the input as its own guide returns the input to the rounding
    of the contract."""
    fwd = R.identity_tables(1)
    win = R.WIN.reshape(-1)
    rng = np.random.default_rng(22)
    faint = (rng.integers(0, 41, size=(1, 1, 12, 13)).astype(np.float32) / np.float32(65535.0)).astype(np.float32)
    x = R.flat_noise_x(1, 1, 12, 13, 21)
    v = NR.stabilised(x, 65535.0, fwd)
    for frac in (0, 4):
        guide = (NR.stabilised(faint, 65535.0, fwd) << frac).astype(np.int32)
        big = R.bm3d_fast(faint, 65535.0, fwd, guide, 2, 3, 4, 0, 1 << 20, np.full(5, (1 << 32) - 1, np.uint32), win, frac)
        # codes <= 40, L = 256: the DC term is at most 10240, E <= 1.05e8 against p = 4.3e9: R <= 97 of 4096, T' <= 243, I / L < 1 code; the AC
        # terms (|T| <= 40 * 128) have R <= 24 and T' <= 30 each, but their signs differ: together well below another code
        assert big.min() >= 0 and big.max() <= 2 << frac
        guide = (v << frac).astype(np.int32)
        one = R.bm3d_fast(x, 65535.0, fwd, guide, 2, 3, 4, 0, 1 << 20, np.ones(5, np.uint32), win, frac)
        # R >= 2048 where T is not 0 and 4095 once E >= 4095: a coefficient loses at most |T| / 4096 + 1, the estimate at most
        # sum (|T| / 4096 + 1) / L <= sqrt(L) max v / 4096 + 1 = 16 * 900 / 4096 + 1 < 5 codes, and the rounding of est one unit more
        err = np.abs(one.astype(np.int64) - (v << frac))
        assert err.max() <= (5 << frac) + 1 and err.mean() <= (1 << frac)
    zero = R.bm3d_fast(x, 65535.0, fwd, np.zeros_like(guide), 2, 3, 4, 0, 1 << 20, np.full(5, (1 << 32) - 1, np.uint32), win, 4)
    assert np.all(zero == 0)                                                     # a guide of 0: E = 0, R = 0


def test_tables():
    from eld_amd import classical as Cl
    for C, mix, strength in ((4, 1, 1.0), (4, 0, 1.0), (9, 0, 1.0), (1, 1, 0.5), (16, 1, 2.0), (2, 1, 1.3)):
        ref = R.bm3d_tables(C, mix, strength)
        got = Cl.bm3d_tables(C, mix, strength)
        assert got[0] == ref[0] and got[2] == ref[2] and isinstance(got[0], int) and isinstance(got[2], int)
        for a, b, dt, n in ((got[1], ref[1], np.uint32, 5), (got[3], ref[3], np.uint32, 5), (got[4], ref[4], np.uint8, 64)):
            assert a.dtype == dt and a.shape == (n,) and np.array_equal(a, b)
        assert np.all(np.diff(got[1].astype(np.int64)) > 0) and np.all(np.diff(got[3].astype(np.int64)) > 0)       # monotone in lg
        assert got[3][0] >= 1 and got[0] < 1 << 30
    tau1, thr, tau2, s2, win = Cl.bm3d_tables(4, 1)
    assert tau1 == 4 * 256 * 256 and tau2 == round(0.64 * 256 * 256)
    assert thr[0] == round(2.7 * 128 * 2) == 691 and thr[4] == round(2.7 * 128 * 8) == 2765
    assert s2[0] == 128 * 128 * 4 and s2[4] == 128 * 128 * 64
    assert Cl.bm3d_tables(4, 0)[1][0] == round(2.7 * 128) == 346 and Cl.bm3d_tables(4, 0)[0] == tau1          # matching does not depend on mix
    w = win.reshape(8, 8)
    assert w[0].tolist() == [3, 5, 6, 7, 7, 6, 5, 3] and w[3].tolist() == [7, 11, 14, 16, 16, 14, 11, 7]
    assert np.array_equal(w, w[::-1]) and np.array_equal(w, w.T) and w.min() == 3 and w.max() == 16
    k = np.kaiser(8, 2.0)
    assert np.array_equal(w, np.rint(16.0 * np.outer(k, k)).astype(np.uint8))                                 # what the literal table is
    for bad in ((0, 0, 1.0), (17, 0, 1.0), (9, 1, 1.0), (3, 1, 1.0), (4, 1, 0.0), (4, 1, float('nan')), (4, 1, 1.0, 0.0), (4, 1, 100.0)):
        with pytest.raises(ValueError):
            Cl.bm3d_tables(*bad)


def test_argument_errors_without_gpu(eld_lib):
    """Every range of the header, refused before any device work (a fake, non-null device pointer is never dereferenced)."""
    par = (ctypes.c_uint32 * 5)(691, 977, 1382, 1955, 2765)
    win = (ctypes.c_uint8 * 64)(*R.WIN.reshape(-1).tolist())
    p = ctypes.c_void_p(4096)
    ok = dict(N=1, C=4, h=8, w=8, S=12, step=3, Gmax=16, mix=1, tau=1000, frac=4)
    need = eld_lib.eld_bm3d_vst_workspace_bytes(1, 4, 8, 8)
    assert need >= 4 * 64 * (8 + 2)                                              # 64-bit numerators and 16-bit codes at the least
    assert eld_lib.eld_bm3d_vst_workspace_bytes(1, 4, 7, 8) == 0 and eld_lib.eld_bm3d_vst_workspace_bytes(1, 17, 8, 8) == 0
    assert eld_lib.eld_bm3d_vst_workspace_bytes(0, 4, 8, 8) == 0

    def call(par=par, win=win, x=p, fwd=p, out=p, guide=None, ws=p, ws_bytes=need, **kw):
        a = dict(ok, **kw)
        return eld_lib.eld_bm3d_vst_f32(x, a['N'], a['C'], a['h'], a['w'], 65535.0, fwd, guide, a['S'], a['step'], a['Gmax'], a['mix'], a['tau'], par, win,
                                        a['frac'], out, ws, ws_bytes, None)

    for kw in (dict(N=0), dict(N=-1), dict(C=0), dict(C=17), dict(h=7), dict(w=7), dict(h=0), dict(w=-8), dict(S=-1), dict(S=17), dict(step=0),
               dict(step=9), dict(Gmax=0), dict(Gmax=3), dict(Gmax=32), dict(Gmax=-2), dict(mix=2), dict(mix=-1), dict(C=3), dict(C=9), dict(C=12),
               dict(frac=-1), dict(frac=5), dict(tau=1 << 30), dict(tau=(1 << 32) - 1)):
        assert call(**kw) == -1, kw
    assert call(par=None) == -1 and call(win=None) == -1 and call(x=None) == -1 and call(fwd=None) == -1 and call(out=None) == -1
    assert call(ws=None) == -1
    assert call(x=ctypes.c_void_p(4098)) == -1 and call(out=ctypes.c_void_p(4097)) == -1 and call(fwd=ctypes.c_void_p(4097)) == -1
    assert call(guide=ctypes.c_void_p(4098)) == -1 and call(ws=ctypes.c_void_p(4100)) == -1
    for k, val in ((0, 0), (63, 17), (20, 255)):
        w = R.WIN.reshape(-1).tolist()
        w[k] = val
        assert call(win=(ctypes.c_uint8 * 64)(*w)) == -1, (k, val)
    zero = (ctypes.c_uint32 * 5)(691, 977, 0, 1955, 2765)
    assert call(par=zero, guide=p) == -1                                         # step 2 divides by E + par
    assert call(ws_bytes=need - 1) == -3 and call(ws_bytes=0) == -3              # ELD_EWS, behind every ELD_EINVAL
    assert call(ws_bytes=need - 1, C=3) == -1


def test_classical_denoiser_arguments():
    from eld_amd import classical as Cl
    d = Cl.ClassicalDenoiser('bayer', 2.0, sigma=3.0)                             # the default method: what it was
    assert (d.in_channels, d.search, d.patch, d.strength, d.label, d.method) == (4, 7, 2, 0.5, 'nlm', 'nlm')
    sh, wt = NR.nlm_weight_table(4, 2, 0.5)
    assert d.sh == sh and np.array_equal(d.wtab, wt)
    b = Cl.ClassicalDenoiser('bayer', 2.0, sigma=3.0, method='bm3d')
    assert (b.in_channels, b.out_channels, b.search, b.step, b.group, b.mix, b.strength, b.label, b.is_classical) == (4, 4, 12, 3, 16, True, 1.0, 'bm3d', True)
    ref = R.bm3d_tables(4, 1)
    assert b.tables[0] == ref[0] and b.tables[2] == ref[2] and all(np.array_equal(b.tables[k], ref[k]) for k in (1, 3, 4))
    xt = Cl.ClassicalDenoiser('xtrans', 2.0, sigma=3.0, method='bm3d')
    assert xt.in_channels == 9 and xt.mix is False and np.array_equal(xt.tables[1], R.bm3d_tables(9, 0)[1])
    assert Cl.ClassicalDenoiser('bayer', 2.0, sigma=3.0, method='bm3d', mix=False).mix is False
    c = Cl.ClassicalDenoiser('bayer', 2.0, sigma=3.0, method='bm3d', search=16, step=1, group=4, strength=0.8)
    assert (c.search, c.step, c.group, c.strength) == (16, 1, 4, 0.8)
    e = c.with_gain(4.0)
    assert (e.K, e.sigma, e.label, e.search, e.step, e.group, e.mix, e.strength) == (4.0, 3.0, 'bm3d', 16, 1, 4, True, 0.8) and c.with_gain(2.0) is c
    for kw in (dict(search=17), dict(search=-1), dict(patch=1), dict(patch=3), dict(step=0), dict(step=9), dict(step=2.5), dict(group=3), dict(group=32),
               dict(group=0), dict(strength=0.0), dict(mix='yes')):
        with pytest.raises(ValueError):
            Cl.ClassicalDenoiser('bayer', 2.0, sigma=3.0, method='bm3d', **kw)
    with pytest.raises(ValueError):
        Cl.ClassicalDenoiser('xtrans', 2.0, sigma=3.0, method='bm3d', mix=True)      # 9 planes: no power of two
    with pytest.raises(ValueError):
        Cl.ClassicalDenoiser('bayer', 2.0, sigma=3.0, method='dct')
    with pytest.raises(ValueError):
        Cl.ClassicalDenoiser('bayer', 2.0, sigma=3.0, search=12)                     # NLM keeps its range


def test_command_lines_parse():
    from eld_amd import classical as Cl
    from eld_amd import evaluate as E
    base = ['a.npy', '-o', 'out', '--K', '2.5', '--sigma', '3']
    a = Cl.parse_method_args(Cl.build_parser(), base)
    assert (a.method, a.search, a.patch, a.strength, a.step, a.group, a.no_mix) == ('nlm', 7, 2, 0.5, 3, 16, False)
    a = Cl.parse_method_args(Cl.build_parser(), base + ['--method', 'bm3d'])
    assert (a.method, a.search, a.patch, a.strength, a.step, a.group, a.no_mix) == ('bm3d', 12, 2, 1.0, 3, 16, False)
    a = Cl.parse_method_args(Cl.build_parser(), base + ['--method', 'bm3d', '--search', '9', '--strength', '0.5', '--step', '4', '--group', '8', '--no-mix'])
    assert (a.search, a.strength, a.step, a.group, a.no_mix) == (9, 0.5, 4, 8, True)
    with pytest.raises(SystemExit):
        Cl.build_parser().parse_args(base + ['--method', 'dct'])
    ev = ['pairs.json', '--ckpt', 'net.pt', '--baseline-K', '2', '--baseline-sigma', '3']
    a = Cl.parse_method_args(E.build_parser(), ev, 'baseline_method', 'baseline_')
    assert (a.baseline_method, a.baseline_search, a.baseline_strength) == ('nlm', 7, 0.5)
    a = Cl.parse_method_args(E.build_parser(), ev + ['--baseline-method', 'bm3d', '--baseline-step', '2'], 'baseline_method', 'baseline_')
    assert (a.baseline_method, a.baseline_search, a.baseline_strength, a.baseline_step, a.baseline_group, a.baseline_no_mix) == ('bm3d', 12, 1.0, 2, 16, False)
    # the report's lines take the label
    assert E.baseline_label({'psnr': 1.0, 'psnr_in': 0.5}) is None and E.baseline_label({'psnr_bm3d': 1.0}) == 'bm3d' and E.baseline_label({'psnr_nlm': 1.0}) == 'nlm'
    row = {'iso': 800, 'ratio': 100.0, 'count': 2, 'psnr': 40.0, 'ssim': 0.9, 'psnr_in': 30.0, 'ssim_in': 0.5}
    plain = E.table_lines([row])
    lines = E.table_lines([dict(row, psnr_bm3d=38.0, ssim_bm3d=0.8)])
    assert lines[0] == plain[0] + ' %9s %8s' % ('PSNR bm3d', 'SSIM bm3d') and lines[1] == plain[1] + ' %9.3f %8.4f' % (38.0, 0.8)
    assert E.table_lines([dict(row, psnr_nlm=38.0, ssim_nlm=0.8)])[0] == plain[0] + ' %9s %8s' % ('PSNR nlm', 'SSIM nlm')


@pytest.fixture(scope='module')
def pipeline():
    """planes -> (target, clipped input, NLM's output, BM3D's output) on the sec. 24 scene at seed 5, computed once"""
    K, sigma, black, white, ratio = 2.0, 3.0, 512, 16383, 100.0
    out = {}
    for C in (4, 9):
        clean = NR.scene_planes(C, 64, 64)
        codes = NR.noisy_codes(clean, K, sigma, black, white, 5)[None]
        target = clean * ratio / (white - black)
        clipped = np.clip((codes[0].astype(np.float64) - black) / (white - black) * ratio, 0.0, 1.0)
        nlm = NR.denoise_planes(codes, K, sigma, [black] * C, white, ratio)[0] if C == 4 else None
        out[C] = (target, clipped, nlm, R.denoise_planes_bm3d(codes, K, sigma, [black] * C, white, ratio)[0])
    return out


def test_reference_pipeline_on_a_bayer_frame(pipeline):
    """4 planes grouped across the planes.  Measured: input 33.67 dB, NLM 46.05 dB, BM3D 48.05 dB (46.54 dB after step 1): +14.4 dB over the
    input, +2.0 dB over NLM; the mean within 1.2 % of the scene's."""
    target, clipped, nlm, out = pipeline[4]
    p_in, p_nlm, p = NR.psnr(clipped, target), NR.psnr(nlm, target), NR.psnr(out, target)
    print('bayer: PSNR in %.2f dB, nlm %.2f dB, bm3d %.2f dB' % (p_in, p_nlm, p))
    assert p - p_in >= 6.0
    assert p - p_nlm >= 1.0
    assert abs(float(out.mean()) / float(target.mean()) - 1.0) < 0.05


def test_reference_pipeline_on_an_xtrans_frame(pipeline):
    """9 planes, every plane alone.  Measured: input 33.70 dB, BM3D 46.97 dB (NLM: 47.06 dB -- a tie, sec. 25): +13.3 dB."""
    target, clipped, _, out = pipeline[9]
    p_in, p = NR.psnr(clipped, target), NR.psnr(out, target)
    print('xtrans: PSNR in %.2f dB, bm3d %.2f dB' % (p_in, p))
    assert p - p_in >= 6.0
    assert abs(float(out.mean()) / float(target.mean()) - 1.0) < 0.05
