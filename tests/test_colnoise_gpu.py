"""GPU tests of the column term of the fused sampler (flag COL, model letter C): the output is the restated float32 chain on the kernel's
own dumped variates bit for bit on every path (vector, scalar, several blocks, one-row blocks, LDS staging and its fallback, Bayer and
X-Trans), the dumped column normal is one value per sensor column and Philox's (column, stream 9) normal, injected variates replay, the
specialised 'PGRCU' kernels equal the runtime-flags kernel, a launch without the flag ignores the field the scale travels in, and the closed
loops: calibrate --column recovers a minted law, validate --structure shows the column variance matched, train_frames trains on 'PGRCU'.

Statistical bounds are 5 standard errors from the counts (the two formulas of tests/test_structure_cpu.py)."""
import contextlib
import io
import json
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from oracle import noise_ref as O          # noqa: E402

import colnoise_ref as CR                  # noqa: E402

FULL = O.SHOT_POISSON | O.READ_TL | O.ROW | O.QUANT
FULLC = FULL | CR.COL
SEED = 2018


@pytest.fixture(scope='module')
def dev(eld_lib):
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def params(N, col=True):
    from eld_amd.noise import NoiseParams
    return [NoiseParams(0.4 + i, 3.0 + i, 15583, 100.0 + 90 * i, tl_lambda=[-0.14285714, 0.0, 0.114285715][i % 3], tl_scale=2.5 + i,
                        row_scale=0.7 + i, col_scale=(1.3 + 0.5 * i) if col else 0.0) for i in range(N)]


def oparams(p):
    return O.Params(K=p[0], g_scale=p[1], saturation=p[2], ratio=p[3], tl_lambda=p.tl_lambda, tl_scale=p.tl_scale, row_scale=p.row_scale,
                    q_step=p.q_step, color_bias=p.color_bias)


PLANES = {'counts': 0, 'n_shot': 1, 'n_read': 2, 't_tl': 3, 'n_row': 4, 'u_q': 5, 'n_col': CR.PLANE_NCOL}


def run(y, plist, flags, ids, dump=False, inject=None, seed=SEED, recs=None):
    from eld_amd.noise import make_records, sample_noise_records
    yt = torch.from_numpy(np.ascontiguousarray(y)).cuda()
    numel = int(np.prod(y.shape))
    nplanes = CR.NPLANES_COL if flags & CR.COL else 6
    dmp = torch.full((nplanes, numel), float('nan'), dtype=torch.float32, device='cuda') if dump else None
    inj = None
    if inject is not None:
        planes = np.zeros((nplanes, numel), np.float32)
        for k, v in inject.items():
            planes[PLANES[k]] = np.asarray(v, np.float32).reshape(-1)
        inj = torch.from_numpy(planes).cuda()
    recs = make_records(plist, ids) if recs is None else recs
    z = sample_noise_records(yt, recs, flags, seed, inject=inj, dump=dmp)
    torch.cuda.synchronize()
    z = z.cpu().numpy()
    if dump:
        d = dmp.cpu().numpy()
        return z, {k: d[i].reshape(y.shape) for k, i in PLANES.items() if i < nplanes}
    return z


def synth(rng, shape):
    return (np.floor(65535 * rng.random(shape, dtype=np.float32) ** 2.2) / 65535).astype(np.float32)


def cfa_flag(shape):
    return CR.XT if shape[1] == 9 else 0


# Bayer: 16-byte path; scalar path; several blocks per image (4096 elements each; the last lies in one plane: one column parity); H = 2 with
# 2 W just beyond / exactly at the LDS column capacity (one block across all planes: fallback to per-element draws / the last staged
# layout); a tail block inside one packed row (vector and scalar).  X-Trans: w % 4 == 0, w % 4 != 0 and an image of two blocks.
W_OVER, W_FIT = CR.LDS_COLS // 2 + 4, CR.LDS_COLS // 2
SHAPES = [(2, 4, 6, 8), (1, 4, 6, 7), (1, 4, 40, 64), (1, 4, 2, W_OVER), (1, 4, 2, W_FIT), (1, 4, 3, 1368), (1, 4, 3, 1367),
          (1, 9, 4, 8), (1, 9, 4, 6), (1, 9, 12, 40)]


@pytest.mark.parametrize('shape', SHAPES)
def test_dumped_variates_replay_and_column_plane(dev, shape):
    N, C, H, W = shape
    assert 2 * W_OVER > CR.LDS_COLS >= 2 * W_FIT and W_OVER % 4 == 0
    rng = np.random.default_rng(1000 * H + W)
    y = synth(rng, shape)
    plist = params(N)
    ids = [40 + 7 * i for i in range(N)]
    flags = FULLC | cfa_flag(shape)
    z, v = run(y, plist, flags, ids, dump=True)
    cols = CR.sensor_cols(C, H, W)
    for i in range(N):
        zi = CR.noise_arith_col(y[i], oparams(plist[i]), flags & ~CR.XT, col_scale=plist[i].col_scale, **{k: a[i] for k, a in v.items()})
        assert np.array_equal(z[i].view(np.uint32), zi.view(np.uint32)), int(np.sum(z[i] != zi))
        mos = CR.unpack(v['n_col'][i])
        assert mos.shape[1] == CR.n_sensor_cols(C, W)
        assert np.array_equal(mos, np.broadcast_to(mos[:1], mos.shape))                 # one normal per sensor column: rows, planes, blocks
        nrm = CR.col_normals(CR.n_sensor_cols(C, W), SEED, ids[i])
        assert np.max(np.abs(mos[0] - nrm)) < 1e-4                                      # Box-Muller of Philox (column, STREAM_COL): hardware log / cos
        assert np.max(np.abs(v['n_col'][i] - nrm[cols])) < 1e-4
        assert np.std(mos[0]) > 0.3                                                     # and they are not all one number
    # the term is in the output: the same launch with the scale at zero differs
    z0 = run(y, params(N, col=False), flags, ids)
    assert not np.array_equal(z0, z)


@pytest.mark.parametrize('shape', [(2, 4, 6, 8), (1, 4, 5, 7), (1, 9, 4, 6)])
def test_injected_variates_replay(dev, shape):
    N = shape[0]
    rng = np.random.default_rng(sum(shape))
    y = synth(rng, shape)
    plist = params(N)
    inj = {'counts': rng.poisson(20.0, shape).astype(np.float32), 't_tl': (3 * rng.standard_normal(shape)).astype(np.float32),
           'n_row': rng.standard_normal(shape).astype(np.float32), 'n_col': rng.standard_normal(shape).astype(np.float32),
           'u_q': rng.uniform(size=shape).astype(np.float32)}
    flags = FULLC | cfa_flag(shape)
    z = run(y, plist, flags, list(range(N)), inject=inj)
    for i in range(N):
        zi = CR.noise_arith_col(y[i], oparams(plist[i]), flags & ~CR.XT, col_scale=plist[i].col_scale, **{k: a[i] for k, a in inj.items()})
        assert np.array_equal(z[i].view(np.uint32), zi.view(np.uint32))


@pytest.mark.parametrize('clip', [0, O.CLIP])
@pytest.mark.parametrize('shape', [(2, 4, 40, 64), (1, 4, 2, W_OVER), (2, 9, 12, 40)])
def test_specialised_equals_runtime_flags(dev, shape, clip):
    """No debug buffers and W % 4 == 0: the compile-time 'PGRCU' kernel runs; with `dump` the runtime-flags kernel.  Same seed, same bits."""
    N = shape[0]
    y = synth(np.random.default_rng(9), shape)
    flags = FULLC | clip | cfa_flag(shape)
    ids = [(3 << 32) | 17, 5][:N]
    zr, _ = run(y, params(N), flags, ids, dump=True)
    zs = run(y, params(N), flags, ids)
    assert np.array_equal(zs.view(np.uint32), zr.view(np.uint32))
    if clip:
        assert zs.min() >= 0.0 and zs.max() <= 1.0


def test_launch_without_the_flag_ignores_reserved(dev):
    from eld_amd.noise import make_records
    shape = (2, 4, 40, 64)
    y = synth(np.random.default_rng(2), shape)
    recs = make_records(params(2, col=False), [8, 9])
    assert recs['reserved'].tolist() == [[0, 0], [0, 0]]
    want = run(y, None, FULL, None, recs=recs)
    junk = recs.copy()
    junk['reserved'][:, 0] = [0xDEADBEEF, 0x7FC00000]            # garbage and a NaN's bits
    junk['reserved'][:, 1] = [0xFFFFFFFF, 17]
    assert np.array_equal(run(y, None, FULL, None, recs=junk).view(np.uint32), want.view(np.uint32))
    zd, _ = run(y, None, FULL, None, recs=junk, dump=True)          # the runtime-flags kernel too
    assert np.array_equal(zd.view(np.uint32), want.view(np.uint32))


def test_einval_before_launch(dev, eld_lib):
    from eld_amd import _lib as L
    from eld_amd.noise import make_records, sample_noise, NoiseParams, _upload

    def rc(C, flags):
        y = torch.zeros((1, C, 4, 8), dtype=torch.float32, device=dev)
        out = torch.full_like(y, 7.0)
        prm = _upload(np.ascontiguousarray(make_records(params(1), [0])).view(np.uint8).reshape(-1), y.device)
        r = eld_lib.eld_noise_forward(L.dptr(y), L.IN_F32, L.dptr(out), L.dptr(prm), 1, C, 4, 8, flags, 1, None, None, L.cur_stream())
        torch.cuda.synchronize()
        if r != 0:
            assert bool((out == 7.0).all())                       # refused before any launch: the output is untouched
        return r
    assert rc(4, L.COL) == 0 and rc(9, L.COL | L.CFA_XTRANS) == 0
    for C, flags in ((3, L.COL), (9, L.COL), (4, L.COL | L.CFA_XTRANS), (8, FULLC), (9, FULLC)):
        assert rc(C, flags) == -1, (C, flags)
    # COL with DARK, on a launch that is valid without COL
    import darknoise_ref as R
    from eld_amd.darkpool import DarkPool
    mos = R.mosaics_of(((20, 28), (24, 40), (22, 30)))
    pool = DarkPool([{'iso': 100, 'bias': mos}], raw_pattern=R.PATTERNS[0], black_level=R.BLACK, white_level=16383, K=(1.5,), device=dev)
    y = torch.zeros((1, 4, 8, 12), dtype=torch.float32, device=dev)
    prm = [NoiseParams(1.5, 0.0, pool.saturation, 120.0, dark=pool.ranges[0])]
    pdu = L.SHOT_POISSON | L.DARK | L.QUANT
    assert bool(torch.isfinite(sample_noise(y, prm, pdu, SEED, [3], dark=pool)).all())
    with pytest.raises(L.EldError, match=r'code -1'):
        sample_noise(y, prm, pdu | L.COL, SEED, [3], dark=pool)


def test_column_statistics(dev):
    """Model C alone on zero input at saturation = ratio = 1: z = n_col * col_scale, nothing white beside it (white share 0)."""
    from eld_amd.noise import NoiseParams
    N, H, W, s = 8, 64, 96, 1.75
    y = np.zeros((N, 4, H, W), np.float32)
    z = run(y, [NoiseParams(1.0, 0.0, 1.0, 1.0, col_scale=s)] * N, CR.COL, list(range(500, 500 + N)))
    ncol = 2 * W
    means = np.stack([CR.unpack(z[i]).astype(np.float64).mean(axis=0) for i in range(N)])        # (N, 2W) column means
    white = 0.0                                                    # variance of a column mean beside the column term: no other term is on
    v = float(np.mean(np.var(means, axis=1, ddof=1)))              # N independent estimates from ncol values each
    se = (s * s + white) * math.sqrt(2.0 / (N * (ncol - 1)))
    print('column-mean variance', v, 'expect', s * s + white, 'se', se)
    assert abs(v - (s * s + white)) < 5 * se
    ev, od = means[:, 0::2].reshape(-1), means[:, 1::2].reshape(-1)  # the two column parities: planes {0, 3} and {1, 2}
    r = float(np.corrcoef(ev, od)[0, 1])
    print('parity correlation', r, 'se', 1.0 / math.sqrt(ev.size - 1))
    assert abs(r) < 5.0 / math.sqrt(ev.size - 1)
    for i in range(N):                                             # planes that share a sensor column share its normal
        assert np.array_equal(z[i, 0], z[i, 3]) and np.array_equal(z[i, 1], z[i, 2]) and not np.array_equal(z[i, 0], z[i, 1])


# ---- closed loops (the sizes of tests/test_calib_gpu.py: five sessions, two 256 x 384 bias frames and six flat pairs each) -----------------
C_SLOPE, C_BIAS = 0.5, math.log(0.6)


def c_law(K):
    return float(np.exp(C_SLOPE * np.log(K) + C_BIAS))


def tl_var(lam):
    """Variance of the unit-scale Tukey-lambda distribution of shape lam != 0."""
    return 2.0 / lam ** 2 * (1.0 / (1 + 2 * lam) - math.gamma(lam + 1) ** 2 / math.gamma(2 * lam + 2))


@pytest.fixture(scope='module')
def column_sessions(eld_lib):
    from eld_amd import _lib as L
    from eld_amd import calibrate as CAL
    from eld_amd.noise import NoiseParams
    from test_calib_gpu import _law, synth_mosaics
    h, w, F, P = 128, 192, 2, 6
    sessions, sid = [], 770000
    for s, K in enumerate([0.5, 1.0, 2.0, 4.0, 8.0]):
        lam = float(CAL.DEFAULT_LAMBDAS[70 + (4, 8, 10, 6, 9)[s]])
        prm = [NoiseParams(1.0, 0.0, 1.0, 1.0, tl_lambda=lam, tl_scale=_law('G_scale', K), row_scale=_law('R_scale', K), col_scale=c_law(K))] * F
        bias = synth_mosaics(prm, L.READ_TL | L.ROW | L.COL, list(range(sid, sid + F)), h, w)        # 'GRC' at saturation = ratio = 1: DN
        sid += F
        S = 16383.0 - 512.0
        levels = np.linspace(300.0, 0.5 * S, P)
        y = torch.from_numpy(np.repeat(levels / S, 2).astype(np.float32)).cuda().view(-1, 1, 1, 1).expand(2 * P, 4, h, w).contiguous()
        flats = synth_mosaics([NoiseParams(K, _law('g_scale', K), S, 1.0)] * (2 * P), L.SHOT_POISSON | L.READ_GAUSS, list(range(sid, sid + 2 * P)),
                              h, w, y=y, dn=S).view(P, 2, 2 * h, 2 * w)
        sid += 2 * P
        sessions.append({'iso': int(100 * K), 'bias': bias.cpu().numpy(), 'flats': flats.cpu().numpy(), 'K': K, 'lambda': lam,
                         'site': _law('G_scale', K) ** 2 * tl_var(lam) + 1.0 / 12.0})
    return sessions


def test_calibrate_column_recovers_the_law(column_sessions):
    from eld_amd import calibrate as CAL
    from test_calib_gpu import SAMPLER_PATTERN
    Hm, Wm = 256, 384
    sess = [{k: s[k] for k in ('iso', 'bias', 'flats')} for s in column_sessions]
    plain, pdiag = CAL.calibrate_camera(sess, SAMPLER_PATTERN, [512.0] * 4, 16383)
    params, diag = CAL.calibrate_camera(sess, SAMPLER_PATTERN, [512.0] * 4, 16383, column=True)
    # without the flag: today's keys; with it: the same numbers plus the column's
    assert set(plain['Profile-1']) == set(CAL.SIGMA_KEYS) and 'column' not in pdiag and all('C_scale' not in fr for fr in pdiag['frames'])
    assert set(params['Profile-1']) == set(CAL.SIGMA_KEYS) | {'C_scale'}
    for k in CAL.SIGMA_KEYS:
        assert params['Profile-1'][k] == plain['Profile-1'][k]
    assert np.array_equal(params['G_shape'], plain['G_shape']) and np.array_equal(params['color_bias'], plain['color_bias'])
    for a, b in zip(diag['frames'], pdiag['frames']):
        assert {k: v for k, v in a.items() if k not in ('C_scale', 'color_bias')} == {k: v for k, v in b.items() if k != 'color_bias'}
    # per frame: C_scale^2 = col_var_sensor, a covariance over the Wm sensor columns of the two row phases' column means, each of variance
    # C^2 + site / (Hm / 2) (site: what is independent from site to site: the Tukey-lambda read noise and the rounding to codes)
    rel = []
    for fr in diag['frames']:
        s = column_sessions[fr['session']]
        C2 = c_law(s['K']) ** 2
        vc = C2 + s['site'] / (Hm // 2)
        se = math.sqrt((vc * vc + C2 * C2) / (Wm - 1))
        print('K', s['K'], 'C_scale^2', fr['C_scale'] ** 2, 'expect', C2, 'se', se)
        assert abs(fr['C_scale'] ** 2 - C2) < 5 * se
        rel.append(se / (2 * C2))                                   # relative s.e. of the frame's C_scale
    # the law: the derivation tests/test_calib_gpu.py gives for R_scale, for columns.  m = 10 frames over log K of sd ~1.0: the slope's s.e. is
    # (relative s.e. of a frame's sample) / (sd(log K) sqrt(m)); the bias' about the same.  That file's bound is 4 such s.e. (0.08 for 0.02).
    x = np.log([fr['K'] for fr in diag['frames']])
    tol = 4 * max(rel) / (float(np.std(x)) * math.sqrt(len(x)))
    law = params['Profile-1']['C_scale']
    print('law', law, 'tol', tol)
    assert abs(law['slope'] - C_SLOPE) < tol and abs(law['bias'] - C_BIAS) < tol
    # the fixed share: two frames of a session were minted with their own sample ids, hence their own column patterns -- none of it is fixed
    assert len(diag['column']) == 5
    N_c = Wm // 2
    for c, s in zip(diag['column'], column_sessions):
        C2 = c_law(s['K']) ** 2
        vc = C2 + s['site'] / (Hm // 2)
        assert abs(c['col_fixed_var']) < 5 * vc / math.sqrt(N_c - 1) and abs(c['fixed_share'] - c['col_fixed_var'] / c['col_var']) < 1e-12


def test_calibrate_cli_column_and_train_frames(column_sessions, tmp_path):
    """calibrate --column writes a table NoiseModel('PGRCU') takes; train_frames --noise PGRCU trains on it and writes a checkpoint."""
    from eld_amd import calibrate as CAL
    from eld_amd import train_frames
    from eld_amd.noise import load_camera_params
    from test_calib_gpu import SAMPLER_PATTERN
    man = {'raw_pattern': SAMPLER_PATTERN, 'black_level': [512] * 4, 'white_level': 16383, 'sessions': []}
    for i, s in enumerate(column_sessions):
        e = {'iso': s['iso'], 'bias': [], 'flats': []}
        for j, u in enumerate(s['bias']):
            np.save(tmp_path / ('b%d_%d.npy' % (i, j)), u[:64, :96])
            e['bias'].append('b%d_%d.npy' % (i, j))
        for j, p in enumerate(s['flats'][:4]):
            np.save(tmp_path / ('f%d_%da.npy' % (i, j)), p[0][:64, :96])
            np.save(tmp_path / ('f%d_%db.npy' % (i, j)), p[1][:64, :96])
            e['flats'].append(['f%d_%da.npy' % (i, j), 'f%d_%db.npy' % (i, j)])
        man['sessions'].append(e)
    (tmp_path / 'm.json').write_text(json.dumps(man))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert CAL.main([str(tmp_path / 'm.json'), '--camera', 'Cam', '--out', str(tmp_path / 'tables'), '--column']) == 0
    text = buf.getvalue()
    assert 'C_scale' in text and 'fixed share' in text
    table = load_camera_params('Cam', str(tmp_path / 'tables'))
    assert set(table['Profile-1']['C_scale']) == {'slope', 'bias', 'sigma'}
    rng = np.random.default_rng(1)
    for i in range(2):
        np.save(tmp_path / ('long%d.npy' % i), (512 + rng.integers(0, 12000, size=(64, 96))).astype(np.uint16))
    (tmp_path / 'sensor.json').write_text(json.dumps({'cfa': 'bayer', 'black_level_per_channel': [512] * 4, 'white_level': 16383,
                                                      'raw_pattern': SAMPLER_PATTERN}))
    ckpt = tmp_path / 'out' / 'model.pt'
    os.makedirs(tmp_path / 'out')
    with contextlib.redirect_stdout(io.StringIO()):
        rc = train_frames.main([str(tmp_path / 'long*.npy'), '--meta', str(tmp_path / 'sensor.json'), '--camera', str(tmp_path / 'tables' / 'Cam_params.npy'),
                                '--noise', 'PGRCU', '--patch', '32', '--steps', '2', '-o', str(ckpt)])
    assert rc == 0 and ckpt.exists() and ckpt.stat().st_size > 0
    # a table without the law is refused, and the message says what to run
    with pytest.raises(ValueError, match='calibrate --column'), contextlib.redirect_stdout(io.StringIO()):
        train_frames.main([str(tmp_path / 'long*.npy'), '--meta', str(tmp_path / 'sensor.json'), '--camera', 'SonyA7S2', '--noise', 'PGRCU',
                           '--patch', '32', '--steps', '2', '-o', str(ckpt)])


def test_validate_structure_shows_the_gap_closed(eld_lib):
    """Frames minted under 'PGRC': validate --structure must show the 'PGRC' synthesis with the sensor's column variance, 'PGR' with none."""
    from eld_amd import validate as V
    PAT, BLACK, WHITE = [[0, 1], [3, 2]], [512.0] * 4, 16383
    HM, WM, F = 256, 384, 3
    K, TL, LAM, ROW, COLS = 2.0, 3.0, 0.14, 1.5, 1.2
    prm = {'K': K, 'g_scale': 0.0, 'tl_scale': TL, 'row_scale': ROW, 'tl_lambda': LAM, 'color_bias': [0.0] * 4, 'col_scale': COLS}
    rec = {'K': K, 'g_scale': 0.0, 'G_scale': TL, 'R_scale': ROW, 'lambda': LAM, 'color_bias': [0.0] * 4, 'C_scale': COLS}
    sessions = []
    for si in range(2):
        codes = []
        for f in range(F + 2):
            clean = None if f < F else np.full((4, HM // 2, WM // 2), 0.05, np.float32)
            codes.append(V.synthesize_codes(clean, prm, 'PGRC', 'bayer', 99, 1000 + 16 * si + f, WHITE, BLACK, shape=(4, HM // 2, WM // 2)).cpu().numpy())
        sessions.append({'iso': 800 * (si + 1), 'bias': np.stack(codes[:F]), 'flats': np.stack(codes[F:])[None]})
    kw = dict(models=('PGR', 'PGRC'), source='frames', radius=64, flat_radius=256, structure=True, lags=2)
    rep = V.validate_camera(sessions, PAT, BLACK, WHITE, diag={'frames': [dict(rec) for _ in range(2 * F)]}, **kw)
    with pytest.raises(ValueError, match='calibrate --column'):      # a diag without the sample cannot feed the letter
        V.validate_camera(sessions, PAT, BLACK, WHITE, diag={'frames': [{k: v for k, v in rec.items() if k != 'C_scale'} for _ in range(2 * F)]}, **kw)
    n_c, N_c = HM // 2, WM // 2
    site = TL ** 2 * tl_var(LAM) + 1.0 / 12.0        # a dark frame: read noise and the rounding to codes are what is independent per site
    se_col = (COLS ** 2 + site / n_c) * math.sqrt(2.0 / (N_c - 1))   # one estimate of col_var; the report's means over frames and groups have no more
    se_fix = math.sqrt(((COLS ** 2 + site / n_c) ** 2) / (N_c - 1))
    for s in rep['structure']['sessions']:
        real, pgr, pgrc = s['real'], s['models']['PGR']['synthetic'], s['models']['PGRC']['synthetic']
        print('real', real['col_var'], real['col_fixed_var'], 'PGR', pgr['col_var'], 'PGRC', pgrc['col_var'], pgrc['col_fixed_var'], 'se', se_col)
        assert abs(real['col_var'] - COLS ** 2) < 5 * se_col
        assert abs(pgrc['col_var'] - real['col_var']) < 5 * math.sqrt(2.0) * se_col
        assert abs(pgr['col_var']) < 5 * (site / n_c) * math.sqrt(2.0 / (N_c - 1))
        assert abs(pgrc['col_fixed_var']) < 5 * se_fix and abs(real['col_fixed_var']) < 5 * se_fix      # a fresh pattern per sample: nothing fixed
        assert abs(pgrc['col_var_sensor'] - real['col_var_sensor']) < 5 * math.sqrt(2.0) * math.sqrt(((COLS ** 2 + site / n_c) ** 2 + COLS ** 4) / (WM - 1))
